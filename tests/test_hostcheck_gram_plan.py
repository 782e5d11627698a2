"""csrc/mcba_gram_plan.h (which launches linearise a shard, and what the host derives from that choice) compiled with g++
(tests/hostcheck/gram_plan_hostcheck.cpp) and held, without a GPU, to the rules it replaced: tests/gram_plan_oracle.py, the overwrite sequence
of the former derive_geometry and the fallbacks of the former launch_gram, gram_chunk_doubles and lm_reduce_chain, transcribed literally
and compared with those functions line by line.  Every comparison is of integers and exact.

The one intended difference: a forced MCBA_GRAM_SPLIT=3 on a shard without a usable tail sizes no chunk scratch (the former code sized a buffer
that no launch touched) -- chunk_doubles is held to the former figure wherever a chunk tail is launched, and to 0 elsewhere."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

import gram_plan_oracle as gpo

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck", "gram_plan_hostcheck.cpp")
WHOLE = ["fused", "roles", "psplit", "role_a"]        # enum GramKind
TAIL = [None, "roles", "chunks", "psplit"]            # enum GramTail
CS = range(1, 41)
NFBS = list(range(1, 260)) + [391, 521, 1000]
NS = (4, 54, 127, 128, 200)
SLOTS = (1024, 1216, 416)


@pytest.fixture(scope="module")
def hc(tmp_path_factory):
    lib = str(tmp_path_factory.mktemp("gram_plan_hostcheck") / "libgram_plan_hostcheck.so")
    subprocess.check_call(["g++", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-o", lib, SRC])
    h = ctypes.CDLL(lib)
    h.hc_gram_plan.argtypes = [ctypes.c_longlong, ctypes.c_void_p, ctypes.c_void_p]
    h.hc_gram_plan.restype = None
    h.hc_gram_xch_doubles.restype = ctypes.c_longlong
    return h


def plans(hc, rows):
    """rows of (C, nfb, N, slots, cw, ps_ok, force_split or None, force_npw or None) -> one dict of columns per call"""
    shapes = np.array([[r[0], r[1], r[2], r[3], r[4], int(r[5]), -1 if r[6] is None else r[6], -1 if r[7] is None else r[7]] for r in rows], dtype=np.int32)
    out = np.full((len(rows), hc.hc_gram_plan_cols()), -7, dtype=np.int64)
    hc.hc_gram_plan(len(rows), ctypes.c_void_p(shapes.ctypes.data), ctypes.c_void_p(out.ctypes.data))
    return out


def check(hc, rows):
    """The five requirements, row by row; returns how often each (whole, tail) was planned."""
    seen = {}
    for r, o in zip(rows, plans(hc, rows).tolist()):
        C, nfb, N, slots, cw, ps_ok, fsplit, fnpw = r
        refused, split, npw, nchunk, whole, tail, head, with_b, ppc, nrun, chunk_doubles, lds, cstride, cinner, cdense, fused_blocks, tail_blocks, fused_quads, ps_groups, cut = o
        want = gpo.parent_plan(C, nfb, N, slots, ps_ok, cw, fsplit, fnpw)
        assert (want is None) == bool(refused), r
        if want is None:
            continue
        wsplit, wnpw, wnchunk = want
        # 1. what was asked for
        assert split == wsplit, (r, o, want)
        if split in (4, 5):
            assert npw == wnpw, (r, o, want)
        if split == 3:
            assert nchunk == wnchunk, (r, o, want)
        # 2. what is launched
        launch = gpo.parent_launch(C, nfb, slots, cw, wsplit, wnchunk)
        assert (WHOLE[whole], TAIL[tail]) == launch, (r, o, launch)
        assert with_b == (cw != 6), r
        # 3. the cut
        assert head % 4 == 0 and 0 <= head <= nfb and head == cut == gpo.parent_head(C, nfb, slots), (r, o)
        assert (tail != 0) <= (0 < head < nfb), (r, o)
        assert fused_blocks == (head if tail else nfb) and tail_blocks == (nfb - head if tail else 0) and fused_quads == (fused_blocks + 3) // 4, (r, o)
        # 4. the chunk scratch, the chunk launch
        if launch[1] == "chunks":
            assert nchunk >= 2 and chunk_doubles == gpo.parent_chunk_doubles(C, nfb, wnchunk, slots) == C * (nfb - head) * nchunk * 88 * 64, (r, o)
            assert ppc == ((N + nchunk - 1) // nchunk + 3) & ~3 and nrun == (N + ppc - 1) // ppc and 1 <= nrun <= nchunk, (r, o)
        else:
            assert chunk_doubles == 0, (r, o)
        # the point split's grid and LDS, as the former launch_gram computed them
        if "psplit" in launch:
            per = 1 if wnpw == 4 else 2
            blocks = nfb if launch[0] == "psplit" else nfb - head
            assert npw in (2, 4) and ps_groups == (blocks + per - 1) // per, (r, o)
            assert lds == 8 * hc.hc_gram_xch_doubles(npw, int(cw != 6)), (r, o)
        # 5. where k_syrk finds the trial cost
        assert (cstride, cinner, cdense) == gpo.parent_cost_slots(C, nfb, slots, wsplit), (r, o)
        seen[launch] = seen.get(launch, 0) + 1
    return seen


def test_unforced_sweep_equals_the_former_rules(hc):
    total = {}
    for slots, ps_ok, cw in itertools.product(SLOTS, (True, False), (12, 6)):
        rows = [(C, nfb, N, slots, cw, ps_ok, None, None) for C in CS for nfb in NFBS for N in NS]
        for k, v in check(hc, rows).items():
            total[(ps_ok, cw) + k] = total.get((ps_ok, cw) + k, 0) + v
    print({k: v for k, v in sorted(total.items(), key=str)})
    # the sweep reaches every plan, with and without the point split's LDS
    for ps_ok in (True, False):
        for launch in [("fused", None), ("roles", None), ("fused", "roles"), ("fused", "chunks")] + ([("psplit", None), ("fused", "psplit")] if ps_ok else []):
            assert total.get((ps_ok, 12) + launch, 0) > 0, (ps_ok, launch)
        assert total.get((ps_ok, 6, "role_a", None), 0) > 0
    assert total.get((True, 6, "psplit", None), 0) > 0


def test_forced_sweep_equals_the_former_rules(hc):
    """Every MCBA_GRAM_SPLIT with MCBA_GRAM_NPW unset, 2 and 4 (and a value that is neither), on a thinned grid that keeps the anchor shapes."""
    cs = (1, 2, 3, 6, 12, 24, 37, 40)
    nfbs = sorted(set(list(range(1, 260, 13)) + [3, 4, 5, 31, 38, 61, 98, 129, 157, 196, 391, 521, 1000]))
    rows = [(C, nfb, N, slots, cw, ps_ok, fs, fn) for C in cs for nfb in nfbs for N in NS for slots in SLOTS for cw in (12, 6) for ps_ok in (True, False)
            for fs in range(6) for fn in (None, 2, 4)]
    rows += [(C, nfb, 54, 1024, 12, True, fs, fn) for C in cs for nfb in nfbs for fs in (None, 4, 5) for fn in (0, 3)]
    seen = check(hc, rows)
    assert all(seen.get(k, 0) > 0 for k in [("fused", None), ("roles", None), ("fused", "roles"), ("fused", "chunks"), ("psplit", None), ("fused", "psplit"), ("role_a", None)])
    # the refusal: a forced point split without its LDS, whatever else is set
    out = plans(hc, [(6, 10, 54, 1024, 12, False, 4, None), (6, 10, 54, 1024, 6, False, 5, 2), (6, 10, 54, 1024, 12, False, 3, None)])
    assert out[:, 0].tolist() == [1, 1, 0]


@pytest.mark.parametrize("C,nfb,N,split,npw,nchunk", [(6, 157, 54, 0, None, None), (6, 196, 54, 5, 4, None), (24, 98, 200, 3, None, 3), (12, 98, 200, 5, 4, None), (2, 129, 54, 4, 2, None),
                                                      (37, 38, 54, 1, None, None), (40, 61, 54, 2, None, None), (37, 31, 54, 5, 2, None), (37, 31, 128, 3, None, 3)])
def test_anchor_shapes_at_1024_slots(hc, C, nfb, N, split, npw, nchunk):
    o = plans(hc, [(C, nfb, N, 1024, 12, True, None, None)])[0]
    assert o[0] == 0 and o[1] == split
    assert npw is None or o[2] == npw
    assert nchunk is None or o[3] == nchunk
    assert gpo.parent_plan(C, nfb, N, 1024, True, 12)[0] == split


def test_role_a_exchange_area_needs_no_opt_in(hc):
    """k_gram_psplit's ROLE 0 instances are left out of the LDS opt-in list (a static_assert in mcba_kernels.hip): their exchange area fits 64 KiB;
    every instance with role B needs the opt-in."""
    assert hc.hc_gram_xch_doubles(4, 0) * 8 <= 65536 and hc.hc_gram_xch_doubles(2, 0) * 8 <= 65536
    assert hc.hc_gram_xch_doubles(4, 1) * 8 == 150016 and hc.hc_gram_xch_doubles(2, 1) * 8 > 65536
