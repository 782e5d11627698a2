"""csrc/mcba_fivepoint_math.h -- the per-lane text of the five-point generator -- compiled with g++ -O2 (tests/hostcheck/fivepoint_hostcheck.cpp) and
held to tests/fivepoint_oracle.py without a GPU, by the rules of that module's docstring (the GPU tier's, tests/test_gpu_fivepoint.py): every
comparable candidate of the oracle within K5 EPS (cond kappa + sigma_1 / sigma_5) of exactly one candidate of its sample, in order; void
samples; the compaction order and the (sample, slot) map; the winner and the pose through twoview_oracle's checkers, the oracle scoring the
table that came back; bad arguments.

MCBA_HOSTCHECK_SANITIZE=1 (opt-in, CPU only): the same harness is also built as a stand-alone program with its own main and
-fsanitize=address,undefined, reads a scene file written here and must exit 0.  Nothing is preloaded; the shared object is never built with a
sanitizer."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import fivepoint_oracle as fo
import twoview_oracle as tvo
from multicam_calibration_amd.triangulation import _cam_blocks

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck", "fivepoint_hostcheck.cpp")
SANITIZE = os.environ.get("MCBA_HOSTCHECK_SANITIZE") == "1"
V = ctypes.c_void_p
SLOTS = fo.SLOTS


def P(a):
    return V(a.ctypes.data) if a is not None else None


@pytest.fixture(scope="module")
def hc(tmp_path_factory):
    lib = str(tmp_path_factory.mktemp("fivepoint_hostcheck") / "libfivepoint_hostcheck.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-o", lib, SRC])
    h = ctypes.CDLL(lib)
    h.hc_fp_candidates.argtypes = [ctypes.c_int, V, V, V, V, V, V]
    h.hc_fp_candidates.restype = None
    h.hc_two_view_ransac5.argtypes = [ctypes.c_size_t, V, V, V, V, ctypes.c_int, V, ctypes.c_double, ctypes.c_int, V, V, V, V, V, V, V, V, V, V]
    return h


def candidates(hc, xa, xb):
    """the test hook: (H, 5, 2) correspondences as they are -> E10 (H, 10, 9), status10 (H, 10), live (H), diag (H, 2)"""
    xa, xb = np.ascontiguousarray(xa, dtype=np.float64), np.ascontiguousarray(xb, dtype=np.float64)
    H = len(xa)
    E10, st, nl, dg = np.full((H, SLOTS, 9), 7.0), np.full((H, SLOTS), 7, np.int32), np.full(H, 7, np.int32), np.full((H, 2), 7.0)
    hc.hc_fp_candidates(H, P(xa), P(xb), P(E10), P(st), P(nl), P(dg))
    return E10, st, nl, dg


def run(hc, ua, ub, ia, ib, samples, threshold, H=None):
    cam, dist = _cam_blocks([np.zeros(6)] * 2, [ia, ib])
    M, H = len(ua), len(samples) if H is None else H
    S = SLOTS * max(H, 1)
    rt, best, inl, pts = np.full(12, 7.0), np.full(4, 7.0), np.full(M, 7, np.uint8), np.full((M, 3), 7.0)
    E, cost, cnt, st, mp, n = np.full((S, 9), 7.0), np.full(S, 7.0), np.full(S, 7, np.uint32), np.full(S, 7, np.int32), np.full(S, 7, np.int32), np.full(1, 7, np.int32)
    smp = np.ascontiguousarray(samples, dtype=np.int32)
    rc = hc.hc_two_view_ransac5(M, P(np.ascontiguousarray(ua)), P(np.ascontiguousarray(ub)), P(cam), P(dist), H, P(smp), threshold, 5, P(rt), P(best), P(inl), P(pts), P(E), P(cost), P(cnt), P(st), P(mp), P(n))
    return rc, dict(rt12=rt, best=best, inliers=inl.astype(bool), points=pts, E=E, cost=cost, count=cnt, status=st, map=mp, n=int(n[0]))


_cache = {}


def case(name, H):
    if (name, H) not in _cache:
        ua, ub, ia, ib, _, _ = fo.pair_of(name)
        smp = fo.draw_samples(len(ua), H, 0)
        prep = tvo.prepare(ua, ub, ia, ib)
        _cache[(name, H)] = (ua, ub, ia, ib, smp, prep, fo.hypotheses(prep, smp))
    return _cache[(name, H)]


@pytest.mark.parametrize("H", [64, 512])
@pytest.mark.parametrize("name", ["thin3", "three"])
def test_candidates_match_the_oracle(hc, name, H):
    ua, ub, ia, ib, smp, prep, hyp = case(name, H)
    E10, st, nl, dg = candidates(hc, prep["na"][smp], prep["nb"][smp])
    print(f"{name} H {H}: smallest sigma_5 / sigma_1 {dg[:, 0].min():.3g}, smallest pivot ratio {dg[:, 1].min():.3g}; live per sample {nl.mean():.2f}, at most {nl.max()}")
    fo.check_candidates(f"{name} H {H}", E10, st, dict(hyp=hyp))
    assert np.array_equal(nl, (st == 1).sum(1))
    # the floors sit well below what the scenes meet (the derivation in DESIGN.md section 8f-17 quotes these figures)
    assert dg[:, 0].min() > 100 * fo.RANK_MIN and dg[:, 1].min() > 100 * fo.PIVOT_MIN
    sr = np.array([c["sigma_ratio"] for c in hyp["per_sample"]])
    pv = np.array([c["pivot"] for c in hyp["per_sample"]])
    assert np.abs(dg[:, 0] / sr - 1).max() < 1e-6 and np.abs(dg[:, 1] / pv - 1).max() < 1e-3


def test_void_samples(hc):
    ua, ub, ia, ib, smp, prep, hyp = case("thin3", 64)
    xa, xb = prep["na"][smp[:4]].copy(), prep["nb"][smp[:4]].copy()
    xa[1, 3], xb[1, 3] = xa[1, 0], xb[1, 0]            # two identical correspondences: the 5 x 9 matrix has rank 4
    xa[2, 4, 1] = np.nan                               # a NaN coordinate
    E10, st, nl, dg = candidates(hc, xa, xb)
    assert nl[0] > 0 and nl[3] > 0 and nl[1] == 0 and nl[2] == 0
    assert (st[1] == -1).all() and (st[2] == -1).all() and np.isnan(E10[1]).all() and np.isnan(E10[2]).all()
    assert dg[1, 0] < fo.RANK_MIN
    assert fo.candidates(xa[1], xb[1])["void"] and fo.candidates(xa[2], xb[2])["void"]


@pytest.mark.parametrize("H", [64, 512])
@pytest.mark.parametrize("name", ["thin3", "three"])
def test_compaction_winner_and_pose(hc, name, H):
    ua, ub, ia, ib, smp, prep, hyp = case(name, H)
    rc, g = run(hc, ua, ub, ia, ib, smp, tvo.THRESHOLD)
    assert rc == 0
    live = fo.compaction(g["status"].reshape(H, SLOTS))
    # the map: the live slots in index order; the tables are in slot order, void slots cost +inf
    assert g["n"] == len(live) and np.array_equal(g["map"][:g["n"]], live) and (g["map"][g["n"]:] == 7).all()
    assert np.isinf(g["cost"][g["status"] != 1]).all() and (g["count"][g["status"] != 1] == 0).all() and np.isfinite(g["cost"][live]).all()
    fo.check_candidates(f"{name} H {H}", g["E"].reshape(H, SLOTS, 9), g["status"].reshape(H, SLOTS), dict(hyp=hyp))
    # the lowest (cost, index) of the packed order is the lowest (cost, 10 sample + slot)
    order = np.lexsort((live, g["cost"][live]))
    assert g["best"][0] == live[order[0]] and g["best"][1] == g["cost"][live[order[0]]]
    # the oracle scores the table that came back: costs, counts, the winner where its two lowest costs differ by more than 1e-6 relative, the pose
    o = tvo.two_view(ua, ub, ia, ib, None, tvo.THRESHOLD, essential_in=g["E"][live])
    packed = dict(g, cost=g["cost"][live], count=g["count"][live], status=g["status"][live], best=np.r_[float(np.searchsorted(live, g["best"][0])), g["best"][1:]])
    tvo.check_scores(f"{name} H {H}", packed, o)
    assert o["comparable"]
    tvo.check_pose(f"{name} H {H}", packed, o)
    # ... and it is the winner of the oracle's own generator
    o5 = fo.two_view5(ua, ub, ia, ib, smp, tvo.THRESHOLD)
    if o5["comparable"]:
        assert int(g["best"][0]) == SLOTS * o5["sample"] + o5["slot"] and np.array_equal(g["inliers"], o5["inliers"])
    if name == "thin3":
        assert g["best"][2] == len(ua)


def test_nothing_live(hc):
    ua, ub, ia, ib, smp, prep, hyp = case("thin3", 64)
    ua2, ub2 = ua.copy(), ub.copy()
    ua2[:5], ub2[:5] = ua[0], ub[0]                    # five identical correspondences
    rc, g = run(hc, ua2, ub2, ia, ib, np.arange(5, dtype=np.int32)[None], tvo.THRESHOLD)
    assert rc == 0 and g["n"] == 1 and g["map"][0] == 0 and (g["status"] == -1).all()
    assert g["best"][0] == 0 and np.isinf(g["best"][1]) and g["best"][2] == 0 and not g["inliers"].any() and np.isnan(g["points"]).all() and np.isnan(g["rt12"]).all()


def test_bad_arguments_write_nothing(hc):
    ua, ub, ia, ib, smp, prep, hyp = case("thin3", 64)
    twice, beyond = smp.copy(), smp.copy()
    twice[17, 4] = twice[17, 2]
    beyond[3, 0] = len(ua)
    for kw in (dict(n=7), dict(H=0), dict(H=1025), dict(threshold=0.0), dict(samples=twice), dict(samples=beyond)):
        n = kw.get("n", len(ua))
        s = kw.get("samples", smp)
        if kw.get("H", 0) > len(s):
            s = fo.draw_samples(len(ua), kw["H"], 0)
        rc, g = run(hc, np.ascontiguousarray(ua[:n]), np.ascontiguousarray(ub[:n]), ia, ib, s, kw.get("threshold", tvo.THRESHOLD), H=kw.get("H"))
        assert rc == 1 and all((g[k] == 7).all() for k in ("rt12", "best", "points", "E", "cost", "count", "status", "map")), kw


def test_stand_alone_program_under_sanitizers(tmp_path):
    if not SANITIZE:
        pytest.skip("opt-in: MCBA_HOSTCHECK_SANITIZE=1")
    exe = str(tmp_path / "fivepoint_hostcheck")
    subprocess.check_call(["g++", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DFP_HOSTCHECK_MAIN", "-o", exe, SRC])
    ua, ub, ia, ib, smp, prep, hyp = case("thin3", 64)
    cam, dist = _cam_blocks([np.zeros(6)] * 2, [ia, ib])
    path = str(tmp_path / "scene.bin")
    with open(path, "wb") as fh:
        fh.write(struct.pack("<qqdq", len(ua), len(smp), tvo.THRESHOLD, 5))
        for a in (ua, ub, cam, dist):
            fh.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
        fh.write(np.ascontiguousarray(smp, dtype=np.int32).tobytes())
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    o5 = fo.two_view5(ua, ub, ia, ib, smp, tvo.THRESHOLD)
    assert f"winner {SLOTS * o5['sample'] + o5['slot']} " in r.stdout and "runtime error" not in r.stderr
