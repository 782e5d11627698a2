"""csrc/mcba_twoview_math.h -- the per-lane text of the two-view RANSAC kernels -- compiled with g++ -O2 (tests/hostcheck/twoview_hostcheck.cpp) and held
to tests/twoview_oracle.py without a GPU, by the rules of that module's docstring (the GPU tier's, tests/test_gpu_twoview.py): E per
well-conditioned hypothesis within K_E EPS (1 / gap_A + 1 / gap_E); with the oracle's own E table handed in, counts exact on decided points and
costs within the derived bound; the winner where it is comparable; R and t to 1e-9; the two-view points within the DLT bound.

MCBA_HOSTCHECK_SANITIZE=1 (opt-in, CPU only): the same harness is also built as a stand-alone program with its own main and
-fsanitize=address,undefined, reads a scene file written here and must exit 0.  Nothing is preloaded; the shared object is never built with a
sanitizer."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import twoview_oracle as tvo
from multicam_calibration_amd.triangulation import _cam_blocks

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck", "twoview_hostcheck.cpp")
SANITIZE = os.environ.get("MCBA_HOSTCHECK_SANITIZE") == "1"
V = ctypes.c_void_p


def P(a):
    return V(a.ctypes.data) if a is not None else None


@pytest.fixture(scope="module")
def hc(tmp_path_factory):
    lib = str(tmp_path_factory.mktemp("twoview_hostcheck") / "libtwoview_hostcheck.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-o", lib, SRC])
    h = ctypes.CDLL(lib)
    h.hc_two_view_ransac.argtypes = [ctypes.c_size_t, V, V, V, V, ctypes.c_int, V, V, ctypes.c_double, ctypes.c_int, V, V, V, V, V, V, V, V]
    h.hc_tv_prepare.argtypes = [ctypes.c_size_t, V, V, V, V, ctypes.c_int, V]
    h.hc_samples_ok.argtypes = [ctypes.c_char_p, V, ctypes.c_size_t, ctypes.c_int, ctypes.c_size_t, V, ctypes.c_char_p, ctypes.c_size_t]
    return h


def run(hc, ua, ub, ia, ib, samples, threshold, essential_in=None, H=None):
    cam, dist = _cam_blocks([np.zeros(6)] * 2, [ia, ib])
    M, H = len(ua), len(samples) if H is None else H
    rt, best, inl, pts = np.full(12, 7.0), np.full(4, 7.0), np.full(M, 7, np.uint8), np.full((M, 3), 7.0)
    E, cost, cnt, st = np.full((H, 9), 7.0), np.full(H, 7.0), np.full(H, 7, np.uint32), np.full(H, 7, np.int32)
    ein = None if essential_in is None else np.ascontiguousarray(essential_in, dtype=np.float64)
    rc = hc.hc_two_view_ransac(M, P(ua), P(ub), P(cam), P(dist), H, P(samples), P(ein), threshold, 5, P(rt), P(best), P(inl), P(pts), P(E), P(cost), P(cnt), P(st))
    return rc, dict(rt12=rt, best=best, inliers=inl.astype(bool), points=pts, E=E, cost=cost, count=cnt, status=st)


_cache = {}


def case(name, H):
    if (name, H) not in _cache:
        ua, ub, ia, ib, _, _ = tvo.pair_of(name)
        smp = tvo.draw_samples(len(ua), H, 0)
        _cache[(name, H)] = (ua, ub, ia, ib, smp, tvo.two_view(ua, ub, ia, ib, smp, tvo.THRESHOLD))
    return _cache[(name, H)]


def test_prepare_matches_the_oracle(hc):
    ua, ub, ia, ib, smp, o = case("outlier", 64)
    cam, dist = _cam_blocks([np.zeros(6)] * 2, [ia, ib])
    out = np.full((8, len(ua)), 7.0)
    hc.hc_tv_prepare(len(ua), P(ua), P(ub), P(cam), P(dist), 5, P(out))
    pr = o["prep"]
    ref = np.stack([pr["pa"][:, 0], pr["pa"][:, 1], pr["pb"][:, 0], pr["pb"][:, 1], pr["na"][:, 0], pr["na"][:, 1], pr["nb"][:, 0], pr["nb"][:, 1]])
    err = np.abs(out - ref) / np.maximum(1.0, np.abs(ref))
    print(f"prepare: worst relative error {err.max():.3g}")
    assert err.max() <= 64 * tvo.EPS * 5     # five rounds of the fixed-point iteration, each a handful of operations


@pytest.mark.parametrize("H", [64, 512])
@pytest.mark.parametrize("name", tvo.SCENES)
def test_scenes_match_the_oracle(hc, name, H):
    ua, ub, ia, ib, smp, o = case(name, H)
    rc, g = run(hc, ua, ub, ia, ib, smp, tvo.THRESHOLD)
    assert rc == 0
    tvo.check_hypotheses(f"{name} H {H}", g["E"], g["status"], o)
    tvo.check_pose(f"{name} H {H}", g, o)
    # scoring alone, on the oracle's own E table
    rc, s = run(hc, ua, ub, ia, ib, smp, tvo.THRESHOLD, essential_in=o["hyp"]["E"])
    assert rc == 0 and np.array_equal(s["E"], o["hyp"]["E"], equal_nan=True)
    tvo.check_scores(f"{name} H {H}", s, o)


def test_void_hypotheses_lose(hc):
    ua, ub, ia, ib, smp, o = case("three", 64)
    E = o["hyp"]["E"].copy()
    E[:5] = np.nan
    E[7, 3] = np.inf
    rc, s = run(hc, ua, ub, ia, ib, smp, tvo.THRESHOLD, essential_in=E)
    ref = tvo.two_view(ua, ub, ia, ib, smp, tvo.THRESHOLD, essential_in=E)
    assert rc == 0 and np.array_equal(s["status"] < 0, np.r_[[True] * 5, False, False, True, [False] * 56])
    assert np.isinf(s["cost"][s["status"] < 0]).all() and (s["count"][s["status"] < 0] == 0).all()
    tvo.check_scores("void", s, ref)
    # all void: hypothesis 0 "wins" with nothing
    rc, s = run(hc, ua, ub, ia, ib, smp[:3], tvo.THRESHOLD, essential_in=np.full((3, 9), np.nan))
    assert rc == 0 and s["best"][0] == 0 and np.isinf(s["best"][1]) and s["best"][2] == 0 and not s["inliers"].any() and np.isnan(s["points"]).all() and np.isnan(s["rt12"]).all()


def test_bad_arguments_write_nothing(hc):
    ua, ub, ia, ib, smp, o = case("three", 64)
    for kw in (dict(n=7), dict(H=0), dict(threshold=0.0)):
        n = kw.get("n", len(ua))
        rc, g = run(hc, np.ascontiguousarray(ua[:n]), np.ascontiguousarray(ub[:n]), ia, ib, smp, kw.get("threshold", tvo.THRESHOLD), H=kw.get("H"))
        assert rc == 1 and (g["rt12"] == 7.0).all() and (g["best"] == 7.0).all() and (g["points"] == 7.0).all()


def samples_ok(hc, who, samples, limit, usable=None):
    """the verdict and the message of csrc/mcba_ransac_host.h's samples_ok on an (rows, size) table"""
    smp = np.ascontiguousarray(samples, dtype=np.int32)
    msg = ctypes.create_string_buffer(b"?" * 255, 256)
    ok = hc.hc_samples_ok(who.encode(), P(smp), smp.shape[0], smp.shape[1], limit, P(usable), msg, 256)
    return bool(ok), msg.value.decode()


def test_sample_check_verdicts_and_messages(hc):
    """The check both two-view entries make of their samples: a valid table passes with no message; an index equal to the limit, a negative one
    and a repeat within a row fail with the entry's name in front of today's texts.  A repeat across rows is no fault."""
    good = tvo.draw_samples(40, 7, 3)
    assert samples_ok(hc, "mcba_two_view_ransac", good, 40) == (True, "")
    assert samples_ok(hc, "mcba_two_view_ransac5", good[:, :5], int(good[:, :5].max()) + 1) == (True, "")
    assert samples_ok(hc, "mcba_two_view_ransac", np.stack([good[0], good[0]]), 40) == (True, "")
    for who in ("mcba_two_view_ransac", "mcba_two_view_ransac5"):
        bad = good.copy()
        bad[6, 7] = 40
        assert samples_ok(hc, who, bad, 40) == (False, who + ": a sample index is outside 0 .. n_points - 1")
        bad[6, 7] = -1
        assert samples_ok(hc, who, bad, 40) == (False, who + ": a sample index is outside 0 .. n_points - 1")
        bad[6, 7] = bad[6, 0]
        assert samples_ok(hc, who, bad, 40) == (False, who + ": an index is repeated within a sample")


def test_stand_alone_program_under_sanitizers(tmp_path):
    if not SANITIZE:
        pytest.skip("opt-in: MCBA_HOSTCHECK_SANITIZE=1")
    exe = str(tmp_path / "twoview_hostcheck")
    subprocess.check_call(["g++", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DTV_HOSTCHECK_MAIN", "-o", exe, SRC])
    ua, ub, ia, ib, smp, o = case("outlier", 64)
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
    assert f"winner {o['winner']} " in r.stdout and "runtime error" not in r.stderr
