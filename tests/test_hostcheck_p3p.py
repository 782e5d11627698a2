"""csrc/mcba_resect_p3p_math.h -- the per-lane text of k_rs3_hypotheses -- compiled with g++ -O2 (tests/hostcheck/p3p_hostcheck.cpp, linked beside
tests/hostcheck/resection_hostcheck.cpp for its scorer) and held to tests/p3p_oracle.py without a GPU, by the rules of that module's docstring
(the GPU tier's, tests/test_gpu_p3p.py): slot by slot the status of every comparable sample and the pose of every live candidate within K_P EPS
cond; with the oracle's own table handed to the existing scorer, counts exact on decided points and costs within the derived bound; the winner
where it is comparable.

MCBA_HOSTCHECK_SANITIZE=1 (opt-in, CPU only): the same harness is also built as a stand-alone program with its own main and
-fsanitize=address,undefined, reads a scene file written here, runs the generator and the scorer, and must exit 0.  Nothing is preloaded; the
shared object is never built with a sanitizer."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import p3p_oracle as po
import resection_oracle as ro
from multicam_calibration_amd.triangulation import _cam_blocks

HERE = os.path.dirname(os.path.abspath(__file__))
SRCS = [os.path.join(HERE, "hostcheck", "p3p_hostcheck.cpp"), os.path.join(HERE, "hostcheck", "resection_hostcheck.cpp")]
SANITIZE = os.environ.get("MCBA_HOSTCHECK_SANITIZE") == "1"
V = ctypes.c_void_p
CASES = [("six", 0), ("six", 3), ("three", 0), ("three", 1), ("flat3", 1), ("thin3", 0)]


def P(a):
    return V(a.ctypes.data) if a is not None else None


@pytest.fixture(scope="module")
def hc(tmp_path_factory):
    lib = str(tmp_path_factory.mktemp("p3p_hostcheck") / "libp3p_hostcheck.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", lib] + SRCS)
    h = ctypes.CDLL(lib)
    h.hc_p3p_candidates.argtypes = [ctypes.c_size_t, V, V, V, V, ctypes.c_int, V, ctypes.c_int, V, V, V]
    h.hc_resect_ransac.argtypes = [ctypes.c_size_t, V, V, V, V, ctypes.c_int, V, V, ctypes.c_double, ctypes.c_int, V, V, V, V, V, V, V]
    h.hc_p3p_roots.argtypes = [V, V]
    return h


def candidates(hc, c, smp, H=None):
    cam, dist = _cam_blocks([np.zeros(6)], [c["intr"]])
    pts, uv = np.ascontiguousarray(c["points"], dtype=np.float64), np.ascontiguousarray(c["uv"], dtype=np.float64)
    H = len(smp) if H is None else H
    pose, st, step = np.full((4 * max(H, 1), 12), 7.0), np.full(4 * max(H, 1), 7, np.int32), np.full((4 * max(H, 1), 6), 7.0)
    rc = hc.hc_p3p_candidates(len(pts), P(pts), P(uv), P(cam), P(dist), H, P(np.ascontiguousarray(smp, dtype=np.int32)), 5, P(pose), P(st), P(step))
    return rc, pose, st, step


def scored(hc, c, table, threshold=po.THRESHOLD):
    cam, dist = _cam_blocks([np.zeros(6)], [c["intr"]])
    pts, uv = np.ascontiguousarray(c["points"], dtype=np.float64), np.ascontiguousarray(c["uv"], dtype=np.float64)
    n, T = len(pts), len(table)
    rt, best, inl = np.full(12, 7.0), np.full(4, 7.0), np.full(n, 7, np.uint8)
    pose, cost, cnt, st = np.full((T, 12), 7.0), np.full(T, 7.0), np.full(T, 7, np.uint32), np.full(T, 7, np.int32)
    rc = hc.hc_resect_ransac(n, P(pts), P(uv), P(cam), P(dist), T, None, P(np.ascontiguousarray(table)), threshold, 5, P(rt), P(best), P(inl), P(pose), P(cost), P(cnt), P(st))
    return rc, dict(rt12=rt, best=best, inliers=inl.astype(bool), pose=pose, cost=cost, count=cnt, status=st)


_cache = {}


def case(name, cam, H=64):
    if (name, cam, H) not in _cache:
        c = po.camera_of(name, cam)
        smp = po.samples_of(c["usable"], H, [0, cam])
        _cache[(name, cam, H)] = (c, smp, po.ransac(c["points"], c["uv"], c["intr"], smp, po.THRESHOLD))
    return _cache[(name, cam, H)]


def test_root_finder_on_known_quartics(hc):
    """products of known factors: every real root found, ascending, none invented; a vanishing leading coefficient has none"""
    rng = np.random.default_rng(4)
    for real, pair in (((-2.0, 0.5, 1.0, 3.0), None), ((0.25, 4.0), (1.0, 0.5)), ((), (0.3, 2.0)), ((-1e-3, 1e3), (-2.0, 1.0)), ((0.9, 1.1, 1.3, 20.0), None)):
        p = np.poly1d([1.0])
        for r in real:
            p = p * np.poly1d([1.0, -r])
        if pair is not None:
            for _ in range((4 - len(real)) // 2):
                p = p * np.poly1d([1.0, -2 * pair[0], pair[0] ** 2 + pair[1] ** 2])
        a = np.ascontiguousarray(p.coeffs[::-1] * rng.uniform(0.5, 2.0) * rng.choice([-1.0, 1.0]))
        out = np.full(4, 7.0)
        n = hc.hc_p3p_roots(P(a), P(out))
        print(real, n, out)
        assert n == len(real) and np.allclose(out[:n], real, rtol=1e-10, atol=0) and (out[n:] == 0).all()
    out = np.full(4, 7.0)
    assert hc.hc_p3p_roots(P(np.array([1.0, -3.0, 2.0, 0.0, 0.0])), P(out)) == 0 and hc.hc_p3p_roots(P(np.array([1.0, np.nan, 2.0, 0.0, 1.0])), P(out)) == 0


@pytest.mark.parametrize("name,cam", CASES)
def test_candidates_scores_and_winner_match_the_oracle(hc, name, cam):
    c, smp, o = case(name, cam)
    hyp = o["hyp"]
    assert po.left_out_share(hyp) <= po.LEFT_OUT_CAP
    rc, pose, st, step = candidates(hc, c, smp)
    assert rc == 0
    po.check_candidates(f"{name} camera {cam}", pose, st, hyp)
    live = hyp["comparable"] & (hyp["status"] > 0)
    last = np.maximum(np.linalg.norm(step[:, :3], axis=1), np.linalg.norm(step[:, 3:], axis=1) / np.maximum(1.0, np.linalg.norm(np.nan_to_num(pose[:, 9:]), axis=1)))
    assert (last[live] <= po.STEP_MAX).all()
    # scoring alone: the oracle's table through the existing scorer
    rc, s = scored(hc, c, hyp["pose"])
    assert rc == 0 and np.array_equal(s["pose"], hyp["pose"], equal_nan=True) and np.array_equal(s["status"], hyp["status"])
    ro.check_scores(f"{name} camera {cam}", s["cost"], s["count"], hyp, o["score"], subset=np.ones(len(hyp["pose"]), bool))
    w, clear = ro.winner(o["score"]["cost"])
    assert not clear or (s["best"][0] == w and np.array_equal(s["inliers"], o["score"]["inlier"][w]))
    # the whole: the build's own table through the scorer
    rc, g = scored(hc, c, pose)
    print(f"winner slot {int(g['best'][0])} (oracle {o['winner']}, comparable {o['comparable']}); inliers {int(g['best'][2])} of {int(g['best'][3])}")
    assert rc == 0 and g["best"][3] == o["n_usable"]
    if o["comparable"]:
        assert g["best"][0] == o["winner"] and g["best"][2] == o["n_inliers"] and (np.abs(g["rt12"] - o["rt12"]) <= hyp["tol"][o["winner"]]).all()
        und = o["score"]["undecided"][o["winner"]]
        assert np.array_equal(g["inliers"][~und], o["inliers"][~und])


def test_degenerate_samples_are_void_in_the_build(hc):
    c = dict(po.camera_of("six", 0))
    pts, i = np.array(c["points"]), np.flatnonzero(c["usable"])[:6]
    pts[i[2]] = pts[i[0]] + 2.5 * (pts[i[1]] - pts[i[0]])
    c["points"] = pts
    smp = i[np.array([[0, 1, 2], [2, 0, 1], [3, 4, 5]])].astype(np.int32)
    rc, pose, st, _ = candidates(hc, c, smp)
    assert rc == 0 and (st[:8] == -1).all() and np.isnan(pose[:8]).all() and (st[8:] == 1).any()
    o = po.sample(pts[smp[0]], ro.prepare(pts, c["uv"], c["intr"])["nx"][smp[0]])
    assert (o["status"] == -1).all()


def test_bad_arguments_write_nothing(hc):
    c, smp, o = case("three", 1)
    for bad, H in ((smp, 0), (smp, 1025), (np.r_[[[0, 1, 1]], smp[1:]], None), (np.r_[[[0, 1, len(c["points"])]], smp[1:]], None), (np.r_[[[0, 1, int(np.flatnonzero(~c["usable"])[0]) if (~c["usable"]).any() else -1]], smp[1:]], None)):
        rc, pose, st, _ = candidates(hc, c, bad, H=H)
        assert rc == 1 and (pose == 7.0).all() and (st == 7).all()


def test_stand_alone_program_under_sanitizers(tmp_path):
    if not SANITIZE:
        pytest.skip("opt-in: MCBA_HOSTCHECK_SANITIZE=1")
    exe = str(tmp_path / "p3p_hostcheck")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DP3P_HOSTCHECK_MAIN", "-o", exe] + SRCS)
    c, smp, o = case("flat3", 1)
    cam, dist = _cam_blocks([np.zeros(6)], [c["intr"]])
    path = str(tmp_path / "scene.bin")
    with open(path, "wb") as fh:
        fh.write(struct.pack("<qqdq", len(c["points"]), len(smp), po.THRESHOLD, 5))
        for a in (c["points"], c["uv"], cam, dist):
            fh.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
        fh.write(np.ascontiguousarray(smp, dtype=np.int32).tobytes())
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"inliers {o['n_inliers']} " in r.stdout and "runtime error" not in r.stderr
