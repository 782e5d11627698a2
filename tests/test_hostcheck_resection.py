"""csrc/mcba_resect_math.h -- the per-lane text of the resection kernels and the polish's loop rs_lm -- compiled with g++ -O2
(tests/hostcheck/resection_hostcheck.cpp) and held to tests/resection_oracle.py without a GPU, by the rules of that module's docstring (the GPU
tier's, tests/test_gpu_resection.py): the pose of every comparable hypothesis within K_P EPS cond; with the oracle's own pose table handed in,
counts exact on decided points and costs within the derived bound; the winner where it is comparable; the normal system within its bounds; rs_lm
against the restated loop and against the pinned goldens of tests/golden/resection.npz.

MCBA_HOSTCHECK_SANITIZE=1 (opt-in, CPU only): the same harness is also built as a stand-alone program with its own main and
-fsanitize=address,undefined, reads a scene file written here, runs the RANSAC and the polish, and must exit 0.  Nothing is preloaded; the shared
object is never built with a sanitizer."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import resection_oracle as ro
from multicam_calibration_amd import ops
from multicam_calibration_amd.triangulation import _cam_blocks

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck", "resection_hostcheck.cpp")
SANITIZE = os.environ.get("MCBA_HOSTCHECK_SANITIZE") == "1"
V = ctypes.c_void_p
TIGHT = dict(ftol=1e-15, xtol=1e-15, gtol=1e-10, max_nfev=200)


def P(a):
    return V(a.ctypes.data) if a is not None else None


@pytest.fixture(scope="module")
def hc(tmp_path_factory):
    lib = str(tmp_path_factory.mktemp("resection_hostcheck") / "libresection_hostcheck.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", lib, SRC])
    h = ctypes.CDLL(lib)
    h.hc_resect_ransac.argtypes = [ctypes.c_size_t, V, V, V, V, ctypes.c_int, V, V, ctypes.c_double, ctypes.c_int, V, V, V, V, V, V, V]
    h.hc_rs_prepare.argtypes = [ctypes.c_size_t, V, V, V, V, ctypes.c_int, V, V]
    h.hc_samples_ok.argtypes = [ctypes.c_char_p, V, ctypes.c_size_t, ctypes.c_int, ctypes.c_size_t, V, ctypes.c_char_p, ctypes.c_size_t]
    h.hc_resect_refine.argtypes = [ctypes.c_int, ctypes.c_size_t, V, V, V, V, V, V, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_int, V, V, V, V]
    return h


def run(hc, points, uv, intr, samples, threshold, poses_in=None, H=None):
    cam, dist = _cam_blocks([np.zeros(6)], [intr])
    points, uv = np.ascontiguousarray(points, dtype=np.float64), np.ascontiguousarray(uv, dtype=np.float64)
    n, H = len(points), (len(samples) if poses_in is None else len(poses_in)) if H is None else H
    rt, best, inl = np.full(12, 7.0), np.full(4, 7.0), np.full(n, 7, np.uint8)
    pose, cost, cnt, st = np.full((max(H, 1), 12), 7.0), np.full(max(H, 1), 7.0), np.full(max(H, 1), 7, np.uint32), np.full(max(H, 1), 7, np.int32)
    smp = None if samples is None else np.ascontiguousarray(samples, dtype=np.int32)
    pin = None if poses_in is None else np.ascontiguousarray(poses_in, dtype=np.float64)
    rc = hc.hc_resect_ransac(n, P(points), P(uv), P(cam), P(dist), H, P(smp), P(pin), threshold, 5, P(rt), P(best), P(inl), P(pose), P(cost), P(cnt), P(st))
    return rc, dict(rt12=rt, best=best, inliers=inl.astype(bool), pose=pose, cost=cost, count=cnt, status=st)


def refine(hc, points, uvs, masks, intrs, starts, loss="linear", f_scale=1.0, active=None, **kw):
    kw = {**dict(ftol=1e-8, xtol=1e-8, gtol=1e-8, max_nfev=50), **kw}
    cam, dist = _cam_blocks(list(starts), list(intrs))
    C, n = len(cam), len(points)
    points, uvs = np.ascontiguousarray(points, dtype=np.float64), np.ascontiguousarray(np.stack(uvs), dtype=np.float64)
    masks = np.ascontiguousarray(np.stack(masks), dtype=np.uint8)
    act = None if active is None else np.ascontiguousarray(active, dtype=np.int32)
    ext, res, sys_, ev = np.full((C, 6), 7.0), np.full((C, 8), 7.0), np.full((C, 29), 7.0), ctypes.c_int(0)
    rc = hc.hc_resect_refine(C, n, P(points), P(uvs), P(masks), P(cam), P(dist), P(act), ops.LOSSES[loss], f_scale, kw["ftol"], kw["xtol"], kw["gtol"], kw["max_nfev"], P(ext), P(res), P(sys_),
                             ctypes.byref(ev))
    return rc, dict(extrinsics=ext, result=res, system=sys_, evaluations=ev.value)


_cache = {}


def case(name, cam, H):
    if (name, cam, H) not in _cache:
        c = ro.camera_of(name, cam)
        smp = ro.samples_of(c["usable"], H, [0, cam])
        _cache[(name, cam, H)] = (c, smp, ro.ransac(c["points"], c["uv"], c["intr"], smp, ro.THRESHOLD))
    return _cache[(name, cam, H)]


def test_prepare_matches_the_oracle(hc):
    c, smp, o = case("outlier", 1, 64)
    cam, dist = _cam_blocks([np.zeros(6)], [c["intr"]])
    n = len(c["points"])
    out, use = np.full((4, n), 7.0), np.full(n, 7, np.uint8)
    hc.hc_rs_prepare(n, P(np.ascontiguousarray(c["points"])), P(np.ascontiguousarray(c["uv"])), P(cam), P(dist), 5, P(out), P(use))
    pr = o["prep"]
    ref = np.stack([pr["px"][:, 0], pr["px"][:, 1], pr["nx"][:, 0], pr["nx"][:, 1]])
    err = np.abs(out - ref) / np.maximum(1.0, np.abs(ref))
    print(f"prepare: worst relative error {err.max():.3g}; usable {int(use.sum())} of {n}")
    assert np.array_equal(use.astype(bool), pr["usable"]) and 0 < use.sum() < n
    assert err.max() <= 64 * ro.EPS * 5     # five rounds of the fixed-point iteration, each a handful of operations


@pytest.mark.parametrize("name,cam,H", [("six", 0, 64), ("six", 3, 64), ("six", 5, 512), ("three", 1, 64), ("three", 2, 64)])
def test_compared_scenes_match_the_oracle(hc, name, cam, H):
    c, smp, o = case(name, cam, H)
    assert ro.left_out_share(o["hyp"]) <= ro.LEFT_OUT_CAP
    rc, g = run(hc, c["points"], c["uv"], c["intr"], smp, ro.THRESHOLD)
    assert rc == 0
    ro.check_hypotheses(f"{name} camera {cam} H {H}", g["pose"], g["status"], o["hyp"])
    assert not o["score"]["undecided"].any()
    print(f"winner {int(g['best'][0])} (oracle {o['winner']}, comparable {o['comparable']}); inliers {int(g['best'][2])} of {int(g['best'][3])}")
    assert g["best"][3] == o["n_usable"]
    if o["comparable"]:
        assert g["best"][0] == o["winner"] and np.array_equal(g["inliers"], o["inliers"]) and g["best"][2] == o["n_inliers"]
        assert (np.abs(g["rt12"] - o["rt12"]) <= o["hyp"]["tol"][o["winner"]]).all()
    # scoring alone, on the oracle's own pose table
    rc, s = run(hc, c["points"], c["uv"], c["intr"], None, ro.THRESHOLD, poses_in=o["hyp"]["pose"])
    assert rc == 0 and np.array_equal(s["pose"], o["hyp"]["pose"], equal_nan=True)
    ro.check_scores(f"{name} camera {cam} H {H}", s["cost"], s["count"], o["hyp"], o["score"], subset=np.ones(H, bool))
    w, clear = ro.winner(o["score"]["cost"])
    assert not clear or (s["best"][0] == w and np.array_equal(s["inliers"], o["score"]["inlier"][w]))


@pytest.mark.parametrize("name,cam", [("outlier", 1), ("twelve", 4)])
def test_scoring_and_winner_with_poses_handed_in(hc, name, cam):
    c, smp, o = case(name, cam, 64)
    rc, s = run(hc, c["points"], c["uv"], c["intr"], None, ro.THRESHOLD, poses_in=o["hyp"]["pose"])
    assert rc == 0
    ro.check_scores(f"{name} camera {cam}", s["cost"], s["count"], o["hyp"], o["score"], subset=np.ones(64, bool))
    w, clear = ro.winner(o["score"]["cost"])
    print(f"winner {int(s['best'][0])} (oracle {w}, clear {clear}); inliers {int(s['best'][2])} of {int(s['best'][3])}")
    assert not clear or (s["best"][0] == w and np.array_equal(s["inliers"], o["score"]["inlier"][w]))


def test_void_hypotheses_lose_and_points_behind_the_camera_count_in_full(hc):
    c, smp, o = case("three", 1, 64)
    pose = o["hyp"]["pose"].copy()
    pose[:5] = np.nan
    pose[7, 3] = np.inf
    half = np.diag([1.0, -1.0, -1.0])     # the camera turned by pi about its x axis: every point that was in front is behind it
    pose[9] = np.r_[(half @ pose[9, :9].reshape(3, 3)).ravel(), half @ pose[9, 9:]]
    rc, s = run(hc, c["points"], c["uv"], c["intr"], None, ro.THRESHOLD, poses_in=pose)
    ref = ro.ransac(c["points"], c["uv"], c["intr"], None, ro.THRESHOLD, poses_in=pose)
    void = np.r_[[True] * 5, False, False, True, [False] * 56]
    assert rc == 0 and np.array_equal(s["status"] < 0, void) and np.isinf(s["cost"][void]).all() and (s["count"][void] == 0).all()
    assert s["count"][9] == 0 and s["cost"][9] == ro.THRESHOLD ** 2 * o["n_usable"]
    ro.check_scores("void", s["cost"], s["count"], ref["hyp"], ref["score"], subset=np.ones(64, bool))
    rc, s = run(hc, c["points"], c["uv"], c["intr"], None, ro.THRESHOLD, poses_in=np.full((3, 12), np.nan))
    assert rc == 0 and s["best"][0] == 0 and np.isinf(s["best"][1]) and s["best"][2] == 0 and not s["inliers"].any() and np.isnan(s["rt12"]).all()


def test_coplanar_samples_are_void(hc):
    """six coplanar points leave the DLT start undefined (eigen-gap at rounding level): void in the oracle and in the build, whatever their order"""
    from test_triangulate_cpu import scene
    import keypoint_scenes as ks
    uvs, ext, intr, X = scene(C=2, P=80, seed=0, noise=0.0)
    n = np.array([0.3, 0.2, 1.0]) / np.linalg.norm([0.3, 0.2, 1.0])
    Xp = X - np.outer((X - X.mean(0)) @ n, n)
    uv = ks.project5(Xp, ext[1], *intr[1]) + np.random.default_rng(0).normal(0, 0.3, (80, 2))
    smp = ro.samples_of(np.ones(80, bool), 64, 1)
    o = ro.ransac(Xp, uv, intr[1], smp, ro.THRESHOLD)
    rc, g = run(hc, Xp, uv, intr[1], smp, ro.THRESHOLD)
    print(f"coplanar: oracle's largest eigen-gap {o['hyp']['gap'].max():.3g} (GAP_MIN {ro.GAP_MIN}); smallest gap of a sample of \"six\" camera 0: {case('six', 0, 64)[2]['hyp']['gap'].min():.3g}")
    assert o["hyp"]["gap"].max() < 1e-12 and case("six", 0, 64)[2]["hyp"]["gap"].min() > 1e-8     # (the rule's margin on either side)
    assert rc == 0 and (o["hyp"]["status"] == -1).all() and (g["status"] == -1).all() and np.isinf(g["cost"]).all() and np.isnan(g["rt12"]).all() and not g["inliers"].any()
    assert g["best"][0] == 0 and g["best"][2] == 0 and g["best"][3] == 80
    # one point lifted 5 mm off the plane: samples that hold it are defined again
    Xq = Xp.copy()
    Xq[smp[0, 0]] += 5.0 * n
    oq = ro.ransac(Xq, uv, intr[1], smp, ro.THRESHOLD)
    rc, q = run(hc, Xq, uv, intr[1], smp, ro.THRESHOLD)
    holds = (smp == smp[0, 0]).any(1)
    ok = oq["hyp"]["comparable"]      # (five points on a plane and one 5 mm off it: defined, but few such samples settle)
    print(f"one point off the plane: {int(holds.sum())} samples hold it, eigen-gaps {oq['hyp']['gap'][holds].min():.3g} .. {oq['hyp']['gap'][holds].max():.3g}, comparable {int(ok.sum())}")
    assert rc == 0 and holds[0] and (q["status"][~holds] == -1).all() and (oq["hyp"]["status"][~holds] == -1).all() and (oq["hyp"]["gap"][holds] >= ro.GAP_MIN).all()
    assert np.array_equal(q["status"][ok], oq["hyp"]["status"][ok])


def test_bad_arguments_write_nothing(hc):
    c, smp, o = case("three", 1, 64)
    bad = smp.copy()
    bad[3, 2] = int(np.flatnonzero(~c["usable"])[0])
    for kw in (dict(H=0), dict(threshold=0.0), dict(samples=bad)):
        rc, g = run(hc, c["points"], c["uv"], c["intr"], kw.get("samples", smp), kw.get("threshold", ro.THRESHOLD), H=kw.get("H"))
        assert rc == 1 and (g["rt12"] == 7.0).all() and (g["best"] == 7.0).all() and (g["cost"] == 7.0).all()


def samples_ok(hc, who, samples, limit, usable=None):
    """the verdict and the message of csrc/mcba_ransac_host.h's samples_ok on an (rows, size) table"""
    smp = np.ascontiguousarray(samples, dtype=np.int32)
    msg = ctypes.create_string_buffer(b"?" * 255, 256)
    ok = hc.hc_samples_ok(who.encode(), P(smp), smp.shape[0], smp.shape[1], limit, P(usable), msg, 256)
    return bool(ok), msg.value.decode()


def test_sample_check_verdicts_and_messages(hc):
    """The check both resection entries make of a camera's samples: a valid table passes with no message; an index equal to the limit, a negative
    one, a point that is not usable for the camera and a repeat within a row fail with the entry's name in front of today's texts.  A point out of
    range is reported as such before its flag is looked up, an unusable point before a repeat."""
    rng = np.random.default_rng(5)
    good = np.stack([rng.choice(30, 6, replace=False) for _ in range(9)]).astype(np.int32)
    usable = np.ones(30, np.uint8)
    assert samples_ok(hc, "mcba_resect_ransac", good, 30, usable) == (True, "")
    assert samples_ok(hc, "mcba_resect_ransac_p3p", good[:, :3], 30) == (True, "")
    for who in ("mcba_resect_ransac", "mcba_resect_ransac_p3p"):
        bad = good.copy()
        bad[8, 5] = 30
        assert samples_ok(hc, who, bad, 30, usable) == (False, who + ": a sample index is outside 0 .. n_points - 1")
        bad[8, 5] = -1
        assert samples_ok(hc, who, bad, 30, usable) == (False, who + ": a sample index is outside 0 .. n_points - 1")
        bad[8, 5] = bad[8, 1]
        assert samples_ok(hc, who, bad, 30, usable) == (False, who + ": an index is repeated within a sample")
        off = usable.copy()
        off[bad[8, 1]] = 0
        assert samples_ok(hc, who, bad, 30, off) == (False, who + ": a sampled point is not usable for its camera")


@pytest.mark.parametrize("loss", ["linear", "soft_l1", "huber", "cauchy", "arctan"])
def test_normal_system_matches_the_oracle(hc, loss):
    c = ro.camera_of("outlier", 1)
    start = ro.perturbed_start(c["ext"], 5)
    for f_scale in (1.0, 2.5):
        rc, g = refine(hc, c["points"], [c["uv"]], [c["usable"]], [c["intr"]], [start], loss=loss, f_scale=f_scale, max_nfev=1)
        assert rc == 0 and g["result"][0, 5] == 0 and g["result"][0, 3] == 1 and np.array_equal(g["extrinsics"][0], start)
        ro.check_system(f"{loss} f_scale {f_scale}", g["system"][0], ro.normal_system(start, c["points"], c["uv"], c["usable"], c["intr"], loss, f_scale))


def test_the_loop_follows_the_restated_one(hc):
    c = ro.camera_of("six", 0)
    start = ro.perturbed_start(c["ext"], 11)
    o = ro.lm(start, c["points"], c["uv"], c["usable"], c["intr"], "soft_l1")
    rc, g = refine(hc, c["points"], [c["uv"]], [c["usable"]], [c["intr"]], [start], loss="soft_l1")
    r = g["result"][0]
    print(f"loop: cost {r[1]:.15g} (oracle {o['cost']:.15g}), nfev {int(r[3])} ({o['nfev']}), status {int(r[5])} ({o['status']}); pose difference {np.abs(g['extrinsics'][0] - o['pose']).max():.3g}")
    assert rc == 0 and r[3] == o["nfev"] and r[4] == o["njev"] and r[5] == o["status"] and r[1] <= r[0]
    assert abs(r[1] - o["cost"]) <= 1e-9 * o["cost"] and (np.abs(g["extrinsics"][0] - o["pose"]) <= 1e-7 * np.maximum(1.0, np.abs(o["pose"]))).all()
    assert g["evaluations"] == r[3] + r[4] - 1


@pytest.mark.parametrize("name", sorted(ro.GOLDEN_CASES))
def test_the_loop_reaches_the_goldens(hc, name):
    i, o = ro.golden_case(name)
    rc, g = refine(hc, i["points"], [i["uv"]], [i["mask"]], [i["intr"]], [i["start"]], loss=i["loss"], **TIGHT)
    r = g["result"][0]
    print(f"{name}: two-start spread {o['spread']:.3g} pinned {o['pinned']}; status {int(r[5])} nfev {int(r[3])}")
    assert rc == 0 and r[1] <= r[0]
    if o["pinned"]:
        ro.check_golden(name, g["extrinsics"][0], r[1], o)


def test_cameras_stop_on_their_own_and_inactive_ones_stay(hc):
    a, b = ro.camera_of("six", 0), ro.camera_of("six", 5)
    sa, sb = ro.perturbed_start(a["ext"], 1), ro.perturbed_start(b["ext"], 2)
    pts = a["points"]      # (each camera against its own triangulation: the two problems share nothing but the call)
    rc, one_a = refine(hc, pts, [a["uv"]], [a["usable"]], [a["intr"]], [sa])
    rc, both = refine(hc, pts, [a["uv"], a["uv"], a["uv"]], [a["usable"]] * 3, [a["intr"]] * 3, [sa, sb, sa], active=[1, 0, 1], max_nfev=50)
    assert rc == 0 and np.array_equal(both["extrinsics"][0], one_a["extrinsics"][0]) and np.array_equal(both["extrinsics"][2], one_a["extrinsics"][0])
    assert np.array_equal(both["extrinsics"][1], sb) and np.isnan(both["result"][1]).all() and np.array_equal(both["result"][0], one_a["result"][0])
    # one camera converged at the start (its own optimum), the other not: the first is evaluated once and never again
    rc, two = refine(hc, pts, [a["uv"], a["uv"]], [a["usable"]] * 2, [a["intr"]] * 2, [one_a["extrinsics"][0], sa], gtol=1e-3)
    assert rc == 0 and two["result"][0, 3] <= 2 and np.abs(two["extrinsics"][0] - one_a["extrinsics"][0]).max() <= 1e-6


def test_stand_alone_program_under_sanitizers(tmp_path):
    if not SANITIZE:
        pytest.skip("opt-in: MCBA_HOSTCHECK_SANITIZE=1")
    exe = str(tmp_path / "resection_hostcheck")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DRS_HOSTCHECK_MAIN", "-o", exe, SRC])
    c, smp, o = case("outlier", 1, 64)
    cam, dist = _cam_blocks([np.zeros(6)], [c["intr"]])
    path = str(tmp_path / "scene.bin")
    with open(path, "wb") as fh:
        fh.write(struct.pack("<qqdq", len(c["points"]), len(smp), ro.THRESHOLD, 5))
        for a in (c["points"], c["uv"], cam, dist):
            fh.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
        fh.write(np.ascontiguousarray(smp, dtype=np.int32).tobytes())
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "winner " in r.stdout and "polish cost" in r.stdout and "runtime error" not in r.stderr
