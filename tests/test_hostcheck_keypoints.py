"""csrc/mcba_keypoint_math.h -- the per-lane text of k_project, k_keypoint_errors and k_tri_refine -- compiled with g++
(tests/hostcheck/keypoints_hostcheck.cpp) and held to the gates of the GPU tier (tests/test_gpu_keypoints.py) without a GPU: the reference's
project_points and the scipy refinement optimum recorded in tests/golden/geometry.npz, numpy restatements, and properties that need no oracle."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import keypoint_scenes as ks
from multicam_calibration_amd import ops
from multicam_calibration_amd.triangulation import _cam_blocks

HERE = os.path.dirname(os.path.abspath(__file__))
GATE_MM = 5e-6   # refinement against the stored optimum (the oracle's own two-start spread is held to 5e-7 by the golden script)
SANITIZE = os.environ.get("MCBA_HOSTCHECK_SANITIZE") == "1"


def P(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


@pytest.fixture(scope="module")
def hc(tmp_path_factory):
    src = os.path.join(HERE, "hostcheck", "keypoints_hostcheck.cpp")
    lib = str(tmp_path_factory.mktemp("keypoints_hostcheck") / "libkeypoints_hostcheck.so")
    flags = ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if SANITIZE else ["-O2"]
    subprocess.check_call(["g++"] + flags + ["-shared", "-fPIC", "-o", lib, src])
    h = ctypes.CDLL(lib)
    h.hc_kp_project.argtypes = [ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    h.hc_kp_rigid.argtypes = [ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    h.hc_kp_errors.argtypes = [ctypes.c_int, ctypes.c_size_t] + [ctypes.c_void_p] * 5
    h.hc_kp_refine.argtypes = [ctypes.c_int, ctypes.c_size_t] + [ctypes.c_void_p] * 4 + [ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    return h


@pytest.fixture(scope="module")
def gold(golden):
    return golden("geometry.npz")


def project(hc, pts, ext, K, d, mode):
    cam, dist = _cam_blocks([ext], [(K, d)])
    flat = np.ascontiguousarray(np.asarray(pts, dtype=np.float64).reshape(-1, 3))
    out = np.empty((1, len(flat), 2))
    hc.hc_kp_project(1, len(flat), P(flat), P(cam), P(dist) if mode == 1 else None, mode, P(out))
    return out[0].reshape(np.shape(pts)[:-1] + (2,))


def refine(hc, start, uvs, ext, intr, loss, f_scale=1.0, max_iterations=100):
    cam, dist = _cam_blocks(ext, intr)
    U = np.ascontiguousarray(np.stack(uvs))
    start = np.ascontiguousarray(start)
    out, info = np.empty_like(start), np.empty((len(start), 4))
    assert hc.hc_kp_refine(len(cam), len(start), P(U), P(cam), P(dist), P(start), ops.LOSSES[loss], f_scale, max_iterations, P(out), P(info)) == 0
    return out, info


def test_projection_matches_the_reference(hc, gold):
    K, ext = gold["pp_K"], gold["pp_ext"]
    cases = [(gold["pp_pts"], ext, np.zeros(2), "pp_plain"), (gold["pp_pts"], ext, gold["pp_d2"], "pp_dist2"), (gold["pp_pts"], ext, gold["pp_d5"][:2], "pp_dist5"),
             (gold["pp_grid"], ext, gold["pp_d2"], "pp_grid_dist2"), (gold["pp_pts"] + np.array([0, 0, 800.0]), np.zeros(6), gold["pp_d2"], "pp_zero_ext")]
    for pts, e, d, key in cases:
        for mode in (0, 1):   # the k1, k2 path (project_only) and the five-coefficient path with p1 = p2 = k3 = 0
            got = project(hc, pts, e, K, d, mode)
            assert np.array_equal(np.isnan(got), np.isnan(gold[key])), key
            np.testing.assert_allclose(got, gold[key], rtol=1e-12, atol=1e-10, err_msg=key)
    # non-zero p1, p2, k3: against the numpy forward model
    got = project(hc, gold["pp_pts"], ext, K, gold["pp_d5"], 1)
    np.testing.assert_allclose(got, ks.project5(gold["pp_pts"], ext, K, gold["pp_d5"]), rtol=1e-12, atol=1e-10)


def test_rigid_transform_matches_the_reference(hc, gold):
    from multicam_calibration_amd.calibration import get_transformation_matrix

    for T, pts, key in ((get_transformation_matrix(gold["rt_t6"]), gold["pp_pts"], "rt_vec"), (gold["rt_T4"], gold["pp_grid"], "rt_mat")):
        flat = np.ascontiguousarray(pts.reshape(-1, 3))
        out = np.empty_like(flat)
        hc.hc_kp_rigid(len(flat), P(flat), P(np.ascontiguousarray(np.r_[T[:3, :3].ravel(), T[:3, 3]])), P(out))
        np.testing.assert_allclose(out.reshape(pts.shape), gold[key], rtol=1e-12, atol=1e-10)


@pytest.mark.parametrize("name", list(ks.SCENES))
def test_errors_match_numpy(hc, gold, name):
    uvs, ext, intr, _ = ks.make(name)
    start = np.ascontiguousarray(gold[f"{name}_start"])
    cam, dist = _cam_blocks(ext, intr)
    U = np.ascontiguousarray(np.stack(uvs))
    err = np.empty(U.shape[:2])
    hc.hc_kp_errors(len(cam), len(start), P(start), P(U), P(cam), P(dist), P(err))
    want = ks.errors(start, uvs, ext, intr)
    assert np.array_equal(np.isnan(err), np.isnan(want))
    np.testing.assert_allclose(err, want, rtol=0, atol=1e-10)


@pytest.mark.parametrize("name,loss", [(n, l) for n in ks.SCENES for l in ks.LOSSES[n]])
def test_refinement_reaches_the_scipy_optimum(hc, gold, name, loss):
    uvs, ext, intr, X = ks.make(name)
    start, want = gold[f"{name}_start"], gold[f"{name}_{loss}"]
    got, info = refine(hc, start, uvs, ext, intr, loss)
    views = (~np.isnan(np.stack(uvs)).any(-1)).sum(0)
    assert np.array_equal(np.isnan(got).any(1), np.isnan(start).any(1)) and np.array_equal(np.isnan(got).any(1), views < 2)
    assert not np.isnan(want[views >= 2]).any()                      # every point with two views has an optimum on record: none is left out
    diff = np.abs(got - want)[views >= 2].max(axis=1)
    print(f"{name} {loss}: max |dX| {diff.max():.3e} mm, iterations mean {info[views >= 2, 2].mean():.1f} max {info[:, 2].max():.0f}")
    assert diff.max() <= GATE_MM
    ok = views >= 2
    assert np.all(info[ok, 0] <= info[ok, 1]) and np.all(info[ok, 3] == 1) and np.all(info[~ok, 3] == -1)
    np.testing.assert_allclose(info[ok, 0], ks.robust_cost(got, uvs, ext, intr, loss)[ok], rtol=1e-9, atol=1e-12)
    again, _ = refine(hc, got, uvs, ext, intr, loss)
    assert np.abs(again - got)[ok].max() < GATE_MM


def test_soft_l1_ends_nearer_the_truth_than_the_start_on_the_outlier_scene(hc, gold):
    uvs, ext, intr, X = ks.make("outlier")
    start = gold["outlier_start"]
    got, _ = refine(hc, start, uvs, ext, intr, "soft_l1")
    ok = ~np.isnan(start).any(1)

    def rms(A):
        return np.sqrt(np.mean(np.sum((A[ok] - X[ok]) ** 2, axis=1)))

    print(f"rms to truth: start {rms(start):.4f} soft_l1 {rms(got):.4f} mm")
    assert rms(got) < rms(start)


def test_noise_free_points_are_recovered(hc):
    from oracle import triangulate_oracle as tri
    from test_triangulate_cpu import scene

    uvs, ext, intr, X = scene(C=5, P=777, seed=21)
    start = tri.triangulate(uvs, ext, intr)                           # five undistortion rounds: good to 1e-6 only
    got, _ = refine(hc, start, uvs, ext, intr, "linear")
    assert np.abs(got - X).max() < 1e-8
    # the same cloud seen through five-coefficient cameras (non-zero p1, p2, k3), detections made by the numpy forward model
    intr5 = [(K, np.r_[d[:2], 1.5e-3 * (-1) ** c, -8e-4, 0.015]) for c, (K, d) in enumerate(intr)]
    uvs5 = [ks.project5(X, ext[c], *intr5[c]) for c in range(len(ext))]
    start5 = tri.triangulate(uvs5, ext, intr5)
    for loss in ("linear", "soft_l1"):
        got, _ = refine(hc, start5, uvs5, ext, intr5, loss)
        assert np.abs(got - X).max() < 1e-8


def test_iteration_limit_and_degenerate_inputs(hc, gold):
    uvs, ext, intr, _ = ks.make("three")
    start = gold["three_start"]
    got, info = refine(hc, start, uvs, ext, intr, "cauchy", max_iterations=0)
    ok = ~np.isnan(start).any(1)
    assert np.array_equal(got[ok], start[ok]) and np.all(info[ok, 2] == 0) and np.all(info[ok, 0] == info[ok, 1])
    nan_start = start.copy()
    nan_start[ok.nonzero()[0][0], 1] = np.nan
    got, info = refine(hc, nan_start, uvs, ext, intr, "linear")
    assert np.isnan(got[ok.nonzero()[0][0]]).all() and info[ok.nonzero()[0][0], 3] == -1


def test_keypoints_hostcheck_under_sanitizers():
    """The same text with -fsanitize=address,undefined, every test of this file in a child process (the ASan runtime has to come first among the
    process' libraries)."""
    if SANITIZE:
        pytest.skip("this IS the sanitizer run")
    asan = subprocess.check_output(["gcc", "-print-file-name=libasan.so"], text=True).strip()
    if not os.path.isabs(asan) or not os.path.exists(asan):
        pytest.skip("libasan.so not found next to gcc")
    preload = " ".join(x for x in (asan, os.environ.get("LD_PRELOAD", "")) if x)
    env = dict(os.environ, MCBA_HOSTCHECK_SANITIZE="1", LD_PRELOAD=preload, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", os.path.abspath(__file__)], env=env, cwd=os.path.join(HERE, ".."), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "passed" in r.stdout and "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
