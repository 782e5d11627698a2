"""The resection's public surface without a GPU: exports, the new symbols beside ABI 7, every ValueError before a device is
touched, seeded sampling that leaves numpy's global generator alone, and ops.McbaError -- not a host path -- where no GPU is visible."""
import ctypes
import inspect
import os

import numpy as np
import pytest

from conftest import ROOT
import multicam_calibration_amd as m
from multicam_calibration_amd import geometry, ops
from test_triangulate_cpu import scene


def small():
    uvs, ext, intr, X = scene(C=2, P=40, seed=2, noise=0.3)
    return X, uvs, intr


def test_exports():
    for name in ("resect_camera", "resect_cameras", "CameraResection", "draw_resection_samples"):
        assert getattr(m, name) is getattr(geometry, name) and name in m.__all__, name
    assert geometry.RESECTION_STATUS == {1: "ok", -1: "fewer than 6 usable points", -2: "too few inliers"}
    sig = inspect.signature(m.resect_camera)
    assert sig.parameters["threshold"].default is inspect.Parameter.empty and sig.parameters["n_hypotheses"].default == 256 and sig.parameters["refine"].default is True
    assert sig.parameters["loss"].default == "soft_l1" and sig.parameters["max_nfev"].default == 50 and sig.parameters["undistort_iterations"].default == 5
    assert "threshold" in inspect.signature(m.resect_cameras).parameters and "return_info" not in inspect.signature(m.resect_cameras).parameters


def test_symbols_and_launch_constants():
    lib = ops.load_library()
    assert lib.mcba_abi_version() == 7
    bound = {s[0] for s in ops.SYMBOLS}
    for name in ("mcba_resect_ransac", "mcba_resect_refine"):
        assert name in bound and hasattr(lib, name)
    src = open(os.path.join(ROOT, "include", "mcba.h")).read()
    for macro, value in (("MCBA_RESECT_MAX_HYPOTHESES", ops.RESECT_MAX_HYPOTHESES), ("MCBA_RESECT_CHUNK", ops.RESECT_CHUNK), ("MCBA_RESECT_POINTS_PER_BLOCK", ops.RESECT_POINTS_PER_BLOCK),
                         ("MCBA_RESECT_SAMPLE", ops.RESECT_SAMPLE), ("MCBA_RESECT_GN_ITERATIONS", ops.RESECT_GN_ITERATIONS), ("MCBA_RESECT_MAX_CAMERAS", ops.RESECT_MAX_CAMERAS),
                         ("MCBA_RESECT_SYSTEM", ops.RESECT_SYSTEM)):
        assert f"#define {macro} {value}" in src, macro
    assert (ops.RESECT_SAMPLE, ops.RESECT_GN_ITERATIONS, ops.RESECT_MAX_HYPOTHESES) == (6, 10, 4096)


@pytest.mark.parametrize("kw,match", [(dict(threshold=0.0), "threshold"), (dict(threshold=-1.0), "threshold"), (dict(n_hypotheses=0), "n_hypotheses"), (dict(n_hypotheses=4097), "n_hypotheses"),
                                      (dict(undistort_iterations=-1), "undistort_iterations"), (dict(loss="l2"), "loss"), (dict(f_scale=0.0), "f_scale"), (dict(max_nfev=1), "max_nfev")])
def test_value_errors_before_any_device(kw, match):
    X, uvs, intr = small()
    args = {**dict(threshold=2.5), **kw}
    with pytest.raises(ValueError, match=match):
        m.resect_camera(X, uvs[0], intr[0], device=10 ** 6, **args)
    with pytest.raises(ValueError, match=match):
        m.resect_cameras(X, uvs, intr, device=10 ** 6, **args)


def test_wrong_shapes():
    X, uvs, intr = small()
    for call in (lambda: m.resect_camera(X[:, :2], uvs[0], intr[0], threshold=2.5), lambda: m.resect_camera(X, uvs[0][:-1], intr[0], threshold=2.5),
                 lambda: m.resect_camera(X, uvs[0].ravel(), intr[0], threshold=2.5), lambda: m.resect_cameras(X, uvs, intr[:1], threshold=2.5),
                 lambda: m.resect_cameras(X, [uvs[0], uvs[1][:-1]], intr, threshold=2.5), lambda: m.resect_cameras(X[:0], [u[:0] for u in uvs], intr, threshold=2.5),
                 lambda: m.resect_cameras(X, [uvs[0]] * 65, [intr[0]] * 65, threshold=2.5)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(TypeError):
        m.resect_camera(X, uvs[0], intr[0])     # threshold has no default


def test_samples_are_seeded_and_leave_the_global_generator_alone():
    np.random.seed(5)
    before = np.random.get_state()[1].copy()
    a, b, c = m.draw_resection_samples(50, 33, [0, 2]), m.draw_resection_samples(50, 33, [0, 2]), m.draw_resection_samples(50, 33, [0, 3])
    assert np.array_equal(np.random.get_state()[1], before)
    assert a.shape == (33, 6) and a.dtype == np.int32 and np.array_equal(a, b) and not np.array_equal(a, c) and a.min() >= 0 and a.max() < 50
    assert all(len(set(r)) == 6 for r in a.tolist())
    ref = np.stack([g.choice(50, 6, replace=False) for g in [np.random.default_rng([0, 2])] for _ in range(33)])
    assert np.array_equal(a, ref)
    assert sorted(m.draw_resection_samples(6, 1, 0)[0].tolist()) == list(range(6))
    with pytest.raises(ValueError):
        m.draw_resection_samples(5, 4, 0)


def test_no_gpu_is_an_error_not_a_host_path():
    n = ctypes.c_int()
    rc = ops.load_library().mcba_device_count(ctypes.byref(n))
    if rc == 0 and n.value > 0:
        pytest.skip("a GPU is visible here")
    X, uvs, intr = small()
    with pytest.raises(ops.McbaError):
        m.resect_camera(X, uvs[0], intr[0], threshold=2.5)
    with pytest.raises(ops.McbaError):
        m.resect_cameras(X, uvs, intr, threshold=2.5)


def test_argument_errors_of_the_library_come_before_the_device():
    """MCBA_ERR_ARG with nothing written, GPU or not: the checks run before a device is looked for"""
    X, uvs, intr = small()
    from multicam_calibration_amd.triangulation import _cam_blocks
    cam, dist = _cam_blocks([np.zeros(6)], [intr[0]])
    X, uv = np.ascontiguousarray(X), np.ascontiguousarray(uvs[0])
    smp = np.arange(6, dtype=np.int32)[None].copy()
    for H, s, thr in ((0, smp, 2.5), (1, np.array([[0, 1, 2, 3, 4, 4]], np.int32), 2.5), (1, np.array([[0, 1, 2, 3, 4, 40]], np.int32), 2.5), (1, smp, 0.0)):
        rt, best, mask = np.full(12, 7.0), np.full(4, 7.0), np.full(40, 7, np.uint8)
        with pytest.raises(ops.McbaError) as e:
            ops.call("mcba_resect_ransac", 1, 40, X.ctypes.data, uv.ctypes.data, cam.ctypes.data, dist.ctypes.data, H, s.ctypes.data, None, thr, 5, 0, rt.ctypes.data, best.ctypes.data, mask.ctypes.data,
                     None, None, None, None, None)
        assert e.value.code == ops.ERR_ARG and (rt == 7).all() and (best == 7).all() and (mask == 7).all()
