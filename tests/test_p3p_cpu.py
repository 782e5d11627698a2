"""The P3P generator's public surface without a GPU: the `solver` keyword and its default, RESECTION_SOLVERS, 3-point
sampling, the new symbol beside ABI 7, the header's macros, every new ValueError before a device is touched, MCBA_ERR_ARG with nothing
written, and ops.McbaError -- not a host path -- where no GPU is visible."""
import ctypes
import inspect
import os

import numpy as np
import pytest

from conftest import ROOT
import multicam_calibration_amd as m
from multicam_calibration_amd import geometry, ops
from multicam_calibration_amd.triangulation import _cam_blocks
from test_triangulate_cpu import scene


def small():
    uvs, ext, intr, X = scene(C=2, P=40, seed=2, noise=0.3)
    return X, uvs, intr


def test_exports_and_the_default_solver():
    assert geometry.RESECTION_SOLVERS == ("dlt6", "p3p")
    assert geometry.RESECTION_STATUS == {1: "ok", -1: "fewer than 6 usable points", -2: "too few inliers"}
    for f in (m.resect_camera, m.resect_cameras):
        sig = inspect.signature(f)
        assert sig.parameters["solver"].default == "dlt6" and sig.parameters["solver"].kind is inspect.Parameter.KEYWORD_ONLY
        assert sig.parameters["n_hypotheses"].default == 256 and "p3p" in f.__doc__ and "fronto-parallel" in f.__doc__
    assert inspect.signature(m.draw_resection_samples).parameters["size"].default == 6
    assert "8f-18" in m.__doc__ and "p3p" in m.__doc__


def test_symbol_abi_and_header_macros():
    lib = ops.load_library()
    assert lib.mcba_abi_version() == 7
    assert "mcba_resect_ransac_p3p" in {s[0] for s in ops.SYMBOLS} and hasattr(lib, "mcba_resect_ransac_p3p")
    src = open(os.path.join(ROOT, "include", "mcba.h")).read()
    for macro, value in (("MCBA_RESECT_P3P_SAMPLE", ops.RESECT_P3P_SAMPLE), ("MCBA_RESECT_P3P_SLOTS", ops.RESECT_P3P_SLOTS), ("MCBA_RESECT_P3P_MAX_SAMPLES", ops.RESECT_P3P_MAX_SAMPLES),
                         ("MCBA_RESECT_P3P_POLISH", ops.RESECT_P3P_POLISH)):
        assert f"#define {macro} {value}\n" in src, macro
    assert (ops.RESECT_P3P_SAMPLE, ops.RESECT_P3P_SLOTS, ops.RESECT_P3P_MAX_SAMPLES, ops.RESECT_P3P_POLISH) == (3, 4, 1024, 5)
    assert ops.RESECT_P3P_SLOTS * ops.RESECT_P3P_MAX_SAMPLES <= ops.RESECT_MAX_HYPOTHESES
    hdr = open(os.path.join(ROOT, "multicam-calibration_amd", "csrc", "mcba_resect_p3p_math.h")).read()
    assert "kP3Sample = 3" in hdr and "kP3Slots = 4" in hdr and "kP3Polish = 5" in hdr


def test_three_point_samples_are_seeded_and_leave_the_global_generator_alone():
    np.random.seed(5)
    before = np.random.get_state()[1].copy()
    a, b, c = m.draw_resection_samples(50, 33, [0, 2], size=3), m.draw_resection_samples(50, 33, [0, 2], size=3), m.draw_resection_samples(50, 33, [0, 3], size=3)
    assert np.array_equal(np.random.get_state()[1], before)
    assert a.shape == (33, 3) and a.dtype == np.int32 and np.array_equal(a, b) and not np.array_equal(a, c) and a.min() >= 0 and a.max() < 50
    assert all(len(set(r)) == 3 for r in a.tolist())
    ref = np.stack([g.choice(50, 3, replace=False) for g in [np.random.default_rng([0, 2])] for _ in range(33)])
    assert np.array_equal(a, ref)
    assert np.array_equal(m.draw_resection_samples(50, 33, [0, 2]), m.draw_resection_samples(50, 33, [0, 2], size=6))
    assert sorted(m.draw_resection_samples(3, 1, 0, size=3)[0].tolist()) == [0, 1, 2]
    for bad in (4, 0, 5, 8):
        with pytest.raises(ValueError, match="size"):
            m.draw_resection_samples(50, 4, 0, size=bad)
    with pytest.raises(ValueError):
        m.draw_resection_samples(2, 4, 0, size=3)


@pytest.mark.parametrize("kw,match", [(dict(solver="p3p", n_hypotheses=0), "n_hypotheses"), (dict(solver="p3p", n_hypotheses=1025), "n_hypotheses"), (dict(solver="epnp"), "solver"),
                                      (dict(solver=None), "solver"), (dict(solver="p3p", threshold=0.0), "threshold"), (dict(solver="p3p", loss="l2"), "loss"),
                                      (dict(solver="p3p", undistort_iterations=-1), "undistort_iterations")])
def test_value_errors_before_any_device(kw, match):
    X, uvs, intr = small()
    args = {**dict(threshold=2.5), **kw}
    with pytest.raises(ValueError, match=match):
        m.resect_camera(X, uvs[0], intr[0], device=10 ** 6, **args)
    with pytest.raises(ValueError, match=match):
        m.resect_cameras(X, uvs, intr, device=10 ** 6, **args)


def test_the_dlt6_bound_is_what_it_was():
    """1025 .. 4096 hypotheses remain valid for the default solver: the argument check passes and the call reaches the device look-up"""
    X, uvs, intr = small()
    with pytest.raises(ValueError, match="n_hypotheses"):
        m.resect_camera(X, uvs[0], intr[0], threshold=2.5, n_hypotheses=4097, device=10 ** 6, solver="dlt6")
    with pytest.raises(ops.McbaError):
        m.resect_camera(X, uvs[0], intr[0], threshold=2.5, n_hypotheses=1025, device=10 ** 6)


def raw(X, uv, intr, H, smp, thr, tables=False):
    cam, dist = _cam_blocks([np.zeros(6)], [intr])
    X, uv = np.ascontiguousarray(X), np.ascontiguousarray(uv)
    T = 4 * max(H, 1)
    out = dict(rt=np.full(12, 7.0), best=np.full(4, 7.0), mask=np.full(len(X), 7, np.uint8), pose=np.full((T, 12), 7.0), cost=np.full(T, 7.0), count=np.full(T, 7, np.uint32),
               status=np.full(T, 7, np.int32), ms=np.full(6, 7.0))
    raw.last = out
    ops.call("mcba_resect_ransac_p3p", 1, len(X), X.ctypes.data, uv.ctypes.data, cam.ctypes.data, dist.ctypes.data, H, smp.ctypes.data, thr, 5, 0, out["rt"].ctypes.data, out["best"].ctypes.data,
             out["mask"].ctypes.data, out["pose"].ctypes.data, out["cost"].ctypes.data, out["count"].ctypes.data, out["status"].ctypes.data, out["ms"].ctypes.data)
    return out


def test_argument_errors_of_the_library_come_before_the_device():
    """MCBA_ERR_ARG with nothing written, GPU or not: the checks run before a device is looked for"""
    X, uvs, intr = small()
    uv = np.array(uvs[0])
    uv[7] = np.nan
    smp = np.arange(3, dtype=np.int32)[None].copy()
    for what, H, s, thr in (("H = 0", 0, smp, 2.5), ("H = 1025", 1025, np.zeros((1025, 3), np.int32), 2.5), ("a repeated index", 1, np.array([[0, 1, 1]], np.int32), 2.5),
                            ("an index out of range", 1, np.array([[0, 1, 40]], np.int32), 2.5), ("a negative index", 1, np.array([[0, -1, 2]], np.int32), 2.5),
                            ("an unusable sampled point", 1, np.array([[0, 7, 2]], np.int32), 2.5), ("threshold = 0", 1, smp, 0.0)):
        with pytest.raises(ops.McbaError) as e:
            raw(X, uv, intr[0], H, np.ascontiguousarray(s), thr)
        print(what, "->", e.value)
        assert e.value.code == ops.ERR_ARG and "mcba_resect_ransac_p3p" in str(e.value), what
        assert all((v == 7).all() for v in raw.last.values()), what


def test_no_gpu_is_an_error_not_a_host_path():
    n = ctypes.c_int()
    rc = ops.load_library().mcba_device_count(ctypes.byref(n))
    if rc == 0 and n.value > 0:
        pytest.skip("a GPU is visible here")
    X, uvs, intr = small()
    with pytest.raises(ops.McbaError):
        m.resect_camera(X, uvs[0], intr[0], threshold=2.5, solver="p3p")
    with pytest.raises(ops.McbaError):
        m.resect_cameras(X, uvs, intr, threshold=2.5, solver="p3p", n_hypotheses=64)
