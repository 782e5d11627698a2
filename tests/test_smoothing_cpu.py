"""smooth_trajectories without a GPU: the exports, the binding, every argument error (raised before a device is touched), MCBA_ERR_ARG with
nothing written, and the loud error where there is no device."""
import ctypes

import numpy as np
import pytest


def test_exports():
    import multicam_calibration_amd as m
    from multicam_calibration_amd import trajectory

    for name in ("smooth_trajectories", "TrajectorySmoothing"):
        assert getattr(m, name) is getattr(trajectory, name) and name in m.__all__, name
    assert m.trajectory is trajectory and "trajectory" in m.__all__
    assert set(trajectory.TRAJECTORY_STATUS) == {1, -1, -2}


def test_symbol_is_exported_and_bound():
    from multicam_calibration_amd import build, ops

    lib = ctypes.CDLL(build.build())
    assert hasattr(lib, "mcba_smooth_trajectories")
    assert "mcba_smooth_trajectories" in {s[0] for s in ops.SYMBOLS}
    assert ops.load_library().mcba_abi_version() == 7
    assert "mcba_smooth.hip" in build.SOURCES and "mcba_smooth_api.hip" in build.SOURCES and "mcba_smooth_math.h" in build.DEPS


def test_argument_errors_come_before_any_device():
    from multicam_calibration_amd import smooth_trajectories

    T, K = 6, 2
    pts, cov = np.zeros((T, K, 3)), np.broadcast_to(np.eye(3), (T, K, 3, 3))
    ok = dict(accel_std=0.1)
    bad = [
        (np.zeros((T, K, 2)), cov, ok), (np.zeros((T, 3)), cov, ok), (np.zeros((0, K, 3)), np.zeros((0, K, 3, 3)), ok), (np.zeros((T, 0, 3)), np.zeros((T, 0, 3, 3)), ok),
        (pts, np.zeros((T, K, 3)), ok), (pts, np.zeros((T + 1, K)), ok),
        (pts, cov, dict(accel_std=0.0)), (pts, cov, dict(accel_std=-1.0)), (pts, cov, dict(accel_std=np.inf)), (pts, cov, dict(accel_std=np.nan)), (pts, cov, dict(accel_std=[0.1, 0.0])),
        (pts, cov, dict(accel_std=[0.1, 0.1, 0.1])),
        (pts, cov, dict(accel_std=0.1, f_scale=0.0)), (pts, cov, dict(accel_std=0.1, f_scale=-1.0)),
        (pts, cov, dict(accel_std=0.1, loss="cauchy")), (pts, cov, dict(accel_std=0.1, loss="arctan")), (pts, cov, dict(accel_std=0.1, loss="tukey")), (pts, cov, dict(accel_std=0.1, loss=lambda z: z)),
        (pts, cov, dict(accel_std=0.1, weights_in=-np.ones((T, K)))), (pts, cov, dict(accel_std=0.1, weights_in=np.full((T, K), np.nan))), (pts, cov, dict(accel_std=0.1, weights_in=np.full((T, K), np.inf))),
        (pts, cov, dict(accel_std=0.1, weights_in=np.ones((T, K + 1)))),
        (pts, cov, dict(accel_std=0.1, max_iterations=0)), (pts, cov, dict(accel_std=0.1, segment=1)), (pts, cov, dict(accel_std=0.1, segment=65)),
    ]
    for p, c, kw in bad:
        with pytest.raises(ValueError):
            smooth_trajectories(p, c, **kw)
    with pytest.raises(ValueError, match="not convex"):
        smooth_trajectories(pts, cov, accel_std=0.1, loss="cauchy")


def test_bad_arguments_of_the_c_call_write_nothing():
    from multicam_calibration_amd import ops

    T, K, M = 5, 2, 3
    pts, cov6, acc, win = np.zeros((T, K, 3)), np.tile([1.0, 0, 0, 1, 0, 1], (T, K, 1)), np.full(K, 0.1), np.ones((T, K))

    def call(T=T, K=K, pts=pts, cov6=cov6, acc=acc, win=None, loss=0, f_scale=3.0, max_iterations=M, xtol=1e-8, segment=0):
        out = [np.full((5, 2, 3), 7.0), np.full((5, 2), 7.0), np.full((5, 2), 7.0), np.full(2, 7, np.int32), np.full(2, 7, np.int32), np.full(2, 7, np.int32), np.full((3, 2, 2), 7.0), np.full(8, 7.0)]
        ms = ctypes.c_double(7.0)
        with pytest.raises(ops.McbaError) as e:
            ops.call("mcba_smooth_trajectories", T, K, None if pts is None else pts.ctypes.data, cov6.ctypes.data, acc.ctypes.data, None if win is None else win.ctypes.data, loss, f_scale,
                     max_iterations, xtol, segment, 0, *[a.ctypes.data for a in out], ctypes.addressof(ms))
        assert e.value.code == ops.ERR_ARG, e.value
        assert all((a == 7).all() for a in out) and ms.value == 7.0

    call(T=0)
    call(K=0)
    call(pts=None)
    call(loss=3)
    call(loss=-1)
    call(f_scale=0.0)
    call(f_scale=float("nan"))
    call(max_iterations=0)
    call(xtol=-1.0)
    call(segment=1)
    call(segment=65)
    call(acc=np.array([0.1, 0.0]))
    call(acc=np.array([0.1, np.inf]))
    call(win=-win)
    call(win=win * np.nan)


def test_no_gpu_is_a_loud_error():
    from multicam_calibration_amd import ops, smooth_trajectories

    n = ctypes.c_int()
    rc = ops.load_library().mcba_device_count(ctypes.byref(n))
    if rc == 0 and n.value > 0:
        pytest.skip("a GPU is visible here")
    with pytest.raises(ops.McbaError):
        smooth_trajectories(np.zeros((6, 2, 3)), 0.1, accel_std=0.1)
