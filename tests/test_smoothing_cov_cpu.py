"""trajectory_uncertainty without a GPU: the exports, the binding, every argument error (raised before a device is touched), MCBA_ERR_ARG with
nothing written, the loud error where there is no device, and the fields smooth_trajectories leaves empty by default."""
import ctypes
import dataclasses

import numpy as np
import pytest


def test_exports():
    import multicam_calibration_amd as m
    from multicam_calibration_amd import trajectory

    for name in ("trajectory_uncertainty", "TrajectoryUncertainty", "smooth_trajectories", "TrajectorySmoothing"):
        assert getattr(m, name) is getattr(trajectory, name) and name in m.__all__, name
    assert set(trajectory.TRAJECTORY_STATUS) == {1, -1, -2}
    assert [f.name for f in dataclasses.fields(trajectory.TrajectoryUncertainty)] == ["covariance", "std", "lag_covariance", "status", "n_usable", "info"]
    names = [f.name for f in dataclasses.fields(trajectory.TrajectorySmoothing)]
    assert names[-4:] == ["info", "covariance", "std", "lag_covariance"]   # appended after info


def test_symbol_is_exported_and_bound():
    from multicam_calibration_amd import build, ops

    lib = ctypes.CDLL(build.build())
    assert hasattr(lib, "mcba_smooth_covariance")
    assert "mcba_smooth_covariance" in {s[0] for s in ops.SYMBOLS}
    assert ops.load_library().mcba_abi_version() == 7
    assert "mcba_smooth_cov.hip" in build.SOURCES and "mcba_smooth_cov_api.hip" in build.SOURCES and "mcba_smooth_cov_math.h" in build.DEPS


def test_argument_errors_come_before_any_device():
    from multicam_calibration_amd import smooth_trajectories, trajectory_uncertainty

    T, K = 6, 2
    pts, cov = np.zeros((T, K, 3)), np.broadcast_to(np.eye(3), (T, K, 3, 3))
    ok = dict(accel_std=0.1)
    bad = [
        (np.zeros((T, K, 2)), cov, ok), (np.zeros((T, 3)), cov, ok), (np.zeros((0, K, 3)), np.zeros((0, K, 3, 3)), ok), (np.zeros((T, 0, 3)), np.zeros((T, 0, 3, 3)), ok),
        (pts, np.zeros((T, K, 3)), ok), (pts, np.zeros((T + 1, K)), ok), (pts, np.zeros((T, K, 6)), ok),
        (pts, cov, dict(accel_std=0.0)), (pts, cov, dict(accel_std=-1.0)), (pts, cov, dict(accel_std=np.inf)), (pts, cov, dict(accel_std=np.nan)), (pts, cov, dict(accel_std=[0.1, 0.0])),
        (pts, cov, dict(accel_std=[0.1, 0.1, 0.1])), (pts, cov, dict(accel_std=1e-170)),
        (pts, cov, dict(accel_std=0.1, weights=-np.ones((T, K)))), (pts, cov, dict(accel_std=0.1, weights=np.full((T, K), np.nan))), (pts, cov, dict(accel_std=0.1, weights=np.full((T, K), np.inf))),
        (pts, cov, dict(accel_std=0.1, weights=np.ones((T, K + 1)))),
        (pts, cov, dict(accel_std=0.1, segment=1)), (pts, cov, dict(accel_std=0.1, segment=65)),
    ]
    for p, c, kw in bad:
        with pytest.raises(ValueError):
            trajectory_uncertainty(p, c, **kw)
    for u in ("yes", 1, None, "Lag"):
        with pytest.raises(ValueError, match="uncertainty"):
            smooth_trajectories(pts, cov, accel_std=0.1, uncertainty=u)
    with pytest.raises(TypeError):
        trajectory_uncertainty(pts, cov, accel_std=0.1, loss="huber")   # the loss plays no part: the weights are given


def test_bad_arguments_of_the_c_call_write_nothing():
    from multicam_calibration_amd import ops

    T, K = 5, 2
    pts, cov6, acc, win = np.zeros((T, K, 3)), np.tile([1.0, 0, 0, 1, 0, 1], (T, K, 1)), np.full(K, 0.1), np.ones((T, K))

    def call(T=T, K=K, pts=pts, cov6=cov6, acc=acc, win=None, segment=0, drop=None):
        out = [np.full((5, 2, 6), 7.0), np.full((4, 2, 9), 7.0), np.full(2, 7, np.int32), np.full(2, 7, np.int32), np.full(8, 7.0)]
        ms = ctypes.c_double(7.0)
        ptrs = [a.ctypes.data for a in out]
        if drop is not None:
            ptrs[drop] = None
        with pytest.raises(ops.McbaError) as e:
            ops.call("mcba_smooth_covariance", T, K, None if pts is None else pts.ctypes.data, None if cov6 is None else cov6.ctypes.data, None if acc is None else acc.ctypes.data,
                     None if win is None else win.ctypes.data, segment, 0, *ptrs, ctypes.addressof(ms))
        assert e.value.code == ops.ERR_ARG, e.value
        assert all((a == 7).all() for a in out) and ms.value == 7.0

    call(T=0)
    call(T=2 ** 31 + 1)
    call(K=0)
    call(K=-1)
    call(pts=None)
    call(cov6=None)
    call(acc=None)
    call(drop=0)   # out_cov6
    call(drop=2)   # status
    call(drop=3)   # n_usable
    call(drop=4)   # info8
    call(segment=1)
    call(segment=65)
    call(segment=-2)
    call(acc=np.array([0.1, 0.0]))
    call(acc=np.array([0.1, np.inf]))
    call(acc=np.array([np.nan, 0.1]))
    call(win=-win)
    call(win=win * np.nan)
    call(win=win * np.inf)


def test_no_gpu_is_a_loud_error():
    from multicam_calibration_amd import ops, trajectory_uncertainty

    n = ctypes.c_int()
    rc = ops.load_library().mcba_device_count(ctypes.byref(n))
    if rc == 0 and n.value > 0:
        pytest.skip("a GPU is visible here")
    with pytest.raises(ops.McbaError):
        trajectory_uncertainty(np.zeros((6, 2, 3)), 0.1, accel_std=0.1, lag=True)


def test_the_new_fields_default_to_none(monkeypatch):
    """uncertainty=False makes no further call: the three fields of the result stay None (a stand-in library call, so that no device is needed)"""
    from multicam_calibration_amd import ops, trajectory

    calls = []

    def fake(name, *args):
        calls.append(name)
        T, K = args[0], args[1]
        np.ctypeslib.as_array(ctypes.cast(args[17], ctypes.POINTER(ctypes.c_int32)), (K,))[:] = 1   # n_iterations
        np.ctypeslib.as_array(ctypes.cast(args[15], ctypes.POINTER(ctypes.c_int32)), (K,))[:] = 1   # status

    monkeypatch.setattr(ops, "call", fake)
    r = trajectory.smooth_trajectories(np.zeros((4, 2, 3)), 0.1, accel_std=0.1)
    assert calls == ["mcba_smooth_trajectories"]
    assert r.covariance is None and r.std is None and r.lag_covariance is None
