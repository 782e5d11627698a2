"""estimate_accel_std and trajectory_evidence without a GPU: the exports, the binding, every argument error (raised before a device is touched),
MCBA_ERR_ARG with nothing written, the refusal of a pooled call that does not fit the budget, the loud error where there is no device."""
import ctypes
import dataclasses

import numpy as np
import pytest


def test_exports():
    import multicam_calibration_amd as m
    from multicam_calibration_amd import trajectory

    for name in ("estimate_accel_std", "trajectory_evidence", "AccelEstimate", "TrajectoryEvidence"):
        assert getattr(m, name) is getattr(trajectory, name) and name in m.__all__, name
    assert set(trajectory.TRAJECTORY_STATUS) == {1, -1, -2}
    assert [f.name for f in dataclasses.fields(trajectory.TrajectoryEvidence)] == ["neg2_log_evidence", "data", "penalty", "log_det", "status", "n_usable", "info"]
    assert [f.name for f in dataclasses.fields(trajectory.AccelEstimate)] == ["accel_std", "log_std", "edge", "status", "n_usable", "grid", "neg2_log_evidence_grid", "neg2_log_evidence",
                                                                              "n_evaluations", "info"]
    for f in (trajectory.smooth_trajectories, trajectory.trajectory_uncertainty, trajectory.refine_trajectories, m.refine_skeleton_trajectories):
        assert "estimate_accel_std" in f.__doc__, f.__name__


def test_symbols_are_exported_and_bound():
    from multicam_calibration_amd import build, ops

    lib = ctypes.CDLL(build.build())
    for sym in ("mcba_smooth_evidence", "mcba_estimate_accel_std"):
        assert hasattr(lib, sym) and sym in {s[0] for s in ops.SYMBOLS}
    assert ops.load_library().mcba_abi_version() == 7
    assert "mcba_smooth_evidence.hip" in build.SOURCES and "mcba_smooth_evidence_api.hip" in build.SOURCES and "mcba_smooth_evidence_math.h" in build.DEPS


def test_argument_errors_come_before_any_device():
    from multicam_calibration_amd import estimate_accel_std, trajectory_evidence

    T, K = 6, 2
    pts, cov = np.zeros((T, K, 3)), np.broadcast_to(np.eye(3), (T, K, 3, 3))
    ok = dict(accel_range=(0.01, 1.0))
    shapes = [(np.zeros((T, K, 2)), cov), (np.zeros((T, 3)), cov), (np.zeros((0, K, 3)), np.zeros((0, K, 3, 3))), (np.zeros((T, 0, 3)), np.zeros((T, 0, 3, 3))), (pts, np.zeros((T, K, 3))),
              (pts, np.zeros((T + 1, K))), (pts, np.zeros((T, K, 6)))]
    for p, c in shapes:
        with pytest.raises(ValueError):
            estimate_accel_std(p, c, **ok)
        with pytest.raises(ValueError):
            trajectory_evidence(p, c, accel_std=0.1)
    common = [dict(weights=-np.ones((T, K))), dict(weights=np.full((T, K), np.nan)), dict(weights=np.full((T, K), np.inf)), dict(weights=np.ones((T, K + 1))), dict(segment=1), dict(segment=65)]
    for kw in common:
        with pytest.raises(ValueError):
            estimate_accel_std(pts, cov, **ok, **kw)
        with pytest.raises(ValueError):
            trajectory_evidence(pts, cov, accel_std=0.1, **kw)
    for acc in (0.0, -1.0, np.inf, np.nan, [0.1, 0.0], [0.1, 0.1, 0.1], 1e-170):
        with pytest.raises(ValueError):
            trajectory_evidence(pts, cov, accel_std=acc)
    for rng in ((0.0, 1.0), (-0.1, 1.0), (0.1, 0.1), (1.0, 0.1), (0.1, np.inf), (np.nan, 1.0), (0.1, np.nan), (1e-170, 1.0), (0.1, 1e170), (0.1,), (0.1, 1.0, 2.0), 0.1):
        with pytest.raises(ValueError, match="accel_range"):
            estimate_accel_std(pts, cov, accel_range=rng)
    with pytest.raises(TypeError):
        estimate_accel_std(pts, cov)   # accel_range is required
    for kw in (dict(n_grid=2), dict(n_grid=0), dict(rtol=1e-7), dict(rtol=1.0), dict(rtol=np.nan), dict(rtol=-1e-3), dict(pool="some"), dict(pool=np.zeros(K + 1, int)), dict(pool=np.zeros(K)),
               dict(pool=np.zeros((K, 1), int))):
        with pytest.raises(ValueError):
            estimate_accel_std(pts, cov, **ok, **kw)
    for Tshort in (1, 2):   # the evidence of two frames does not depend on accel_std
        with pytest.raises(ValueError, match="3 frames"):
            estimate_accel_std(np.zeros((Tshort, K, 3)), 0.1, **ok)
    with pytest.raises(TypeError):
        estimate_accel_std(pts, cov, **ok, loss="huber")   # no robust loss inside the estimator: the weights are given


def _estimate_call(ops, T=5, K=2, pts=0, cov6=0, lo=0.01, hi=1.0, G=5, rtol=1e-3, win=None, pool=None, segment=0, drop=None):
    pts = np.zeros((5, 2, 3)) if isinstance(pts, int) else pts
    cov6 = np.tile([1.0, 0, 0, 1, 0, 1], (5, 2, 1)) if isinstance(cov6, int) else cov6
    out = [np.full(2, 7.0), np.full(2, 7.0), np.full(2, 7, np.int32), np.full(2, 7, np.int32), np.full(2, 7, np.int32), np.full(5, 7.0), np.full((5, 2), 7.0), np.full(2, 7.0), np.full(1, 7, np.int32),
           np.full(8, 7.0)]
    ms = ctypes.c_double(7.0)
    ptrs = [a.ctypes.data for a in out]
    if drop is not None:
        ptrs[drop] = None
    with pytest.raises(ops.McbaError) as e:
        ops.call("mcba_estimate_accel_std", T, K, None if pts is None else pts.ctypes.data, None if cov6 is None else cov6.ctypes.data, lo, hi, G, rtol, None if win is None else win.ctypes.data,
                 None if pool is None else pool.ctypes.data, segment, 0, *ptrs, ctypes.addressof(ms))
    assert e.value.code == ops.ERR_ARG, e.value
    assert all((a == 7).all() for a in out) and ms.value == 7.0
    return str(e.value)


def test_bad_arguments_of_the_c_calls_write_nothing():
    from multicam_calibration_amd import ops

    win = np.ones((5, 2))
    call = lambda **kw: _estimate_call(ops, **kw)   # noqa: E731
    for kw in (dict(T=0), dict(T=2), dict(T=2 ** 31 + 1), dict(K=0), dict(K=-1), dict(pts=None), dict(cov6=None), dict(lo=0.0), dict(lo=-1.0), dict(lo=1.0, hi=1.0), dict(lo=2.0), dict(hi=np.inf),
               dict(hi=np.nan), dict(lo=np.nan), dict(lo=1e-170), dict(G=2), dict(rtol=1e-7), dict(rtol=1.0), dict(rtol=np.nan), dict(segment=1), dict(segment=65), dict(segment=-2), dict(win=-win),
               dict(win=win * np.nan), dict(win=win * np.inf), dict(pool=np.array([0, 2], np.int32)), dict(pool=np.array([-1, 0], np.int32))):
        call(**kw)
    for drop in range(10):
        call(drop=drop)

    def evidence(T=5, K=2, acc=np.full(2, 0.1), win=None, segment=0, drop=None):
        pts, cov6 = np.zeros((5, 2, 3)), np.tile([1.0, 0, 0, 1, 0, 1], (5, 2, 1))
        out = [np.full((2, 4), 7.0), np.full(2, 7, np.int32), np.full(2, 7, np.int32), np.full(8, 7.0)]
        ptrs = [a.ctypes.data for a in out]
        if drop is not None:
            ptrs[drop] = None
        with pytest.raises(ops.McbaError) as e:
            ops.call("mcba_smooth_evidence", T, K, pts.ctypes.data, cov6.ctypes.data, None if acc is None else acc.ctypes.data, None if win is None else win.ctypes.data, segment, 0, *ptrs, None)
        assert e.value.code == ops.ERR_ARG, e.value
        assert all((a == 7).all() for a in out)

    for kw in (dict(T=0), dict(T=2 ** 31 + 1), dict(K=0), dict(acc=None), dict(acc=np.array([0.1, 0.0])), dict(acc=np.array([np.nan, 0.1])), dict(acc=np.array([0.1, np.inf])), dict(segment=1),
               dict(segment=65), dict(win=-win), dict(win=win * np.nan), dict(drop=0), dict(drop=1), dict(drop=2), dict(drop=3)):
        evidence(**kw)


def test_pooled_call_that_does_not_fit_the_budget_is_refused_by_name(monkeypatch):
    from multicam_calibration_amd import ops

    monkeypatch.setenv("MCBA_SMOOTH_BUDGET_MB", "0.001")
    msg = _estimate_call(ops, pool=np.zeros(2, np.int32))
    assert "MCBA_SMOOTH_BUDGET_MB" in msg


def test_no_gpu_is_a_loud_error():
    from multicam_calibration_amd import estimate_accel_std, ops, trajectory_evidence

    n = ctypes.c_int()
    rc = ops.load_library().mcba_device_count(ctypes.byref(n))
    if rc == 0 and n.value > 0:
        pytest.skip("a GPU is visible here")
    with pytest.raises(ops.McbaError):
        trajectory_evidence(np.zeros((6, 2, 3)), 0.1, accel_std=0.1)
    with pytest.raises(ops.McbaError):
        estimate_accel_std(np.zeros((6, 2, 3)), 0.1, accel_range=(0.01, 1.0), pool="all")
