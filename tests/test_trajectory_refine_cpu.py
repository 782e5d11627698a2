"""refine_trajectories without a GPU: the exports, the binding, every argument error (raised before a device is touched), MCBA_ERR_ARG with
nothing written, the chunk rule of the C call against the oracle's count, and the loud error where there is no device."""
import ctypes

import numpy as np
import pytest

import trajectory_refine_oracle as tro
from test_hostcheck_traj_refine import CHUNK_SHAPES, build, check_chunk_rule

C, T, K = 3, 6, 2


def rig(C=C):
    s = tro.make_scene(C, T, K, seed=41, p_drop=0.0)
    return s["truth"], s["uvs"], s["ext"], s["intr"]


def test_exports():
    import multicam_calibration_amd as m
    from multicam_calibration_amd import trajectory

    for name in ("refine_trajectories", "refine_trajectories_system", "TrajectoryRefinement", "TrajectoryRefinementSystem", "TRAJECTORY_REFINE_STATUS"):
        assert getattr(m, name) is getattr(trajectory, name) and name in m.__all__, name
    assert set(trajectory.TRAJECTORY_REFINE_STATUS) == {1, -1, -2, -3} and set(trajectory.TRAJECTORY_STATUS) == {1, -1, -2}
    assert "smooth_trajectories(...).points" in trajectory.refine_trajectories.__doc__


def test_symbols_are_exported_and_bound():
    from multicam_calibration_amd import build as lib_build, ops

    lib = ctypes.CDLL(lib_build.build())
    for name in ("mcba_refine_trajectories", "mcba_refine_trajectories_system"):
        assert hasattr(lib, name) and name in {s[0] for s in ops.SYMBOLS}
    assert ops.load_library().mcba_abi_version() == 7
    assert "mcba_traj_refine.hip" in lib_build.SOURCES and "mcba_traj_refine_api.hip" in lib_build.SOURCES and "mcba_traj_refine_math.h" in lib_build.DEPS


def test_argument_errors_come_before_any_device():
    from multicam_calibration_amd import refine_trajectories, refine_trajectories_system

    x, uv, ext, intr = rig()
    ok = dict(accel_std=0.1)
    wide = tro.make_scene(4, T, K, seed=41, p_drop=0.0)
    ext65, intr65 = [wide["ext"][0]] * 65, [wide["intr"][0]] * 65
    bad = [
        (np.zeros((T, K, 2)), uv, ext, intr, ok), (np.zeros((T, 3)), uv, ext, intr, ok), (np.zeros((0, K, 3)), np.zeros((C, 0, K, 2)), ext, intr, ok),
        (np.zeros((T, 0, 3)), np.zeros((C, T, 0, 2)), ext, intr, ok),
        (x, uv[:2], ext, intr, ok), (x, uv[:, :5], ext, intr, ok), (x, uv[..., :1], ext, intr, ok), (x, list(uv[:, :, :1]), ext, intr, ok), (x, uv, ext[:2], intr, ok),
        (x, np.zeros((65, T, K, 2)), ext65, intr65, ok),
        (x, uv, ext, intr, dict(accel_std=0.0)), (x, uv, ext, intr, dict(accel_std=-1.0)), (x, uv, ext, intr, dict(accel_std=np.inf)), (x, uv, ext, intr, dict(accel_std=np.nan)),
        (x, uv, ext, intr, dict(accel_std=[0.1, 0.0])), (x, uv, ext, intr, dict(accel_std=[0.1] * 3)),
        (x, uv, ext, intr, dict(accel_std=0.1, pixel_std=0.0)), (x, uv, ext, intr, dict(accel_std=0.1, pixel_std=-0.5)), (x, uv, ext, intr, dict(accel_std=0.1, pixel_std=np.nan)),
        (x, uv, ext, intr, dict(accel_std=0.1, pixel_std=[0.5, 0.5, 0.0])), (x, uv, ext, intr, dict(accel_std=0.1, pixel_std=[0.5, 0.5])),
        (x, uv, ext, intr, dict(accel_std=0.1, f_scale=0.0)), (x, uv, ext, intr, dict(accel_std=0.1, f_scale=-1.0)),
        (x, uv, ext, intr, dict(accel_std=0.1, loss="cauchy")), (x, uv, ext, intr, dict(accel_std=0.1, loss="arctan")), (x, uv, ext, intr, dict(accel_std=0.1, loss="tukey")),
        (x, uv, ext, intr, dict(accel_std=0.1, loss=lambda z: z)),
        (x, uv, ext, intr, dict(accel_std=0.1, weights=-np.ones((C, T, K)))), (x, uv, ext, intr, dict(accel_std=0.1, weights=np.full((C, T, K), np.inf))),
        (x, uv, ext, intr, dict(accel_std=0.1, weights=np.ones((C, T, K + 1)))), (x, uv, ext, intr, dict(accel_std=0.1, weights=np.ones((T, K)))),
        (x, uv, ext, intr, dict(accel_std=0.1, segment=1)), (x, uv, ext, intr, dict(accel_std=0.1, segment=65)),
    ]
    for p, u, e, i, kw in bad:
        with pytest.raises(ValueError):
            refine_trajectories(p, u, e, i, **kw)
        with pytest.raises(ValueError):
            refine_trajectories_system(p, u, e, i, **kw)
    for kw in (dict(max_iterations=0), dict(xtol=-1.0), dict(uncertainty="yes"), dict(uncertainty=1)):
        with pytest.raises(ValueError):
            refine_trajectories(x, uv, ext, intr, accel_std=0.1, **kw)
    with pytest.raises(ValueError, match="not convex"):
        refine_trajectories(x, uv, ext, intr, accel_std=0.1, loss="cauchy")


def test_bad_arguments_of_the_c_calls_write_nothing():
    from multicam_calibration_amd import ops

    x, uv, ext, intr = rig()
    uv = np.ascontiguousarray(uv)
    cam, dist = tro.tco.camera_blocks(ext, intr)
    ps, acc, w, M = np.full(C, 0.5), np.full(K, 0.1), np.ones((C, T, K)), 3

    def call(T=T, K=K, C=C, uv=uv, w=None, ps=ps, x=x, acc=acc, loss=0, f_scale=3.0, max_iterations=M, xtol=1e-8, segment=0, lag_only=False):
        p = lambda a: None if a is None else a.ctypes.data
        loop = [np.full((6, 2, 3), 7.0), np.full((6, 2, 6), 7.0), np.full(2, 7, np.int32), np.full(2, 7, np.int32), np.full(2, 7, np.int32), np.full(2, 7, np.int32), np.full(2, 7.0),
                np.full((M, 2, 3), 7.0), None if lag_only else np.full((6, 2, 6), 7.0), np.full((5, 2, 9), 7.0), np.full(8, 7.0)]
        ms = ctypes.c_double(7.0)
        with pytest.raises(ops.McbaError) as e:
            ops.call("mcba_refine_trajectories", T, K, C, p(uv), p(cam), p(dist), p(w), p(ps), p(x), p(acc), loss, f_scale, max_iterations, xtol, segment, 0, *[p(a) for a in loop], ctypes.addressof(ms))
        assert e.value.code == ops.ERR_ARG, e.value
        assert all((a == 7).all() for a in loop if a is not None) and ms.value == 7.0
        if lag_only or max_iterations != M or xtol != 1e-8:
            return
        sysd = [np.full((6, 2, 6), 7.0), np.full((6, 2, 3), 7.0), np.full((6, 2, 3), 7.0), np.full(2, 7, np.int32), np.full(2, 7, np.int32), np.full(2, 7, np.int32), np.full(2, 7.0), np.full(2, 7.0),
                np.full((2, 4), 7.0), np.full(8, 7.0)]
        with pytest.raises(ops.McbaError) as e:
            ops.call("mcba_refine_trajectories_system", T, K, C, p(uv), p(cam), p(dist), p(w), p(ps), p(x), p(acc), loss, f_scale, segment, 0, *[p(a) for a in sysd], ctypes.addressof(ms))
        assert e.value.code == ops.ERR_ARG, e.value
        assert all((a == 7).all() for a in sysd) and ms.value == 7.0

    call(T=0)
    call(K=0)
    call(C=0)
    call(C=65)
    call(uv=None)
    call(x=None)
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
    call(ps=np.array([0.5, 0.0, 0.5]))
    call(ps=np.array([0.5, -1.0, 0.5]))
    call(ps=np.array([0.5, np.nan, 0.5]))
    call(w=-w)
    call(w=w * np.inf)
    call(lag_only=True)


def test_chunk_rule_against_the_oracles_count(tmp_path_factory):
    """(the header's rule, compiled for the host as tests/test_hostcheck_traj_refine.py compiles it)"""
    hc = build(tmp_path_factory)
    for T, segment in CHUNK_SHAPES:
        check_chunk_rule(hc, T, segment)


def test_no_gpu_is_a_loud_error():
    from multicam_calibration_amd import ops, refine_trajectories, refine_trajectories_system

    n = ctypes.c_int()
    rc = ops.load_library().mcba_device_count(ctypes.byref(n))
    if rc == 0 and n.value > 0:
        pytest.skip("a GPU is visible here")
    x, uv, ext, intr = rig()
    with pytest.raises(ops.McbaError):
        refine_trajectories(x, uv, ext, intr, accel_std=0.1)
    with pytest.raises(ops.McbaError):
        refine_trajectories_system(x, uv, ext, intr, accel_std=0.1)
