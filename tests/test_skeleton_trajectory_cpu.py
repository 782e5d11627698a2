"""refine_skeleton_trajectories without a GPU: the exports, the binding, every argument error (raised before a device is touched), MCBA_ERR_ARG of the
C calls with nothing written -- the call over its memory budget among them --, and the loud error where there is no device."""
import ctypes

import numpy as np
import pytest

import skeleton_oracle as sko
import skeleton_trajectory_oracle as sto

C, T, K = 3, 6, 5
BONES = np.array([[0, 1], [1, 2], [1, 3], [3, 4]])


def rig():
    s = sto.make_scene(C, T, BONES, K, seed=81, p_drop=0.0)
    return s["truth"], s["uvs"], s["ext"], s["intr"], s["bone_length"]


def test_exports():
    import multicam_calibration_amd as m
    from multicam_calibration_amd import skeleton

    for name in ("refine_skeleton_trajectories", "refine_skeleton_trajectories_system", "SkeletonTrajectoryRefinement", "SkeletonTrajectorySystem"):
        assert getattr(m, name) is getattr(skeleton, name) and name in m.__all__, name
    doc = skeleton.refine_skeleton_trajectories.__doc__
    assert "flat valley" in doc and "nearly rigid" in doc and "MCBA_SMOOTH_BUDGET_MB" in doc


def test_symbols_are_exported_and_bound():
    from multicam_calibration_amd import build as lib_build, ops

    lib = ctypes.CDLL(lib_build.build())
    for name in ("mcba_refine_skeleton_trajectories", "mcba_refine_skeleton_trajectories_system"):
        assert hasattr(lib, name) and name in {s[0] for s in ops.SYMBOLS}
    assert ops.load_library().mcba_abi_version() == 7
    assert "mcba_skeltraj.hip" in lib_build.SOURCES and "mcba_skeltraj_api.hip" in lib_build.SOURCES and "mcba_skeltraj_math.h" in lib_build.DEPS


def test_argument_errors_come_before_any_device():
    from multicam_calibration_amd import refine_skeleton_trajectories, refine_skeleton_trajectories_system

    x, uv, ext, intr, L = rig()
    good = dict(accel_std=0.15, bones=BONES, bone_length=L, bone_std=0.5)
    bad = [dict(accel_std=0.0), dict(accel_std=np.ones(K + 1)), dict(accel_std=np.inf), dict(bones=np.array([[0, 1], [1, 2], [2, 0], [3, 4]])), dict(bones=np.array([[0, 1], [1, 1], [1, 3], [3, 4]])),
           dict(bones=np.array([[0, 1], [1, 0], [1, 3], [3, 4]])), dict(bones=np.array([[0, 1], [1, 2], [1, 3], [3, K]])), dict(bone_length=L[:-1]), dict(bone_length=-L), dict(bone_std=0.0),
           dict(bone_std=np.nan), dict(loss="cauchy"), dict(loss="arctan"), dict(loss="nope"), dict(f_scale=0.0), dict(pixel_std=-1.0), dict(weights=-np.ones((C, T, K))),
           dict(weights=np.ones((C, T))), dict(cg_tol=0.0), dict(cg_tol=1.0), dict(cg_tol=np.nan), dict(cg_max=0), dict(segment=1), dict(segment=65)]
    for fn in (refine_skeleton_trajectories, refine_skeleton_trajectories_system):
        for b in bad:
            with pytest.raises(ValueError):
                fn(x, uv, ext, intr, **dict(good, **b))
        with pytest.raises(ValueError):
            fn(x[:, :, :2], uv, ext, intr, **good)
        with pytest.raises(ValueError):
            fn(x, uv[:2], ext, intr, **good)
        with pytest.raises(ValueError):
            fn(np.zeros((T, 65, 3)), np.zeros((C, T, 65, 2)), ext, intr, accel_std=0.15, bones=sko.chain(65), bone_length=np.ones(64), bone_std=0.5)
    for b in (dict(max_iterations=0), dict(xtol=-1.0)):
        with pytest.raises(ValueError):
            refine_skeleton_trajectories(x, uv, ext, intr, **dict(good, **b))


def c_arguments():
    x, uv, ext, intr, L = rig()
    cam, dist = sto.tco.camera_blocks(ext, intr)
    parent, child = sko.parents_of(BONES, K)
    Lk, sk = np.ones(K), np.ones(K)
    Lk[child], sk[child] = L, 0.5
    return dict(T=T, K=K, C=C, uv=np.ascontiguousarray(uv), cam=cam, dist=dist, w=None, ps=np.full(C, 0.5), x=np.ascontiguousarray(x), acc=np.full(K, 0.15), parent=parent.astype(np.int32), L=Lk, s=sk,
                loss=0, f_scale=3.0, max_iterations=30, xtol=1e-8, cg_tol=1e-6, cg_max=200, segment=0)


def call_loop(a, out):
    from multicam_calibration_amd import ops

    p = lambda v: None if v is None else v.ctypes.data
    ms = ctypes.c_double(7.0)
    ops.call("mcba_refine_skeleton_trajectories", a["T"], a["K"], a["C"], p(a["uv"]), p(a["cam"]), p(a["dist"]), p(a["w"]), p(a["ps"]), p(a["x"]), p(a["acc"]), p(a["parent"]), p(a["L"]), p(a["s"]),
             a["loss"], a["f_scale"], a["max_iterations"], a["xtol"], a["cg_tol"], a["cg_max"], a["segment"], 0, *[p(o) for o in out], ctypes.addressof(ms))


def call_system(a, out):
    from multicam_calibration_amd import ops

    p = lambda v: None if v is None else v.ctypes.data
    ms = ctypes.c_double(7.0)
    ops.call("mcba_refine_skeleton_trajectories_system", a["T"], a["K"], a["C"], p(a["uv"]), p(a["cam"]), p(a["dist"]), p(a["w"]), p(a["ps"]), p(a["x"]), p(a["acc"]), p(a["parent"]), p(a["L"]),
             p(a["s"]), a["loss"], a["f_scale"], a["cg_tol"], a["cg_max"], a["segment"], 0, *[p(o) for o in out], ctypes.addressof(ms))


def outputs():
    d, i = lambda *s: np.full(s, 7.0), lambda *s: np.full(s, 7, np.int32)
    loop = [d(T, K, 3), d(T, K, 6), i(K), i(K), i(K), i(1), i(1), d(1), d(1), d(30, 4), d(T, K), d(T, K, 3), d(8)]
    system = [d(T, K, 6), d(T, K, 3), d(T, K, 3), d(T, K, 3), i(K), i(K), i(K), i(1), d(1), d(1), d(1), d(1), d(4), d(2, T, K, 3), d(8)]
    return loop, system


BAD_C = [dict(T=0), dict(K=0), dict(K=65), dict(C=0), dict(C=65), dict(uv=None), dict(acc=None), dict(parent=None), dict(L=None), dict(s=None), dict(loss=3), dict(loss=-1), dict(f_scale=0.0),
         dict(cg_tol=0.0), dict(cg_tol=1.0), dict(cg_tol=float("nan")), dict(cg_max=0), dict(segment=1), dict(segment=65), dict(ps=np.array([0.5, 0.0, 0.5])), dict(acc=np.zeros(K)),
         dict(parent=np.array([-1, 0, 1, 1, 5], np.int32)), dict(parent=np.array([1, 0, 1, 1, 3], np.int32)), dict(parent=np.array([-1, 1, 1, 1, 3], np.int32)),
         dict(L=np.array([1.0, -1.0, 1.0, 1.0, 1.0])), dict(s=np.array([1.0, 0.0, 1.0, 1.0, 1.0])), dict(w=-np.ones((C, T, K)))]


def test_bad_arguments_of_the_c_calls_write_nothing():
    from multicam_calibration_amd import ops

    for b in BAD_C + [dict(max_iterations=0), dict(xtol=-1.0)]:
        loop, _ = outputs()
        with pytest.raises(ops.McbaError) as e:
            call_loop(dict(c_arguments(), **b), loop)
        assert e.value.code == ops.ERR_ARG and all((o == 7).all() for o in loop), b
    for b in BAD_C:
        _, system = outputs()
        with pytest.raises(ops.McbaError) as e:
            call_system(dict(c_arguments(), **b), system)
        assert e.value.code == ops.ERR_ARG and all((o == 7).all() for o in system), b
    for k in range(13):
        loop, _ = outputs()
        loop[k] = None
        with pytest.raises(ops.McbaError) as e:
            call_loop(c_arguments(), loop)
        assert e.value.code == ops.ERR_ARG


def test_a_call_over_the_budget_is_refused_before_any_device(monkeypatch):
    """bones couple the tracks: the call is one chunk, and one that does not fit MCBA_SMOOTH_BUDGET_MB fails with an error that names the knob"""
    from multicam_calibration_amd import ops

    need = sto.chunk_doubles(T, K, C, None) * 8 / 1048576.0
    monkeypatch.setenv("MCBA_SMOOTH_BUDGET_MB", repr(need * 0.999))
    for call, out in zip((call_loop, call_system), outputs()):
        with pytest.raises(ops.McbaError, match="MCBA_SMOOTH_BUDGET_MB") as e:
            call(c_arguments(), out)
        assert e.value.code == ops.ERR_ARG and all((o == 7).all() for o in out)


def test_no_gpu_is_a_loud_error():
    from multicam_calibration_amd import ops, refine_skeleton_trajectories, refine_skeleton_trajectories_system

    n = ctypes.c_int(0)
    rc = ops.load_library().mcba_device_count(ctypes.byref(n))
    if rc == 0 and n.value > 0:
        pytest.skip("a GPU is visible here")
    x, uv, ext, intr, L = rig()
    for fn in (refine_skeleton_trajectories, refine_skeleton_trajectories_system):
        with pytest.raises(ops.McbaError):
            fn(x, uv, ext, intr, accel_std=0.15, bones=BONES, bone_length=L, bone_std=0.5)
