"""refine_skeleton and estimate_bone_lengths without a GPU: the exports, the binding, the walk from bones to parents, every argument error
(raised before a device is touched), MCBA_ERR_ARG with nothing written, and the loud error where there is no device."""
import ctypes

import numpy as np
import pytest

import skeleton_oracle as sko

C, T, K = 3, 4, 5
BONES = np.array([[0, 1], [1, 2], [1, 3], [3, 4]])


def rig(C=C):
    s = sko.make_scene(C, T, BONES, K, seed=71, p_drop=0.0)
    return s["truth"], s["uvs"], s["ext"], s["intr"], s["bone_length"]


def test_exports():
    import multicam_calibration_amd as m
    from multicam_calibration_amd import skeleton

    for name in ("refine_skeleton", "refine_skeleton_system", "estimate_bone_lengths", "SkeletonRefinement", "SkeletonSystem", "BoneLengths"):
        assert getattr(m, name) is getattr(skeleton, name) and name in m.__all__, name
    assert m.skeleton is skeleton and set(skeleton.KEYPOINT_STATUS) == {2, 1, -1, -2} and set(skeleton.FRAME_STATUS) == {1, 0, -1}
    assert "two solutions" in skeleton.refine_skeleton.__doc__


def test_symbols_are_exported_and_bound():
    from multicam_calibration_amd import build as lib_build, ops

    lib = ctypes.CDLL(lib_build.build())
    for name in ("mcba_refine_skeleton", "mcba_refine_skeleton_system", "mcba_bone_lengths"):
        assert hasattr(lib, name) and name in {s[0] for s in ops.SYMBOLS}
    assert ops.load_library().mcba_abi_version() == 7
    assert "mcba_skeleton.hip" in lib_build.SOURCES and "mcba_skeleton_api.hip" in lib_build.SOURCES and "mcba_skeleton_math.h" in lib_build.DEPS


@pytest.mark.parametrize("name,K,bones", [("chain", 9, sko.chain(9)), ("star", 9, sko.star(9)), ("two_pieces", 7, np.array([[0, 2], [2, 5], [1, 3], [3, 4], [3, 6]])),
                                          ("random_64", 64, sko.random_tree(64, 3)), ("reversed", 4, np.array([[3, 2], [2, 1], [1, 0]])), ("none", 3, np.zeros((0, 2), int))])
def test_bones_become_parents_by_the_walk_from_the_lowest_keypoint(name, K, bones):
    from multicam_calibration_amd.skeleton import forest_parents

    parent, child = forest_parents(bones, K)
    ref_parent, ref_child = sko.parents_of(bones, K)
    assert np.array_equal(parent, ref_parent) and np.array_equal(child, ref_child)
    assert all(parent[child[e]] in bones[e] and child[e] in bones[e] for e in range(len(bones)))
    roots = np.flatnonzero(parent < 0)
    assert roots[0] == 0 and (name != "two_pieces" or list(roots) == [0, 1])     # the lowest-numbered keypoint of each piece


def test_argument_errors_come_before_any_device():
    from multicam_calibration_amd import estimate_bone_lengths, refine_skeleton, refine_skeleton_system

    x, uv, ext, intr, L = rig()
    ok = dict(bones=BONES, bone_length=L, bone_std=0.5)
    wide = sko.make_scene(4, T, BONES, K, seed=71, p_drop=0.0)
    ext65, intr65 = [wide["ext"][0]] * 65, [wide["intr"][0]] * 65
    x65, uv65 = np.zeros((T, 65, 3)), np.zeros((C, T, 65, 2))
    bad = [
        (np.zeros((T, K, 2)), uv, ext, intr, ok), (np.zeros((T, 3)), uv, ext, intr, ok), (np.zeros((0, K, 3)), np.zeros((C, 0, K, 2)), ext, intr, ok),
        (x, uv[:2], ext, intr, ok), (x, uv[:, :3], ext, intr, ok), (x, uv[..., :1], ext, intr, ok), (x, list(uv[:, :, :1]), ext, intr, ok), (x, uv, ext[:2], intr, ok),
        (x, np.zeros((65, T, K, 2)), ext65, intr65, ok),
        (x65, uv65, ext, intr, dict(bones=sko.chain(65), bone_length=np.ones(64), bone_std=0.5)),                                   # K = 65
        (x, uv, ext, intr, dict(ok, bones=np.array([[0, 1], [1, 2], [2, 0], [3, 4]]))),                                             # a cycle
        (x, uv, ext, intr, dict(ok, bones=np.array([[0, 1], [1, 2], [1, 3], [3, 5]]))), (x, uv, ext, intr, dict(ok, bones=np.array([[0, 1], [1, 2], [1, 3], [-1, 4]]))),   # a bad index
        (x, uv, ext, intr, dict(ok, bones=np.array([[0, 1], [1, 2], [1, 3], [3, 3]]))), (x, uv, ext, intr, dict(ok, bones=np.array([[0, 1], [1, 2], [1, 3], [1, 0]]))),    # a self-bone, a repeat
        (x, uv, ext, intr, dict(ok, bones=BONES.ravel())), (x, uv, ext, intr, dict(ok, bones=BONES + 0.5)),
        (x, uv, ext, intr, dict(ok, bone_std=0.0)), (x, uv, ext, intr, dict(ok, bone_std=-1.0)), (x, uv, ext, intr, dict(ok, bone_std=np.nan)), (x, uv, ext, intr, dict(ok, bone_std=np.inf)),
        (x, uv, ext, intr, dict(ok, bone_std=[0.5, 0.5, 0.0, 0.5])), (x, uv, ext, intr, dict(ok, bone_std=[0.5] * 3)),
        (x, uv, ext, intr, dict(ok, bone_length=L * 0)), (x, uv, ext, intr, dict(ok, bone_length=-L)), (x, uv, ext, intr, dict(ok, bone_length=L[:3])), (x, uv, ext, intr, dict(ok, bone_length=10.0)),
        (x, uv, ext, intr, dict(ok, bone_length=np.r_[L[:3], np.nan])),
        (x, uv, ext, intr, dict(ok, pixel_std=0.0)), (x, uv, ext, intr, dict(ok, pixel_std=-0.5)), (x, uv, ext, intr, dict(ok, pixel_std=np.nan)),
        (x, uv, ext, intr, dict(ok, pixel_std=[0.5, 0.5, 0.0])), (x, uv, ext, intr, dict(ok, pixel_std=[0.5, 0.5])),
        (x, uv, ext, intr, dict(ok, f_scale=0.0)), (x, uv, ext, intr, dict(ok, f_scale=-1.0)), (x, uv, ext, intr, dict(ok, loss="tukey")), (x, uv, ext, intr, dict(ok, loss=lambda z: z)),
        (x, uv, ext, intr, dict(ok, weights=-np.ones((C, T, K)))), (x, uv, ext, intr, dict(ok, weights=np.full((C, T, K), np.inf))),
        (x, uv, ext, intr, dict(ok, weights=np.ones((C, T, K + 1)))), (x, uv, ext, intr, dict(ok, weights=np.ones((T, K)))),
    ]
    for p, u, e, i, kw in bad:
        with pytest.raises(ValueError):
            refine_skeleton(p, u, e, i, **kw)
        with pytest.raises(ValueError):
            refine_skeleton_system(p, u, e, i, **kw)
    for kw in (dict(max_iterations=0), dict(xtol=-1.0), dict(covariance="yes"), dict(covariance=1)):
        with pytest.raises(ValueError):
            refine_skeleton(x, uv, ext, intr, **ok, **kw)
    for lam in (-1.0, np.nan, np.inf):
        with pytest.raises(ValueError):
            refine_skeleton_system(x, uv, ext, intr, lam=lam, **ok)
    with pytest.raises(ValueError, match="cycle"):
        refine_skeleton(x, uv, ext, intr, **dict(ok, bones=np.array([[0, 1], [1, 2], [2, 0], [3, 4]])))
    for pts, bones in ((np.zeros((T, 3)), BONES), (np.zeros((0, K, 3)), BONES), (x, np.zeros((0, 2), int)), (x, BONES.ravel()), (x, BONES + 2), (x, BONES - 1), (x, BONES.astype(float))):
        with pytest.raises(ValueError):
            estimate_bone_lengths(pts, bones)


def test_bad_arguments_of_the_c_calls_write_nothing():
    from multicam_calibration_amd import ops

    x, uv, ext, intr, L = rig()
    uv = np.ascontiguousarray(uv)
    cam, dist = sko.tco.camera_blocks(ext, intr)
    parent = np.array([-1, 0, 1, 1, 3], np.int32)
    ps, w, Lk, sk = np.full(C, 0.5), np.ones((C, T, K)), np.r_[0.0, L], np.r_[0.0, np.full(4, 0.5)]
    p = lambda a: None if a is None else a.ctypes.data

    def call(T=T, K=K, C=C, uv=uv, w=None, ps=ps, x=x, parent=parent, Lk=Lk, sk=sk, loss=0, f_scale=3.0, max_iterations=5, xtol=1e-8, lam=1e-4, cov_only=False, loop_only=False):
        loop = [np.full((4, 5, 3), 7.0), np.full((4, 5), 7, np.int32), np.full(4, 7, np.int32), np.full(4, 7, np.int32), np.full(4, 7.0), np.full(4, 7.0), np.full((4, 5), 7.0),
                np.full((4, 5, 6), 7.0), None if cov_only else np.full((4, 5, 6), 7.0), None if cov_only else np.full((4, 5, 3), 7.0), np.full(8, 7.0)]
        ms = ctypes.c_double(7.0)
        with pytest.raises(ops.McbaError) as e:
            ops.call("mcba_refine_skeleton", T, K, C, p(uv), p(cam), p(dist), p(w), p(ps), p(x), p(parent), p(Lk), p(sk), loss, f_scale, max_iterations, xtol, 0, *[p(a) for a in loop],
                     ctypes.addressof(ms))
        assert e.value.code == ops.ERR_ARG, e.value
        assert all((a == 7).all() for a in loop if a is not None) and ms.value == 7.0
        if cov_only or loop_only:
            return
        sysd = [np.full((4, 5, 6), 7.0), np.full((4, 5, 3), 7.0), np.full((4, 5, 3), 7.0), np.full((4, 5, 3), 7.0), np.full((4, 5), 7, np.int32), np.full(4, 7, np.int32), np.full(4, 7.0),
                np.full(4, 7.0), np.full(4, 7.0), np.full(8, 7.0)]
        with pytest.raises(ops.McbaError) as e:
            ops.call("mcba_refine_skeleton_system", T, K, C, p(uv), p(cam), p(dist), p(w), p(ps), p(x), p(parent), p(Lk), p(sk), loss, f_scale, lam, 0, *[p(a) for a in sysd], ctypes.addressof(ms))
        assert e.value.code == ops.ERR_ARG, e.value
        assert all((a == 7).all() for a in sysd) and ms.value == 7.0

    call(T=0)
    call(K=0)
    call(K=65)
    call(C=0)
    call(C=65)
    call(uv=None)
    call(x=None)
    call(parent=None)
    call(Lk=None)
    call(loss=5)
    call(loss=-1)
    call(f_scale=0.0)
    call(f_scale=float("nan"))
    call(max_iterations=0, loop_only=True)
    call(xtol=-1.0, loop_only=True)
    call(parent=np.array([1, 2, 0, 1, 3], np.int32))      # a cycle
    call(parent=np.array([-1, 1, 1, 1, 3], np.int32))     # its own parent
    call(parent=np.array([-1, 0, 5, 1, 3], np.int32))     # outside 0 .. K - 1
    call(parent=np.array([-2, 0, 1, 1, 3], np.int32))
    call(Lk=np.r_[0.0, L[:3], 0.0])
    call(Lk=np.r_[0.0, L[:3], np.nan])
    call(sk=np.r_[0.0, 0.5, 0.5, -0.5, 0.5])
    call(sk=np.r_[0.0, 0.5, 0.5, np.inf, 0.5])
    call(ps=np.array([0.5, 0.0, 0.5]))
    call(ps=np.array([0.5, np.nan, 0.5]))
    call(w=-w)
    call(w=w * np.inf)
    call(cov_only=True)

    pts, bones = np.ascontiguousarray(x), np.ascontiguousarray(BONES, dtype=np.int32)
    for kw in (dict(T=0), dict(K=0), dict(E=0), dict(E=65536), dict(pts=None), dict(bones=None), dict(bones=np.ascontiguousarray(BONES + 1, dtype=np.int32)),
               dict(bones=np.ascontiguousarray(BONES - 1, dtype=np.int32))):
        a = dict(T=T, K=K, E=4, pts=pts, bones=bones)
        a.update(kw)
        out = [np.full(4, 7.0), np.full(4, 7.0), np.full(4, 7, np.int32)]
        ms = ctypes.c_double(7.0)
        with pytest.raises(ops.McbaError) as e:
            ops.call("mcba_bone_lengths", a["T"], a["K"], p(a["pts"]), a["E"], p(a["bones"]), 0, *[p(o) for o in out], ctypes.addressof(ms))
        assert e.value.code == ops.ERR_ARG and all((o == 7).all() for o in out) and ms.value == 7.0


def test_no_gpu_is_a_loud_error():
    from multicam_calibration_amd import estimate_bone_lengths, ops, refine_skeleton, refine_skeleton_system

    n = ctypes.c_int()
    rc = ops.load_library().mcba_device_count(ctypes.byref(n))
    if rc == 0 and n.value > 0:
        pytest.skip("a GPU is visible here")
    x, uv, ext, intr, L = rig()
    with pytest.raises(ops.McbaError):
        refine_skeleton(x, uv, ext, intr, bones=BONES, bone_length=L, bone_std=0.5)
    with pytest.raises(ops.McbaError):
        refine_skeleton_system(x, uv, ext, intr, bones=BONES, bone_length=L, bone_std=0.5)
    with pytest.raises(ops.McbaError):
        estimate_bone_lengths(x, BONES)
