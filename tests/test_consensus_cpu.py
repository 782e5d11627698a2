"""triangulate_consensus without a GPU: every argument error is raised before a device is touched (here there may be none to touch), at the
public function and at the C entry point, and an empty input returns empty arrays."""
import ctypes

import numpy as np
import pytest

import multicam_calibration_amd as m
from multicam_calibration_amd import ops

from test_triangulate_cpu import scene

NO_DEVICE = 10 ** 6   # an ordinal no machine has: a call that got as far as the device would fail with another error


def test_python_argument_errors():
    uvs, ext, intr, _ = scene(C=3, P=10, seed=2)
    with pytest.raises(TypeError):
        m.triangulate_consensus(uvs, ext, intr, device=NO_DEVICE)       # threshold has no default
    for kw in (dict(threshold=0.0), dict(threshold=-1.0), dict(threshold=np.nan), dict(threshold=2.5, min_views=1), dict(threshold=2.5, loss="l2"), dict(threshold=2.5, f_scale=0.0),
               dict(threshold=2.5, max_iterations=-1), dict(threshold=2.5, undistort_iterations=-1)):
        with pytest.raises(ValueError):
            m.triangulate_consensus(uvs, ext, intr, device=NO_DEVICE, **kw)
    with pytest.raises(ValueError):
        m.triangulate_consensus(uvs[:2], ext, intr, threshold=2.5, device=NO_DEVICE)
    with pytest.raises(NotImplementedError):
        m.triangulate_consensus(uvs[:1], ext[:1], intr[:1], threshold=2.5, device=NO_DEVICE)
    uv65, ext65, intr65, _ = scene(C=65, P=3, seed=2)
    with pytest.raises(NotImplementedError):
        m.triangulate_consensus(uv65, ext65, intr65, threshold=2.5, device=NO_DEVICE)
    assert m.geometry.CONSENSUS_STATUS[-2] == "no consensus" and set(m.geometry.STATUS.items()) <= set(m.geometry.CONSENSUS_STATUS.items())


def test_no_points_need_no_device():
    uvs, ext, intr, _ = scene(C=4, P=10, seed=2)
    none = [u[:0] for u in uvs]
    pts, inl, info, err = m.triangulate_consensus(none, ext, intr, threshold=2.5, return_info=True, return_errors=True, device=NO_DEVICE)
    assert pts.shape == (0, 3) and inl.shape == (4, 0) and inl.dtype == bool and err.shape == (4, 0)
    assert info["pair"].shape == (0, 2) and all(info[k].shape == (0,) for k in ("n_inliers", "hypothesis_cost", "cost", "cost0", "n_iterations", "status"))
    pts, inl = m.triangulate_consensus(none, ext, intr, threshold=2.5, device=NO_DEVICE)
    assert pts.shape == (0, 3) and inl.shape == (4, 0)


def test_c_entry_point_refuses_bad_arguments_with_a_reason():
    lib = ops.load_library()
    C, P = 3, 4
    uv, cam, out, words = np.zeros((C, P, 2)), np.zeros((C, 12)), np.zeros((P, 3)), np.zeros(P, dtype=np.uint64)

    def call(n_cameras=C, threshold=2.5, min_views=2, und=5, loss=0, f_scale=1.0, max_it=100, uvs=uv, points=out, inliers=words, n_points=P):
        return lib.mcba_triangulate_consensus(n_cameras, n_points, None if uvs is None else uvs.ctypes.data, cam.ctypes.data, None, threshold, min_views, und, loss, f_scale, max_it, NO_DEVICE,
                                              None if points is None else points.ctypes.data, None if inliers is None else inliers.ctypes.data, None, None, None)

    for kw, word in ((dict(n_cameras=1), "cameras"), (dict(n_cameras=65), "cameras"), (dict(threshold=0.0), "threshold"), (dict(threshold=float("nan")), "threshold"), (dict(min_views=1), "min_views"),
                     (dict(loss=5), "loss"), (dict(loss=-1), "loss"), (dict(f_scale=0.0), "f_scale"), (dict(max_it=-1), "iterations"), (dict(und=-1), "iterations"), (dict(uvs=None), "non-NULL"),
                     (dict(points=None), "non-NULL"), (dict(inliers=None), "non-NULL")):
        assert call(**kw) == ops.ERR_ARG, kw
        assert word in lib.mcba_last_error().decode(), (kw, lib.mcba_last_error().decode())
    assert call(n_points=0) == ops.OK                                   # nothing to do: returns before the device
