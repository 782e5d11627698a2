"""Per-detection weights without a GPU: the keyword exists on the five functions, and what is refused is refused on the
host -- by the Python layer (ValueError: a wrong shape, a negative or an infinite weight, weights= without refine=True) and by the C ABI before
it touches a device (MCBA_ERR_ARG)."""
import inspect

import numpy as np
import pytest

import multicam_calibration_amd as m
from test_triangulate_cpu import scene


def test_the_keyword_exists_and_defaults_to_none():
    for fn in (m.triangulate, m.refine_triangulation, m.triangulation_uncertainty, m.refine_extrinsics, m.geometry.refine_extrinsics_system):
        p = inspect.signature(fn).parameters["weights"]
        assert p.default is None and p.kind is inspect.Parameter.KEYWORD_ONLY, fn.__name__
    lib = m.ops.load_library()
    for name in ("mcba_triangulate_refine_weighted", "mcba_triangulation_covariance_weighted", "mcba_refine_extrinsics_weighted", "mcba_refine_extrinsics_system_weighted"):
        assert hasattr(lib, name)
    assert lib.mcba_abi_version() == 7


def test_refusals_on_the_host():
    uvs, ext, intr, X = scene(C=3, P=20, seed=1, noise=0.3, p_unseen=0.1)
    w = np.ones((3, 20))
    bad_planes = ((w[:, :-1], "weights must be"), (w.T, "weights must be"), (-w, "not negative"), (np.where(np.arange(20) == 3, np.inf, w), "finite"))
    for bad, why in bad_planes:
        with pytest.raises(ValueError, match=why):
            m.refine_triangulation(X, uvs, ext, intr, weights=bad)
        with pytest.raises(ValueError, match=why):
            m.triangulate(uvs, ext, intr, refine=True, weights=bad)
        with pytest.raises(ValueError, match=why):
            m.triangulation_uncertainty(X, uvs, ext, intr, weights=bad)
        with pytest.raises(ValueError, match=why):
            m.refine_extrinsics(uvs, ext, intr, points=X, weights=bad)
        with pytest.raises(ValueError, match=why):
            m.geometry.refine_extrinsics_system(uvs, ext, intr, points=X, held=np.zeros(3, np.int32), lam=0.0, weights=bad)
    for kw in ({}, {"refine": False}):
        with pytest.raises(ValueError, match="refine=True"):
            m.triangulate(uvs, ext, intr, weights=w, **kw)


def test_the_c_abi_refuses_before_it_touches_a_device():
    uvs, ext, intr, X = scene(C=3, P=20, seed=1, noise=0.3, p_unseen=0.1)
    lib, ops = m.ops.load_library(), m.ops
    uv = np.ascontiguousarray(np.stack(uvs))
    cam, dist = m.triangulation._cam_blocks(ext, intr)
    pts, out = np.ascontiguousarray(X), np.empty((20, 3))
    a = lambda x: x.ctypes.data   # noqa: E731
    for bad in (-np.ones((3, 20)), np.full((3, 20), np.inf)):
        assert lib.mcba_triangulate_refine_weighted(3, 20, a(uv), a(bad), a(cam), a(dist), a(pts), 0, 0, 1.0, 10, 0, a(out), None, None) == ops.ERR_ARG
        assert b"weights" in lib.mcba_last_error()
        det, views, status, info = np.empty((20, 6)), np.empty(20, np.int32), np.empty(20, np.int32), np.zeros(8)
        assert lib.mcba_triangulation_covariance_weighted(3, 20, a(pts), a(uv), a(bad), a(cam), a(dist), None, 0, 1.0, 1.0, 0, a(det), None, a(views), a(status), a(info), None) == ops.ERR_ARG
        held, e, res, hist = np.zeros(3, np.int32), np.empty((3, 6)), np.zeros(16), np.zeros((4, 3))
        assert lib.mcba_refine_extrinsics_weighted(3, 20, a(uv), a(bad), a(cam), a(dist), a(pts), a(held), 0, 1, 0, 1.0, 1e-8, 1e-8, 1e-8, 3, 0, a(e), a(out), a(status), a(res), a(hist), 4) == ops.ERR_ARG
        system = np.empty(32 * 32 + 33 * 3 + 4)
        assert lib.mcba_refine_extrinsics_system_weighted(3, 20, a(uv), a(bad), a(cam), a(dist), a(pts), a(held), 0, 1.0, 0.0, 0, None, None, a(status), a(system), None, None, a(np.zeros(4))) == ops.ERR_ARG
