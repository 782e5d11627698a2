"""refine_cameras without a GPU: what is refused before any device is touched, the packing of the free mask and the held bits, the prior's cost and
gradient (the header's functions, compiled with g++) against finite differences, and kpcam_oracle.solve12 against kpba_oracle.solve where nothing
intrinsic is free."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import kpba_oracle as ko
import kpcam_oracle as kc
from multicam_calibration_amd import geometry
from multicam_calibration_amd.geometry import refine_cameras, refine_cameras_system

HERE = os.path.dirname(os.path.abspath(__file__))


def small(C=3, P=12):
    uvs, ext, intr, X = ko.scene(C=C, P=P, seed=5, noise=0.3, p_unseen=0.0)
    return [np.array(u) for u in uvs], np.array(ext), intr, np.array(X)


def test_exports():
    import multicam_calibration_amd as m

    for name in ("refine_cameras", "CameraRefinement"):
        assert getattr(m, name) is getattr(geometry, name) and name in m.__all__
    assert hasattr(geometry, "refine_cameras_system")


def test_thirteen_cameras_are_refused_with_the_way_out():
    uvs, ext, intr, X = small(C=13, P=4)
    with pytest.raises(NotImplementedError, match=r'refine_extrinsics\(reduction="tiled"\)'):
        refine_cameras(uvs, ext, intr, points=X)
    with pytest.raises(NotImplementedError, match="2 to 12 cameras"):
        refine_cameras_system(uvs, ext, intr, points=X, held=np.zeros((13, 12), bool), lam=0.0)
    with pytest.raises(NotImplementedError):
        refine_cameras(uvs[:1], ext[:1], intr[:1], points=X)


@pytest.mark.parametrize("bad", [("focus",), "principle", ("focal", 3), np.ones((3, 5), bool), np.ones((3, 6)), np.ones((2, 6), bool)])
def test_bad_free_intrinsics(bad):
    uvs, ext, intr, X = small()
    with pytest.raises(ValueError, match="free_intrinsics"):
        refine_cameras(uvs, ext, intr, points=X, free_intrinsics=bad)


@pytest.mark.parametrize("bad", [np.zeros(6), -np.ones(6), np.r_[1.0, np.nan, 1, 1, 1, 1], np.ones(5), np.ones((2, 6)), np.full(6, 1e-200)])
def test_bad_prior_std(bad):
    uvs, ext, intr, X = small()
    with pytest.raises(ValueError, match="intrinsics_prior_std"):
        refine_cameras(uvs, ext, intr, points=X, intrinsics_prior_std=bad)


def test_what_refine_extrinsics_refuses_is_refused():
    uvs, ext, intr, X = small()
    for kw in (dict(loss="l2"), dict(f_scale=0.0), dict(max_nfev=1), dict(ftol=-1.0), dict(gauge_camera=3), dict(gauge_camera=1, scale_camera=1), dict(points=X[:5]),
               dict(inliers=np.ones((3, 11), bool)), dict(weights=-np.ones((3, 12)))):
        with pytest.raises(ValueError):
            refine_cameras(uvs, ext, intr, **{"points": X, **kw})
    with pytest.raises(ValueError, match="held"):
        refine_cameras_system(uvs, ext, intr, points=X, held=np.zeros((3, 6), bool), lam=0.0)
    with pytest.raises(ValueError, match="step"):
        refine_cameras_system(uvs, ext, intr, points=X, held=np.zeros((3, 12), bool), lam=0.0, step=(np.zeros((3, 6)), np.zeros((3, 6))))


def test_free_mask_and_bit_packing():
    f = geometry._free_intrinsics_mask
    assert not f((), 4).any() and f("focal", 2).tolist() == [[True, True, False, False, False, False]] * 2
    assert f(["distortion", "principal"], 1).tolist() == [[False, False, True, True, True, True]]
    assert f(("focal", "principal", "distortion"), 3).all()
    m = np.zeros((3, 6), bool)
    m[1, 0] = m[2, 5] = True
    got = f(m, 3)
    assert np.array_equal(got, m) and got is not m
    for groups in ((), ("focal",), ("principal", "distortion")):
        assert np.array_equal(f(groups, 3), kc.free_mask(3, groups))
    held = np.zeros((3, 12), bool)
    held[0, 6:] = True
    held[1, 9] = True
    held[2] = [False, True] * 6
    bits = geometry._held_bits12(held, 3)
    assert bits.dtype == np.int32 and bits.tolist() == [0xFC0, 1 << 9, 0b101010101010] and np.array_equal(bits, kc.held_bits12(held))
    assert geometry._held_bits12(bits, 3) is not None and np.array_equal(geometry._held_bits12(bits, 3), bits)
    assert np.array_equal(((bits[:, None] >> np.arange(12)) & 1).astype(bool), held)


def test_prior_weights():
    w = geometry._prior_weights
    assert w(None, 3) is None
    std = np.array([4.0, 5.0, 2.0, np.inf, 0.5, 0.005])
    assert np.array_equal(w(std, 2), np.tile(1 / std ** 2, (2, 1))) and w(std, 2)[0, 3] == 0.0
    full = np.arange(1.0, 19.0).reshape(3, 6)
    assert np.array_equal(w(full, 3), 1 / full ** 2) and w(full, 3).flags.c_contiguous


def test_intrinsics_come_back_in_the_format_given():
    K = np.array([[900.0, 0, 640], [0, 905, 512], [0, 0, 1]])
    t = np.array([910.0, 911, 641, 513, -0.11, 0.03])
    for d in (np.array([-0.1, 0.02, 1e-3, -5e-4, 0.01]), np.array([[-0.1, 0.02, 1e-3, -5e-4, 0.01]]), np.array([-0.1, 0.02, 1e-3, -5e-4]), np.zeros(5)):
        (K2, d2), = geometry._intrinsics_like([(K, d)], [t])
        assert K2[0, 0] == 910 and K2[1, 1] == 911 and K2[0, 2] == 641 and K2[1, 2] == 513 and K2[0, 1] == 0 and K[0, 0] == 900
        assert d2.shape == d.shape and np.array_equal(d2.ravel()[:2], t[4:]) and np.array_equal(d2.ravel()[2:], d.ravel()[2:]) and d.ravel()[0] in (-0.1, 0.0)


@pytest.fixture(scope="module")
def hc(tmp_path_factory):
    lib = str(tmp_path_factory.mktemp("kpcam_cpu") / "libkpcam_hostcheck.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-o", lib, os.path.join(HERE, "hostcheck", "kpcam_hostcheck.cpp")])
    h = ctypes.CDLL(lib)
    h.hc_kpcam_prior_cost.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 4
    h.hc_kpcam_prior_cost.restype = ctypes.c_double
    h.hc_kpcam_prior_gradient.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    h.hc_kpcam_prior_gradient.restype = ctypes.c_double
    return h


def test_prior_cost_and_gradient_against_finite_differences(hc):
    """the header's prior (what kpcam_lm adds to the cost and to the gradient) against the oracle's statement and central differences of it"""
    rng = np.random.default_rng(11)
    C = 3
    theta0 = np.concatenate([np.tile([900.0, 905, 640, 512, -0.1, 0.02], (C, 1)), rng.normal(size=(C, 6))], axis=1)
    theta = theta0 + rng.normal(size=(C, 12)) * np.r_[4, 4, 2, 2, 0.005, 0.005, np.ones(6)]
    std = kc.prior_std_of(theta0[:, :6])
    std[1, 2] = np.inf
    pw = np.ascontiguousarray(geometry._prior_weights(std, C))
    held = np.zeros((C, 12), bool)
    held[2, 0] = held[0, 6:] = True
    bits = kc.held_bits12(held)
    A = lambda a: ctypes.c_void_p(a.ctypes.data)   # noqa: E731
    cost = lambda th: hc.hc_kpcam_prior_cost(C, A(bits), A(pw), A(np.ascontiguousarray(th)), A(theta0))   # noqa: E731
    ref = kc.prior_cost(theta[:, :6], theta0[:, :6], std, held)
    print(f"prior cost {cost(theta):.15g} oracle {ref:.15g}")
    assert abs(cost(theta) / ref - 1) <= 1e-14 and cost(theta0) == 0.0 and hc.hc_kpcam_prior_cost(C, A(bits), None, A(theta), A(theta0)) == 0.0
    for k in range(12 * C):
        c, i = divmod(k, 12)
        g = hc.hc_kpcam_prior_gradient(A(pw), k, A(theta), A(theta0))
        h = 1e-4 * max(1.0, abs(theta[c, i]))
        up, dn = theta.copy(), theta.copy()
        up[c, i] += h
        dn[c, i] -= h
        fd = (cost(up) - cost(dn)) / (2 * h)   # (exact for a quadratic but for rounding)
        if held[c, i] and i < 6:
            assert fd == 0.0   # a held scalar has no prior cost; the loop never asks for its gradient
            continue
        assert abs(g - fd) <= 1e-9 * max(1.0, abs(g)), (k, g, fd)
        assert (g == 0.0) == (i >= 6 or not np.isfinite(std[c, i]))


def test_solve12_with_nothing_free_is_kpba_oracle_solve():
    uvs, ext, intr, X = ko.make_scene("c2")
    e0, p0 = ko.perturbed_start(ext, X, 0, 2001)
    a = ko.solve(uvs, e0, intr, p0)
    b = kc.solve12(uvs, e0, intr, kc.theta6_of(intr), p0, kc.free_mask(2, ()))
    print(f"extrinsics {ko.relative_spread(a['extrinsics'], b['extrinsics']):.3g} cost {a['cost']:.15g} {b['cost']:.15g}")
    assert np.array_equal(b["held"][:, 6:], a["held"]) and b["held"][:, :6].all() and b["prior_cost"] == 0.0
    assert ko.relative_spread(a["extrinsics"], b["extrinsics"]) <= 1e-9 and abs(a["cost"] / b["cost"] - 1) <= 1e-12 and np.array_equal(b["theta6"], kc.theta6_of(intr))
    with pytest.raises(ValueError):
        kc.solve12(uvs, e0, intr, kc.theta6_of(intr), p0, kc.free_mask(2, ("focal",)), prior_std=kc.prior_std_of(kc.theta6_of(intr)), loss="soft_l1")
