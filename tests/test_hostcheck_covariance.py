"""csrc/mcba_cov_math.h -- the per-lane text of the covariance kernels (csrc/mcba_cov.hip) -- compiled with g++ (tests/hostcheck/cov_hostcheck.cpp,
plain -O2) and held, without a GPU, to the bound of the GPU tier (tests/test_gpu_covariance.py) against tests/covariance_oracle.py at the same
shapes: max |Sigma - Sigma_ref| / sqrt(Sigma_ref,ii Sigma_ref,jj) <= 64 cond_2(H_scaled) 2.2e-16 for the camera block and every frame block.
The Schur complement the camera routine starts from, and the frame blocks' inputs, are the oracle's U, V, W."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import covariance_oracle as cvo

HERE = os.path.dirname(os.path.abspath(__file__))


def P(a):
    return ctypes.c_void_p(a.ctypes.data)


@pytest.fixture(scope="module")
def hc(tmp_path_factory):
    src = os.path.join(HERE, "hostcheck", "cov_hostcheck.cpp")
    lib = str(tmp_path_factory.mktemp("cov_hostcheck") / "libcov_hostcheck.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-o", lib, src])
    h = ctypes.CDLL(lib)
    h.hc_cov_cameras.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_double, ctypes.c_void_p]
    h.hc_cov_frames.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p]
    h.hc_cov_frames.restype = None
    return h


def system_rows(C, cw):
    """positions in the 12 C camera parameters of the camera system's variables (ops.Problem.cam_index)"""
    return np.arange(12 * C) if cw == 12 else (12 * np.arange(C)[:, None] + 6 + np.arange(6)[None, :]).ravel()


def host_covariance(hc, o, C, F, cw, gauge, sigma2):
    """the host build's camera covariance (12 C x 12 C, zeros where held) and frame blocks from the oracle's U, V, W"""
    rows = system_rows(C, cw)
    n = len(rows)
    S = np.zeros((12 * C, 12 * C))
    for c in range(C):
        S[12 * c : 12 * c + 12, 12 * c : 12 * c + 12] = o["U"][c]
    Wf = np.ascontiguousarray(o["W"].transpose(1, 0, 2, 3).reshape(F, 12 * C, 6))   # (F, 12 C, 6)
    for f in range(F):
        if not o["nodata"][f]:
            S -= Wf[f] @ np.linalg.solve(o["V"][f], Wf[f].T)
    S = np.ascontiguousarray(S[np.ix_(rows, rows)])
    cam = np.empty((n, n))
    assert hc.hc_cov_cameras(n, cw, gauge, P(S), sigma2, P(cam)) == -1
    W = np.ascontiguousarray(Wf[:, rows])
    V = np.ascontiguousarray(o["V"])
    fr, flag = np.empty((F, 6, 6)), np.empty(F, np.int32)
    hc.hc_cov_frames(F, n, P(V), P(W), P(cam), sigma2, P(fr), P(flag))
    full = np.zeros((12 * C, 12 * C))
    full[np.ix_(rows, rows)] = cam
    return full, fr, flag


@pytest.mark.parametrize("name", sorted(cvo.CASES))
def test_host_build_matches_the_oracle(hc, name):
    pr, o = cvo.case(name)
    C, F = pr["uvs"].shape[:2]
    assert F == cvo.KEPT_FRAMES.get(name, F)
    kw = pr["kwargs"]
    cam, fr, flag = host_covariance(hc, o, C, F, 6 if kw["fix_intrinsics"] else 12, kw["gauge_camera"], o["sigma2"])
    e_cam, e_fr = cvo.rel_err(cam, o["camera_covariance"]), cvo.rel_err(fr, o["pose_covariance"])
    e_std = cvo.rel_err_std(np.sqrt(np.diagonal(cam)), np.sqrt(np.diagonal(o["camera_covariance"])))
    print(f"{name}: cond {o['cond']:.3g} bound {o['bound']:.3g} cameras {e_cam:.3g} frames {e_fr:.3g} std {e_std:.3g}  (in units of cond eps: {e_cam / (o['cond'] * cvo.EPS):.2f} / {e_fr / (o['cond'] * cvo.EPS):.2f})")
    assert (flag == 0).all()
    assert e_cam <= o["bound"] and e_fr <= o["bound"] and e_std <= o["bound"]
    # exact properties of the arithmetic itself
    assert np.array_equal(cam, cam.T) and np.array_equal(fr, fr.transpose(0, 2, 1))
    assert (cam[o["held"]] == 0.0).all() and (cam[:, o["held"]] == 0.0).all()
    assert (np.linalg.eigvalsh(fr) > 0).all()
    # the frame stage alone, from the host build's own camera covariance: in units of cond_2(V_f) eps (covariance_oracle.FRAME_BOUND_FACTOR)
    ref, cond_v = cvo.frame_reference(o, cam, o["sigma2"])
    e_stage = cvo.frame_stage_error(fr, ref, cond_v)
    print(f"{name}: frame stage {e_stage:.3g} cond(V_f) eps (bound {cvo.FRAME_BOUND_FACTOR:g}), cond(V_f) {np.nanmin(cond_v):.3g} .. {np.nanmax(cond_v):.3g}")
    assert e_stage <= cvo.FRAME_BOUND_FACTOR


@pytest.mark.parametrize("name", sorted(cvo.CASES))
def test_frame_stage_host_spread(name):
    """the number FRAME_BOUND_FACTOR is 25 times of: two float64 numpy evaluations of the frame-stage formula against the long-double one, in
    units of cond_2(V_f) eps, and the long-double one against the oracle's own blocks within the oracle's bound"""
    pr, o = cvo.case(name)
    ref, cond_v = cvo.frame_reference(o, o["camera_covariance"], o["sigma2"])
    spread = [cvo.frame_stage_error(cvo.frame_reference(o, o["camera_covariance"], o["sigma2"], np.float64, how)[0], ref, cond_v) for how in ("cho_solve", "inverse")]
    good = ~o["nodata"]
    e_oracle = cvo.rel_err(ref[good], o["pose_covariance"][good])
    print(f"{name}: cho_solve {spread[0]:.3g} inverse {spread[1]:.3g} cond(V_f) eps; long double against the oracle {e_oracle:.3g} (bound {o['bound']:.3g})")
    assert max(spread) <= cvo.FRAME_HOST_SPREAD and cvo.FRAME_BOUND_FACTOR == 25 * cvo.FRAME_HOST_SPREAD == 450
    assert e_oracle <= o["bound"]
    assert cvo.FRAME_BOUND_FACTOR * np.nanmax(cond_v) <= 0.02 * cvo.BOUND_FACTOR * o["cond"]   # the stage bound is what it is for: far below the end-to-end one


def test_expected_group_switches_where_the_lds_formula_says():
    """k_cov_frames takes 8 frames per workgroup up to n = 312 (26 cameras: 152 640 B of the 160 KiB) and 4 from n = 324 (164 928 B) to the cap;
    every 6-wide system (at most 26 cameras, n = 156) takes 8; a forced group wins where it fits"""
    assert cvo.frames_lds(312, 8) == 152640 and cvo.frames_lds(324, 8) == 164928 and cvo.LDS_LIMIT == 163840
    for C in range(2, 41):
        assert cvo.expected_group(12 * C) == (8 if 12 * C <= 312 else 4), C
    for C in range(2, 27):
        assert cvo.expected_group(6 * C) == 8, C
    assert cvo.expected_group(24, force=4) == 4 and cvo.expected_group(120, force=4) == 4 and cvo.expected_group(480, force=8) == 4 and cvo.expected_group(480, force=5) == 4
    assert [cvo.expected_ld(n) for n in (24, 96, 156, 192, 312, 324, 480)] == [64, 128, 192, 192, 320, 384, 512]


def test_long_double_inverse():
    """inverse_longdouble on a Hilbert-like matrix against numpy's float64 inverse (cond 5e5: agreement to cond eps), and A A^-1 = I in long double"""
    n = 6
    A = 1.0 / (np.arange(n)[:, None] + np.arange(n)[None, :] + 1.0) + np.eye(n) * 1e-3
    Ai = cvo.inverse_longdouble(A)
    assert np.abs(Ai @ A.astype(np.longdouble) - np.eye(n)).max() <= 1e-13
    assert np.abs(Ai.astype(np.float64) - np.linalg.inv(A)).max() <= 1e-9 * np.abs(Ai).max()
    with pytest.raises(np.linalg.LinAlgError):
        cvo.inverse_longdouble(np.array([[1.0, 2.0], [2.0, 1.0]]))


def test_frame_without_data_and_failing_pivot(hc):
    """a frame whose V is zero gets a NaN block and flag 1; one that is not positive definite but holds data flag 2; an indefinite Schur complement
    names its pivot"""
    pr, o = cvo.case("c2_f4")
    n = 24
    V = np.ascontiguousarray(o["V"]).copy()
    W = np.ascontiguousarray(o["W"].transpose(1, 0, 2, 3).reshape(4, n, 6)).copy()
    V[1] = 0.0
    W[1] = 0.0
    V[2, 3, 3] = -1.0
    cam = np.ascontiguousarray(o["camera_covariance"])
    fr, flag = np.empty((4, 6, 6)), np.empty(4, np.int32)
    hc.hc_cov_frames(4, n, P(V), P(W), P(cam), o["sigma2"], P(fr), P(flag))
    assert flag.tolist() == [0, 1, 2, 0]
    assert np.isnan(fr[1]).all() and np.isnan(fr[2]).all() and np.isfinite(fr[[0, 3]]).all()
    S = np.eye(n)
    S[13, 13] = -2.0
    out = np.empty((n, n))
    assert hc.hc_cov_cameras(n, 12, 0, P(S), 1.0, P(out)) == 13
    S[13, 13] = 1.0
    S[14, 15] = S[15, 14] = 2.0   # positive diagonal, indefinite: the factorisation finds it at pivot 15
    assert hc.hc_cov_cameras(n, 12, 0, P(S), 1.0, P(out)) == 15
