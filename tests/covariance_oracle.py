"""Numpy statement of the definition of calibration_uncertainty (multicam-calibration_amd/uncertainty.py) -- the reference of
tests/test_hostcheck_covariance.py and tests/test_gpu_covariance.py.

H = J^T diag(w) J with w = rho'((f / f_scale)^2) (oracle.ba_oracle.normal_equations with curv_floor = 1), assembled densely; the six
extrinsics of the gauge camera (and, with fix_intrinsics, the six intrinsics of every camera) are deleted, so are the six columns of a frame
without data; the rest is Jacobi-scaled, factorised with scipy's Cholesky, inverted and unscaled.  sigma2 = sum w f^2 / (m - p) unless sigma
is given.  Also returned: cond_2 of the scaled matrix, which the tests' bound is a multiple of."""
import functools

import numpy as np
import scipy.linalg

from multicam_calibration_amd import synth
from oracle import ba_oracle as bo

EPS = 2.2e-16
BOUND_FACTOR = 64.0   # bound = 64 cond_2(H_scaled) eps: the forward error of inverting a matrix whose entries carry a few eps of summation error

# (C, F, missing, gauge_camera, loss, fix_intrinsics, sigma): the shapes both tiers are held to
CASES = {
    "c2_f4": dict(C=2, F=4),                                                                 # fewer frames than one 64-frame record tile; n = 24 is not a multiple of 16
    "c2_f130": dict(C=2, F=130),                                                             # two full record tiles plus two frames
    "c3_f30_missing_cauchy_gauge2": dict(C=3, F=30, missing=0.3, gauge_camera=2, loss="cauchy"),   # zero W_cf blocks, gauge not on camera 0, a weight far from 1
    "c10_f8": dict(C=10, F=8),                                                               # n = 120: beyond the 9-camera switch of the reduced solve, panel staging
    "c10_f8_fixed_gauge3": dict(C=10, F=8, fix_intrinsics=True, gauge_camera=3),             # the 6-wide camera block (n = 60)
    "c3_f70_missing_linear_sigma": dict(C=3, F=70, missing=0.3, loss="linear", sigma=0.2),   # sigma2 passed in; tile boundary with missing data
    # ---- wide rigs: the natural group switch of k_cov_frames, the panel loop of diag_blocks past two panels, the camera chain past two wavefronts
    "c8_f9": dict(C=8, F=9),                                                                 # n = 96: two panels, the second half wide (wavefronts 2 and 3 idle); F one past a group of 8
    "c16_f7": dict(C=16, F=7),                                                               # n = 192 = ld: no padding, KP - n = 0; F one short of a group
    "c26_f9_gauge25": dict(C=26, F=9, gauge_camera=25),                                      # the last natural G = 8 (152 640 B of LDS), five panels, the gauge on the last camera
    "c27_f5_missing": dict(C=27, F=5, missing=0.3),                                          # the first natural G = 4: six panels, the last half wide; F one past a group of 4
    "c40_f9_missing_huber_fs07": dict(C=40, F=9, missing=0.3, loss="huber", f_scale=0.7),    # the cap, n = 480: eight wavefronts of the factor, eight blocks of k_cov_cam_linv
    "c26_f8_fixed_gauge3": dict(C=26, F=8, fix_intrinsics=True, gauge_camera=3),             # the 6-wide cap: n = 156, KP = 160, ld = 192; F exactly one group
    "c3_f63_arctan_fs05": dict(C=3, F=63, loss="arctan", f_scale=0.5),                       # one short of a lane tile of k_cov_check / a record tile; arctan off scale 1
    "c3_f64_arctan_fs05": dict(C=3, F=64, loss="arctan", f_scale=0.5),
    "c3_f65_arctan_fs05": dict(C=3, F=65, loss="arctan", f_scale=0.5),
    "c2_f15": dict(C=2, F=15),                                                               # F one short of, at and one past two groups of 8
    "c2_f16": dict(C=2, F=16),
    "c2_f17": dict(C=2, F=17),
    "c2_f3": dict(C=2, F=3),                                                                 # with c2_f4: the same edges of one forced group of 4
    "c2_f5": dict(C=2, F=5),
}
# the frames make_case keeps of each new case (its complete-in-two-cameras filter drops none at these seeds): asserted by both tiers
KEPT_FRAMES = {"c8_f9": 9, "c16_f7": 7, "c26_f9_gauge25": 9, "c27_f5_missing": 5, "c40_f9_missing_huber_fs07": 9, "c26_f8_fixed_gauge3": 8, "c3_f63_arctan_fs05": 63,
               "c3_f64_arctan_fs05": 64, "c3_f65_arctan_fs05": 65, "c2_f15": 15, "c2_f16": 16, "c2_f17": 17, "c2_f3": 3, "c2_f5": 5}

LDS_LIMIT = 160 * 1024   # the opt-in LDS of a gfx950 workgroup


def frames_lds(n, G):
    """bytes of LDS k_cov_frames asks for (csrc/mcba_cov.hip, cov_frames_lds): R = 6 G rows of Y at stride KP + 2, the staging buffer of
    diag_blocks (a 32 x 80 chunk of Sigma, later Z as R x 66), V^-1 packed (21) and the output block (36) per frame"""
    KP, R = (n + 31) // 32 * 32, 6 * G
    return 8 * (R * (KP + 2) + max(32 * 80, R * 66) + G * 21 + G * 36)


def expected_group(n, force=0):
    """frames per workgroup of k_cov_frames at n camera-system variables: 8 if its LDS fits, else 4; `force` (MCBA_COV_FRAMES_G) wins if it fits"""
    if force in (4, 8) and frames_lds(n, force) <= LDS_LIMIT:
        return force
    return next((G for G in (8, 4) if frames_lds(n, G) <= LDS_LIMIT), 0)


def expected_ld(n):
    """row stride of the camera block on the device: n rounded up to a multiple of 64"""
    return (n + 63) // 64 * 64


def make_case(C, F, missing=0.0, gauge_camera=0, loss="soft_l1", fix_intrinsics=False, sigma=None, f_scale=1.0):
    """synth.make_problem at N = 54, the frames seen complete by at least two cameras, the TRUE parameters."""
    p = synth.make_problem(C, F, missing=missing)
    keep = np.nonzero((~np.isnan(p["uvs"]).any((-1, -2))).sum(0) > 1)[0]
    uvs = np.ascontiguousarray(p["uvs"][:, keep])
    cam, poses = p["true_cam"], p["true_poses"][keep]
    ext = cam[:, 6:].copy()
    intr = []
    for c in range(C):
        K = np.eye(3)
        K[0, 0], K[1, 1], K[0, 2], K[1, 2] = cam[c, :4]
        intr.append((K, np.array([cam[c, 4], cam[c, 5], 0.0, 0.0, 0.0])))
    return dict(uvs=uvs, obj=p["obj"], extrinsics=ext, intrinsics=intr, poses=poses, x=np.concatenate([cam.ravel(), poses.ravel()]),
                kwargs=dict(gauge_camera=gauge_camera, loss=loss, f_scale=f_scale, fix_intrinsics=fix_intrinsics, sigma=sigma))


def held_camera_params(C, gauge_camera, fix_intrinsics):
    held = np.zeros(12 * C, bool)
    held[12 * gauge_camera + 6 : 12 * gauge_camera + 12] = True
    if fix_intrinsics:
        held.reshape(C, 12)[:, :6] = True
    return held


def covariance(x, uvs, obj, gauge_camera=0, loss="soft_l1", f_scale=1.0, fix_intrinsics=False, sigma=None):
    C, F = uvs.shape[:2]
    U, gc, V, gf, W, cost = bo.normal_equations(x, uvs, obj, loss, f_scale, curv_floor=1.0)
    nc = 12 * C
    H = np.zeros((nc + 6 * F, nc + 6 * F))
    for c in range(C):
        H[12 * c : 12 * c + 12, 12 * c : 12 * c + 12] = U[c]
    for f in range(F):
        s = slice(nc + 6 * f, nc + 6 * f + 6)
        H[s, s] = V[f]
        for c in range(C):
            H[12 * c : 12 * c + 12, s] = W[c, f]
            H[s, 12 * c : 12 * c + 12] = W[c, f].T
    nodata = np.isnan(uvs).all((0, 2, 3))
    free = np.concatenate([~held_camera_params(C, gauge_camera, fix_intrinsics), np.repeat(~nodata, 6)])
    idx = np.nonzero(free)[0]
    Hs = H[np.ix_(idx, idx)]
    d = np.sqrt(np.diagonal(Hs))
    A = Hs / np.outer(d, d)
    cond = float(np.linalg.cond(A))
    inv = scipy.linalg.cho_solve(scipy.linalg.cho_factor(A, lower=True), np.eye(len(idx))) / np.outer(d, d)
    inv = 0.5 * (inv + inv.T)

    valid = ~np.isnan(uvs)
    fres = np.where(valid, uvs - bo.predict_from_x(x, C, obj), 0.0)
    w = bo.loss_rho((fres / f_scale) ** 2, loss)[1]
    m, p = int(valid.sum()), len(idx)
    if sigma is not None:
        sigma2 = float(sigma) ** 2
    else:
        sigma2 = float(np.sum(np.where(valid, w * fres * fres, 0.0)) / (m - p)) if m > p else float("nan")

    full = np.zeros_like(H)
    full[np.ix_(idx, idx)] = sigma2 * inv
    cam_cov = full[:nc, :nc]
    pose_cov = np.stack([full[nc + 6 * f : nc + 6 * f + 6, nc + 6 * f : nc + 6 * f + 6] for f in range(F)])
    pose_cov[nodata] = np.nan
    std = np.sqrt(np.diagonal(cam_cov)).reshape(C, 12)
    return dict(camera_covariance=cam_cov, pose_covariance=pose_cov, intrinsics_std=std[:, :6], extrinsics_std=std[:, 6:], pose_std=np.sqrt(np.diagonal(pose_cov, axis1=1, axis2=2)),
                sigma2=sigma2, n_residuals=m, n_free=p, cond=cond, bound=BOUND_FACTOR * cond * EPS, U=U, V=V, W=W, held=held_camera_params(C, gauge_camera, fix_intrinsics), nodata=nodata)


def noise_scale(x, uvs, obj, gauge_camera=0, loss="soft_l1", f_scale=1.0, fix_intrinsics=False, sigma=None):
    """(sigma2, m, p) from the residuals alone -- sum w f^2 / (m - p), no dense H: the reference of k_cov_wss at sizes `covariance` cannot hold"""
    C, F = uvs.shape[:2]
    valid = ~np.isnan(uvs)
    f = np.where(valid, uvs - bo.predict_from_x(x, C, obj), 0.0)
    w = bo.loss_rho((f / f_scale) ** 2, loss)[1]
    m = int(valid.sum())
    p = int((~held_camera_params(C, gauge_camera, fix_intrinsics)).sum()) + 6 * int((~np.isnan(uvs).all((0, 2, 3))).sum())
    return float(np.sum(np.where(valid, w * f * f, 0.0), dtype=np.longdouble) / (m - p)), m, p


def inverse_longdouble(A):
    """the inverse of a symmetric positive definite matrix in np.longdouble: Cholesky A = L L^T, L^-1 by forward substitution, L^-T L^-1"""
    A = np.asarray(A, dtype=np.longdouble)
    n = len(A)
    L = np.zeros_like(A)
    for j in range(n):
        d = A[j, j] - L[j, :j] @ L[j, :j]
        if not d > 0:
            raise np.linalg.LinAlgError(f"pivot {j} is not positive")
        L[j, j] = np.sqrt(d)
        L[j + 1 :, j] = (A[j + 1 :, j] - L[j + 1 :, :j] @ L[j, :j]) / L[j, j]
    Li = np.zeros_like(A)
    for j in range(n):
        Li[j, j] = 1 / L[j, j]
        for i in range(j + 1, n):
            Li[i, j] = -(L[i, j:i] @ Li[j:i, j]) / L[i, i]
    return Li.T @ Li


def camera_reference(S0, held, sigma2):
    """sigma2 S_g^-1 of the device's own Schur complement S0 (n x n, its upper triangle: what k_cov_cam_factor reads), the held rows and columns
    deleted and reported as zeros, Jacobi-scaled, inverted in long double.  Returns (covariance as float64, cond_2 of the scaled matrix)."""
    S = np.triu(S0) + np.triu(S0, 1).T
    idx = np.flatnonzero(~held)
    A = S[np.ix_(idx, idx)]
    d = np.sqrt(np.diagonal(A))
    As = A / np.outer(d, d)
    inv = inverse_longdouble(As) / np.outer(d, d).astype(np.longdouble)
    full = np.zeros(S.shape)
    full[np.ix_(idx, idx)] = (sigma2 * inv).astype(np.float64)
    return full, float(np.linalg.cond(As))


# The frame stage alone: Sigma_ff = sigma2 V_f^-1 + V_f^-1 W_f^T Sigma_cc W_f V_f^-1 from a GIVEN camera covariance.  Its error does not carry
# cond_2(H): the only inverse is the 6 x 6 one, so the bound is a multiple of cond_2 of the Jacobi-scaled V_f.  The multiple, by the rule of
# BOUND_FACTOR (module docstring of tests/test_gpu_covariance.py), is measured without the code under test: the spread of two float64 numpy
# evaluations of the same formula (cho_solve of the scaled V_f; numpy's explicit inverse of the unscaled one) around the long-double one, times the
# margin of 25 for a different order of additions (the 4-deep MFMA chunks of diag_blocks).  Over every case of CASES the spread is at most
# 17.0 cond_2(V_f) eps (explicit inverse: 17.0 on "c40_f9_missing_huber_fs07", 16.3 on "c2_f4", 14.2 on "c27_f5_missing"; cho_solve: 11.6 on "c16_f7", 10.3 on
# "c27_f5_missing") -- far from 1 because Y Sigma_cc Y^T sums over a camera covariance whose entries span twelve orders of magnitude and cancel.
# Rounded up: FRAME_HOST_SPREAD = 18, FRAME_BOUND_FACTOR = 25 x 18 = 450 (tests/test_hostcheck_covariance.py::test_frame_stage_host_spread prints the
# spread per case and holds it to 18).  cond_2 of the scaled V_f is 20 .. 55 where cond_2 of the scaled H is 2e4 .. 4e8: the bound is 2e-12 .. 6e-12
# against 3e-10 .. 5e-6, two orders below 64 cond_2(H) eps on the 6-wide cases and four to six on the others.  Neither number was tuned against a GPU.
FRAME_HOST_SPREAD = 18.0
FRAME_BOUND_FACTOR = 25.0 * FRAME_HOST_SPREAD


def frame_system_rows(C, fix_intrinsics):
    return (12 * np.arange(C)[:, None] + 6 + np.arange(6)[None, :]).ravel() if fix_intrinsics else np.arange(12 * C)


def frame_reference(o, camera_covariance, sigma2, dtype=np.longdouble, how="cholesky"):
    """(blocks (F, 6, 6) as float64, cond_2 of the scaled V_f (F,)) of the frame stage from the oracle's V, W and a given (12 C, 12 C) camera
    covariance; NaN for a frame without data.  dtype float64 with how = "cho_solve" / "inverse": the host evaluations the spread is measured with."""
    V, W = o["V"], o["W"]
    C, F = W.shape[:2]
    Wf = W.transpose(1, 0, 2, 3).reshape(F, 12 * C, 6)
    S = np.asarray(camera_covariance, dtype=dtype)
    out, cond = np.full((F, 6, 6), np.nan), np.full(F, np.nan)
    for f in np.flatnonzero(~o["nodata"]):
        d = np.sqrt(np.diagonal(V[f]))
        Vs = V[f] / np.outer(d, d)
        cond[f] = np.linalg.cond(Vs)
        if dtype is np.longdouble:
            Vi = inverse_longdouble(Vs) / np.outer(d, d).astype(dtype)
        elif how == "cho_solve":
            Vi = scipy.linalg.cho_solve(scipy.linalg.cho_factor(Vs, lower=True), np.eye(6)) / np.outer(d, d)
        else:
            Vi = np.linalg.inv(V[f])
        Y = Vi @ Wf[f].astype(dtype).T
        blk = sigma2 * Vi + Y @ S @ Y.T
        out[f] = (0.5 * (blk + blk.T)).astype(np.float64)
    return out, cond


def frame_stage_error(got, ref, cond):
    """max over the frames with data of rel_err(got_f, ref_f) / (cond_f EPS): the frame stage's error in units of cond_2(V_f) eps"""
    keep = np.flatnonzero(~np.isnan(cond))
    return max(rel_err(got[f], ref[f]) / (cond[f] * EPS) for f in keep)


@functools.lru_cache(maxsize=None)
def case(name):
    """(problem, oracle) of CASES[name], computed once per process and shared: leave both unchanged."""
    pr = make_case(**CASES[name])
    return pr, covariance(pr["x"], pr["uvs"], pr["obj"], **pr["kwargs"])


def rel_err(got, ref):
    """max |got - ref| / sqrt(ref_ii ref_jj) over the entries whose two variances are positive (square matrices, or stacks of them)."""
    got, ref = np.asarray(got), np.asarray(ref)
    d = np.sqrt(np.diagonal(ref, axis1=-2, axis2=-1))
    scale = d[..., :, None] * d[..., None, :]
    ok = scale > 0
    return float(np.max(np.abs(got - ref)[ok] / scale[ok])) if ok.any() else 0.0


def rel_err_std(got, ref):
    """max |got - ref| / ref over the entries whose reference is positive; where it is 0 (a held parameter) `got` must be 0 exactly"""
    got, ref = np.asarray(got), np.asarray(ref)
    ok = ref > 0
    assert (got[ref == 0] == 0.0).all()
    return float(np.max(np.abs(got - ref)[ok] / ref[ok])) if ok.any() else 0.0
