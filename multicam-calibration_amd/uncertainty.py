"""calibration_uncertainty -- how good a calibration is: the covariance of the camera parameters and of every board pose at the point
`bundle_adjust()` returned (or at any other), computed on the GPU from the Schur system of one linearisation.

The reference has no counterpart: scipy's OptimizeResult carries `jac` and leaves inverting J^T J to the user -- which is exactly singular
(the 6-DoF gauge freedom) and 60 072 x 60 072 at the size this package exists for.  OpenCV users know the result as calibrateCameraExtended's
stdDeviationsIntrinsics / stdDeviationsExtrinsics.

triangulation_uncertainty -- how good a triangulated point is: per point, the 3 x 3 covariance from the detection noise and, given the camera
covariance above, from the uncertainty of the calibration."""
import ctypes
import warnings
from dataclasses import dataclass

import numpy as np

from . import ops
from .api import serialize_params
from .geometry import _keypoint_inputs, _weight_plane

MAX_CAMERAS = 40   # the dense handle's limit (ops.Problem); the sparse-Schur handle of wider rigs is not covered yet


@dataclass
class CalibrationUncertainty:
    camera_covariance: np.ndarray    # (12C, 12C), column order of result.x's camera part; zero rows / columns for held parameters
    intrinsics_std: np.ndarray       # (C, 6): fx fy cx cy k1 k2
    extrinsics_std: np.ndarray       # (C, 6): rotation vector, translation
    camera_correlation: np.ndarray   # (12C, 12C); NaN where a standard deviation is 0
    pose_covariance: object          # (F, 6, 6), NaN for a frame without data; None with frame_covariance=False
    pose_std: object                 # (F, 6)
    sigma2: float
    n_residuals: int
    n_free: int
    info: dict                       # n_degenerate_frames, kernel_ms, group (frames per workgroup of k_cov_frames; 0 without frame blocks), ld (row stride of the camera block on the device)


def calibration_uncertainty(all_calib_uvs, all_extrinsics, all_intrinsics, calib_objpoints, calib_poses, *, gauge_camera=0, loss="soft_l1", f_scale=1.0, sigma=None,
                            fix_intrinsics=False, frame_covariance=True, device=0):
    """Covariance of a calibration.  The arguments are those `bundle_adjust()` takes and returns:

        ext, intr, poses, use_frames, result = bundle_adjust(uvs, ext0, intr0, objpoints, poses0)
        unc = calibration_uncertainty(uvs[:, use_frames], ext, intr, objpoints, poses)
        print(unc.intrinsics_std, unc.extrinsics_std)

    With H = J^T diag(w) J (J the analytic Jacobian, w = rho'((f / f_scale)^2) per present scalar) in blocks U_c, V_f, W_cf:
    camera_covariance = sigma2 S_g^-1, S = blockdiag(U) - sum_f W_f V_f^-1 W_f^T restricted to the free camera parameters;
    pose_covariance[f] = sigma2 V_f^-1 + Y_f camera_covariance Y_f^T, Y_f = V_f^-1 W_f^T.  This is the Gauss-Newton (IRLS-weighted)
    approximation of the covariance, not a sandwich (M-estimator) one.

    gauge_camera: the camera whose six extrinsics are held fixed (the convention calibrate() produces: the root camera is the zero vector); their
    variances and covariances are exact zeros.  fix_intrinsics: the six intrinsics of every camera are held as well.
    sigma: the detection noise in pixels if known; None estimates sigma2 = sum w f^2 / (m - p) from the residuals (NaN, with a warning, if
    there are no more present scalars m than free parameters p).
    A frame without any detection gets a NaN block, leaves p and is counted in info["n_degenerate_frames"].
    ValueError: a callable loss, more than 40 cameras, gauge_camera out of range, a Schur complement that is not positive definite (the message
    names the pivot and its camera and parameter).  Without a GPU: ops.McbaError -- there is no host path."""
    if callable(loss):
        raise ValueError("calibration_uncertainty: named losses only (one of %s)" % sorted(ops.LOSSES))
    if loss not in ops.LOSSES:
        raise ValueError(f"loss must be one of {sorted(ops.LOSSES)}")
    uvs = np.ascontiguousarray(all_calib_uvs, dtype=np.float64)
    if uvs.ndim != 4 or uvs.shape[3] != 2:
        raise ValueError("all_calib_uvs must be (C, F, N, 2)")
    C, F = uvs.shape[:2]
    if C > MAX_CAMERAS:
        raise ValueError(f"calibration_uncertainty: {C} cameras -- the sparse-Schur handle of rigs with more than {MAX_CAMERAS} cameras is not covered yet")
    gauge_camera = int(gauge_camera)
    if not 0 <= gauge_camera < C:
        raise ValueError(f"gauge_camera must be in 0..{C - 1}")
    if sigma is not None and not float(sigma) >= 0:
        raise ValueError("sigma must be >= 0")
    x = serialize_params(all_extrinsics, all_intrinsics, np.asarray(calib_poses, dtype=np.float64).reshape(F, 6))

    prob = ops.Problem(uvs, calib_objpoints, device=device, loss=loss, f_scale=f_scale)
    try:
        if fix_intrinsics and not prob.set_camera_block(6):
            raise ValueError("calibration_uncertainty: fix_intrinsics holds at most 26 cameras")
        prob.set_params(0, x)
        cam, frames, info = prob.covariance(0, gauge_camera, None if sigma is None else float(sigma) ** 2, frames=bool(frame_covariance))
        idx = prob.cam_index
    finally:
        prob.close()

    sigma2, m, p = float(info[0]), int(info[1]), int(info[2])
    if sigma is None and not m > p:
        warnings.warn(f"calibration_uncertainty: {m} residuals for {p} free parameters -- the noise scale cannot be estimated (pass sigma)", RuntimeWarning, stacklevel=2)
    full = np.zeros((12 * C, 12 * C))
    full[np.ix_(idx, idx)] = cam
    std = np.sqrt(np.diagonal(full)).reshape(C, 12)
    with np.errstate(divide="ignore", invalid="ignore"):
        corr = full / np.outer(std.ravel(), std.ravel())
    corr[np.arange(12 * C), np.arange(12 * C)] = np.where(std.ravel() > 0, 1.0, np.nan)
    pose_std = None
    if frames is not None:
        with np.errstate(invalid="ignore"):
            pose_std = np.sqrt(np.diagonal(frames, axis1=1, axis2=2))
    return CalibrationUncertainty(camera_covariance=full, intrinsics_std=std[:, :6].copy(), extrinsics_std=std[:, 6:].copy(), camera_correlation=corr, pose_covariance=frames,
                                  pose_std=pose_std, sigma2=sigma2, n_residuals=m, n_free=p, info={"n_degenerate_frames": int(info[3]), "kernel_ms": float(info[5]), "group": int(info[6]), "ld": int(info[7])})


POINT_STATUS = {1: "ok", -1: "too few views", -2: "degenerate"}


@dataclass
class TriangulationUncertainty:
    covariance: np.ndarray             # (P, 3, 3): detection + calibration term; NaN unless status is 1
    std: np.ndarray                    # (P, 3)
    detection_covariance: np.ndarray   # (P, 3, 3): sigma2 H^-1
    calibration_covariance: object     # (P, 3, 3): G Sigma_cc G^T; None without a camera covariance
    n_views: np.ndarray                # (P,)
    status: np.ndarray                 # (P,): a key of POINT_STATUS
    sigma2: float
    n_residuals: int
    n_free: int
    info: dict                         # n_unusable, n_degenerate, kernel_ms, group (points per workgroup of k_tricov_cal; 0 without a camera covariance), ld (row stride of the uploaded camera covariance)


def _camera_covariance(camera_covariance, C):
    """the (12 C, 12 C) array of the argument, checked: finite, symmetric to 1e-12 of sqrt(S_ii S_jj)"""
    if camera_covariance is None:
        return None
    cov = np.ascontiguousarray(getattr(camera_covariance, "camera_covariance", camera_covariance), dtype=np.float64)
    if cov.shape != (12 * C, 12 * C):
        raise ValueError(f"camera_covariance must be ({12 * C}, {12 * C}) for {C} cameras, got {cov.shape}")
    if not np.isfinite(cov).all():
        raise ValueError("camera_covariance must be finite")
    d = np.sqrt(np.abs(np.diagonal(cov)))
    if (np.abs(cov - cov.T) > 1e-12 * np.outer(d, d)).any():
        raise ValueError("camera_covariance must be symmetric (to 1e-12 of sqrt(S_ii S_jj))")
    return cov


def _unpack3(packed):
    """(P, 6) packed 00 01 02 11 12 22 -> (P, 3, 3), the same bits at (k, l) and (l, k)"""
    return np.ascontiguousarray(packed[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(-1, 3, 3))


def triangulation_uncertainty(points, all_uvs, all_extrinsics, all_intrinsics, *, camera_covariance=None, sigma=None, inliers=None, loss="linear", f_scale=1.0, device=0, weights=None):
    """Covariance of triangulated points.  `points` (P, 3) is where the cost is linearised: the result means what it says only at a minimiser
    of the robust reprojection cost, which is what `refine_triangulation` and `triangulate_consensus` return (with the same loss and f_scale);
    all_uvs, all_extrinsics, all_intrinsics are exactly what those take (raw detections, NaN = unseen; the five-coefficient forward model).

        X = refine_triangulation(triangulate(uvs, ext, intr), uvs, ext, intr, loss="linear")
        unc = triangulation_uncertainty(X, uvs, ext, intr, camera_covariance=calibration_uncertainty(...))
        print(unc.std)        # the units of the extrinsics' translations

    Per point, over the cameras that see it: f = detection - projection, w = rho'((f / f_scale)^2) per scalar, A_c = d(u, v)/dX,
    B_c = d(u, v)/d(the camera's 12 entries of result.x: fx fy cx cy k1 k2, rotation vector, translation; p1, p2, k3 are constants),
    H = sum_c A_c^T W_c A_c.  detection_covariance = sigma2 H^-1; calibration_covariance = G Sigma_cc G^T with G_c = H^-1 A_c^T W_c B_c
    (how the re-triangulated point moves with the cameras); covariance is their sum.  This is the Gauss-Newton (IRLS-weighted) approximation
    `calibration_uncertainty` uses, not a sandwich estimator.  Only per-point marginals: covariances between points are not reported,
    although the points share Sigma_cc.

    camera_covariance: None (the detection term alone), a (12 C, 12 C) array, or a CalibrationUncertainty (its camera_covariance); finite and
    symmetric.  Zero rows and columns (a gauge camera) are ordinary input.
    sigma: the detection noise in pixels if known; None pools sigma2 = sum w f^2 / (m - 3 P_u) over the P_u points of status 1 with their m
    present scalars (NaN, with a RuntimeWarning, if m <= 3 P_u).
    inliers: None, or the (C, P) mask `triangulate_consensus` returns: a camera that is False for a point is treated as not seeing it.
    weights: None, or (C, P) per-detection weights w >= 0 as `refine_triangulation` takes them (relative inverse variances; 0 or NaN =
    unseen): f, A_c and B_c of a detection are scaled by sqrt(w), so H, G, both terms and the pooled sigma2 = sum rho' w f^2 / (m - 3 P_u) are
    those of the weighted problem, m and n_views counting the detections of positive weight.  With true inverse variances as weights sigma2
    is about 1; `sigma` stays the standard deviation of a detection of weight 1.  With inliers the mask zeroes weights.
    status (POINT_STATUS): -1 fewer than two views or a NaN in the point; -2 degenerate (H, Jacobi-scaled by its diagonal, has a Cholesky
    pivot whose square is below 1e-12: two cameras with one centre, a point on the baseline).  Both terms are NaN for such points and they
    leave the pooled sums.
    ValueError: a callable or unknown loss, a camera covariance or mask of the wrong shape.  NotImplementedError: fewer than 2 or more than 64
    cameras.  Without a GPU: ops.McbaError -- there is no host path."""
    if callable(loss):
        raise ValueError("triangulation_uncertainty: named losses only (one of %s)" % sorted(ops.LOSSES))
    if loss not in ops.LOSSES:
        raise ValueError(f"loss must be one of {sorted(ops.LOSSES)}")
    if not f_scale > 0:
        raise ValueError("`f_scale` must be positive.")
    if sigma is not None and not float(sigma) >= 0:
        raise ValueError("sigma must be >= 0")
    pts, uvs, cam, dist = _keypoint_inputs(points, all_uvs, all_extrinsics, all_intrinsics)
    C, P = uvs.shape[:2]
    if not 2 <= C <= 64:
        raise NotImplementedError("triangulation_uncertainty() supports 2 to 64 cameras")
    cov = _camera_covariance(camera_covariance, C)
    if inliers is not None:
        mask = np.asarray(inliers)
        if mask.shape != (C, P) or mask.dtype != np.bool_:
            raise ValueError(f"inliers must be the ({C}, {P}) bool mask of triangulate_consensus")
        uvs = np.where(mask[:, :, None], uvs, np.nan)   # (a copy: the one that is uploaded)
    w = _weight_plane(weights, C, P)
    det, cal = np.empty((P, 6)), None if cov is None else np.empty((P, 6))
    views, status, info = np.empty(P, np.int32), np.empty(P, np.int32), np.zeros(8)
    ms = ctypes.c_double(0.0)
    tail = (cam.ctypes.data, dist.ctypes.data, None if cov is None else cov.ctypes.data, ops.LOSSES[loss], float(f_scale), float("nan") if sigma is None else float(sigma) ** 2, int(device),
            det.ctypes.data, None if cal is None else cal.ctypes.data, views.ctypes.data, status.ctypes.data, info.ctypes.data, ctypes.addressof(ms))
    if w is None:
        ops.call("mcba_triangulation_covariance", C, P, pts.ctypes.data, uvs.ctypes.data, *tail)
    else:
        ops.call("mcba_triangulation_covariance_weighted", C, P, pts.ctypes.data, uvs.ctypes.data, w.ctypes.data, *tail)
    sigma2, m, nfree = float(info[0]), int(info[1]), int(info[2])
    if sigma is None and not m > nfree:
        warnings.warn(f"triangulation_uncertainty: {m} residuals for {nfree} point coordinates -- the noise scale cannot be estimated (pass sigma)", RuntimeWarning, stacklevel=2)
    det3 = _unpack3(det)
    cal3 = None if cal is None else _unpack3(cal)
    total = det3 if cal3 is None else det3 + cal3
    with np.errstate(invalid="ignore"):
        std = np.sqrt(np.diagonal(total, axis1=1, axis2=2))
    return TriangulationUncertainty(covariance=total, std=std, detection_covariance=det3, calibration_covariance=cal3, n_views=views, status=status, sigma2=sigma2, n_residuals=m,
                                    n_free=nfree, info={"n_unusable": int(info[3]), "n_degenerate": int(info[4]), "kernel_ms": float(info[5]), "group": int(info[6]), "ld": int(info[7])})
