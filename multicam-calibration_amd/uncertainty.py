"""calibration_uncertainty -- how good a calibration is: the covariance of the camera parameters and of every board pose at the point
`bundle_adjust()` returned (or at any other), computed on the GPU from the Schur system of one linearisation.

The reference has no counterpart: scipy's OptimizeResult carries `jac` and leaves inverting J^T J to the user -- which is exactly singular
(the 6-DoF gauge freedom) and 60 072 x 60 072 at the size this package exists for.  OpenCV users know the result as calibrateCameraExtended's
stdDeviationsIntrinsics / stdDeviationsExtrinsics."""
import warnings
from dataclasses import dataclass

import numpy as np

from . import ops
from .api import serialize_params

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
    info: dict                       # n_degenerate_frames, kernel_ms


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
                                  pose_std=pose_std, sigma2=sigma2, n_residuals=m, n_free=p, info={"n_degenerate_frames": int(info[3]), "kernel_ms": float(info[5])})
