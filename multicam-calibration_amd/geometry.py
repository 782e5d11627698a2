"""The reference's `geometry.py` surface: keypoints through a calibration on the GPU, the small matrix helpers on the host.

GPU (`csrc/mcba_keypoints.hip`; no numpy fallback -- without a device every one of them raises `ops.McbaError`):
  project_points                 geometry.py:277 -- k1, k2 only, any leading shape, nothing special behind the camera, NaN in -> NaN out
  project_to_cameras             every camera from one upload of the points; distortion="radial2" (the reference's model) or "opencv5"
                                 (the forward five-coefficient model k1 k2 p1 p2 k3 that undistort_points inverts)
  apply_rigid_transform          geometry.py:128
  keypoint_reprojection_errors   |detection - projection| per (camera, point) and the exact per-camera nan-medians
  refine_triangulation           per point, Levenberg-Marquardt on the robust reprojection cost from a start such as triangulate()'s
  triangulate_consensus          (`csrc/mcba_consensus.hip`; no counterpart in the reference) per point, every camera
                                 pair's two-view point scored against all detections, the inlier cameras named, the point refitted on them
  refine_extrinsics              (`csrc/mcba_kpba.hip`; no counterpart in the reference) free-point bundle adjustment:
                                 the extrinsics and every 3-D point jointly on the robust reprojection cost of the raw detections
                                 (2 to 24 cameras; reduction="tiled", `csrc/mcba_kpba_tiled.hip`: up to 64)
  refine_extrinsics_system       one evaluation of refine_extrinsics laid open: the reduced system and the point steps as the kernels wrote them
  estimate_relative_pose         (`csrc/mcba_twoview.hip`; no counterpart in the reference) two-view RANSAC: the pose of one
                                 camera relative to another from the keypoints both detect, known intrinsics, nothing else
  extrinsics_from_keypoints      the rig's extrinsics from keypoints alone: a spanning tree of such pairs, a scale chain, refine_extrinsics
  resect_camera, resect_cameras  (`csrc/mcba_resect.hip`; the reference resects only a planar board) the pose of a camera from
                                 known 3-D points and its own detections: PnP RANSAC (6-point DLT + Gauss-Newton hypotheses), a pose-only polish
The refinements (refine_triangulation onwards; of the resection, its polish) use the five-coefficient forward model on the RAW (distorted) detections: no undistortion iteration, so none of its truncation
error.  With p1 = p2 = k3 = 0 (all bundle_adjust returns) the model is project_points'.

Host (numpy, the reference's formulas): rigid_transform_from_correspondences (returns (t, rmsd); the one in flatibration.py returns t alone),
get_projection_matrix, euclidean_to_homogenous, homogeneous_to_euclidean, and rodrigues / rodrigues_inv / get_transformation_matrix /
get_transformation_vector re-exported from calibration.py.
"""
from dataclasses import dataclass

import numpy as np

from . import ops
from .calibration import rodrigues, rodrigues_inv, get_transformation_matrix, get_transformation_vector  # noqa: F401
from .triangulation import _cam_blocks, _stack_uvs, _weight_plane, DEFAULT_MAX_ITERATIONS

STATUS = {1: "converged", 0: "iteration limit", -1: "too few views"}


def _points(points):
    pts = np.asarray(points, dtype=np.float64)
    if pts.ndim < 1 or pts.shape[-1] != 3:
        raise ValueError("points must have shape (..., 3)")
    return pts.shape[:-1], np.ascontiguousarray(pts.reshape(-1, 3))


def _project(flat, cam, dist, device):
    C, P = len(cam), len(flat)
    out = np.empty((C, P, 2))
    if P:
        ops.call("mcba_project_points", C, P, flat.ctypes.data, cam.ctypes.data, None if dist is None else dist.ctypes.data, int(device), out.ctypes.data, None)
    return out


def project_points(points, extrinsics, camera_matrix, dist_coefs=None, *, device=0):
    """points (..., 3) in world coordinates -> (..., 2) pixels in the camera (extrinsics (6,), camera_matrix (3, 3)).  Only k1, k2 of
    dist_coefs are used, as in the reference (geometry.py:309); None = no distortion."""
    d = np.zeros(2) if dist_coefs is None else np.ravel(np.asarray(dist_coefs, dtype=np.float64))[:2]
    if d.size < 2:
        raise ValueError("dist_coefs needs at least k1, k2")
    cam, _ = _cam_blocks([extrinsics], [(camera_matrix, d)])
    lead, flat = _points(points)
    return _project(flat, cam, None, device)[0].reshape(lead + (2,))


def project_to_cameras(points, all_extrinsics, all_intrinsics, *, distortion="radial2", device=0):
    """points (..., 3) -> (C, ..., 2): the points go to the device once, every camera is projected from that copy.
    distortion "radial2": project_points' model per camera; "opencv5": the forward model with k1 k2 p1 p2 k3."""
    if distortion not in ("radial2", "opencv5"):
        raise ValueError("distortion must be 'radial2' or 'opencv5'")
    if len(all_extrinsics) != len(all_intrinsics) or len(all_extrinsics) < 1:
        raise ValueError("one (camera_matrix, dist_coefs) per entry of all_extrinsics, at least one camera")
    cam, dist = _cam_blocks(all_extrinsics, all_intrinsics)
    lead, flat = _points(points)
    out = _project(flat, cam, dist if distortion == "opencv5" else None, device)
    return out.reshape((len(cam),) + lead + (2,))


def apply_rigid_transform(transform, points, *, device=0):
    """transform (6,) (rotation vector, translation) or (4, 4); points (..., 3) -> (..., 3)."""
    T = np.asarray(transform, dtype=np.float64)
    if T.shape == (6,):
        T = get_transformation_matrix(T)
    if T.shape != (4, 4):
        raise ValueError("transform must have shape (6,) or (4, 4)")
    lead, flat = _points(points)
    out = np.empty_like(flat)
    if len(flat):
        T12 = np.ascontiguousarray(np.r_[T[:3, :3].ravel(), T[:3, 3]])
        ops.call("mcba_rigid_transform", len(flat), flat.ctypes.data, T12.ctypes.data, int(device), out.ctypes.data)
    return out.reshape(lead + (3,))


def _keypoint_inputs(points, all_uvs, all_extrinsics, all_intrinsics):
    uvs = _stack_uvs(all_uvs, all_extrinsics, all_intrinsics)
    pts = np.ascontiguousarray(points, dtype=np.float64)
    if pts.shape != (uvs.shape[1], 3):
        raise ValueError("points must be (n_points, 3), one row per row of the cameras' uvs")
    cam, dist = _cam_blocks(all_extrinsics, all_intrinsics)
    return pts, uvs, cam, dist


def keypoint_reprojection_errors(points, all_uvs, all_extrinsics, all_intrinsics, *, device=0, arrays=True):
    """(errors (C, P), median_error (C,)): the distance in pixels between each camera's detection and the reprojection of the 3-D point; NaN
    where the camera does not see the point (a NaN coordinate in its detection) or the point has a NaN.  median_error[c] is
    np.nanmedian(errors[c]) bit for bit (an exact select on the device), NaN for a camera that sees nothing.  arrays=False: errors is None
    (the rows stay on the device, only the medians come back)."""
    pts, uvs, cam, dist = _keypoint_inputs(points, all_uvs, all_extrinsics, all_intrinsics)
    C, P = uvs.shape[:2]
    med = np.full(C, np.nan)
    err = np.empty((C, P)) if arrays else None
    if P:
        ops.call("mcba_keypoint_errors", C, P, pts.ctypes.data, uvs.ctypes.data, cam.ctypes.data, dist.ctypes.data, int(device), None if err is None else err.ctypes.data, med.ctypes.data, None)
    return err, med


def refine_triangulation(points, all_uvs, all_extrinsics, all_intrinsics, *, loss="soft_l1", f_scale=1.0, max_iterations=DEFAULT_MAX_ITERATIONS, device=0, return_info=False, weights=None):
    """Per point, minimise 0.5 sum rho(f^2) over X from the start `points` (P, 3): f = the 2 (cameras that see the point) residuals
    detection - projection in pixels, rho and f_scale exactly scipy.optimize.least_squares' (loss one of linear, soft_l1, huber, cauchy,
    arctan).  Points seen by fewer than two cameras, or whose start has a NaN, come back NaN.  A point is never made worse: a step is taken
    only when the robust cost does not rise, and if none is, the start is returned.  2 to 64 cameras.

    Levenberg-Marquardt per point (Marquardt damping from 1e-4, a tenth on an accepted step, tenfold on a rejected one); it stops when the
    step is below 1e-12 (1 + |X|), when an accepted step gains less than 1e-15 of the cost, when the gradient is below 1e-12, or after
    max_iterations (default 100) linearisations -- a point that is done costs nothing further, the others go on.

    weights: None, or (C, P) per-detection weights w >= 0, the relative inverse variance of each detection (a pose estimator's
    confidence).  A detection of weight w enters the cost exactly as if it and fx, fy, cx, cy of its camera had been multiplied by sqrt(w):
    its residual pair is scaled by sqrt(w) before the loss.  w = 0 or NaN: the detection is unseen, like a NaN detection (the views count
    detections of positive weight).  ValueError: another shape, a negative or infinite weight.  The same keyword, with the same meaning,
    on `triangulate(refine=True)`, `triangulation_uncertainty`, `refine_extrinsics` and `refine_extrinsics_system`.

    return_info=True: (points, info) with per-point arrays info["cost"] (robust cost at the result), info["cost0"] (at the start),
    info["n_iterations"], info["status"] (1 converged, 0 iteration limit, -1 too few views: `geometry.STATUS`)."""
    if loss not in ops.LOSSES:
        raise ValueError(f"loss must be one of {sorted(ops.LOSSES)}")
    if not f_scale > 0:
        raise ValueError("`f_scale` must be positive.")
    if int(max_iterations) < 0:
        raise ValueError("max_iterations must not be negative")
    pts, uvs, cam, dist = _keypoint_inputs(points, all_uvs, all_extrinsics, all_intrinsics)
    C, P = uvs.shape[:2]
    if not 2 <= C <= 64:
        raise NotImplementedError("refine_triangulation() supports 2 to 64 cameras")
    w = _weight_plane(weights, C, P)
    out = np.empty((P, 3))
    info = np.empty((P, 4))
    if P and w is not None:
        ops.call("mcba_triangulate_refine_weighted", C, P, uvs.ctypes.data, w.ctypes.data, cam.ctypes.data, dist.ctypes.data, pts.ctypes.data, 0, ops.LOSSES[loss], float(f_scale),
                 int(max_iterations), int(device), out.ctypes.data, info.ctypes.data, None)
    elif P:
        ops.call("mcba_triangulate_refine", C, P, uvs.ctypes.data, cam.ctypes.data, dist.ctypes.data, pts.ctypes.data, 0, ops.LOSSES[loss], float(f_scale), int(max_iterations), int(device),
                 out.ctypes.data, info.ctypes.data, None)
    if not return_info:
        return out
    return out, dict(cost=info[:, 0].copy(), cost0=info[:, 1].copy(), n_iterations=info[:, 2].astype(np.int64), status=info[:, 3].astype(np.int64))


CONSENSUS_STATUS = {1: "converged", 0: "iteration limit", -1: "too few views", -2: "no consensus"}


def triangulate_consensus(all_uvs, all_extrinsics, all_intrinsics, *, threshold, min_views=2, loss="linear", f_scale=1.0, max_iterations=DEFAULT_MAX_ITERATIONS, undistort_iterations=5,
                          device=0, return_info=False, return_errors=False):
    """Which camera's detection of a point is wrong, and the point without it: (points (P, 3), inliers (C, P) bool).

    Per point, every camera pair that sees it (both coordinates of the detection non-NaN) gives a hypothesis: triangulate()'s two-view point
    (`undistort_iterations` rounds).  A camera that sees the point is an inlier of a hypothesis when the point lies in front of it and its
    raw detection is within `threshold` pixels of the five-coefficient projection.  The hypothesis of lowest truncated cost -- e^2 per inlier,
    threshold^2 per other seeing camera -- wins (an exact tie: the first pair in the order (0,1), (0,2), ..., (1,2), ...); the enumeration is
    exhaustive, nothing is sampled.  The point is then refitted on the winner's inliers alone as refine_triangulation does (`loss`, default
    plain least squares, `f_scale`, `max_iterations`; max_iterations=0 returns the winning hypothesis itself).  The mask is the winner's: it is
    not voted again after the refit.  `threshold` has no default: the right value is the detector's noise.  2 to 64 cameras.

    A point no pair sees comes back NaN with an empty mask (status -1); a winner with fewer than `min_views` (>= 2) inliers gives NaN with the
    mask still reported (status -2).

    return_info=True: also a dict of per-point arrays -- n_inliers, pair (P, 2) (the winning pair, -1 where none), hypothesis_cost, cost and
    cost0 (the refit's cost at the result and at its start), n_iterations, status (`geometry.CONSENSUS_STATUS`).
    return_errors=True: also errors (C, P), keypoint_reprojection_errors' at the returned points (computed on the device from the same upload)."""
    if not threshold > 0:
        raise ValueError("`threshold` (pixels) must be positive.")
    if int(min_views) < 2:
        raise ValueError("min_views must be at least 2")
    if loss not in ops.LOSSES:
        raise ValueError(f"loss must be one of {sorted(ops.LOSSES)}")
    if not f_scale > 0:
        raise ValueError("`f_scale` must be positive.")
    if int(max_iterations) < 0 or int(undistort_iterations) < 0:
        raise ValueError("max_iterations and undistort_iterations must not be negative")
    uvs = _stack_uvs(all_uvs, all_extrinsics, all_intrinsics)
    C, P = uvs.shape[:2]
    if not 2 <= C <= 64:
        raise NotImplementedError("triangulate_consensus() supports 2 to 64 cameras")
    cam, dist = _cam_blocks(all_extrinsics, all_intrinsics)
    out = np.empty((P, 3))
    words = np.zeros(P, dtype=np.uint64)
    info = np.empty((P, 8)) if return_info else None
    err = np.empty((C, P)) if return_errors else None
    if P:
        ops.call("mcba_triangulate_consensus", C, P, uvs.ctypes.data, cam.ctypes.data, dist.ctypes.data, float(threshold), int(min_views), int(undistort_iterations), ops.LOSSES[loss],
                 float(f_scale), int(max_iterations), int(device), out.ctypes.data, words.ctypes.data, None if info is None else info.ctypes.data,
                 None if err is None else err.ctypes.data, None)
    inliers = ((words[None, :] >> np.arange(C, dtype=np.uint64)[:, None]) & np.uint64(1)).astype(bool)
    res = (out, inliers)
    if return_info:
        res += (dict(n_inliers=info[:, 0].astype(np.int64), pair=info[:, 1:3].astype(np.int64), hypothesis_cost=info[:, 3].copy(), cost=info[:, 4].copy(), cost0=info[:, 5].copy(),
                     n_iterations=info[:, 6].astype(np.int64), status=info[:, 7].astype(np.int64)),)
    if return_errors:
        res += (err,)
    return res


REFINE_POINT_STATUS = {1: "used", -1: "too few views", -2: "zero diagonal"}
MAX_REFINE_CAMERAS = 24
MAX_REFINE_CAMERAS_TILED = 64
REDUCTIONS = {"resident": 0, "tiled": 1}   # MCBA_KPBA_RESIDENT, MCBA_KPBA_TILED of include/mcba.h


def _reduction_limit(who, reduction, C):
    """the code of `reduction`; ValueError for an unknown one, NotImplementedError for a camera count its reduction does not take"""
    if not isinstance(reduction, str) or reduction not in REDUCTIONS:
        raise ValueError(f"reduction must be one of {sorted(REDUCTIONS)}")
    if reduction == "tiled":
        if not 2 <= C <= MAX_REFINE_CAMERAS_TILED:
            raise NotImplementedError(f"{who}(reduction=\"tiled\") supports 2 to {MAX_REFINE_CAMERAS_TILED} cameras, got {C}: four bands of 16 cameras")
    elif not 2 <= C <= MAX_REFINE_CAMERAS:
        raise NotImplementedError(f"{who}() supports 2 to {MAX_REFINE_CAMERAS} cameras, got {C}: the resident reduction holds the reduced camera system to 144 rows (nine matrix-core tiles); "
                                  f"reduction=\"tiled\" takes up to {MAX_REFINE_CAMERAS_TILED}")
    return REDUCTIONS[reduction]


@dataclass
class ExtrinsicsRefinement:
    extrinsics: np.ndarray     # (C, 6)
    points: np.ndarray         # (P, 3); NaN rows where point_status is not 1
    cost: float
    cost0: float
    optimality: float          # inf-norm of the gradient over the free parameters
    nfev: int
    njev: int
    status: int                # scipy's: 0 max_nfev, 1 gtol, 2 ftol, 3 xtol
    message: str
    success: bool
    point_status: np.ndarray   # (P,): a key of REFINE_POINT_STATUS
    held: np.ndarray           # (C, 6) bool: parameters that were not free
    scale: float               # factor of the closing rescale about the gauge camera's centre
    history: np.ndarray        # (evaluations, 3): cost, damping, accepted
    info: dict                 # kernel_ms, reduce_ms, n_reduce, step_ms, n_step, group, reduction, band, band_pairs, gauge_camera, scale_camera


def _camera_centres(ext):
    return np.stack([-rodrigues(e[:3]).T @ e[3:] for e in ext])


def refine_extrinsics(all_uvs, all_extrinsics, all_intrinsics, *, points=None, inliers=None, gauge_camera=0, scale_camera=None, loss="soft_l1", f_scale=1.0, ftol=1e-8, xtol=1e-8, gtol=1e-8,
                      max_nfev=100, verbose=0, device=0, weights=None, reduction="resident"):
    """Move drifted cameras back with the detections that show the drift: free-point bundle adjustment.  Minimises
    0.5 f_scale^2 sum rho((f / f_scale)^2) over the present scalars f = detection - projection, jointly over the extrinsics of the cameras and
    every 3-D point; the intrinsics stay fixed.  all_uvs, all_extrinsics, all_intrinsics as `triangulate` takes them (raw detections, NaN =
    unseen; the five-coefficient forward model of project_to_cameras(distortion="opencv5")); loss and f_scale are scipy's.

        res = refine_extrinsics(uvs, ext, intr, inliers=triangulate_consensus(uvs, ext, intr, threshold=3.0)[1])
        print(res.message, res.cost0, "->", res.cost);  ext = res.extrinsics

    points: (P, 3) start; None = triangulate(all_uvs, all_extrinsics, all_intrinsics).  inliers: None, or the (C, P) mask of
    triangulate_consensus: a camera that is False for a point is treated as not seeing it.  weights: None, or (C, P) per-detection weights
    as `refine_triangulation` takes them: the reduction, the cost, the trial cost and the point steps are those of the weighted problem; a
    detection of weight 0 or NaN is unseen (for points=None, point_status and the camera no used point sees alike); with inliers the mask
    zeroes weights.
    Gauge: with fixed intrinsics the cost does not change under a rigid motion or a global scale.  All six extrinsics of `gauge_camera` are held.
    The scale is fixed by holding one scalar of `scale_camera` (default: the camera whose centre is farthest from the gauge camera's at the
    start): the component of its translation along which d = -R_j (c_j - c_0) is largest in magnitude -- scaling the rig about c_0 moves t_j
    along d.  A camera that no used point sees is held whole.  `held` reports all of it.  After the iteration camera centres and points are
    rescaled about c_0 by `scale`, so that |c_j - c_0| is what it was at the start (the metric scale of the board calibration); this changes
    no projection.
    Levenberg-Marquardt (Marquardt damping, the bundle-adjustment tick's curvature weights); a trial is accepted when the robust cost does not
    rise, so the result is never worse than the start.  ftol, xtol, gtol, max_nfev, status, message, success: scipy.optimize.least_squares'.
    point_status (REFINE_POINT_STATUS): -1 fewer than two views or a NaN start, -2 a zero diagonal in the point's 3 x 3 block; such points
    come back NaN and take no part.  history: per evaluation the cost, the damping and whether it was accepted; verbose=2 prints it.
    ValueError: an unknown loss, f_scale <= 0, max_nfev < 2 (the start and one trial are the least a run needs), gauge_camera == scale_camera,
    arrays of the wrong shape, an unknown reduction.  NotImplementedError: fewer than 2 or more than 24 cameras (the reduced system is held to
    144 rows), with reduction="tiled" more than 64.  Without a GPU: ops.McbaError -- there is no host path.
    reduction: "resident" (a workgroup keeps the whole reduced system in registers: 2 to 24 cameras) or "tiled" (`csrc/mcba_kpba_tiled.hip`:
    cameras in bands of 16, the system in band pairs: 2 to 64 cameras).  The same system, loop, gauge and closing step; the sums are in another
    order, so results agree to rounding, not bit for bit.  info gains band and band_pairs (0 for "resident")."""
    from . import solver
    from .triangulation import triangulate

    if callable(loss) or loss not in ops.LOSSES:
        raise ValueError(f"loss must be one of {sorted(ops.LOSSES)}")
    if not f_scale > 0:
        raise ValueError("`f_scale` must be positive.")
    if int(max_nfev) < 2:
        raise ValueError("max_nfev must be at least 2: the start and one trial are the least a run needs")
    if min(ftol, xtol, gtol) < 0:
        raise ValueError("ftol, xtol and gtol must not be negative")
    uvs = _stack_uvs(all_uvs, all_extrinsics, all_intrinsics)
    C, P = uvs.shape[:2]
    red = _reduction_limit("refine_extrinsics", reduction, C)
    if P < 1:
        raise ValueError("refine_extrinsics() needs at least one point")
    ext0 = np.ascontiguousarray(all_extrinsics, dtype=np.float64)
    if ext0.shape != (C, 6) or not np.isfinite(ext0).all():
        raise ValueError("all_extrinsics must be finite (rotation vector, translation) rows, one per camera")
    gauge_camera = int(gauge_camera)
    if not 0 <= gauge_camera < C:
        raise ValueError("gauge_camera is not a camera of the rig")
    centres = _camera_centres(ext0)
    if scale_camera is None:
        scale_camera = int(np.argmax(np.linalg.norm(centres - centres[gauge_camera], axis=1)))
    scale_camera = int(scale_camera)
    if not 0 <= scale_camera < C:
        raise ValueError("scale_camera is not a camera of the rig")
    if scale_camera == gauge_camera:
        raise ValueError("gauge_camera == scale_camera: the scale is fixed by the distance between two different cameras")
    if inliers is not None:
        mask = np.asarray(inliers)
        if mask.shape != (C, P) or mask.dtype != np.bool_:
            raise ValueError(f"inliers must be the ({C}, {P}) bool mask of triangulate_consensus")
        uvs = np.where(mask[:, :, None], uvs, np.nan)   # (a copy: the one that is uploaded)
    w = _weight_plane(weights, C, P)
    if points is None:
        start_uvs = uvs if w is None else np.where((w > 0)[:, :, None], uvs, np.nan)
        pts = np.ascontiguousarray(triangulate(list(start_uvs), all_extrinsics, all_intrinsics, device=device))
    else:
        pts = np.ascontiguousarray(points, dtype=np.float64)
        if pts.shape != (P, 3):
            raise ValueError("points must be (n_points, 3), one row per row of the cameras' uvs")
    cam, dist = _cam_blocks(all_extrinsics, all_intrinsics)
    d = -rodrigues(ext0[scale_camera, :3]) @ (centres[scale_camera] - centres[gauge_camera])
    held_bits = np.zeros(C, dtype=np.int32)
    held_bits[gauge_camera] = 63
    held_bits[scale_camera] |= 1 << (3 + int(np.argmax(np.abs(d))))
    ext, out, status, res = np.empty((C, 6)), np.empty((P, 3)), np.empty(P, np.int32), np.zeros(16)
    hist = np.zeros((int(max_nfev) + 1, 3))
    tail = (held_bits.ctypes.data, gauge_camera, scale_camera, ops.LOSSES[loss], float(f_scale), float(ftol), float(xtol), float(gtol), int(max_nfev), int(device), ext.ctypes.data, out.ctypes.data,
            status.ctypes.data, res.ctypes.data, hist.ctypes.data, len(hist))
    if red:
        ops.call("mcba_refine_extrinsics_reduction", C, P, uvs.ctypes.data, None if w is None else w.ctypes.data, red, cam.ctypes.data, dist.ctypes.data, pts.ctypes.data, *tail)
    elif w is None:
        ops.call("mcba_refine_extrinsics", C, P, uvs.ctypes.data, cam.ctypes.data, dist.ctypes.data, pts.ctypes.data, *tail)
    else:
        ops.call("mcba_refine_extrinsics_weighted", C, P, uvs.ctypes.data, w.ctypes.data, cam.ctypes.data, dist.ctypes.data, pts.ctypes.data, *tail)
    hist = hist[:min(int(res[7]), len(hist))].copy()
    code = int(res[5])
    if verbose == 2:
        print("{0:^15}{1:^15}{2:^15}{3:^15}{4:^15}".format("Iteration", "Total nfev", "Cost", "Cost reduction", "Damping"))
        it, last = 0, None
        for k, (c, lam, acc) in enumerate(hist):
            if acc:
                print("{0:^15}{1:^15}{2:^15.4e}{3:^15}{4:^15.2e}".format(it, k + 1, c, "" if last is None else "%.2e" % (last - c), lam))
                it, last = it + 1, c
    if verbose >= 1:
        print(solver.TERMINATION_MESSAGES[code])
        print("Function evaluations {0}, initial cost {1:.4e}, final cost {2:.4e}, first-order optimality {3:.2e}.".format(int(res[3]), res[1], res[0], res[2]))
    held = ((held_bits[:, None] >> np.arange(6)) & 1).astype(bool)
    return ExtrinsicsRefinement(extrinsics=ext, points=out, cost=float(res[0]), cost0=float(res[1]), optimality=float(res[2]), nfev=int(res[3]), njev=int(res[4]), status=code,
                                message=solver.TERMINATION_MESSAGES[code], success=code > 0, point_status=status, held=held, scale=float(res[6]), history=hist,
                                info={"kernel_ms": float(res[8]), "reduce_ms": float(res[9]), "n_reduce": int(res[10]), "step_ms": float(res[11]), "n_step": int(res[12]), "group": int(res[13]),
                                      "reduction": reduction, "band": int(res[14]), "band_pairs": int(res[15]), "gauge_camera": gauge_camera, "scale_camera": scale_camera})


def refine_extrinsics_system(all_uvs, all_extrinsics, all_intrinsics, *, points, held, lam, loss="soft_l1", f_scale=1.0, step=None, device=0, weights=None, reduction="resident"):
    """One evaluation of refine_extrinsics laid open (`mcba_refine_extrinsics_system`; tests and diagnostics): the loop's own set-up and kernels
    run once at (all_extrinsics, points) and the damping lam, and what they wrote comes back as it is.  held: (C, 6) bool or (C,) bit words,
    taken as given -- no gauge, scale or blind-camera rule.  weights: None or (C, P), as refine_extrinsics takes them.  step: None, or (ext_trial (C, 6), dtheta (C, 6)): also the back-substitution.
    Returns a dict: point_status (P,); system (the raw NP NP + 33 C + 4 doubles) and its views YY (NP, NP), acc (C, 33) = U_c packed lower
    (21) | g_c (6) | sum_p Y_cp z_p (6), cost, count (present scalars of the used points), gmax (max |g_p|), tail (the fourth trailing scalar);
    group, workgroups (the partial systems summed), NP, kernel_ms, reduction, band (cameras per band) and band_pairs (both 0 for "resident"); with a
    step trial_points (P, 3) and step4 = trial cost, sum dX^2, 0, sum X^2.  reduction: as refine_extrinsics takes it."""
    if callable(loss) or loss not in ops.LOSSES:
        raise ValueError(f"loss must be one of {sorted(ops.LOSSES)}")
    uvs = _stack_uvs(all_uvs, all_extrinsics, all_intrinsics)
    C, P = uvs.shape[:2]
    red = _reduction_limit("refine_extrinsics_system", reduction, C)
    pts = np.ascontiguousarray(points, dtype=np.float64)
    if pts.shape != (P, 3):
        raise ValueError("points must be (n_points, 3), one row per row of the cameras' uvs")
    held = np.asarray(held)
    if held.shape == (C, 6):
        held = (held.astype(bool).astype(np.int32) << np.arange(6, dtype=np.int32)).sum(1)
    held_bits = np.ascontiguousarray(held, dtype=np.int32)
    if held_bits.shape != (C,):
        raise ValueError("held must be (n_cameras, 6) bool or (n_cameras,) bit words")
    cam, dist = _cam_blocks(all_extrinsics, all_intrinsics)
    NP = (6 * C + 15) // 16 * 16
    status, system, info = np.empty(P, np.int32), np.empty(NP * NP + 33 * C + 4), np.zeros(8)
    trial = step4 = ext_trial = dtheta = None
    if step is not None:
        ext_trial, dtheta = (np.ascontiguousarray(a, dtype=np.float64) for a in step)
        if ext_trial.shape != (C, 6) or dtheta.shape != (C, 6):
            raise ValueError("step must be (ext_trial (n_cameras, 6), dtheta (n_cameras, 6))")
        trial, step4 = np.empty((P, 3)), np.empty(4)
    addr = lambda a: None if a is None else a.ctypes.data   # noqa: E731
    w = _weight_plane(weights, C, P)
    tail = (cam.ctypes.data, dist.ctypes.data, pts.ctypes.data, held_bits.ctypes.data, ops.LOSSES[loss], float(f_scale), float(lam), int(device), addr(ext_trial), addr(dtheta), status.ctypes.data,
            system.ctypes.data, addr(trial), addr(step4), info.ctypes.data)
    if red:
        ops.call("mcba_refine_extrinsics_system_reduction", C, P, uvs.ctypes.data, addr(w), red, *tail)
    elif w is None:
        ops.call("mcba_refine_extrinsics_system", C, P, uvs.ctypes.data, *tail)
    else:
        ops.call("mcba_refine_extrinsics_system_weighted", C, P, uvs.ctypes.data, w.ctypes.data, *tail)
    out = dict(point_status=status, system=system, YY=system[:NP * NP].reshape(NP, NP), acc=system[NP * NP:NP * NP + 33 * C].reshape(C, 33), cost=float(system[-4]), count=float(system[-3]),
               gmax=float(system[-2]), tail=float(system[-1]), group=int(info[0]), workgroups=int(info[1]), NP=int(info[2]), kernel_ms=float(info[3]),
               reduction=reduction, band=int(info[4]), band_pairs=int(info[5]))
    if step is not None:
        out.update(trial_points=trial, step4=step4)
    return out


# ---------------------------------------------------------------- camera refinement with free intrinsics
INTRINSIC_GROUPS = {"focal": (0, 1), "principal": (2, 3), "distortion": (4, 5)}   # columns of (fx fy cx cy k1 k2)
MAX_REFINE_CAMERAS_FREE_INTRINSICS = 12


@dataclass
class CameraRefinement:
    extrinsics: np.ndarray     # (C, 6)
    intrinsics: list           # (camera_matrix, dist_coefs) per camera, in the format given: fx fy cx cy k1 k2 updated, the rest as given
    points: np.ndarray         # (P, 3); NaN rows where point_status is not 1
    cost: float                # robust cost + prior_cost
    prior_cost: float          # 0.5 sum ((theta - theta_0) / std)^2 over the free intrinsic scalars
    cost0: float
    optimality: float          # inf-norm of the gradient over the free parameters (the prior's share included)
    nfev: int
    njev: int
    status: int                # scipy's: 0 max_nfev, 1 gtol, 2 ftol, 3 xtol
    message: str
    success: bool
    point_status: np.ndarray   # (P,): a key of REFINE_POINT_STATUS
    held: np.ndarray           # (C, 12) bool in the order fx fy cx cy k1 k2 | rotation vector | translation: parameters that were not free
    scale: float               # factor of the closing rescale about the gauge camera's centre
    history: np.ndarray        # (evaluations, 3): cost (prior included), damping, accepted
    info: dict                 # kernel_ms, reduce_ms, n_reduce, step_ms, n_step, group, gauge_camera, scale_camera


def _free_intrinsics_mask(free_intrinsics, C):
    """(C, 6) bool from a collection of group names or a (C, 6) boolean array"""
    if isinstance(free_intrinsics, str):
        free_intrinsics = (free_intrinsics,)
    names = list(free_intrinsics) if not isinstance(free_intrinsics, np.ndarray) else None
    if names is not None and all(isinstance(n, str) for n in names):
        free = np.zeros((C, 6), dtype=bool)
        for n in names:
            if n not in INTRINSIC_GROUPS:
                raise ValueError(f"free_intrinsics: unknown group {n!r}; the groups are {sorted(INTRINSIC_GROUPS)}")
            free[:, INTRINSIC_GROUPS[n]] = True
        return free
    free = np.asarray(free_intrinsics)
    if free.shape != (C, 6) or free.dtype != np.bool_:
        raise ValueError(f"free_intrinsics must be a collection of {sorted(INTRINSIC_GROUPS)} or a ({C}, 6) bool array in the order fx fy cx cy k1 k2")
    return free.copy()


def _prior_weights(intrinsics_prior_std, C):
    """None, or the (C, 6) plane of 1 / std^2 (0 where std is inf)"""
    if intrinsics_prior_std is None:
        return None
    std = np.asarray(intrinsics_prior_std, dtype=np.float64)
    if std.shape == (6,):
        std = np.broadcast_to(std, (C, 6))
    if std.shape != (C, 6):
        raise ValueError(f"intrinsics_prior_std must be None, (6,) or ({C}, 6): one std per fx fy cx cy k1 k2")
    if not (std > 0).all():   # (NaN compares false)
        raise ValueError("intrinsics_prior_std must be positive (inf: no prior on that scalar)")
    with np.errstate(over="ignore", divide="ignore"):
        w = np.ascontiguousarray(1.0 / (std * std))
    if np.isinf(w).any():
        raise ValueError("intrinsics_prior_std is too small: 1 / std^2 is not finite")
    return w


def _held_bits12(held, C):
    held = np.asarray(held)
    if held.shape == (C, 12):
        held = (held.astype(bool).astype(np.int32) << np.arange(12, dtype=np.int32)).sum(1)
    bits = np.ascontiguousarray(held, dtype=np.int32)
    if bits.shape != (C,):
        raise ValueError("held must be (n_cameras, 12) bool or (n_cameras,) bit words, in the order fx fy cx cy k1 k2 | rotation vector | translation")
    return bits


def _refine_cameras_limit(who, C):
    if not 2 <= C <= MAX_REFINE_CAMERAS_FREE_INTRINSICS:
        raise NotImplementedError(f"{who}() takes 2 to {MAX_REFINE_CAMERAS_FREE_INTRINSICS} cameras, got {C}: 12 scalars per camera hold the reduced system to 144 rows; "
                                  'refine_extrinsics(reduction="tiled") refines the extrinsics alone of up to 64 cameras')


def _intrinsics_like(all_intrinsics, theta6):
    out = []
    for (K, d), t in zip(all_intrinsics, theta6):
        K2 = np.array(K, dtype=np.float64)
        K2[0, 0], K2[1, 1], K2[0, 2], K2[1, 2] = t[:4]
        d2 = np.array(d, dtype=np.float64)
        flat = d2.reshape(-1)   # (a view: (5,), (1, 5) and (5, 1) alike)
        if flat.size < 2:
            if np.any(t[4:6] != 0):
                d2 = np.r_[flat, np.zeros(2 - flat.size)]
                d2[:2] = t[4:6]
            elif flat.size == 1:
                flat[0] = t[4]
        else:
            flat[:2] = t[4:6]
        out.append((K2, d2))
    return out


def refine_cameras(all_uvs, all_extrinsics, all_intrinsics, *, free_intrinsics=("focal",), intrinsics_prior_std=None, points=None, inliers=None, weights=None, gauge_camera=0, scale_camera=None,
                   loss="soft_l1", f_scale=1.0, ftol=1e-8, xtol=1e-8, gtol=1e-8, max_nfev=100, verbose=0, device=0):
    """`refine_extrinsics` with the intrinsics among the unknowns: free-point bundle adjustment over the extrinsics, the chosen intrinsic scalars
    of every camera and every 3-D point.  For a rig whose intrinsics are only nominal, or a lens that was refocused: `refine_extrinsics` would
    move the camera to absorb an error that belongs to fx, fy.

        unc = calibration_uncertainty(...)                                   # from the board calibration, if there was one
        res = refine_cameras(uvs, ext, intr, free_intrinsics=("focal", "principal"), intrinsics_prior_std=unc.intrinsics_std)
        ext, intr = res.extrinsics, res.intrinsics

    free_intrinsics: any subset of "focal" (fx, fy), "principal" (cx, cy), "distortion" (k1, k2), or a (C, 6) bool array in the order
    fx fy cx cy k1 k2; () frees nothing: refine_extrinsics' problem through these kernels.  p1, p2, k3 stay constants.
    intrinsics_prior_std: None, (6,) or (C, 6) positive numbers, inf = no prior on that scalar (CalibrationUncertainty.intrinsics_std passes
    straight in): the cost gains 0.5 sum ((theta - theta_0) / std)^2 over the free intrinsic scalars, theta_0 the intrinsics given; plain
    quadratic, never through the robust loss.  Keypoints alone determine intrinsics weakly (compact scenes moved fx, fy by 5 to 7 % at
    0.3 px of noise): a prior is advised whenever one is known.
    points, inliers, weights, gauge_camera, scale_camera, loss, f_scale, ftol, xtol, gtol, max_nfev, verbose: as refine_extrinsics takes
    them.  The gauge is refine_extrinsics': the six extrinsics of gauge_camera and one translation scalar of scale_camera are held, the
    closing rescale restores the baseline; the intrinsics of the gauge camera are free like any other camera's.  A camera that no used point
    sees is held whole, all 12 scalars.
    Returns a CameraRefinement; `cost` includes `prior_cost`.  ValueError: an unknown group, a mask of the wrong shape, a std that is zero,
    negative or NaN, and what refine_extrinsics refuses.  NotImplementedError: fewer than 2 or more than 12 cameras (12 C <= 144 rows) --
    refine_extrinsics(reduction="tiled") takes the extrinsics alone of up to 64.  Without a GPU: ops.McbaError -- there is no host path."""
    from . import solver
    from .triangulation import triangulate

    if callable(loss) or loss not in ops.LOSSES:
        raise ValueError(f"loss must be one of {sorted(ops.LOSSES)}")
    if not f_scale > 0:
        raise ValueError("`f_scale` must be positive.")
    if int(max_nfev) < 2:
        raise ValueError("max_nfev must be at least 2: the start and one trial are the least a run needs")
    if min(ftol, xtol, gtol) < 0:
        raise ValueError("ftol, xtol and gtol must not be negative")
    uvs = _stack_uvs(all_uvs, all_extrinsics, all_intrinsics)
    C, P = uvs.shape[:2]
    _refine_cameras_limit("refine_cameras", C)
    free = _free_intrinsics_mask(free_intrinsics, C)
    pw = _prior_weights(intrinsics_prior_std, C)
    if P < 1:
        raise ValueError("refine_cameras() needs at least one point")
    ext0 = np.ascontiguousarray(all_extrinsics, dtype=np.float64)
    if ext0.shape != (C, 6) or not np.isfinite(ext0).all():
        raise ValueError("all_extrinsics must be finite (rotation vector, translation) rows, one per camera")
    gauge_camera = int(gauge_camera)
    if not 0 <= gauge_camera < C:
        raise ValueError("gauge_camera is not a camera of the rig")
    centres = _camera_centres(ext0)
    if scale_camera is None:
        scale_camera = int(np.argmax(np.linalg.norm(centres - centres[gauge_camera], axis=1)))
    scale_camera = int(scale_camera)
    if not 0 <= scale_camera < C:
        raise ValueError("scale_camera is not a camera of the rig")
    if scale_camera == gauge_camera:
        raise ValueError("gauge_camera == scale_camera: the scale is fixed by the distance between two different cameras")
    if inliers is not None:
        mask = np.asarray(inliers)
        if mask.shape != (C, P) or mask.dtype != np.bool_:
            raise ValueError(f"inliers must be the ({C}, {P}) bool mask of triangulate_consensus")
        uvs = np.where(mask[:, :, None], uvs, np.nan)   # (a copy: the one that is uploaded)
    w = _weight_plane(weights, C, P)
    if points is None:
        start_uvs = uvs if w is None else np.where((w > 0)[:, :, None], uvs, np.nan)
        pts = np.ascontiguousarray(triangulate(list(start_uvs), all_extrinsics, all_intrinsics, device=device))
    else:
        pts = np.ascontiguousarray(points, dtype=np.float64)
        if pts.shape != (P, 3):
            raise ValueError("points must be (n_points, 3), one row per row of the cameras' uvs")
    cam, dist = _cam_blocks(all_extrinsics, all_intrinsics)
    d = -rodrigues(ext0[scale_camera, :3]) @ (centres[scale_camera] - centres[gauge_camera])
    held12 = np.concatenate([~free, np.zeros((C, 6), dtype=bool)], axis=1)
    held12[gauge_camera, 6:] = True
    held12[scale_camera, 9 + int(np.argmax(np.abs(d)))] = True
    held_bits = _held_bits12(held12, C)
    cams, out, status, res = np.empty((C, 12)), np.empty((P, 3)), np.empty(P, np.int32), np.zeros(16)
    hist = np.zeros((int(max_nfev) + 1, 3))
    addr = lambda a: None if a is None else a.ctypes.data   # noqa: E731
    ops.call("mcba_refine_cameras", C, P, uvs.ctypes.data, addr(w), cam.ctypes.data, dist.ctypes.data, pts.ctypes.data, held_bits.ctypes.data, addr(pw), gauge_camera, scale_camera, ops.LOSSES[loss],
             float(f_scale), float(ftol), float(xtol), float(gtol), int(max_nfev), int(device), cams.ctypes.data, out.ctypes.data, status.ctypes.data, res.ctypes.data, hist.ctypes.data, len(hist))
    hist = hist[:min(int(res[7]), len(hist))].copy()
    code = int(res[5])
    if verbose == 2:
        print("{0:^15}{1:^15}{2:^15}{3:^15}{4:^15}".format("Iteration", "Total nfev", "Cost", "Cost reduction", "Damping"))
        it, last = 0, None
        for k, (c, lam, acc) in enumerate(hist):
            if acc:
                print("{0:^15}{1:^15}{2:^15.4e}{3:^15}{4:^15.2e}".format(it, k + 1, c, "" if last is None else "%.2e" % (last - c), lam))
                it, last = it + 1, c
    if verbose >= 1:
        print(solver.TERMINATION_MESSAGES[code])
        print("Function evaluations {0}, initial cost {1:.4e}, final cost {2:.4e}, first-order optimality {3:.2e}.".format(int(res[3]), res[1], res[0], res[2]))
    held = ((held_bits[:, None] >> np.arange(12)) & 1).astype(bool)
    return CameraRefinement(extrinsics=cams[:, 6:].copy(), intrinsics=_intrinsics_like(all_intrinsics, cams[:, :6]), points=out, cost=float(res[0]), prior_cost=float(res[14]), cost0=float(res[1]),
                            optimality=float(res[2]), nfev=int(res[3]), njev=int(res[4]), status=code, message=solver.TERMINATION_MESSAGES[code], success=code > 0, point_status=status, held=held,
                            scale=float(res[6]), history=hist,
                            info={"kernel_ms": float(res[8]), "reduce_ms": float(res[9]), "n_reduce": int(res[10]), "step_ms": float(res[11]), "n_step": int(res[12]), "group": int(res[13]),
                                  "gauge_camera": gauge_camera, "scale_camera": scale_camera})


def refine_cameras_system(all_uvs, all_extrinsics, all_intrinsics, *, points, held, lam, loss="soft_l1", f_scale=1.0, step=None, device=0, weights=None):
    """One evaluation of refine_cameras laid open (`mcba_refine_cameras_system`; tests and diagnostics), the counterpart of
    refine_extrinsics_system: the loop's own set-up and kernels run once at (all_extrinsics, all_intrinsics, points) and the damping lam, and
    what they wrote comes back as it is.  held: (C, 12) bool or (C,) bit words in the order fx fy cx cy k1 k2 | rotation vector |
    translation, taken as given -- no gauge, scale or blind-camera rule.  The prior does not enter: the kernels never see it.
    step: None, or (cameras_trial (C, 12), dtheta (C, 12)): also the back-substitution, the trial cost under the trial intrinsics and extrinsics.
    Returns a dict: point_status (P,); system (the raw NP NP + 102 C + 4 doubles, NP = 12 C rounded up to 16) and its views YY (NP, NP),
    acc (C, 102) = U_c packed lower (78) | g_c (12) | sum_p Y_cp z_p (12), cost, count, gmax, tail; group, workgroups, NP, kernel_ms; with a
    step trial_points (P, 3) and step4 = trial cost, sum dX^2, 0, sum X^2."""
    if callable(loss) or loss not in ops.LOSSES:
        raise ValueError(f"loss must be one of {sorted(ops.LOSSES)}")
    uvs = _stack_uvs(all_uvs, all_extrinsics, all_intrinsics)
    C, P = uvs.shape[:2]
    _refine_cameras_limit("refine_cameras_system", C)
    pts = np.ascontiguousarray(points, dtype=np.float64)
    if pts.shape != (P, 3):
        raise ValueError("points must be (n_points, 3), one row per row of the cameras' uvs")
    held_bits = _held_bits12(held, C)
    cam, dist = _cam_blocks(all_extrinsics, all_intrinsics)
    NP = (12 * C + 15) // 16 * 16
    status, system, info = np.empty(P, np.int32), np.empty(NP * NP + 102 * C + 4), np.zeros(4)
    trial = step4 = cam_trial = dtheta = None
    if step is not None:
        cam_trial, dtheta = (np.ascontiguousarray(a, dtype=np.float64) for a in step)
        if cam_trial.shape != (C, 12) or dtheta.shape != (C, 12):
            raise ValueError("step must be (cameras_trial (n_cameras, 12), dtheta (n_cameras, 12))")
        trial, step4 = np.empty((P, 3)), np.empty(4)
    addr = lambda a: None if a is None else a.ctypes.data   # noqa: E731
    w = _weight_plane(weights, C, P)
    ops.call("mcba_refine_cameras_system", C, P, uvs.ctypes.data, addr(w), cam.ctypes.data, dist.ctypes.data, pts.ctypes.data, held_bits.ctypes.data, ops.LOSSES[loss], float(f_scale), float(lam),
             int(device), addr(cam_trial), addr(dtheta), status.ctypes.data, system.ctypes.data, addr(trial), addr(step4), info.ctypes.data)
    out = dict(point_status=status, system=system, YY=system[:NP * NP].reshape(NP, NP), acc=system[NP * NP:NP * NP + 102 * C].reshape(C, 102), cost=float(system[-4]), count=float(system[-3]),
               gmax=float(system[-2]), tail=float(system[-1]), group=int(info[0]), workgroups=int(info[1]), NP=int(info[2]), kernel_ms=float(info[3]))
    if step is not None:
        out.update(trial_points=trial, step4=step4)
    return out


# ---------------------------------------------------------------- extrinsics from keypoints alone
RELATIVE_POSE_STATUS = {1: "ok", -1: "fewer than 8 common points", -2: "too few inliers", -3: "too few points for the scale"}
MAX_HYPOTHESES = ops.TWOVIEW_MAX_HYPOTHESES
MAX_FIVEPOINT_SAMPLES = ops.TWOVIEW5_MAX_SAMPLES
SOLVERS = ("8point", "5point")


def _draw(n, n_hypotheses, seed, size):
    """the drawer behind draw_samples and draw_resection_samples: one generator, one choice() without replacement per hypothesis, in order"""
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(np.stack([rng.choice(int(n), int(size), replace=False) for _ in range(int(n_hypotheses))]), dtype=np.int32)


def draw_samples(n_common, n_hypotheses, seed, size=8):
    """(n_hypotheses, size) int32: per hypothesis `size` (8, or 5 for the five-point solver) different indices in 0 .. n_common - 1, one
    `np.random.default_rng(seed).choice(n_common, size, replace=False)` each from a generator of its own -- the global numpy generator is never
    touched.  seed: anything default_rng takes (an int, a sequence of ints)."""
    if int(size) not in (8, ops.TWOVIEW5_SAMPLE):
        raise ValueError("size must be 8 (the 8-point solver) or 5 (the five-point solver)")
    if int(n_common) < 8:
        raise ValueError("a sample needs 8 different correspondences")
    return _draw(n_common, n_hypotheses, seed, size)


def _rotation_vector(R):
    """rodrigues_inv with the cosine clipped to [-1, 1]: a product of rotations may have a trace a rounding above 3"""
    v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    n = np.linalg.norm(v)
    return v * np.arccos(np.clip((np.trace(R) - 1) / 2, -1.0, 1.0)) / (n + (n == 0))


def _min_inliers(n_common):
    return max(16, n_common // 10)


def _intrinsics_rows(intrinsics_a, intrinsics_b):
    return _cam_blocks([np.zeros(6), np.zeros(6)], [intrinsics_a, intrinsics_b])


def estimate_relative_pose(uvs_a, uvs_b, intrinsics_a, intrinsics_b, *, threshold, n_hypotheses=512, seed=0, undistort_iterations=5, refine=False, loss="soft_l1", f_scale=1.0, device=0,
                           return_info=False, solver="8point"):
    """The pose of camera b relative to camera a from the keypoints both detect, with known intrinsics and nothing else:
    (transform (6,), inliers (P,) bool), transform = the rotation vector and the UNIT translation of x_b = R x_a + t (a two-view geometry
    has no scale).  uvs_a, uvs_b: (P, 2) raw detections, NaN = unseen; intrinsics: (camera_matrix, dist_coefs) each.

    Two-view RANSAC on the GPU (`mcba_two_view_ransac`, `csrc/mcba_twoview.hip`): `n_hypotheses` (at most 4096) 8-point essential matrices from
    samples drawn on the host (`draw_samples(n_common, n_hypotheses, seed)`), each scored over all common points by the truncated squared
    Sampson distance of the undistorted pixels, sum min(e^2, threshold^2); the lowest (cost, index) wins, its inliers are e^2 <= threshold^2;
    of the four (R, t) of the winner the one with most inliers in front of both cameras is returned.  `threshold` (pixels) has no default: it
    is the detector's noise.  Seeded, without atomics: two calls return the same bits.  A planar scene or a purely rotating pair is
    degenerate for the 8-point estimate: it shows as few inliers (status -2), not as an exception.  A THIN scene does not show: see `solver`.

    solver="5point" (`mcba_two_view_ransac5`, `csrc/mcba_fivepoint.hip`): the hypotheses are the essential matrices
    -- up to ten -- of `n_hypotheses` samples of FIVE correspondences (`draw_samples(..., size=5)`; at most 1024 samples), the minimal solver
    for calibrated cameras; scoring, winner and vote are the same kernels.  This is the generator for THIN scenes -- keypoints of an animal on
    an arena floor, a slab a few millimetres deep: there the 8-point estimate is not short of inliers but WRONG with status 1 (on the
    project's slab scenes it keeps a quarter to a half of the points and an essential matrix up to 0.68 from the true one in Frobenius norm),
    while the five-point winner keeps every point from an eighth of the samples.  Still out of scope, for either solver: the EXACTLY planar
    cloud -- there the essential matrix has a twin that every point satisfies; on a prototype at depth sigma 0 the twin won two pairs of three,
    at 1 mm the margins were thin, at 5 mm the right matrix won every pair with the second-best cost 1.07 to 1.41 x the winner's -- and the
    purely rotating pair.  The default stays "8point": nothing changes for a caller who does not ask.

    refine=True: `refine_extrinsics` on the two cameras with the inlier mask (`loss`, `f_scale`), |t| renormalised to 1.
    return_info=True: also a dict -- n_common, n_inliers, cost, hypothesis (the winner's index in the scored order; "5point": among the live
    candidates), sample and slot ("5point": the winner is candidate `slot` of sample `sample`; "8point": sample = hypothesis, slot = 0),
    n_scored (the candidates that were scored: n_hypotheses, or the live candidates of the five-point samples), n_in_front, points (P, 3: the two-view point of every inlier in
    camera a's frame at unit baseline, NaN elsewhere), status (`RELATIVE_POSE_STATUS`: 1 ok, -1 fewer than 8 common points: transform NaN,
    -2 fewer than max(16, a tenth of the common points) inliers: the estimate is returned but not to be trusted), samples, kernel_ms (the
    call's kernels, then prepare, hypotheses, score, finish, pose)."""
    if not threshold > 0:
        raise ValueError("`threshold` (pixels) must be positive.")
    if solver not in SOLVERS:
        raise ValueError(f"solver must be one of {SOLVERS}, got {solver!r}")
    five = solver == "5point"
    H = int(n_hypotheses)
    if five and not 1 <= H <= MAX_FIVEPOINT_SAMPLES:
        raise ValueError(f"n_hypotheses counts samples for solver='5point' and must be 1 .. {MAX_FIVEPOINT_SAMPLES}")
    if not 1 <= H <= MAX_HYPOTHESES:
        raise ValueError(f"n_hypotheses must be 1 .. {MAX_HYPOTHESES}")
    if int(undistort_iterations) < 0:
        raise ValueError("undistort_iterations must not be negative")
    ua, ub = np.asarray(uvs_a, dtype=np.float64), np.asarray(uvs_b, dtype=np.float64)
    if ua.ndim != 2 or ua.shape[1] != 2 or ua.shape != ub.shape:
        raise ValueError("uvs_a and uvs_b must both be (n_points, 2)")
    P = len(ua)
    idx = np.flatnonzero(np.isfinite(ua).all(1) & np.isfinite(ub).all(1))
    M = len(idx)
    transform, inliers, points = np.full(6, np.nan), np.zeros(P, dtype=bool), np.full((P, 3), np.nan)
    info = dict(n_common=M, n_inliers=0, cost=np.nan, hypothesis=-1, sample=-1, slot=-1, n_scored=0, n_in_front=0, points=points, status=-1, samples=None, kernel_ms=np.zeros(6))
    if M >= 8:
        cam, dist = _intrinsics_rows(intrinsics_a, intrinsics_b)
        ca, cb = np.ascontiguousarray(ua[idx]), np.ascontiguousarray(ub[idx])
        rt, best, mask, pts, ms = np.empty(12), np.empty(4), np.empty(M, dtype=np.uint8), np.empty((M, 3)), np.zeros(6)
        if five:
            samples = draw_samples(M, H, seed, size=ops.TWOVIEW5_SAMPLE)
            slot_status = np.empty(ops.TWOVIEW5_SLOTS * H, dtype=np.int32)
            ops.call("mcba_two_view_ransac5", M, ca.ctypes.data, cb.ctypes.data, cam.ctypes.data, dist.ctypes.data, H, samples.ctypes.data, float(threshold), int(undistort_iterations), int(device),
                     rt.ctypes.data, best.ctypes.data, mask.ctypes.data, pts.ctypes.data, None, None, None, slot_status.ctypes.data, ms.ctypes.data)
            won = int(best[0])
            place = dict(hypothesis=int((slot_status[:won] == 1).sum()), sample=won // ops.TWOVIEW5_SLOTS, slot=won % ops.TWOVIEW5_SLOTS, n_scored=max(1, int((slot_status == 1).sum())))
        else:
            samples = draw_samples(M, H, seed)
            ops.call("mcba_two_view_ransac", M, ca.ctypes.data, cb.ctypes.data, cam.ctypes.data, dist.ctypes.data, H, samples.ctypes.data, None, float(threshold), int(undistort_iterations), int(device),
                     rt.ctypes.data, best.ctypes.data, mask.ctypes.data, pts.ctypes.data, None, None, None, None, ms.ctypes.data)
            place = dict(hypothesis=int(best[0]), sample=int(best[0]), slot=0, n_scored=H)
        inliers[idx] = mask.astype(bool)
        points[idx] = pts
        n_in = int(best[2])
        if np.isfinite(rt).all():
            transform = np.r_[_rotation_vector(rt[:9].reshape(3, 3)), rt[9:]]
        info.update(n_inliers=n_in, cost=float(best[1]), n_in_front=int(best[3]), status=1 if n_in >= _min_inliers(M) else -2, samples=samples, kernel_ms=ms, **place)
        if refine and np.isfinite(transform).all():
            res = refine_extrinsics([ua, ub], np.stack([np.zeros(6), transform]), [intrinsics_a, intrinsics_b], inliers=np.stack([inliers, inliers]), gauge_camera=0, scale_camera=1, loss=loss,
                                    f_scale=f_scale, device=device)
            transform = res.extrinsics[1].copy()
            transform[3:] /= np.linalg.norm(transform[3:])
            info["refinement"] = res
    return (transform, inliers, info) if return_info else (transform, inliers)


@dataclass
class KeypointExtrinsics:
    extrinsics: np.ndarray     # (C, 6); the root's row is the exact zero vector
    points: np.ndarray         # (P, 3) in the root camera's frame
    tree: list                 # [(i, j), ...]: camera j placed from camera i, in the order of placement
    edges: list                # per tree edge a dict: cameras, n_common, n_inliers, cost, scale, status
    edge_inliers: np.ndarray   # (C, P) bool: row j = the inliers of the edge that placed camera j (the root's row is empty)
    refinement: object         # the ExtrinsicsRefinement, or None
    scale_camera: int
    info: dict                 # root, baseline, kernel_ms (the two-view calls), rescale (factor of the closing rescale), reduction


def _rescale_about(ext, points, root, scale_camera, baseline):
    centres = _camera_centres(ext)
    c0 = centres[root]
    s = float(baseline) / np.linalg.norm(centres[scale_camera] - c0)
    out = np.array(ext, dtype=np.float64)
    for k in range(len(out)):
        if k != root:
            out[k, 3:] = -rodrigues(out[k, :3]) @ (c0 + s * (centres[k] - c0))
    return out, c0 + s * (np.asarray(points) - c0), s


def extrinsics_from_keypoints(all_uvs, all_intrinsics, *, threshold, root=0, n_hypotheses=512, seed=0, baseline=1.0, scale_camera=None, refine=True, loss="soft_l1", f_scale=1.0, min_common=16,
                              reduction=None, device=0, solver="8point", **refine_kwargs):
    """The extrinsics of a rig from the pose estimator's keypoints alone -- known intrinsics, no board, no starting calibration -- as a
    `KeypointExtrinsics`: the initialiser in front of `refine_extrinsics` and `triangulate`.  all_uvs: per camera (P, 2) raw detections, NaN =
    unseen; all_intrinsics: per camera (camera_matrix, dist_coefs).  The frame is camera `root`'s (its extrinsics are the exact zero vector).

    The reconstruction is metric ONLY through `baseline`: keypoints fix the rig up to one global scale, and the result is scaled so that the
    distance between the centres of `root` and `scale_camera` (None: the other camera of the first tree edge) is exactly `baseline`.  Pass
    the one distance you have measured, in the unit you want the translations and points in.

    1. the maximum spanning tree of the co-visibility counts (`calibration.get_camera_spanning_tree`'s rule on the (C, P) plane of seen
       points), edges in order of distance from `root`; a tree edge with fewer than `min_common` common points: ValueError naming the cameras;
    2. `estimate_relative_pose` per tree edge (i, j), seed [seed, i, j], `threshold`, `n_hypotheses`, `solver` ("8point", the default, or
       "5point": the generator for thin scenes -- keypoints on an arena floor --, where the 8-point edges are wrong with status 1; see
       `estimate_relative_pose`; with it `n_hypotheses` counts samples, at most 1024); an edge of status -2 (too few inliers:
       a planar scene, a pure rotation, a wrong threshold): ValueError;
    3. the scale chain, in tree order: the first edge has scale 1; for a later edge (i -> j), X = `triangulate` over the cameras placed so
       far, Y = the edge's two-view points in camera i's frame, s = median(|R_i X + t_i| / |Y|) over the edge's inliers with finite X,
       T_j = [R | s t] o T_i; fewer than 8 such points: status -3, ValueError;
    4. refine=True: `refine_extrinsics(all_uvs, start, all_intrinsics, points=None, gauge_camera=root, scale_camera=..., loss=loss,
       f_scale=f_scale, reduction=..., **refine_kwargs)`; reduction None = "resident" up to 24 cameras, "tiled" beyond; more than 64 cameras:
       NotImplementedError.  refine=False returns the chained start and its `triangulate` points;
    5. the closing rescale about the root to `baseline`.
    Out of scope: loop closure over pairs outside the tree, unknown intrinsics, per-detection weights."""
    from .calibration import _spanning_tree
    from .triangulation import triangulate

    uvs = np.ascontiguousarray(np.stack([np.asarray(u, dtype=np.float64) for u in all_uvs]))
    if uvs.ndim != 3 or uvs.shape[2] != 2 or len(all_intrinsics) != len(uvs):
        raise ValueError("all_uvs must be one (n_points, 2) array per camera, matching all_intrinsics")
    C, P = uvs.shape[:2]
    if C < 2:
        raise ValueError("extrinsics_from_keypoints() needs at least two cameras")
    if C > MAX_REFINE_CAMERAS_TILED:
        raise NotImplementedError(f"extrinsics_from_keypoints() supports 2 to {MAX_REFINE_CAMERAS_TILED} cameras, got {C}")
    root = int(root)
    if not 0 <= root < C:
        raise ValueError("root is not a camera of the rig")
    if not baseline > 0:
        raise ValueError("`baseline` must be positive.")
    if reduction is None:
        reduction = "resident" if C <= MAX_REFINE_CAMERAS else "tiled"
    _reduction_limit("extrinsics_from_keypoints", reduction, C)
    if solver not in SOLVERS:
        raise ValueError(f"solver must be one of {SOLVERS}, got {solver!r}")
    if solver == "5point" and not 1 <= int(n_hypotheses) <= MAX_FIVEPOINT_SAMPLES:
        raise ValueError(f"n_hypotheses counts samples for solver='5point' and must be 1 .. {MAX_FIVEPOINT_SAMPLES}")
    seen = np.isfinite(uvs).all(-1)
    tree = [(int(i), int(j)) for i, j in _spanning_tree(seen, root)]
    for i, j in tree:
        n = int((seen[i] & seen[j]).sum())
        if n < int(min_common):
            raise ValueError(f"cameras {i} and {j} share {n} points, fewer than min_common = {int(min_common)}: the rig is not connected by keypoints")
    if scale_camera is None:
        scale_camera = tree[0][1] if tree[0][0] == root else tree[0][0]
    scale_camera = int(scale_camera)
    if not 0 <= scale_camera < C or scale_camera == root:
        raise ValueError("scale_camera must be a camera of the rig other than root")
    intr = list(all_intrinsics)
    T = {root: (np.eye(3), np.zeros(3))}
    edges, edge_inliers, kernel_ms = [], np.zeros((C, P), dtype=bool), 0.0
    for n, (i, j) in enumerate(tree):
        tr, inl, info = estimate_relative_pose(uvs[i], uvs[j], intr[i], intr[j], threshold=threshold, n_hypotheses=n_hypotheses, seed=[int(seed), i, j], device=device, return_info=True, solver=solver)
        kernel_ms += float(info["kernel_ms"][0])
        edge = dict(cameras=(i, j), n_common=info["n_common"], n_inliers=info["n_inliers"], cost=info["cost"], scale=np.nan, status=info["status"])
        edges.append(edge)
        if info["status"] != 1:
            raise ValueError(f"cameras {i} and {j}: {RELATIVE_POSE_STATUS[info['status']]} ({info['n_inliers']} of {info['n_common']} common points within {threshold} px)")
        R, t = rodrigues(tr[:3]), tr[3:]
        Ri, ti = T[i]
        s = 1.0
        if n > 0:
            placed = sorted(T)
            X = triangulate([uvs[c] for c in placed], np.stack([np.r_[_rotation_vector(T[c][0]), T[c][1]] for c in placed]), [intr[c] for c in placed], device=device)
            Y = info["points"]
            ok = inl & np.isfinite(X).all(1) & np.isfinite(Y).all(1)
            if int(ok.sum()) < 8:
                edge["status"] = -3
                raise ValueError(f"cameras {i} and {j}: {RELATIVE_POSE_STATUS[-3]} ({int(ok.sum())} inliers are also seen by two placed cameras)")
            s = float(np.median(np.linalg.norm(X[ok] @ Ri.T + ti, axis=1) / np.linalg.norm(Y[ok], axis=1)))
        edge["scale"] = s
        T[j] = (R @ Ri, R @ ti + s * t)
        edge_inliers[j] = inl
    ext0 = np.zeros((C, 6))
    for c in range(C):
        if c != root:
            ext0[c] = np.r_[_rotation_vector(T[c][0]), T[c][1]]
    res = None
    if refine:
        res = refine_extrinsics(list(uvs), ext0, intr, points=None, gauge_camera=root, scale_camera=scale_camera, loss=loss, f_scale=f_scale, reduction=reduction, device=device, **refine_kwargs)
        ext, pts = res.extrinsics, res.points
    else:
        ext, pts = ext0, triangulate(list(uvs), ext0, intr, device=device)
    ext, pts, factor = _rescale_about(ext, pts, root, scale_camera, baseline)
    return KeypointExtrinsics(extrinsics=ext, points=pts, tree=tree, edges=edges, edge_inliers=edge_inliers, refinement=res, scale_camera=scale_camera,
                              info=dict(root=root, baseline=float(baseline), kernel_ms=kernel_ms, rescale=factor, reduction=reduction))


# ---------------------------------------------------------------- camera resection
RESECTION_STATUS = {1: "ok", -1: "fewer than 6 usable points", -2: "too few inliers"}
MAX_RESECTION_HYPOTHESES = ops.RESECT_MAX_HYPOTHESES
MAX_RESECTION_CAMERAS = ops.RESECT_MAX_CAMERAS
RESECTION_SOLVERS = ("dlt6", "p3p")     # the hypothesis generators of resect_camera / resect_cameras (SURVEY.md sections 8f-16, 8f-18)
MAX_RESECTION_P3P_SAMPLES = ops.RESECT_P3P_MAX_SAMPLES


def draw_resection_samples(n_usable, n_hypotheses, seed, size=6):
    """(n_hypotheses, size) int32: per hypothesis `size` different indices in 0 .. n_usable - 1, one
    `np.random.default_rng(seed).choice(n_usable, size, replace=False)` each from a generator of its own -- the global numpy generator is never
    touched.  seed: anything default_rng takes (an int, a sequence of ints).  The indices count the camera's usable points in their order.
    size: 6 (the samples of solver="dlt6") or 3 (solver="p3p")."""
    if size not in (ops.RESECT_SAMPLE, ops.RESECT_P3P_SAMPLE):
        raise ValueError("size must be 6 (dlt6) or 3 (p3p)")
    if int(n_usable) < size:
        raise ValueError(f"a sample needs {size} different points")
    return _draw(n_usable, n_hypotheses, seed, size)


def _min_resection_inliers(n_usable):
    return max(12, n_usable // 10)


@dataclass
class CameraResection:
    extrinsics: np.ndarray     # (C, 6) rotation vector, translation of x_cam = R X + t; NaN rows where status is -1
    inliers: np.ndarray        # (C, P) bool: the winning hypothesis' inliers
    status: np.ndarray         # (C,) RESECTION_STATUS
    n_usable: np.ndarray       # (C,) points with a finite position and a finite detection
    n_inliers: np.ndarray      # (C,)
    cost: np.ndarray           # (C,) the winner's truncated cost, sum min(e^2, threshold^2) in px^2
    hypothesis: np.ndarray     # (C,) the winner's index, -1 where status is -1; solver="p3p": its slot, the sample is hypothesis // 4
    refined_cost: np.ndarray   # (C,) the polish: robust cost 0.5 sum rho(f^2) over the inliers' raw detections at the result; NaN where it did not run
    optimality: np.ndarray     # (C,) inf-norm of its gradient
    nfev: np.ndarray           # (C,) its evaluations
    lm_status: np.ndarray      # (C,) scipy's: 0 max_nfev, 1 gtol, 2 ftol, 3 xtol; -1 where it did not run
    info: dict                 # samples (per camera, indices into 0 .. P - 1, None where status is -1), ransac_extrinsics (C, 6): the winning
    #                            hypotheses before the polish, kernel_ms: dict(ransac=(total, prepare, hypotheses, score, finish, mask), polish=the span of its evaluations)


def _resect(points, uvs, intr, seeds, threshold, n_hypotheses, undistort_iterations, refine, loss, f_scale, ftol, xtol, gtol, max_nfev, device, solver="dlt6"):
    if not threshold > 0:
        raise ValueError("`threshold` (pixels) must be positive.")
    if solver not in RESECTION_SOLVERS:
        raise ValueError(f"solver must be one of {RESECTION_SOLVERS}")
    H = int(n_hypotheses)
    p3p = solver == "p3p"
    size, h_max = (ops.RESECT_P3P_SAMPLE, MAX_RESECTION_P3P_SAMPLES) if p3p else (ops.RESECT_SAMPLE, MAX_RESECTION_HYPOTHESES)
    if not 1 <= H <= h_max:
        raise ValueError(f"n_hypotheses must be 1 .. {h_max}" + (" samples with solver=\"p3p\"" if p3p else ""))
    if int(undistort_iterations) < 0:
        raise ValueError("undistort_iterations must not be negative")
    if loss not in ops.LOSSES:
        raise ValueError(f"loss must be one of {sorted(ops.LOSSES)}")
    if not f_scale > 0:
        raise ValueError("`f_scale` must be positive.")
    if int(max_nfev) < 2:
        raise ValueError("max_nfev must be at least 2")
    pts = np.ascontiguousarray(points, dtype=np.float64)
    if pts.ndim != 2 or pts.shape[1] != 3 or len(pts) == 0:
        raise ValueError("points must be (n_points, 3), at least one")
    if uvs.ndim != 3 or uvs.shape[1:] != (len(pts), 2) or len(uvs) != len(intr):
        raise ValueError("one (n_points, 2) array of detections and one (camera_matrix, dist_coefs) per camera, matching points, required")
    C, P = len(uvs), len(pts)
    if not 1 <= C <= MAX_RESECTION_CAMERAS:
        raise ValueError(f"1 .. {MAX_RESECTION_CAMERAS} cameras per call")
    cam, dist = _cam_blocks([np.zeros(6)] * C, intr)
    usable = np.isfinite(pts).all(1)[None, :] & np.isfinite(uvs).all(2)
    n_usable = usable.sum(1)
    samples, per_camera = np.zeros((C, H, size), dtype=np.int32), [None] * C
    for c in range(C):
        if n_usable[c] >= ops.RESECT_SAMPLE:
            samples[c] = np.flatnonzero(usable[c]).astype(np.int32)[draw_resection_samples(n_usable[c], H, seeds[c], size=size)]
            per_camera[c] = samples[c]
    rt, best, mask, ms = np.empty((C, 12)), np.empty((C, 4)), np.zeros((C, P), dtype=np.uint8), np.zeros(6)
    if p3p:
        ops.call("mcba_resect_ransac_p3p", C, P, pts.ctypes.data, uvs.ctypes.data, cam.ctypes.data, dist.ctypes.data, H, samples.ctypes.data, float(threshold), int(undistort_iterations), int(device),
                 rt.ctypes.data, best.ctypes.data, mask.ctypes.data, None, None, None, None, ms.ctypes.data)
    else:
        ops.call("mcba_resect_ransac", C, P, pts.ctypes.data, uvs.ctypes.data, cam.ctypes.data, dist.ctypes.data, H, samples.ctypes.data, None, float(threshold), int(undistort_iterations), int(device),
                 rt.ctypes.data, best.ctypes.data, mask.ctypes.data, None, None, None, None, ms.ctypes.data)
    ext = np.full((C, 6), np.nan)
    for c in range(C):
        if np.isfinite(rt[c]).all():
            ext[c] = np.r_[_rotation_vector(rt[c, :9].reshape(3, 3)), rt[c, 9:]]
    n_in = best[:, 2].astype(np.int64)
    status = np.where(n_usable < ops.RESECT_SAMPLE, -1, np.where(n_in >= np.maximum(12, n_usable // 10), 1, -2)).astype(np.int32)
    out = CameraResection(extrinsics=ext, inliers=mask.astype(bool), status=status, n_usable=n_usable.astype(np.int64), n_inliers=n_in, cost=best[:, 1].copy(),
                          hypothesis=best[:, 0].astype(np.int64), refined_cost=np.full(C, np.nan), optimality=np.full(C, np.nan), nfev=np.zeros(C, dtype=np.int64),
                          lm_status=np.full(C, -1, dtype=np.int64), info=dict(samples=per_camera, ransac_extrinsics=ext.copy(), kernel_ms=dict(ransac=ms, polish=0.0)))
    active = np.ascontiguousarray((status != -1) & np.isfinite(ext).all(1), dtype=np.int32)
    if refine and active.any():
        cam[:, 6:] = np.where(active[:, None] != 0, ext, 0.0)
        new, res, pms = np.empty((C, 6)), np.empty((C, 8)), np.zeros(2)
        ops.call("mcba_resect_refine", C, P, pts.ctypes.data, uvs.ctypes.data, mask.ctypes.data, cam.ctypes.data, dist.ctypes.data, active.ctypes.data, ops.LOSSES[loss], float(f_scale), float(ftol),
                 float(xtol), float(gtol), int(max_nfev), int(device), new.ctypes.data, res.ctypes.data, None, pms.ctypes.data)
        on = active != 0
        out.extrinsics[on] = new[on]
        out.refined_cost[on], out.optimality[on] = res[on, 1], res[on, 2]
        out.nfev[on], out.lm_status[on] = res[on, 3].astype(np.int64), res[on, 5].astype(np.int64)
        out.info["kernel_ms"]["polish"] = float(pms[0])
        out.info["polish_evaluations"] = int(pms[1])
    return out


def resect_cameras(points, all_uvs, all_intrinsics, *, threshold, n_hypotheses=256, seed=0, undistort_iterations=5, refine=True, loss="soft_l1", f_scale=1.0, ftol=1e-8, xtol=1e-8, gtol=1e-8,
                   max_nfev=50, device=0, solver="dlt6"):
    """Resection: the pose of every camera from known 3-D points and that camera's own 2-D detections of them -> `CameraResection`.
    points: (P, 3) in the world frame, a NaN row = unknown; all_uvs: per camera (P, 2) raw detections, NaN = unseen; all_intrinsics: per
    camera (camera_matrix, dist_coefs).  A point is usable for a camera when its position and its detection are finite.  The cameras are
    independent problems solved in one call of the library (`mcba_resect_ransac`, `csrc/mcba_resect.hip`: the camera is a grid dimension);
    camera c draws its samples from the seed `[seed, c]`, so row c equals `resect_camera(..., seed=[seed, c])`.  No camera's former pose is
    an input: a knocked, refocused or newly added camera is placed against the points the others triangulate.

    PnP RANSAC on the GPU: per camera `n_hypotheses` (at most 4096) poses, each the 6-point DLT of a host-drawn sample
    (`draw_resection_samples(n_usable, n_hypotheses, seed)`) settled by ten Gauss-Newton iterations on its six points, each scored over all
    usable points by the truncated squared reprojection error of the undistorted pixels, sum min(e^2, threshold^2), a point behind the
    camera counting in full; the lowest (cost, index) wins, its inliers are e^2 <= threshold^2 in front of the camera.  `threshold` (pixels)
    has no default: it is the detector's noise.  Seeded, without atomics: two calls return the same bits.

    status (`RESECTION_STATUS`): 1 ok; -1 fewer than 6 usable points: the row is NaN, nothing is launched for that camera, the others are
    unaffected; -2 fewer than max(12, a tenth of the usable points) inliers: the estimate is returned but not to be trusted -- coplanar
    points end here, not in an exception: the 6-point DLT is degenerate for them, a sample whose DLT start is not defined (eigen-gap below
    1e-10) is void, and with every hypothesis void the row is NaN and has no inlier.

    refine=True: every camera of status 1 or -2 is polished on its inliers by a pose-only Levenberg-Marquardt (`mcba_resect_refine`): the
    robust cost (`loss`, `f_scale`, as `refine_extrinsics`) of the raw detections under the five-coefficient model, the points fixed; ftol,
    xtol, gtol, max_nfev and `lm_status` are scipy.optimize.least_squares'.  The cost never rises, every camera stops on its own.
    refine=False: the winning hypotheses.

    solver (`RESECTION_SOLVERS`): "dlt6", the default, is the generator above.  "p3p" (`mcba_resect_ransac_p3p`, `csrc/mcba_resect_p3p.hip`,
    SURVEY.md section 8f-18) draws `n_hypotheses` (at most 1024) SAMPLES of three points (`draw_resection_samples(..., size=3)`); each gives up
    to four poses -- the real roots of Grunert's quartic, settled by five Gauss-Newton iterations on the three points --, all of them scored
    like any hypothesis: four table slots per sample, `hypothesis` is the winning slot and `hypothesis // 4` its sample.  Scoring, status
    rules (a camera still needs 6 usable points) and the polish are the same.  Use "p3p" where the points lie in or near a plane (floor marks,
    arena landmarks, an animal flatter than the noise: the 6-point DLT has no defined start there, and between 0.05 mm of depth and the noise
    it can win with a wrong pose and status 1), and where more than about a third of the detections are wrong (a clean 3-point sample is
    drawn 1 / (1 - outlier share)^3 times as often as a clean 6-point one).  Use "dlt6" otherwise: six points average the noise of a
    hypothesis, and a sample costs one slot of scoring, not four.  Caveat: a plane seen nearly fronto-parallel from far away has a second pose
    of almost equal reprojection cost; the scorer picks the lower cost and promises nothing more."""
    uvs = np.ascontiguousarray(np.stack([np.asarray(u, dtype=np.float64) for u in all_uvs])) if len(all_uvs) else np.zeros((0, 0, 2))
    return _resect(points, uvs, list(all_intrinsics), [[int(seed), c] for c in range(len(uvs))] if np.ndim(seed) == 0 else [list(np.ravel(seed)) + [c] for c in range(len(uvs))], threshold,
                   n_hypotheses, undistort_iterations, refine, loss, f_scale, ftol, xtol, gtol, max_nfev, device, solver)


def resect_camera(points, uvs, intrinsics, *, threshold, n_hypotheses=256, seed=0, undistort_iterations=5, refine=True, loss="soft_l1", f_scale=1.0, ftol=1e-8, xtol=1e-8, gtol=1e-8, max_nfev=50,
                  device=0, return_info=False, solver="dlt6"):
    """One camera of `resect_cameras`: (transform (6,), inliers (P,) bool), transform = (rotation vector, translation) of x_cam = R X + t,
    the convention of `all_extrinsics` everywhere; NaN when fewer than 6 points are usable.  points: (P, 3), uvs: (P, 2) raw detections,
    intrinsics: (camera_matrix, dist_coefs); the samples come from `seed` itself.  return_info=True: also the `CameraResection` of the one camera.
    solver: "dlt6" or "p3p" as there -- "p3p" for coplanar or nearly coplanar points and for heavy outlier shares, `n_hypotheses` (at most
    1024) then counts 3-point samples of up to four poses each; a nearly fronto-parallel distant plane has a second pose of almost equal
    cost, and the lower cost wins."""
    u = np.asarray(uvs, dtype=np.float64)
    if u.ndim != 2:
        raise ValueError("uvs must be (n_points, 2)")
    r = _resect(points, np.ascontiguousarray(u[None]), [intrinsics], [seed], threshold, n_hypotheses, undistort_iterations, refine, loss, f_scale, ftol, xtol, gtol, max_nfev, device, solver)
    return (r.extrinsics[0], r.inliers[0], r) if return_info else (r.extrinsics[0], r.inliers[0])


# ---------------------------------------------------------------- host helpers (numpy; the reference's formulas)
def euclidean_to_homogenous(x_euclidean):
    """(..., d) -> (..., d + 1) with a trailing 1 (geometry.py:232)."""
    x = np.asarray(x_euclidean)
    return np.concatenate((x, np.ones(x.shape[:-1] + (1,))), axis=-1)


def homogeneous_to_euclidean(x_homogenous):
    """(..., d + 1) -> (..., d): the leading coordinates over the last (geometry.py:255)."""
    x = np.asarray(x_homogenous)
    return x[..., :-1] / x[..., -1:]


def get_projection_matrix(extrinsics, intrinsics):
    """P = K [R | t] (3, 4) from extrinsics (6,) and intrinsics (camera_matrix, dist_coefs) (geometry.py:200)."""
    camera_matrix, _ = intrinsics
    return np.matmul(camera_matrix, get_transformation_matrix(extrinsics)[:3])


def rigid_transform_from_correspondences(source_points, target_points):
    """(t (6,), rmsd): the rigid transform that takes source_points (..., 3) onto target_points in the least-squares sense (Kabsch: SVD of the
    centred cross-covariance, a reflection turned back into a rotation) and the root mean square distance left (geometry.py:68)."""
    from .flatibration import rigid_transform_from_correspondences as fit

    source = np.asarray(source_points, dtype=np.float64).reshape(-1, 3)
    target = np.asarray(target_points, dtype=np.float64).reshape(-1, 3)
    t = fit(source, target)
    T = get_transformation_matrix(t)
    moved = np.matmul(T, euclidean_to_homogenous(source)[..., np.newaxis])[..., :3, 0]
    return t, np.sqrt(np.mean(np.sum((moved - target) ** 2, axis=1)))
