"""smooth_trajectories -- the fixed-interval smoother of keypoint tracks: T frames x K keypoints of triangulated points and their per-frame
covariances in, gap-free tracks out; trajectory_uncertainty -- the covariance of every smoothed point and, on request,
of neighbouring frames (section 8f-20); refine_trajectories -- the same tracks refined on the raw detections, the maximum-likelihood fit of what
was measured (section 8f-21); estimate_accel_std and trajectory_evidence -- accel_std, which all of them require, from the tracks themselves:
the maximum of the smoother's evidence (section 8f-24).  The smoother fills the frames fewer than two cameras saw, trusts each frame exactly as much
as `triangulation_uncertainty` says, and with a robust loss discounts gross triangulation errors.

The reference has no counterpart (its flatibration tutorial loads keypoints that an outside tool smoothed in time).  Everything runs on the GPU:
per track and IRLS iteration one block-pentadiagonal SPD system, solved by a recursive partitioned (Schur) elimination."""
import ctypes
from dataclasses import dataclass

import numpy as np

from . import ops
from .triangulation import _cam_blocks

TRAJECTORY_STATUS = {1: "ok", -1: "fewer than two usable frames", -2: "a block pivot below the threshold"}
TRAJECTORY_REFINE_STATUS = {1: "ok", -1: "fewer than two usable frames", -2: "a block pivot below the threshold", -3: "a non-finite start"}
LOSSES = {"linear": 0, "soft_l1": 1, "huber": 2}
SEGMENT_MIN, SEGMENT_MAX = 2, 64
MAX_CAMERAS = 64   # of the calls on raw detections: the camera table of one launch


@dataclass
class TrajectorySmoothing:
    points: np.ndarray        # (T, K, 3): every frame filled for a track of status 1, NaN otherwise
    weights: np.ndarray       # (T, K): the last IRLS weights rho'(d^2 / f_scale^2), 0 on unusable frames
    mahalanobis2: np.ndarray  # (T, K): d_t^2 at the result, NaN on unusable frames
    status: np.ndarray        # (K,): a key of TRAJECTORY_STATUS
    n_usable: np.ndarray      # (K,)
    n_iterations: np.ndarray  # (K,): linear solves done
    cost: np.ndarray          # (K,): the objective at the result, NaN unless the status is 1
    history: np.ndarray       # (iterations, K, 2): per solve the objective at its result and its step max |x_new - x_old| (inf for the first); NaN where a track no longer ran
    info: dict                # kernel_ms, levels, segment, tracks_per_chunk, chunks, device_bytes
    covariance: np.ndarray = None      # uncertainty=True or "lag": TrajectoryUncertainty.covariance at the returned weights
    std: np.ndarray = None             # ... and its std
    lag_covariance: np.ndarray = None  # uncertainty="lag": TrajectoryUncertainty.lag_covariance


@dataclass
class TrajectoryUncertainty:
    covariance: np.ndarray      # (T, K, 3, 3): Z_tt of every frame, unusable ones included (there: the interpolation uncertainty); NaN unless the status is 1
    std: np.ndarray             # (T, K, 3): the square roots of its diagonal
    lag_covariance: np.ndarray  # (T - 1, K, 3, 3): Z_{t,t+1}, rows of frame t (not symmetric); None unless lag=True
    status: np.ndarray          # (K,): a key of TRAJECTORY_STATUS
    n_usable: np.ndarray        # (K,)
    info: dict                  # kernel_ms, levels, segment, tracks_per_chunk, chunks, device_bytes


def _covariance_planes(covariance, T, K):
    """(T, K, 6) packed 00 01 02 11 12 22 from (T, K, 3, 3), or from a scalar / (K,) / (T, K) standard deviation (isotropic)"""
    cov = np.asarray(covariance, dtype=np.float64)
    if cov.shape == (T, K, 3, 3):
        return np.ascontiguousarray(np.stack([cov[..., 0, 0], cov[..., 0, 1], cov[..., 0, 2], cov[..., 1, 1], cov[..., 1, 2], cov[..., 2, 2]], axis=-1))
    if cov.shape in ((), (K,), (T, K)):
        var = np.broadcast_to(cov * cov, (T, K))
        out = np.zeros((T, K, 6))
        out[..., 0] = out[..., 3] = out[..., 5] = var
        return out
    raise ValueError(f"covariance must be ({T}, {K}, 3, 3), or a scalar, ({K},) or ({T}, {K}) standard deviation; got {cov.shape}")


def _track_arguments(points, covariance, accel_std):
    """the arrays every call of this module takes, checked: points (T, K, 3), cov6 (T, K, 6), accel_std (K,)"""
    pts = np.ascontiguousarray(points, dtype=np.float64)
    if pts.ndim != 3 or pts.shape[2] != 3:
        raise ValueError("points must be (T, K, 3)")
    T, K = pts.shape[:2]
    if T == 0 or K == 0:
        raise ValueError("points must hold at least one frame and one track")
    return pts, _covariance_planes(covariance, T, K), _accel_argument(accel_std, K)


def _accel_argument(accel_std, K):
    """accel_std, a scalar or (K,), as (K,), checked"""
    acc = np.asarray(accel_std, dtype=np.float64)
    if acc.shape not in ((), (K,)):
        raise ValueError(f"accel_std must be a scalar or ({K},)")
    acc = np.ascontiguousarray(np.broadcast_to(acc, (K,)))
    with np.errstate(over="ignore", divide="ignore"):
        if not (np.isfinite(acc).all() and (acc > 0).all() and np.isfinite(1.0 / (acc * acc)).all()):
            raise ValueError("accel_std must be positive and finite")
    return acc


def _weights_argument(weights, name, T, K):
    """a (T, K) weights array under its parameter's name, checked; None stays None"""
    if weights is None:
        return None
    win = np.ascontiguousarray(weights, dtype=np.float64)
    if win.shape != (T, K):
        raise ValueError(f"{name} must be ({T}, {K})")
    if not (np.isfinite(win).all() and (win >= 0).all()):
        raise ValueError(f"{name} must be finite and not negative")
    return win


def _check_segment(segment):
    if segment is not None and not SEGMENT_MIN <= int(segment) <= SEGMENT_MAX:
        raise ValueError(f"segment must be None or {SEGMENT_MIN} .. {SEGMENT_MAX}")


def _check_loss(loss, caller, loop="the backtracking Gauss-Newton loop is for", known=LOSSES):
    """the loops of this module and of refine_skeleton_trajectories take the three convex losses; known: what an unknown loss is told the choice is"""
    if callable(loss) or loss not in LOSSES:
        if not callable(loss) and loss in ("cauchy", "arctan"):
            raise ValueError(f"{caller}: loss {loss!r} is not convex -- {loop} linear, soft_l1 and huber")
        raise ValueError(f"loss must be one of {sorted(known)}")


def _loop_arguments(max_iterations, xtol):
    """max_iterations as an int, both checked"""
    max_iterations = int(max_iterations)
    if max_iterations < 1:
        raise ValueError("max_iterations must be at least 1")
    if not xtol >= 0:
        raise ValueError("xtol must not be negative")
    return max_iterations


def _detection_arguments(caller, noun, start, all_uvs, all_extrinsics, all_intrinsics, pixel_std, f_scale, weights, max_keypoints=None):
    """the checked arrays every call on raw detections takes: pts (T, K, 3), uvs (C, T, K, 2), cam (C, 12), dist (C, 5), pstd (C,), w (C, T, K) or
    None.  caller and noun ("track" or "keypoint") go into the messages; max_keypoints: the caller's limit on K, if it has one.  The order of
    the checks is the order in which a call reports what is wrong: the loss first (the caller's), then these -- start, the cameras, all_uvs,
    pixel_std, f_scale, weights -- then the caller's further arguments (accel_std, the bones, cg_tol, cg_max, segment)"""
    pts = np.ascontiguousarray(start, dtype=np.float64)
    if pts.ndim != 3 or pts.shape[2] != 3:
        raise ValueError("start must be (T, K, 3)")
    T, K = pts.shape[:2]
    if T == 0 or K == 0:
        raise ValueError(f"start must hold at least one frame and one {noun}")
    if max_keypoints is not None and K > max_keypoints:
        raise ValueError(f"{caller} supports at most {max_keypoints} keypoints")
    if len(all_extrinsics) != len(all_intrinsics) or len(all_extrinsics) < 1:
        raise ValueError("one (camera_matrix, dist_coefs) per entry of all_extrinsics, at least one camera")
    C = len(all_extrinsics)
    if C > MAX_CAMERAS:
        raise ValueError(f"{caller} supports at most {MAX_CAMERAS} cameras")
    if len(all_uvs) != C:
        raise ValueError(f"all_uvs must be ({C}, {T}, {K}, 2), or a list of {C} arrays ({T}, {K}, 2)")
    uvs = [np.asarray(u, dtype=np.float64) for u in all_uvs]
    if any(u.shape != (T, K, 2) for u in uvs):
        raise ValueError(f"all_uvs must be ({C}, {T}, {K}, 2), or a list of {C} arrays ({T}, {K}, 2)")
    uvs = np.ascontiguousarray(np.stack(uvs))
    cam, dist = _cam_blocks(all_extrinsics, all_intrinsics)
    pstd = np.asarray(pixel_std, dtype=np.float64)
    if pstd.shape not in ((), (C,)):
        raise ValueError(f"pixel_std must be a scalar or ({C},)")
    pstd = np.ascontiguousarray(np.broadcast_to(pstd, (C,)))
    with np.errstate(over="ignore", divide="ignore"):
        if not (np.isfinite(pstd).all() and (pstd > 0).all() and np.isfinite(1.0 / pstd).all()):
            raise ValueError("pixel_std must be positive and finite")
    if not (np.isfinite(f_scale) and f_scale > 0):
        raise ValueError("`f_scale` must be positive.")
    w = None
    if weights is not None:
        w = np.ascontiguousarray(weights, dtype=np.float64)
        if w.shape != (C, T, K):
            raise ValueError(f"weights must be ({C}, {T}, {K}): one per camera, frame and {noun}, got {w.shape}")
        if (w < 0).any() or np.isinf(w).any():
            raise ValueError("weights must be finite and not negative (0 or NaN: the detection is unseen)")
    return pts, uvs, cam, dist, pstd, w


def smooth_trajectories(points, covariance, *, accel_std, loss="linear", f_scale=3.0, weights_in=None, max_iterations=50, xtol=1e-8, segment=None, device=0, uncertainty=False):
    """Smooth K independent keypoint tracks of T frames.  Per track k, with unknowns x_t in R^3, minimise

        0.5 f^2 sum_t rho(d_t^2 / f^2) + 0.5 / a_k^2 sum_{t=1}^{T-2} |x_{t-1} - 2 x_t + x_{t+1}|^2,    d_t^2 = (x_t - p_t)^T Sigma_t^-1 (x_t - p_t)

    points (T, K, 3): p, NaN = missing.  covariance (T, K, 3, 3): Sigma, for example
    `triangulation_uncertainty(...).covariance.reshape(T, K, 3, 3)`; a scalar, (K,) or (T, K) standard deviation means isotropic.
    accel_std: a, the standard deviation of the second difference in the points' unit per frame^2; a scalar or (K,), positive and finite.
    estimate_accel_std() finds it from the tracks themselves.
    loss: scipy's "linear", "soft_l1" or "huber" rho; f = f_scale is in units of Mahalanobis distance.  "cauchy" and "arctan" are refused:
    the loop below is a majorise-minimise scheme only for a convex rho, and on a scene with 10 % gross errors it settled far from the truth
    (arctan) or did not settle in 30 iterations (cauchy).

    A frame is usable when p_t and Sigma_t are finite and Sigma_t is positive definite (every pivot of its Jacobi-scaled Cholesky factor has a
    square >= 1e-12, the rule of triangulation_uncertainty).  An unusable frame has no data term and is filled by the smoothness term: a gap gets
    the natural cubic through its neighbours, a missing end is extrapolated linearly.

    The robust losses are solved by iteratively reweighted least squares: weights w_t = rho'(d_t^2 / f^2) start at 1 (or at weights_in, (T, K),
    finite and >= 0), every iteration is one linear solve, and a track stops when max |x_new - x_old| < xtol max |x_new| or at max_iterations;
    the objective never rises.  The linear loss is one solve.  max_iterations=1 with weights_in is one solve with exactly those weights.
    segment: pairs of frames between two separators of the elimination, 2 .. 64 (None: the library default); a tuning knob, the result is the
    same to rounding.

    status (TRAJECTORY_STATUS): -1 fewer than two usable frames (the system is positive definite exactly from two on); -2 a pivot of a
    Jacobi-scaled 6 x 6 block whose square fell below 1e-12.  Such a track is NaN; the others are unaffected.
    uncertainty: True or "lag" -- after the solve, trajectory_uncertainty() at the returned weights with the same segment and device fills
    covariance and std (and, for "lag", lag_covariance).  False (the default): the three fields are None and the call is the solve alone.

    ValueError (before a device is touched): wrong shapes, T == 0 or K == 0, accel_std <= 0 or not finite, f_scale <= 0, a loss outside the
    three, a negative or non-finite weights_in, max_iterations < 1, segment out of range, uncertainty not one of False, True, "lag".
    Without a GPU: ops.McbaError -- there is no host path."""
    if not any(uncertainty is u for u in (False, True)) and uncertainty != "lag":
        raise ValueError('uncertainty must be False, True or "lag"')
    _check_loss(loss, "smooth_trajectories", "the reweighting loop is a majorise-minimise scheme only for")
    pts, cov6, acc = _track_arguments(points, covariance, accel_std)
    T, K = pts.shape[:2]
    if not (np.isfinite(f_scale) and f_scale > 0):
        raise ValueError("`f_scale` must be positive.")
    win = _weights_argument(weights_in, "weights_in", T, K)
    max_iterations = _loop_arguments(max_iterations, xtol)
    _check_segment(segment)

    out, w, d2 = np.empty((T, K, 3)), np.empty((T, K)), np.empty((T, K))
    status, nus, nit = np.empty(K, np.int32), np.empty(K, np.int32), np.empty(K, np.int32)
    hist, info = np.empty((max_iterations, K, 2)), np.zeros(8)
    ms = ctypes.c_double(0.0)
    ops.call("mcba_smooth_trajectories", T, K, pts.ctypes.data, cov6.ctypes.data, acc.ctypes.data, None if win is None else win.ctypes.data, LOSSES[loss], float(f_scale), max_iterations,
             float(xtol), 0 if segment is None else int(segment), int(device), out.ctypes.data, w.ctypes.data, d2.ctypes.data, status.ctypes.data, nus.ctypes.data, nit.ctypes.data, hist.ctypes.data,
             info.ctypes.data, ctypes.addressof(ms))
    n = int(nit.max())
    hist = np.ascontiguousarray(hist[:n])
    cost = np.full(K, np.nan)
    ran = (status == 1) & (nit > 0)
    cost[ran] = hist[nit[ran] - 1, np.flatnonzero(ran), 0]
    res = TrajectorySmoothing(points=out, weights=w, mahalanobis2=d2, status=status, n_usable=nus, n_iterations=nit, cost=cost, history=hist, info=_info(info))
    if uncertainty is not False:
        u = _uncertainty(pts, cov6, acc, w, uncertainty == "lag", segment, device)
        res.covariance, res.std, res.lag_covariance = u.covariance, u.std, u.lag_covariance
    return res


def _info(info8):
    return {"kernel_ms": float(info8[4]), "levels": int(info8[0]), "segment": int(info8[1]), "tracks_per_chunk": int(info8[2]), "chunks": int(info8[3]), "device_bytes": int(info8[6])}


_SYM = np.array([[0, 1, 2], [1, 3, 4], [2, 4, 5]])


def trajectory_uncertainty(points, covariance, *, accel_std, weights=None, lag=False, segment=None, device=0):
    """The covariance of every smoothed point.  Per track let A = blockdiag(w_t Sigma_t^-1) + a^-2 (D2^T D2 (x) I3) be
    exactly the matrix of smooth_trajectories (same arguments, same usable-frame rule, w_t = 0 on unusable frames) and Z = A^-1.  Returned:

        covariance[t, k] = Z_tt for every frame -- on an unusable frame it is the interpolation uncertainty of the filled point;
        std[t, k] = the square roots of its diagonal;
        lag_covariance[t, k] = Z_{t,t+1}, t = 0 .. T - 2 (lag=True only; not symmetric, rows belong to frame t).

    The covariance of a frame-to-frame displacement is  Cov(x_{t+1} - x_t) = Z_tt + Z_{t+1,t+1} - Z_{t,t+1} - Z_{t,t+1}^T;  it is left to the
    caller because it cancels: form it where the precision it needs is known.

    For the linear loss (weights=None) Z is the exact posterior covariance under the second-difference prior.  For soft_l1 / huber pass
    weights = result.weights = rho'(d^2 / f^2): Z is then the weighted-least-squares covariance at those weights.  The rho'' term of a
    Hessian-based covariance is out of scope.  covariance takes the three forms of smooth_trajectories.  Every Z is conditional on accel_std:
    estimate_accel_std() finds it from the tracks themselves.

    Everything runs on the GPU: the elimination of the smoother once, then a selected inversion over the same separator tree.  Two calls return
    the same bits, whatever the chunking.  status as in smooth_trajectories; a track of status -1 or -2 is NaN throughout.
    ValueError (before a device is touched): wrong shapes, T == 0 or K == 0, accel_std <= 0 or not finite, a negative or non-finite weight,
    segment out of range.  Without a GPU: ops.McbaError -- there is no host path."""
    pts, cov6, acc = _track_arguments(points, covariance, accel_std)
    T, K = pts.shape[:2]
    win = _weights_argument(weights, "weights", T, K)
    _check_segment(segment)
    return _uncertainty(pts, cov6, acc, win, bool(lag), segment, device)


def _uncertainty(pts, cov6, acc, win, lag, segment, device):
    """the call itself, on checked arrays: points (T, K, 3), cov6 (T, K, 6), acc (K,), win (T, K) or None"""
    T, K = pts.shape[:2]
    c6, l9 = np.empty((T, K, 6)), np.empty((T - 1, K, 9)) if lag else None
    status, nus, info = np.empty(K, np.int32), np.empty(K, np.int32), np.zeros(8)
    ms = ctypes.c_double(0.0)
    ops.call("mcba_smooth_covariance", T, K, pts.ctypes.data, cov6.ctypes.data, acc.ctypes.data, None if win is None else win.ctypes.data, 0 if segment is None else int(segment), int(device),
             c6.ctypes.data, None if l9 is None else l9.ctypes.data, status.ctypes.data, nus.ctypes.data, info.ctypes.data, ctypes.addressof(ms))
    full = np.ascontiguousarray(c6[..., _SYM])
    with np.errstate(invalid="ignore"):
        std = np.sqrt(full[..., (0, 1, 2), (0, 1, 2)])
    return TrajectoryUncertainty(covariance=full, std=std, lag_covariance=None if l9 is None else l9.reshape(T - 1, K, 3, 3), status=status, n_usable=nus, info=_info(info))


@dataclass
class TrajectoryEvidence:
    neg2_log_evidence: np.ndarray  # (K,): N(a) = data + penalty + log_det + 6 (T - 2) log a; NaN unless the status is 1
    data: np.ndarray               # (K,): sum_t w_t d_t^2 at the linear solve
    penalty: np.ndarray            # (K,): a^-2 sum_t |x_{t-1} - 2 x_t + x_{t+1}|^2 there
    log_det: np.ndarray            # (K,): log det A(a)
    status: np.ndarray             # (K,): a key of TRAJECTORY_STATUS
    n_usable: np.ndarray           # (K,)
    info: dict                     # kernel_ms, levels, segment, tracks_per_chunk, chunks, device_bytes, log_det_ms (the log-determinant kernels and the final sums)


@dataclass
class AccelEstimate:
    accel_std: np.ndarray               # (K,): the estimate, pooled tracks sharing their unit's; NaN unless the status is 1
    log_std: np.ndarray                 # (K,): the standard deviation of log accel_std from the curvature of N; NaN on an edge or without curvature
    edge: np.ndarray                    # (K,): -1 the minimum lies on accel_range[0], +1 on accel_range[1], 0 inside
    status: np.ndarray                  # (K,): a key of TRAJECTORY_STATUS; -2: a pivot was refused at every candidate of the track's unit
    n_usable: np.ndarray                # (K,)
    grid: np.ndarray                    # (G,): the candidates of the grid
    neg2_log_evidence_grid: np.ndarray  # (G, K): every track's N on the grid; NaN where a pivot was refused and for tracks that do not run
    neg2_log_evidence: np.ndarray       # (K,): the track's N at accel_std
    n_evaluations: int                  # linear solves per track: n_grid + 2 + rounds + 2
    info: dict                          # as TrajectoryEvidence.info, and evaluations


def _evidence_info(info8):
    out = _info(info8)
    out["log_det_ms"] = float(info8[7])
    return out


def trajectory_evidence(points, covariance, *, accel_std, weights=None, segment=None, device=0):
    """One evaluation of the smoother's evidence laid open.  Per track, with A(a) exactly the matrix of
    trajectory_uncertainty (same arguments, same usable-frame rule, w_t = weights, 1 by default and 0 on unusable frames), x(a) its linear solve
    and a = accel_std,

        N(a) = sum_t w_t d_t^2(x) + a^-2 sum_t |x_{t-1} - 2 x_t + x_{t+1}|^2 + log det A(a) + 6 (T - 2) log a

    is -2 x the log restricted marginal likelihood of a, up to a constant in a: the exact evidence of the model of loss="linear", and with
    weights from a robust run the evidence of the reweighted model.  Returned per track: N, its data term, its penalty and log det A, which is
    summed on the GPU from the Cholesky factors the elimination stores.  Two calls return the same bits, whatever the chunking.
    status as in smooth_trajectories; a track of status -1 or -2 is NaN throughout.  ValueError and ops.McbaError as trajectory_uncertainty."""
    pts, cov6, acc = _track_arguments(points, covariance, accel_std)
    T, K = pts.shape[:2]
    win = _weights_argument(weights, "weights", T, K)
    _check_segment(segment)
    out4, status, nus, info = np.empty((K, 4)), np.empty(K, np.int32), np.empty(K, np.int32), np.zeros(8)
    ms = ctypes.c_double(0.0)
    ops.call("mcba_smooth_evidence", T, K, pts.ctypes.data, cov6.ctypes.data, acc.ctypes.data, None if win is None else win.ctypes.data, 0 if segment is None else int(segment), int(device),
             out4.ctypes.data, status.ctypes.data, nus.ctypes.data, info.ctypes.data, ctypes.addressof(ms))
    return TrajectoryEvidence(neg2_log_evidence=out4[:, 0].copy(), data=out4[:, 1].copy(), penalty=out4[:, 2].copy(), log_det=out4[:, 3].copy(), status=status, n_usable=nus,
                              info=_evidence_info(info))


def estimate_accel_std(points, covariance, *, accel_range, n_grid=17, rtol=1e-3, weights=None, pool=None, segment=None, device=0):
    """Estimate accel_std from the tracks themselves: the value that maximises the smoother's evidence, that is,
    minimises N(a) of trajectory_evidence.  points, covariance, weights, segment as there.  accel_range = (lo, hi), 0 < lo < hi: the search
    stays inside it.  pool: None -- every track gets its own estimate; "all" -- one value for every running track; a (K,) array of integer
    labels -- one value per label; a unit's objective is the sum of its running tracks' N.

    The rule is deterministic: N on a grid of n_grid >= 3 values spaced evenly in log a, its first argmin g*; a golden-section search in log a
    on the two grid steps around g* until the bracket is narrower than rtol (in [1e-6, 1)); the estimate is the evaluated candidate with the
    lowest N.  log_std = sqrt(2 / kappa) with kappa the second difference of N at log a +- 0.2: the standard deviation of log accel_std in
    the Laplace approximation.  A minimum on the first or the last grid value is reported as edge = -1 or +1 with accel_std = lo or hi and
    log_std NaN: widen the range.  With the defaults that is 17 + 16 + 2 linear solves per track; the detections cross to the GPU once.

    The model is the weighted Gaussian one: no robust loss runs inside the estimator.  For outlier-laden tracks pass
    weights = smooth_trajectories(..., loss="soft_l1", accel_std=provisional).weights.  The estimate carries over to refine_trajectories and
    refine_skeleton_trajectories, whose prior is the same.

    status (TRAJECTORY_STATUS): -1 fewer than two usable frames; -2 a pivot was refused at every candidate.  Such a track is NaN.  Two calls
    return the same bits; an unpooled call also whatever the chunking.  A pooled call runs as one chunk and is refused (ops.McbaError naming
    MCBA_SMOOTH_BUDGET_MB) when it does not fit the device-memory budget.
    ValueError (before a device is touched): the errors of trajectory_uncertainty, T < 3 (with two frames the evidence does not depend on
    accel_std), accel_range not 0 < lo < hi with finite inverse squares, n_grid < 3, rtol outside [1e-6, 1), a pool that is none of the three
    forms.  Without a GPU: ops.McbaError -- there is no host path."""
    rng = np.asarray(accel_range, dtype=np.float64)
    if rng.shape != (2,):
        raise ValueError("accel_range must be (lo, hi)")
    lo, hi = float(rng[0]), float(rng[1])
    with np.errstate(over="ignore", divide="ignore"):
        if not (np.isfinite(rng).all() and 0 < lo < hi and np.isfinite(1.0 / (rng * rng)).all() and (1.0 / (rng * rng) > 0).all()):
            raise ValueError("accel_range must be 0 < lo < hi, finite, with finite inverse squares")
    pts, cov6, _ = _track_arguments(points, covariance, lo)
    T, K = pts.shape[:2]
    if T < 3:
        raise ValueError("estimate_accel_std needs at least 3 frames: with 2 the evidence does not depend on accel_std")
    n_grid = int(n_grid)
    if n_grid < 3:
        raise ValueError("n_grid must be at least 3")
    if not 1e-6 <= rtol < 1:
        raise ValueError("rtol must lie in [1e-6, 1)")
    win = _weights_argument(weights, "weights", T, K)
    _check_segment(segment)
    if pool is None:
        units = None
    elif isinstance(pool, str):
        if pool != "all":
            raise ValueError('pool must be None, "all" or a (K,) array of integer labels')
        units = np.zeros(K, np.int32)
    else:
        lab = np.asarray(pool)
        if lab.shape != (K,) or lab.dtype.kind not in "iu":
            raise ValueError(f'pool must be None, "all" or a ({K},) array of integer labels')
        units = np.ascontiguousarray(np.unique(lab, return_inverse=True)[1].reshape(K), dtype=np.int32)
    acc, ls, nb = np.empty(K), np.empty(K), np.empty(K)
    edge, status, nus, nev = np.empty(K, np.int32), np.empty(K, np.int32), np.empty(K, np.int32), np.zeros(1, np.int32)
    grid, ng, info = np.empty(n_grid), np.empty((n_grid, K)), np.zeros(8)
    ms = ctypes.c_double(0.0)
    ops.call("mcba_estimate_accel_std", T, K, pts.ctypes.data, cov6.ctypes.data, lo, hi, n_grid, float(rtol), None if win is None else win.ctypes.data,
             None if units is None else units.ctypes.data, 0 if segment is None else int(segment), int(device), acc.ctypes.data, ls.ctypes.data, edge.ctypes.data, status.ctypes.data,
             nus.ctypes.data, grid.ctypes.data, ng.ctypes.data, nb.ctypes.data, nev.ctypes.data, info.ctypes.data, ctypes.addressof(ms))
    inf = _evidence_info(info)
    inf["evaluations"] = int(info[5])
    return AccelEstimate(accel_std=acc, log_std=ls, edge=edge, status=status, n_usable=nus, grid=grid, neg2_log_evidence_grid=ng, neg2_log_evidence=nb, n_evaluations=int(nev[0]), info=inf)


@dataclass
class TrajectoryRefinement:
    points: np.ndarray        # (T, K, 3): every frame filled for a track of status 1, NaN otherwise
    information: np.ndarray   # (T, K, 3, 3): H_t, the Gauss-Newton matrix of the frame's detections at the result (rank 2 on a single frame, 0 on an unseen one)
    status: np.ndarray        # (K,): a key of TRAJECTORY_REFINE_STATUS
    n_usable: np.ndarray      # (K,): frames two cameras or more see
    n_single: np.ndarray      # (K,): frames exactly one camera sees
    n_iterations: np.ndarray  # (K,): linear solves done
    cost: np.ndarray          # (K,): the objective at the result, NaN unless the status is 1
    history: np.ndarray       # (iterations, K, 3): per iteration the objective after it, the accepted step alpha max |d| and alpha; NaN where a track no longer ran
    info: dict                # kernel_ms, levels, segment, tracks_per_chunk, chunks, device_bytes
    covariance: np.ndarray = None      # uncertainty=True or "lag": (T, K, 3, 3), Z_tt of the inverse of the Gauss-Newton matrix at the result
    std: np.ndarray = None             # ... and the square roots of its diagonal
    lag_covariance: np.ndarray = None  # uncertainty="lag": (T - 1, K, 3, 3), Z_{t,t+1}, rows of frame t


@dataclass
class TrajectoryRefinementSystem:
    information: np.ndarray   # (T, K, 3, 3): H_t at the given points
    gradient: np.ndarray      # (T, K, 3): G, the gradient of the whole objective
    step: np.ndarray          # (T, K, 3): d, the solution of (blockdiag(H) + a^-2 D2^T D2 (x) I3) d = -G
    data_cost: np.ndarray     # (K,): the data term of the objective at the points
    penalty_cost: np.ndarray  # (K,): its smoothness term
    trial_costs: np.ndarray   # (K, 4): the objective at x + alpha d, alpha = 1, 1/2, 1/4, 1/8
    status: np.ndarray        # (K,): a key of TRAJECTORY_REFINE_STATUS
    n_usable: np.ndarray      # (K,)
    n_single: np.ndarray      # (K,)
    info: dict                # as TrajectoryRefinement.info


def _refine_arguments(start, all_uvs, all_extrinsics, all_intrinsics, accel_std, pixel_std, loss, f_scale, weights, segment):
    """the checked arrays both refinement calls take: start (T, K, 3), uvs (C, T, K, 2), cam (C, 12), dist (C, 5), acc (K,), pstd (C,), w (C, T, K) or None"""
    _check_loss(loss, "refine_trajectories")
    pts, uvs, cam, dist, pstd, w = _detection_arguments("refine_trajectories", "track", start, all_uvs, all_extrinsics, all_intrinsics, pixel_std, f_scale, weights)
    acc = _accel_argument(accel_std, pts.shape[1])
    _check_segment(segment)
    return pts, uvs, cam, dist, acc, pstd, w


def refine_trajectories(start, all_uvs, all_extrinsics, all_intrinsics, *, accel_std, pixel_std=1.0, loss="linear", f_scale=3.0, weights=None, max_iterations=30, xtol=1e-8, segment=None,
                        device=0, uncertainty=False):
    """Refine K independent keypoint tracks of T frames on their raw detections.  Per track k, with unknowns x_t in
    R^3, minimise

        0.5 sum_t sum_{c sees (t,k)} f^2 [rho(ru^2 / f^2) + rho(rv^2 / f^2)] + 0.5 / a_k^2 sum_{t=1}^{T-2} |x_{t-1} - 2 x_t + x_{t+1}|^2,
        (ru, rv) = sqrt(w_ctk) (detection - projection_c(x_t)) / pixel_std_c

    start (T, K, 3): where the iteration begins -- the intended start is `smooth_trajectories(...).points`, which has every frame filled.
    all_uvs (C, T, K, 2) or a list of C arrays (T, K, 2): raw detections, NaN = unseen.  all_extrinsics, all_intrinsics: the cameras as
    `refine_triangulation` takes them (the five-coefficient forward model), at most 64.  accel_std: a, a scalar or (K,); estimate_accel_std()
    finds it from triangulated tracks, and the estimate carries over because the prior is the same.  pixel_std: the
    detection noise in pixels, a scalar or (C,).  loss: scipy's "linear", "soft_l1" or "huber" rho per scalar residual, f = f_scale in units
    of pixel_std; "cauchy" and "arctan" are refused.  weights: None or (C, T, K) per-detection weights as `refine_triangulation` takes them
    (0 or NaN: the detection is unseen).

    A frame is usable when two cameras or more see it and single when exactly one does; a single frame still pins two of the point's three
    coordinates, which the two-stage chain triangulate -> smooth_trajectories discards.  A track runs when it has at least two usable frames
    (they pin the motions linear in time, the null space of the smoothness term) and its start is finite throughout.

    Gauss-Newton in step form: per iteration one linearisation, one solve of the block-pentadiagonal system by the smoother's elimination
    (`segment` as there), one evaluation of the objective at x + alpha d for alpha = 1, 1/2, 1/4, 1/8: the largest alpha whose objective is
    not above the current one is taken (none: the track stops where it is, alpha = 0 in its history), and a track stops when
    alpha max |d| < xtol max |x| or after max_iterations.  The objective never rises.  Two calls return the same bits, whatever the chunking.

    status (TRAJECTORY_REFINE_STATUS): -1 fewer than two usable frames; -2 a refused 6 x 6 pivot; -3 a non-finite start.  Such a track is NaN
    throughout; the others are unaffected.
    uncertainty: True or "lag" -- covariance and std (and, for "lag", lag_covariance) are Z_tt (and Z_{t,t+1}) of the inverse of the
    Gauss-Newton matrix blockdiag(H_t) + a^-2 D2^T D2 (x) I3 at the returned points: the covariance in units where pixel_std is the detection noise.

    ValueError (before a device is touched): wrong shapes, T == 0 or K == 0, more than 64 cameras, accel_std, pixel_std or f_scale not positive
    and finite, a loss outside the three, a negative or infinite weight, max_iterations < 1, xtol < 0, segment out of range, uncertainty not one
    of False, True, "lag".  Without a GPU: ops.McbaError -- there is no host path."""
    if not any(uncertainty is u for u in (False, True)) and uncertainty != "lag":
        raise ValueError('uncertainty must be False, True or "lag"')
    pts, uvs, cam, dist, acc, pstd, w = _refine_arguments(start, all_uvs, all_extrinsics, all_intrinsics, accel_std, pixel_std, loss, f_scale, weights, segment)
    C, T, K = uvs.shape[:3]
    max_iterations = _loop_arguments(max_iterations, xtol)
    out, h6 = np.empty((T, K, 3)), np.empty((T, K, 6))
    status, nus, nsg, nit = (np.empty(K, np.int32) for _ in range(4))
    cost, hist, info = np.empty(K), np.empty((max_iterations, K, 3)), np.zeros(8)
    c6 = np.empty((T, K, 6)) if uncertainty is not False else None
    l9 = np.empty((T - 1, K, 9)) if uncertainty == "lag" else None
    ms = ctypes.c_double(0.0)
    ops.call("mcba_refine_trajectories", T, K, C, uvs.ctypes.data, cam.ctypes.data, dist.ctypes.data, None if w is None else w.ctypes.data, pstd.ctypes.data, pts.ctypes.data, acc.ctypes.data,
             LOSSES[loss], float(f_scale), max_iterations, float(xtol), 0 if segment is None else int(segment), int(device), out.ctypes.data, h6.ctypes.data, status.ctypes.data, nus.ctypes.data,
             nsg.ctypes.data, nit.ctypes.data, cost.ctypes.data, hist.ctypes.data, None if c6 is None else c6.ctypes.data, None if l9 is None else l9.ctypes.data, info.ctypes.data,
             ctypes.addressof(ms))
    res = TrajectoryRefinement(points=out, information=np.ascontiguousarray(h6[..., _SYM]), status=status, n_usable=nus, n_single=nsg, n_iterations=nit, cost=cost,
                               history=np.ascontiguousarray(hist[:int(nit.max())]), info=_info(info))
    if c6 is not None:
        res.covariance = np.ascontiguousarray(c6[..., _SYM])
        with np.errstate(invalid="ignore"):
            res.std = np.sqrt(res.covariance[..., (0, 1, 2), (0, 1, 2)])
        res.lag_covariance = None if l9 is None else l9.reshape(T - 1, K, 3, 3)
    return res


def refine_trajectories_system(points, all_uvs, all_extrinsics, all_intrinsics, *, accel_std, pixel_std=1.0, loss="linear", f_scale=3.0, weights=None, segment=None, device=0):
    """One evaluation of refine_trajectories laid open, at `points` (T, K, 3) and before anything is accepted: the information blocks H_t, the
    gradient G of the whole objective, the step d of (blockdiag(H) + a^-2 D2^T D2 (x) I3) d = -G, the data and the smoothness term of the objective
    at the points and the objective at x + alpha d for alpha = 1, 1/2, 1/4, 1/8 -- what a test holds against a dense oracle.  Arguments, statuses
    and errors as refine_trajectories; a track whose status is not 1 is NaN throughout."""
    pts, uvs, cam, dist, acc, pstd, w = _refine_arguments(points, all_uvs, all_extrinsics, all_intrinsics, accel_std, pixel_std, loss, f_scale, weights, segment)
    C, T, K = uvs.shape[:3]
    h6, g, d = np.empty((T, K, 6)), np.empty((T, K, 3)), np.empty((T, K, 3))
    status, nus, nsg = (np.empty(K, np.int32) for _ in range(3))
    dc, pc, tc, info = np.empty(K), np.empty(K), np.empty((K, 4)), np.zeros(8)
    ms = ctypes.c_double(0.0)
    ops.call("mcba_refine_trajectories_system", T, K, C, uvs.ctypes.data, cam.ctypes.data, dist.ctypes.data, None if w is None else w.ctypes.data, pstd.ctypes.data, pts.ctypes.data,
             acc.ctypes.data, LOSSES[loss], float(f_scale), 0 if segment is None else int(segment), int(device), h6.ctypes.data, g.ctypes.data, d.ctypes.data, status.ctypes.data,
             nus.ctypes.data, nsg.ctypes.data, dc.ctypes.data, pc.ctypes.data, tc.ctypes.data, info.ctypes.data, ctypes.addressof(ms))
    return TrajectoryRefinementSystem(information=np.ascontiguousarray(h6[..., _SYM]), gradient=g, step=d, data_cost=dc, penalty_cost=pc, trial_costs=tc, status=status, n_usable=nus,
                                      n_single=nsg, info=_info(info))
