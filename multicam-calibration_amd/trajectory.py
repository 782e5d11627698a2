"""smooth_trajectories -- the fixed-interval smoother of keypoint tracks: T frames x K keypoints of triangulated points and their per-frame
covariances in, gap-free tracks out; trajectory_uncertainty -- the covariance of every smoothed point and, on request,
of neighbouring frames (section 8f-20).  It fills the frames fewer than two cameras saw, trusts each frame exactly as much
as `triangulation_uncertainty` says, and with a robust loss discounts gross triangulation errors.

The reference has no counterpart (its flatibration tutorial loads keypoints that an outside tool smoothed in time).  Everything runs on the GPU:
per track and IRLS iteration one block-pentadiagonal SPD system, solved by a recursive partitioned (Schur) elimination."""
import ctypes
from dataclasses import dataclass

import numpy as np

from . import ops

TRAJECTORY_STATUS = {1: "ok", -1: "fewer than two usable frames", -2: "a block pivot below the threshold"}
LOSSES = {"linear": 0, "soft_l1": 1, "huber": 2}
SEGMENT_MIN, SEGMENT_MAX = 2, 64


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
    cov6 = _covariance_planes(covariance, T, K)
    acc = np.asarray(accel_std, dtype=np.float64)
    if acc.shape not in ((), (K,)):
        raise ValueError(f"accel_std must be a scalar or ({K},)")
    acc = np.ascontiguousarray(np.broadcast_to(acc, (K,)))
    with np.errstate(over="ignore", divide="ignore"):
        if not (np.isfinite(acc).all() and (acc > 0).all() and np.isfinite(1.0 / (acc * acc)).all()):
            raise ValueError("accel_std must be positive and finite")
    return pts, cov6, acc


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


def smooth_trajectories(points, covariance, *, accel_std, loss="linear", f_scale=3.0, weights_in=None, max_iterations=50, xtol=1e-8, segment=None, device=0, uncertainty=False):
    """Smooth K independent keypoint tracks of T frames.  Per track k, with unknowns x_t in R^3, minimise

        0.5 f^2 sum_t rho(d_t^2 / f^2) + 0.5 / a_k^2 sum_{t=1}^{T-2} |x_{t-1} - 2 x_t + x_{t+1}|^2,    d_t^2 = (x_t - p_t)^T Sigma_t^-1 (x_t - p_t)

    points (T, K, 3): p, NaN = missing.  covariance (T, K, 3, 3): Sigma, for example
    `triangulation_uncertainty(...).covariance.reshape(T, K, 3, 3)`; a scalar, (K,) or (T, K) standard deviation means isotropic.
    accel_std: a, the standard deviation of the second difference in the points' unit per frame^2; a scalar or (K,), positive and finite.
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
    if callable(loss) or loss not in LOSSES:
        if loss in ("cauchy", "arctan"):
            raise ValueError(f"smooth_trajectories: loss {loss!r} is not convex -- the reweighting loop is a majorise-minimise scheme only for linear, soft_l1 and huber")
        raise ValueError(f"loss must be one of {sorted(LOSSES)}")
    pts, cov6, acc = _track_arguments(points, covariance, accel_std)
    T, K = pts.shape[:2]
    if not (np.isfinite(f_scale) and f_scale > 0):
        raise ValueError("`f_scale` must be positive.")
    win = _weights_argument(weights_in, "weights_in", T, K)
    max_iterations = int(max_iterations)
    if max_iterations < 1:
        raise ValueError("max_iterations must be at least 1")
    if not xtol >= 0:
        raise ValueError("xtol must not be negative")
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
    Hessian-based covariance is out of scope.  covariance takes the three forms of smooth_trajectories.

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
