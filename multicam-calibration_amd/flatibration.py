"""Floor-plane alignment ("flatibration") on the GPU: SURVEY.md section 8f-5; reference multicam_calibration/flatibration.py.

Same signatures and return values as the reference's four public functions; extra arguments are keyword-only.  The per-point work
runs in HIP kernels (csrc/mcba_flat.hip, include/mcba.h "floor-plane alignment"); the host keeps what is O(100) scalars:

  get_floor_points  per frame the keypoint of smallest (largest) z, np.argmin / np.argmax semantics (mcba_flat_floor_points).
  flatibrate        what the reference gets from sklearn's RANSACRegressor(residual_threshold=...) with its defaults (LinearRegression,
                    min_samples 3, max_trials 100, stop_probability 0.99, absolute-error loss, the global numpy RNG), then the rigid
                    transform of the four-point correspondence.  The 100 subsets are drawn up front from a COPY of the global RNG
                    exactly as sklearn's sample_without_replacement draws them; one launch scores every hypothesis against every point
                    (exact inlier count + the inliers' moments, from which the R^2 tie-break and the final least-squares fit follow);
                    sklearn's sequential loop is replayed over those scalars, and the global RNG is then left where sklearn leaves it.
  center_arena      the transformed points' percentiles / median (exact order statistics by radix select on the device) or mean.
  flip_z_axis       6-vector arithmetic on the host.

sklearn is not imported.  Without a GPU every function but flip_z_axis raises ops.McbaError.
"""
import numpy as np

from . import ops
from .calibration import get_transformation_matrix, get_transformation_vector, rodrigues_inv

MIN_SAMPLES = 3  # sklearn RANSACRegressor defaults for a LinearRegression estimator on 2 features
MAX_TRIALS = 100
STOP_PROBABILITY = 0.99
MAX_KEYPOINTS = 2048  # MCBA_FLAT_MAX_KEYPOINTS
_EPSILON = np.spacing(1)  # sklearn/linear_model/_ransac.py


def _concat(a):
    return np.concatenate(a) if isinstance(a, list) else a


# ------------------------------------------------------------------ get_floor_points (flatibration.py:40-60)
def get_floor_points(keypoints, z_points_down=False, *, device=0, return_index=False):
    """keypoints (n_frames, n_keypoints, 3), or a list of such arrays (concatenated).  Returns (n_frames, 3): per frame the keypoint
    with the smallest z (the largest if z_points_down), exactly as np.argmin / np.argmax pick it.  return_index: also the indices."""
    kp = np.asarray(_concat(keypoints))
    if kp.ndim != 3 or kp.shape[2] != 3:
        raise ValueError("keypoints must have shape (n_frames, n_keypoints, 3)")
    F, K = kp.shape[:2]
    if K == 0:
        raise ValueError("attempt to get argmin of an empty sequence")
    if K > MAX_KEYPOINTS:
        raise NotImplementedError("get_floor_points supports at most %d keypoints per frame" % MAX_KEYPOINTS)
    data = np.ascontiguousarray(kp, dtype=np.float64)
    out = np.empty((F, 3))
    idx = np.empty(F, dtype=np.int32)
    ops.call("mcba_flat_floor_points", F, K, data.ctypes.data, int(bool(z_points_down)), int(device), out.ctypes.data, idx.ctypes.data, None)
    if np.issubdtype(kp.dtype, np.floating) and kp.dtype != np.float64:
        out = out.astype(kp.dtype)  # (exact: the values were widened, compared and copied)
    return (out, idx.astype(np.intp)) if return_index else out


# ------------------------------------------------------------------ RANSAC: sklearn's draws, its loop, its final fit
def sample_subset(n, rng):
    """sklearn.utils.random.sample_without_replacement(n, 3, method="auto", random_state=rng), restated: the permutation method for
    0.01 < 3 / n < 0.99, tracking selection (scalar randint, duplicates redrawn) below, reservoir sampling above (n == 3 only)."""
    ratio = MIN_SAMPLES / n
    if 0.01 < ratio < 0.99:
        return rng.permutation(n)[:MIN_SAMPLES]
    if ratio < 0.2:
        out, seen = np.empty(MIN_SAMPLES, dtype=int), set()
        for i in range(MIN_SAMPLES):
            j = rng.randint(n)
            while j in seen:
                j = rng.randint(n)
            seen.add(j)
            out[i] = j
        return out
    out = np.arange(MIN_SAMPLES)
    for i in range(MIN_SAMPLES, n):
        j = rng.randint(0, i + 1)
        if j < MIN_SAMPLES:
            out[j] = i
    return out


def draw_subsets(n, trials=MAX_TRIALS):
    """The subsets of `trials` RANSAC trials, drawn from a copy of numpy's global RNG.  Returns (trials, 3) indices and the RNG state
    after each trial's draw (states[k] = after k trials; states[0] = now).  The global RNG itself is not touched."""
    rng = np.random.RandomState()
    rng.set_state(np.random.get_state())
    states = [rng.get_state()]
    idx = np.empty((trials, MIN_SAMPLES), dtype=np.intp)
    for t in range(trials):
        idx[t] = sample_subset(n, rng)
        states.append(rng.get_state())
    return idx, states


def hypotheses(points, idx):
    """LinearRegression().fit of z on (x, y) for each 3-point subset: centred least squares, minimum-norm when the three xy points are
    collinear (lstsq's cut-off max(shape) * eps).  Returns (T, 3) = (a, b, c) of z = a x + b y + c."""
    X = points[idx, :2]
    y = points[idx, 2]
    xm = X.mean(axis=1)
    ym = y.mean(axis=1)
    coef = np.einsum("tij,tj->ti", np.linalg.pinv(X - xm[:, None], rcond=MIN_SAMPLES * _EPSILON), y - ym[:, None])
    return np.column_stack([coef, ym - np.einsum("ti,ti->t", xm, coef)])


def _centred(counts, moments):
    n = np.asarray(counts, dtype=np.float64)
    X, Y, R, XX, XY, YY, XR, YR, RR = np.asarray(moments, dtype=np.float64).T
    with np.errstate(divide="ignore", invalid="ignore"):
        return n, X, Y, R, XX - X * X / n, XY - X * Y / n, YY - Y * Y / n, XR - X * R / n, YR - Y * R / n, RR


def r2_scores(planes, counts, moments):
    """sklearn's estimator.score on each hypothesis' inliers (r2_score, force_finite) from the kernel's moments.  The inliers' z is
    a x + b y + c + r, so SS_tot = a^2 Sxx + 2ab Sxy + b^2 Syy + 2a Sxr + 2b Syr + Srr of centred moments; SS_res = sum r^2."""
    a, b = planes[:, 0], planes[:, 1]
    n, X, Y, R, Sxx, Sxy, Syy, Sxr, Syr, RR = _centred(counts, moments)
    with np.errstate(divide="ignore", invalid="ignore"):
        Srr = RR - R * R / n
        sstot = a * a * Sxx + 2 * a * b * Sxy + b * b * Syy + 2 * a * Sxr + 2 * b * Syr + Srr
        score = np.where(RR == 0, 1.0, np.where(sstot == 0, 0.0, 1 - RR / sstot))
    return np.where(n < 2, np.nan, score)  # r2_score: "not well-defined with less than two samples"


def dynamic_max_trials(n_inliers, n_samples, min_samples=MIN_SAMPLES, probability=STOP_PROBABILITY):
    """sklearn.linear_model._ransac._dynamic_max_trials."""
    inlier_ratio = n_inliers / float(n_samples)
    nom = max(_EPSILON, 1 - probability)
    denom = max(_EPSILON, 1 - inlier_ratio**min_samples)
    if nom == 1:
        return 0
    if denom == 1:
        return float("inf")
    return abs(float(np.ceil(np.log(nom) / np.log(denom))))


def replay(counts, scores, n_samples, max_trials=MAX_TRIALS):
    """sklearn's sequential RANSAC loop over per-trial (inlier count, score).  Returns (winning trial or -1, n_trials, tie margin): the
    smallest |score difference| that decided a tie in inlier count (inf if none did)."""
    best_n, best_score, best, limit, t, margin = 1, -np.inf, -1, max_trials, 0, np.inf
    while t < limit:
        t += 1
        k, s = int(counts[t - 1]), float(scores[t - 1])
        if k < best_n:
            continue
        if k == best_n and best >= 0:
            margin = min(margin, abs(s - best_score))
        if k == best_n and s < best_score:
            continue
        best_n, best_score, best = k, s, t - 1
        limit = min(limit, dynamic_max_trials(best_n, n_samples))
    return best, t, margin


def final_fit(plane, count, moment, shift):
    """LinearRegression().fit on the winning inliers from their moments (centred 2 x 2 normal equations; minimum norm when the inliers'
    xy are collinear).  Returns (a, b, c)."""
    a, b, c = plane
    n, X, Y, R, Sxx, Sxy, Syy, Sxr, Syr, _ = _centred([count], [moment])
    n, X, Y, R, Sxx, Sxy, Syy, Sxr, Syr = (float(v[0]) if np.ndim(v) else float(v) for v in (n, X, Y, R, Sxx, Sxy, Syy, Sxr, Syr))
    S = np.array([[Sxx, Sxy], [Sxy, Syy]])
    rcond = (max(n, 2) * _EPSILON) ** 2  # lstsq's cut-off on the singular values of the centred data, squared: S = Xc^T Xc
    sv = np.linalg.svd(S, compute_uv=False)
    if sv[1] > rcond * sv[0]:
        coef = np.array([a, b]) + np.linalg.solve(S, [Sxr, Syr])
    else:  # regress z itself (not the residual) so that the minimum-norm solution is lstsq's
        coef = np.linalg.pinv(S, rcond=rcond) @ (S @ np.array([a, b]) + np.array([Sxr, Syr]))
    xbar, ybar = shift[0] + X / n, shift[1] + Y / n
    return coef[0], coef[1], c + R / n + (a - coef[0]) * xbar + (b - coef[1]) * ybar


def rigid_transform_from_correspondences(source, target):
    """Least-squares rotation + translation taking source onto target (Kabsch: SVD of the centred cross-covariance, reflection
    removed).  Returns the 6-vector (rotation vector, translation)."""
    source = np.asarray(source, dtype=np.float64).reshape(-1, 3)
    target = np.asarray(target, dtype=np.float64).reshape(-1, 3)
    cs, ct = source.mean(axis=0), target.mean(axis=0)
    U, _, Vt = np.linalg.svd((source - cs).T @ (target - ct))
    R = Vt.T @ U.T
    if np.linalg.det(R) < 0:
        Vt[-1, :] *= -1
        R = Vt.T @ U.T
    return np.concatenate([rodrigues_inv(R), ct - R @ cs])


def plane_transform(a, b, c):
    """The rigid transform that takes the plane z = a x + b y + c to z = 0: (0, 0, c) to the origin, (1, 0, a) onto the x axis, (0, 1, b)
    onto the y axis and the normal (-a, -b, 1) onto the z axis, each keeping its length (flatibration.py:84-112)."""
    ex, ey, ez = np.array([1.0, 0.0, a]), np.array([0.0, 1.0, b]), np.array([-a, -b, 1.0])
    o = np.array([0.0, 0.0, c])
    source = np.array([o, o + ex, o + ey, o + ez])
    target = np.vstack([np.zeros(3), np.diag([np.linalg.norm(ex), np.linalg.norm(ey), np.linalg.norm(ez)])])
    return rigid_transform_from_correspondences(source, target)


def ransac_plane(points, residual_threshold=10, *, device=0, forced_trials=None, return_stats=False):
    """sklearn RANSACRegressor(residual_threshold).fit(points[:, :2], points[:, 2]) with its defaults.  Returns (a, b, c), n_trials and
    (with return_stats) a dict of the per-trial counts / scores / planes and the tie margin.  Leaves numpy's global RNG in the state
    sklearn leaves it in.  forced_trials: score exactly that many trials and skip the replay (measurement; the RNG is not advanced)."""
    P = np.ascontiguousarray(points, dtype=np.float64)
    n = P.shape[0]
    trials = MAX_TRIALS if forced_trials is None else int(forced_trials)
    idx, states = draw_subsets(n, trials)
    planes = np.ascontiguousarray(hypotheses(P, idx))
    counts = np.empty(trials, dtype=np.uint64)
    moments = np.empty((trials, 9))
    shift = np.ascontiguousarray(P[0, :2])
    ops.call("mcba_flat_ransac", n, P.ctypes.data, trials, planes.ctypes.data, float(residual_threshold), shift.ctypes.data, int(device), counts.ctypes.data,
             moments.ctypes.data, None, None)
    scores = r2_scores(planes, counts, moments)
    if forced_trials is not None:
        best, n_trials, margin = int(np.argmax(counts)), trials, np.inf
    else:
        best, n_trials, margin = replay(counts, scores, n)
    if best < 0:
        raise ValueError("RANSAC could not find a valid consensus set. All `max_trials` iterations were skipped because each randomly chosen sub-sample "
                         "failed the passing criteria. See estimator attributes for diagnostics (n_skips*).")
    if forced_trials is None:
        np.random.set_state(states[n_trials])
    plane = final_fit(planes[best], counts[best], moments[best], shift)
    stats = dict(counts=counts, scores=scores, planes=planes, best=best, tie_margin=margin, subsets=idx)
    return (plane, n_trials, stats) if return_stats else (plane, n_trials)


def inlier_mask(points, plane, residual_threshold, *, device=0):
    """The inliers of one plane on the device (the same test the scoring kernel counts): n bytes -> bool."""
    P = np.ascontiguousarray(points, dtype=np.float64)
    pl = np.ascontiguousarray(plane, dtype=np.float64)
    mask = np.empty(P.shape[0], dtype=np.uint8)
    counts, moments, shift = np.empty(1, dtype=np.uint64), np.empty((1, 9)), np.ascontiguousarray(P[0, :2])
    ops.call("mcba_flat_ransac", P.shape[0], P.ctypes.data, 1, pl.ctypes.data, float(residual_threshold), shift.ctypes.data, int(device), counts.ctypes.data,
             moments.ctypes.data, mask.ctypes.data, None)
    return mask.astype(bool)


def _floor_array(floor_points):
    P = np.asarray(_concat(floor_points), dtype=np.float64)
    if P.ndim != 2 or P.shape[1] != 3:
        raise ValueError("floor_points must have shape (n_points, 3)")
    return P


# ------------------------------------------------------------------ flatibrate (flatibration.py:63-114)
def flatibrate(floor_points, residual_threshold=10, *, return_inliers=False, device=0):
    """Rigid transform (6-vector: rotation vector, translation) that maps the RANSAC floor plane of floor_points to the XY plane.
    return_inliers: also the inlier mask of the winning trial (RANSACRegressor.inlier_mask_)."""
    P = _floor_array(floor_points)
    if not np.isfinite(P).all():
        raise ValueError("Input contains NaN or infinity.")
    if P.shape[0] < MIN_SAMPLES:
        raise ValueError("`min_samples` may not be larger than number of samples: n_samples = %d." % P.shape[0])
    (a, b, c), n_trials, stats = ransac_plane(P, residual_threshold, device=device, return_stats=True)
    transform = plane_transform(a, b, c)
    if return_inliers:
        return transform, inlier_mask(P, stats["planes"][stats["best"]], residual_threshold, device=device)
    return transform


# ------------------------------------------------------------------ flip_z_axis (flatibration.py:117-136)
def flip_z_axis(transform):
    """Compose the transform with a rotation by 180 degrees about the X axis."""
    return get_transformation_vector(np.diag([1.0, -1.0, -1.0, 1.0]) @ get_transformation_matrix(np.asarray(transform, dtype=np.float64)))


# ------------------------------------------------------------------ center_arena (flatibration.py:139-191)
def _percentile_ranks(n, q):
    """numpy's 'linear' method (np.percentile's default): virtual index (n - 1) q and its two neighbours, as _get_indexes clips them."""
    vi = (n - 1) * q
    prev = np.floor(vi)
    nxt = prev + 1
    above = vi >= n - 1
    prev[above] = n - 1
    nxt[above] = n - 1
    below = vi < 0
    prev[below] = 0
    nxt[below] = 0
    gamma = np.asarray(vi - np.where(above, -1.0, prev), dtype=np.float64)  # (numpy subtracts the index -1 there; the lerp of equal values ignores it)
    return prev.astype(np.int64), nxt.astype(np.int64), gamma


def _lerp(a, b, t):
    """numpy's _lerp: a + (b - a) t, and b - (b - a)(1 - t) where t >= 0.5."""
    d = b - a
    return np.where(t >= 0.5, b - d * (1 - t), a + d * t)


def arena_center(transform, floor_points, center_method="midrange", range_pctl=1, *, device=0):
    """The XY centre of the transformed floor points that center_arena() moves to the origin: (2,) float64."""
    if center_method not in ("midrange", "mean", "median"):
        raise ValueError("center_method should be 'midrange', 'mean', or 'median'")
    P = np.ascontiguousarray(_floor_array(floor_points))
    n = P.shape[0]
    if n == 0:
        raise ValueError("floor_points is empty")
    T = get_transformation_matrix(np.asarray(transform, dtype=np.float64))
    rt12 = np.ascontiguousarray(np.concatenate([T[:3, :3].ravel(), T[:3, 3]]))
    if center_method == "midrange":
        q = np.true_divide(np.asarray([range_pctl, 100 - range_pctl]), 100)
        if q.min() < 0 or q.max() > 1:
            raise ValueError("Percentiles must be in the range [0, 100]")
        prev, nxt, gamma = _percentile_ranks(n, q)
        ranks = np.array([prev[0], nxt[0], prev[1], nxt[1]], dtype=np.int64)
    elif center_method == "median":
        ranks = np.array([(n - 1) // 2, n // 2], dtype=np.int64)
    else:
        ranks = np.zeros(0, dtype=np.int64)
    values = np.empty((2, max(len(ranks), 1)))
    sums = np.empty(2)
    nans = np.empty(2, dtype=np.uint64)
    ops.call("mcba_flat_order_stats", n, P.ctypes.data, rt12.ctypes.data, len(ranks), ranks.ctypes.data, int(device), values.ctypes.data, sums.ctypes.data,
             nans.ctypes.data, None)
    if center_method == "mean":
        return sums / n
    if center_method == "median":
        center = values[:, 0] if n % 2 else (values[:, 0] + values[:, 1]) / 2.0  # np.median: np.mean of the middle one or two
    else:
        lo = _lerp(values[:, 0], values[:, 1], gamma[0])
        hi = _lerp(values[:, 2], values[:, 3], gamma[1])
        center = (lo + hi) / 2.0
    return np.where(nans > 0, np.nan, center)


def center_arena(transform, floor_points, center_method="midrange", range_pctl=1, *, device=0):
    """Compose the transform with the XY translation that moves the arena's centre (robust midrange, mean or median of the transformed
    floor points) to the origin."""
    center = arena_center(transform, floor_points, center_method, range_pctl, device=device)
    translation = np.array([0.0, 0.0, 0.0, -center[0], -center[1], 0.0])
    return get_transformation_vector(get_transformation_matrix(translation) @ get_transformation_matrix(np.asarray(transform, dtype=np.float64)))
