"""Numpy statement of camera resection, the checker of the host build (tests/test_hostcheck_resection.py) and of the GPU
tier (tests/test_gpu_resection.py).

Stages, each a function here:
  prepare      the detections through oracle/triangulate_oracle.undistort_points; undistorted pixels, ((x - cx) / fx, (y - cy) / fy), the usable flag
  hypothesis   6 index-selected points: Hartley normalisation (3-D: mean distance sqrt 3, 2-D: sqrt 2), the eigenvector of the smallest eigenvalue
               of the 12 x 12 normal matrix of the rows [X 1 0 -uX -u], [0 X 1 -vX -v] (np.linalg.eigh), de-normalised, det of the left block made
               positive, R = U V^T (np.linalg.svd), t = p_4 / mean singular value; then exactly GN_ITERATIONS Gauss-Newton iterations on the six
               points: residuals pi(R X + t) - x in normalised coordinates, update R <- exp(omega) R, t <- exp(omega) t + delta.  Void (+inf)
               when anything is not finite, when the DLT's eigen-gap lambda_2 / lambda_12 is below GAP_MIN = 1e-10 (the null vector is known
               to EPS / gap: below that the start is what the eigen-solver's rounding makes of a null space of several dimensions, as for six
               coplanar points, and two correct solvers disagree on it) or when a sample point ends with z <= 0
  score        e^2 = |K pi(R X + t) - undistorted uv|^2, +inf where z <= 0; cost = sum min(e^2, threshold^2); inlier <=> e^2 <= threshold^2, z > 0
  winner       the lowest (cost, index)
  mask         the winner's inliers
  normal       the polish's system at a pose: f = raw detection - projection of the five-coefficient model (tricov_oracle.camera_rows), B its
               columns 6 .. 11, curvature weights and rho' of kpba_oracle.loss_terms; J^T W J (6 x 6), gradient, robust cost, count
  lm           the loop: Marquardt damping lam diag, tenfold rule, accept when the cost does not rise, scipy's ftol / xtol / gtol tests

The Gauss-Newton step has two routes: the normal equations (np.linalg.solve on the equilibrated J^T J) and np.linalg.lstsq on the column-scaled J.
`step` of an iteration: max(|omega|, |delta| / max(1, |t|)).  A hypothesis is COMPARABLE when the step of iteration GN_ITERATIONS is at most
STEP_MAX = 1e-10, the cond_2 of the equilibrated J^T J of that iteration is below COND_MAX = 1e8, and it is not void.  The hypotheses left out are
at most LEFT_OUT_CAP = 5 % of a scene's, asserted on the oracle alone (tests/test_resection_oracle_cpu.py) for the scenes of the element-wise
comparison: "six" (64 and 512 hypotheses) and "three" (64), each camera against the oracle's triangulation of the others.

Tolerance of a comparable hypothesis' pose: K_P EPS cond per entry of R, times max(1, |t|) per entry of t.  K_P is 8 x the worst multiple of
EPS cond seen between the two routes over the comparable hypotheses of those scenes, and at least the project's 64.
Measured (tests/test_resection_oracle_cpu.py prints it): worst multiple K_P_MEASURED below.

Per-point bound on e: BOUND_FACTOR EPS times the magnitudes that meet in the projection, (|P_0| . |X~| + |a / z| |P_2| . |X~|) / |z| + |u| and the
same for v.  A point whose e is within that bound of the threshold is undecided, and so is one whose z is within BOUND_FACTOR EPS |P_2| . |X~|
of 0 (never more than 1 % of the points; the chosen scenes have none).  Counts are exact on decided points; the bound of a hypothesis' cost is
the sum over the decided inliers of 2 e b + b^2, |threshold^2 - e^2| + 2 e b + b^2 per undecided point (threshold^2 for one undecided in z),
and M EPS cost for the order of the sum.

The winner's index is compared only when the two lowest costs differ by more than 1e-6 relative and no left-out hypothesis costs less than 1.5 x
the winner."""
import os

import numpy as np

import keypoint_scenes as ks
import kpba_oracle as ko
import tricov_oracle as tco
from oracle import triangulate_oracle as tri

EPS = 2.2e-16
BOUND_FACTOR = 64.0
GN_ITERATIONS = 10
SAMPLE = 6
STEP_MAX, COND_MAX, LEFT_OUT_CAP = 1e-10, 1e8, 0.05
GAP_MIN = 1e-10               # RS_DLT_GAP_MIN of csrc/mcba_resect_math.h: EPS / gap = 2e-6, the last start whose sixth digit is defined
K_P_MEASURED = 2.51           # the worst multiple between the two routes (module docstring): "three" camera 0; "six" 2.35; so K_P = max(64, 20.1) = 64
K_P = max(64.0, 8 * K_P_MEASURED)
THRESHOLD = 2.5
COMPARED = (("six", 64), ("six", 512), ("three", 64))   # (scene, hypotheses) of the element-wise comparison
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resection.npz")
GOLDEN_CASES = {"six_c0": ("six", 0, "linear"), "six_c5": ("six", 5, "linear"), "three_c1": ("three", 1, "linear"),
                **{f"outlier_c1_{loss}": ("outlier", 1, loss) for loss in ko.LOSS_NAMES}}
START_SEEDS = (3001, 3002)
LAMBDA0, LAMBDA_MIN, LAMBDA_MAX = 1e-4, 1e-12, 1e12


# ---------------------------------------------------------------- inputs
def draw_samples(M, H, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.choice(M, SAMPLE, replace=False) for _ in range(H)]).astype(np.int32)


_scene_cache = {}


def camera_of(name, cam):
    """dict(points (P, 3): the oracle's triangulation of the OTHER cameras, uv (P, 2), intr, ext: the scene's truth for the camera, usable (P))"""
    if (name, cam) not in _scene_cache:
        uvs, ext, intr, _ = ks.make(name)
        others = [c for c in range(len(ext)) if c != cam]
        with np.errstate(all="ignore"):
            pts = tri.triangulate([uvs[c] for c in others], ext[others], [intr[c] for c in others])
        uv = np.asarray(uvs[cam], dtype=np.float64)
        for a in (pts, uv):
            a.setflags(write=False)
        _scene_cache[(name, cam)] = dict(points=pts, uv=uv, intr=intr[cam], ext=np.array(ext[cam]), usable=np.isfinite(pts).all(1) & np.isfinite(uv).all(1), n_cameras=len(ext))
    return _scene_cache[(name, cam)]


def samples_of(usable, H, seed):
    """(H, 6) indices into 0 .. P - 1: draw_samples over the usable points, mapped through their index list"""
    idx = np.flatnonzero(usable)
    return idx[draw_samples(len(idx), H, seed)].astype(np.int32)


def k4(intr):
    K = np.asarray(intr[0], dtype=np.float64)
    return np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]])


def d5(intr):
    return np.r_[np.ravel(intr[1]), np.zeros(5)][:5]


def prepare(points, uv, intr, iterations=5):
    """dict(px (P, 2) undistorted pixels, nx (P, 2) normalised, usable (P)); rows of unusable points are 0"""
    points, uv = np.asarray(points, dtype=np.float64), np.asarray(uv, dtype=np.float64)
    usable = np.isfinite(points).all(1) & np.isfinite(uv).all(1)
    px = np.zeros((len(uv), 2))
    px[usable] = tri.undistort_points(uv[usable], intr[0], d5(intr), iterations=iterations)
    k = k4(intr)
    return dict(px=px, nx=np.where(usable[:, None], (px - k[2:]) / k[:2], 0.0), usable=usable)


# ---------------------------------------------------------------- the hypothesis
def skew(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0.0]])


def dlt_pose(X, x):
    """(R, t, eigen-gap lambda_2 / lambda_12) of six world points X (6, 3) at normalised coordinates x (6, 2)"""
    c3 = X.mean(0)
    dist = np.sqrt(((X - c3) ** 2).sum(1)).mean()
    s3 = np.sqrt(3.0) / dist if dist > 0 else 1.0
    m2 = x.mean(0)
    dist2 = np.sqrt(((x - m2) ** 2).sum(1)).mean()
    s2 = np.sqrt(2.0) / dist2 if dist2 > 0 else 1.0
    Xn, xn = s3 * (X - c3), s2 * (x - m2)
    A = np.zeros((12, 12))
    one, zero = np.ones((6, 1)), np.zeros((6, 4))
    A[0::2] = np.c_[Xn, one, zero, -xn[:, :1] * Xn, -xn[:, :1]]
    A[1::2] = np.c_[zero, Xn, one, -xn[:, 1:] * Xn, -xn[:, 1:]]
    w, V = np.linalg.eigh(A.T @ A)
    Pn = V[:, 0].reshape(3, 4)
    T3 = np.eye(4)
    T3[:3, :3] *= s3
    T3[:3, 3] = -s3 * c3
    T2i = np.array([[1 / s2, 0, m2[0]], [0, 1 / s2, m2[1]], [0, 0, 1.0]])
    Pm = T2i @ Pn @ T3
    if np.linalg.det(Pm[:, :3]) < 0:
        Pm = -Pm
    U, s, Vt = np.linalg.svd(Pm[:, :3])
    return U @ Vt, Pm[:, 3] / s.mean(), float(w[1] / w[11]) if w[11] > 0 else 0.0


def gn_system(R, t, X, x):
    """(J (12, 6), r (12)) of the six points in normalised coordinates; unknowns (omega, delta) of the left-multiplicative update"""
    Xc = X @ R.T + t
    z = Xc[:, 2]
    p = Xc[:, :2] / z[:, None]
    r = (p - x).ravel()
    J = np.zeros((12, 6))
    for k in range(6):
        N = np.array([[1 / z[k], 0, -p[k, 0] / z[k]], [0, 1 / z[k], -p[k, 1] / z[k]]])
        J[2 * k:2 * k + 2, :3] = -N @ skew(Xc[k])
        J[2 * k:2 * k + 2, 3:] = N
    return J, r


def gn_step(J, r, route):
    """(step (6), cond_2 of the equilibrated J^T J)"""
    s = np.sqrt((J * J).sum(0))
    s = np.where(s > 0, s, 1.0)
    Js = J / s
    A = Js.T @ Js
    cond = float(np.linalg.cond(A))
    if route == "normal":
        y = np.linalg.solve(A, -(Js.T @ r))
    else:
        y = np.linalg.lstsq(Js, -r, rcond=None)[0]
    return y / s, cond


def hypothesis(X, x, route="normal", iterations=GN_ITERATIONS):
    """dict(pose (12: R row-major, t) or NaN, status, step: of the last iteration, cond: of its equilibrated J^T J, gap: the DLT's)"""
    nan12 = np.full(12, np.nan)
    gap = 0.0
    with np.errstate(all="ignore"):
        try:
            R, t, gap = dlt_pose(X, x)
            if not gap >= GAP_MIN:
                raise np.linalg.LinAlgError("the DLT start is not defined")
            step, cond = np.inf, np.inf
            for _ in range(iterations):
                J, r = gn_system(R, t, X, x)
                y, cond = gn_step(J, r, route)
                R, t = ks.rodrigues(y[:3]) @ R, ks.rodrigues(y[:3]) @ t + y[3:]
                step = max(np.linalg.norm(y[:3]), np.linalg.norm(y[3:]) / max(1.0, np.linalg.norm(t)))
            pose = np.r_[R.ravel(), t]
            ok = np.isfinite(pose).all() and ((X @ R.T + t)[:, 2] > 0).all()
        except np.linalg.LinAlgError:
            ok = False
    if not ok:
        return dict(pose=nan12, status=-1, step=np.inf, cond=np.inf, gap=gap if np.isfinite(gap) else 0.0)
    return dict(pose=pose, status=1, step=float(step), cond=float(cond), gap=gap)


def hypotheses(points, prep, samples, route="normal"):
    """dict(pose (H, 12), status (H), step, cond, gap (H), comparable (H) bool, tol (H, 12))"""
    H = len(samples)
    out = dict(pose=np.empty((H, 12)), status=np.empty(H, np.int32), step=np.empty(H), cond=np.empty(H), gap=np.empty(H))
    for h, s in enumerate(samples):
        o = hypothesis(np.asarray(points)[s], prep["nx"][s], route)
        for k in out:
            out[k][h] = o[k]
    out["comparable"] = (out["status"] > 0) & (out["step"] <= STEP_MAX) & (out["cond"] < COND_MAX)
    out["tol"] = pose_tolerance(out["pose"], out["cond"])
    return out


def pose_tolerance(pose, cond, k=None):
    with np.errstate(invalid="ignore"):
        scale = np.c_[np.ones((len(pose), 9)), np.repeat(np.maximum(1.0, np.linalg.norm(pose[:, 9:], axis=1))[:, None], 3, 1)]
        return (K_P if k is None else k) * EPS * cond[:, None] * scale


def left_out_share(hyp):
    """the share of a scene's hypotheses that the element-wise comparison leaves out, void samples not included"""
    alive = hyp["status"] > 0
    return float((alive & ~hyp["comparable"]).sum() / len(alive))


def route_multiple(points, prep, samples):
    """the worst |pose_normal - pose_lstsq| over EPS cond (t entries over max(1, |t|)) among the comparable hypotheses"""
    a, b = hypotheses(points, prep, samples, "normal"), hypotheses(points, prep, samples, "lstsq")
    ok = a["comparable"] & b["comparable"]
    unit = pose_tolerance(a["pose"], a["cond"], k=1.0)
    return float((np.abs(a["pose"] - b["pose"])[ok] / unit[ok]).max()) if ok.any() else 0.0


# ---------------------------------------------------------------- scoring
def pixel_matrix(pose, intr):
    K = np.asarray(intr[0], dtype=np.float64)
    return K @ np.c_[pose[:9].reshape(3, 3), pose[9:]]


def errors(pose, points, prep, intr):
    """(e^2 (P) with +inf where z <= 0, bound on e (P), undecided in z (P)) over all points; unusable points: e^2 NaN"""
    KP = pixel_matrix(pose, intr)
    Xh = np.c_[np.where(prep["usable"][:, None], points, 0.0), np.ones(len(points))]
    with np.errstate(all="ignore"):
        a, b, z = Xh @ KP[0], Xh @ KP[1], Xh @ KP[2]
        m0, m1, m2 = np.abs(Xh) @ np.abs(KP[0]), np.abs(Xh) @ np.abs(KP[1]), np.abs(Xh) @ np.abs(KP[2])
        du, dv = a / z - prep["px"][:, 0], b / z - prep["px"][:, 1]
        e2 = np.where(z > 0, du * du + dv * dv, np.inf)
        bound = BOUND_FACTOR * EPS * ((m0 + np.abs(a / z) * m2) / np.abs(z) + np.abs(prep["px"][:, 0]) + (m1 + np.abs(b / z) * m2) / np.abs(z) + np.abs(prep["px"][:, 1]))
        zund = np.abs(z) <= BOUND_FACTOR * EPS * m2
    return np.where(prep["usable"], e2, np.nan), bound, zund & prep["usable"]


def score(pose_table, status, points, prep, intr, threshold):
    """per hypothesis: cost (inf for a void one), count, cost_bound, undecided (H, P) bool, inlier (H, P) bool"""
    H, P = len(pose_table), len(points)
    t2 = threshold * threshold
    use = prep["usable"]
    cost, count, cb = np.full(H, np.inf), np.zeros(H, np.int64), np.zeros(H)
    und, inl = np.zeros((H, P), bool), np.zeros((H, P), bool)
    for h in range(H):
        if status[h] < 0:
            continue
        e2, b, zund = errors(pose_table[h], points, prep, intr)
        with np.errstate(invalid="ignore"):
            e = np.sqrt(e2)
            inl[h] = use & (e2 <= t2)
            und[h] = use & ((np.abs(e - threshold) <= b) | zund)
        term = np.where(inl[h], e2, t2)[use]
        cost[h], count[h] = term.sum(), inl[h].sum()
        eb = np.where(np.isfinite(e) & np.isfinite(b), 2 * e * b + b * b, 0.0)
        near = und[h] & ~zund
        cb[h] = eb[inl[h] & ~und[h]].sum() + (np.abs(t2 - e2[near]) + eb[near]).sum() + t2 * zund.sum() + use.sum() * EPS * cost[h]
    return dict(cost=cost, count=count, cost_bound=cb, undecided=und, inlier=inl)


def winner(cost):
    """(index of the lowest (cost, index), whether the index is comparable by the gap rule alone)"""
    order = np.lexsort((np.arange(len(cost)), cost))
    w = int(order[0])
    clear = len(cost) < 2 or not np.isfinite(cost[order[1]]) or (cost[order[1]] - cost[w]) > 1e-6 * cost[w]
    return w, bool(clear and np.isfinite(cost[w]))


def winner_comparable(sc, hyp):
    w, clear = winner(sc["cost"])
    out = ~hyp["comparable"] & np.isfinite(sc["cost"])
    return w, clear and bool(hyp["comparable"][w]) and not (sc["cost"][out] < 1.5 * sc["cost"][w]).any()


def ransac(points, uv, intr, samples, threshold, poses_in=None, iterations=5):
    """every stage on one camera: prep, hyp, score, winner, comparable, rt12, inliers (P), n_inliers, cost, n_usable"""
    points = np.asarray(points, dtype=np.float64)
    prep = prepare(points, uv, intr, iterations)
    if poses_in is None:
        hyp = hypotheses(points, prep, samples)
    else:
        pose = np.asarray(poses_in, dtype=np.float64).reshape(-1, 12)
        st = np.where(np.isfinite(pose).all(1), 1, -1).astype(np.int32)
        hyp = dict(pose=pose, status=st, comparable=st > 0, tol=np.zeros((len(pose), 12)), step=np.zeros(len(pose)), cond=np.ones(len(pose)))
    sc = score(hyp["pose"], hyp["status"], points, prep, intr, threshold)
    w, comparable = winner_comparable(sc, hyp)
    return dict(prep=prep, hyp=hyp, score=sc, winner=w, comparable=comparable, rt12=hyp["pose"][w], inliers=sc["inlier"][w], n_inliers=int(sc["count"][w]), cost=float(sc["cost"][w]),
                n_usable=int(prep["usable"].sum()))


def min_inliers(n_usable):
    return max(12, n_usable // 10)


def rodrigues_inv(R):
    c = np.clip((np.trace(R) - 1) / 2, -1, 1)
    th = np.arccos(c)
    w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    return w / 2 if th < 1e-12 else w * th / (2 * np.sin(th))


def transform_of(rt12):
    return np.r_[rodrigues_inv(rt12[:9].reshape(3, 3)), rt12[9:]]


# ---------------------------------------------------------------- the rules, applied to what a build returns
def check_hypotheses(tag, pose, status, hyp):
    ok = hyp["comparable"]
    ratio = float((np.abs(pose - hyp["pose"])[ok] / hyp["tol"][ok]).max()) if ok.any() else 0.0
    print(f"{tag}: pose error / tolerance {ratio:.3g} over {int(ok.sum())} comparable of {len(ok)}; left out {left_out_share(hyp):.3%}; void {int((hyp['status'] < 0).sum())}")
    assert np.array_equal(np.asarray(status)[ok], hyp["status"][ok]) and ratio <= 1
    return ratio


def check_scores(tag, cost, count, hyp, sc, subset=None):
    ok = hyp["comparable"] if subset is None else subset
    und = sc["undecided"][ok]
    slack = und.sum(1)
    dc = np.abs(np.asarray(count, dtype=np.int64)[ok] - sc["count"][ok])
    with np.errstate(invalid="ignore"):
        cr = np.abs(np.asarray(cost)[ok] - sc["cost"][ok]) / np.maximum(sc["cost_bound"][ok], 1e-300)
    cr = np.where(np.isfinite(sc["cost"][ok]), cr, 0.0)
    print(f"{tag}: undecided points {und.mean() if und.size else 0.0:.3%}; count differences {int(dc.max()) if dc.size else 0} (allowed {int(slack.max()) if slack.size else 0}); cost error / bound {cr.max() if cr.size else 0:.3g}")
    assert (und.mean() if und.size else 0.0) <= 0.01
    assert (dc <= slack).all() and (cr <= 1).all()
    void = ~np.isfinite(sc["cost"]) & ok
    assert np.isinf(np.asarray(cost)[void]).all()


# ---------------------------------------------------------------- the polish
def normal_system(pose6, points, uv, mask, intr, loss="linear", f_scale=1.0):
    """dict(A (6, 6) = J^T W J, g (6) the gradient, cost, count, sys (29): the library's packing) over the masked, usable points"""
    points, uv = np.asarray(points, dtype=np.float64), np.asarray(uv, dtype=np.float64)
    use = np.asarray(mask, bool) & np.isfinite(points).all(1) & np.isfinite(uv).all(1)
    theta = np.r_[k4(intr), d5(intr)[:2], pose6]
    proj, _, B = tco.camera_rows(points[use], theta, d5(intr))
    f = (uv[use] - proj).astype(ko.LD)
    r0, r1, w = ko.loss_terms(f, loss, f_scale)
    B6 = B[:, :, 6:].astype(ko.LD)
    A = np.einsum("pki,pk,pkj->ij", B6, w, B6)
    g = -np.einsum("pki,pk->i", B6, r1 * f)
    cost = ko.LD(0.5) * ko.LD(f_scale) ** 2 * r0.sum()
    A, g = A.astype(np.float64), g.astype(np.float64)
    return dict(A=A, g=g, cost=float(cost), count=int(use.sum()), sys=np.r_[A[np.triu_indices(6)], g, float(cost), float(use.sum())],
                scale=np.sqrt(np.outer(np.diag(A), np.diag(A))), fnorm=float(np.sqrt((f * f).sum())))


def robust_cost(pose6, points, uv, mask, intr, loss="linear", f_scale=1.0):
    use = np.asarray(mask, bool) & np.isfinite(points).all(1) & np.isfinite(uv).all(1)
    f = np.asarray(uv)[use] - ks.project5(np.asarray(points)[use], pose6, intr[0], d5(intr))
    return float(0.5 * f_scale ** 2 * ks.rho((f / f_scale) ** 2, loss).sum())


def lm(pose6, points, uv, mask, intr, loss="linear", f_scale=1.0, ftol=1e-8, xtol=1e-8, gtol=1e-8, max_nfev=50):
    """the loop restated: dict(pose, cost, cost0, optimality, nfev, njev, status, history [(cost, lam, accepted)])"""
    x = np.array(pose6, dtype=np.float64)
    s = normal_system(x, points, uv, mask, intr, loss, f_scale)
    cost = cost0 = s["cost"]
    nfev = njev = 1
    lam, hist = LAMBDA0, [(cost, LAMBDA0, True)]
    opt = float(np.abs(s["g"]).max()) if s["count"] else 0.0
    status = 1 if opt <= gtol else -1
    while status == -1:
        if nfev >= max_nfev:
            status = 0
            break
        while True:
            A = s["A"] + lam * np.diag(np.diag(s["A"]))
            d = np.diag(A)
            ok = (d > 0).all()
            if ok:
                sc = 1 / np.sqrt(d)
                try:
                    L = np.linalg.cholesky(A * np.outer(sc, sc))
                    ok = (np.diag(L) ** 2 > 1e-14).all()
                except np.linalg.LinAlgError:
                    ok = False
            if ok:
                break
            lam *= 10
            if not lam < LAMBDA_MAX:
                status = 3
                break
        if status != -1:
            break
        step = sc * np.linalg.solve(L.T, np.linalg.solve(L, -sc * s["g"]))
        small = np.linalg.norm(step) < xtol * (xtol + np.linalg.norm(x))
        c = robust_cost(x + step, points, uv, mask, intr, loss, f_scale)
        nfev += 1
        if c <= cost:
            gain, cost, x = cost - c, c, x + step
            hist.append((c, lam, True))
            lam = max(0.1 * lam, LAMBDA_MIN)
            s = normal_system(x, points, uv, mask, intr, loss, f_scale)
            njev += 1
            opt = float(np.abs(s["g"]).max())
            status = 1 if opt <= gtol else (2 if gain <= ftol * cost else (3 if small else -1))
        else:
            hist.append((c, lam, False))
            lam *= 10
            if small or not lam < LAMBDA_MAX:
                status = 3
    return dict(pose=x, cost=cost, cost0=cost0, optimality=opt, nfev=nfev, njev=njev, status=status, history=hist)


def check_system(tag, got, o):
    """a camera's 29 numbers against normal_system: entries of J^T W J within BOUND_FACTOR EPS count of sqrt(A_ii A_jj) (every term of a sum is
    bounded by it), the gradient within the same multiple of sqrt(A_ii) |f| sqrt(count)-free Cauchy-Schwarz bound, the cost relative, the count exact"""
    n = max(o["count"], 1)
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = got[:21]
    A = A + np.triu(A, 1).T
    ra = float((np.abs(A - o["A"]) / np.maximum(BOUND_FACTOR * EPS * n * o["scale"], 1e-300)).max()) if o["count"] else 0.0
    gb = BOUND_FACTOR * EPS * n * np.sqrt(np.diag(o["A"])) * max(o["fnorm"], 1e-300)
    rg = float((np.abs(got[21:27] - o["g"]) / np.maximum(gb, 1e-300)).max()) if o["count"] else 0.0
    rc = abs(got[27] - o["cost"]) / max(BOUND_FACTOR * EPS * n * o["cost"], 1e-300) if o["count"] else 0.0
    print(f"{tag}: J^T W J error / bound {ra:.3g}; gradient {rg:.3g}; cost {rc:.3g}; count {int(got[28])} (oracle {o['count']})")
    assert int(got[28]) == o["count"] and ra <= 1 and rg <= 1 and rc <= 1


# ---------------------------------------------------------------- the goldens of the polish
def perturbed_start(ext, seed):
    rng = np.random.default_rng(seed)
    return np.r_[ext[:3] + rng.normal(0, 0.02, 3), ext[3:] + rng.normal(0, 20.0, 3)]


_golden = None


def golden():
    global _golden
    if _golden is None:
        _golden = dict(np.load(GOLDEN, allow_pickle=False))
    return _golden


def golden_case(name):
    """the inputs of a case (points, uv, intr, mask = every usable point, loss, the first start) and its stored optimum"""
    sc, cam, loss = GOLDEN_CASES[name]
    c = camera_of(sc, cam)
    g = golden()
    return dict(points=c["points"], uv=c["uv"], intr=c["intr"], mask=c["usable"], loss=loss, start=perturbed_start(c["ext"], START_SEEDS[0])), \
        dict(pose=g[f"{name}/pose"], cost=float(g[f"{name}/cost"]), spread=float(g[f"{name}/spread"]), pinned=bool(g[f"{name}/pinned"]))


def check_golden(tag, pose, cost, o):
    """the bars of tests/kpba_oracle.check_result for a pinned case: the cost not above the stored one by more than 1e-10 relative, the six scalars within 1e-6 relative"""
    err = float((np.abs(pose - o["pose"]) / np.maximum(1.0, np.abs(o["pose"]))).max())
    print(f"{tag}: cost {cost:.15g} golden {o['cost']:.15g} ratio-1 {cost / o['cost'] - 1:.3g}; pose {err:.3g} (bar 1e-6)")
    assert cost <= o["cost"] * (1 + 1e-10) and err <= 1e-6
