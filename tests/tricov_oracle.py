"""Numpy statement of triangulation_uncertainty, the checker of the host build (tests/test_hostcheck_tricov.py) and of the
GPU tier (tests/test_gpu_tricov.py).  Per point X, over the cameras c that see it:

    f_c = detection - project5(X)                 (keypoint_scenes.project5: the five-coefficient forward model on raw detections)
    A_c = d(u, v)/dX,  B_c = d(u, v)/d(theta_c)   theta_c = (fx fy cx cy k1 k2 | rotation vector | translation); p1, p2, k3 constants
    w   = rho'((f / f_scale)^2) per scalar,  H = sum_c A_c^T W_c A_c
    detection term    sigma2 H^-1                 H inverted through scipy's Cholesky factor of D H D, D = diag(H)^-1/2
    calibration term  G Sigma_cc G^T              G_c = H^-1 A_c^T W_c B_c, zero for a camera that does not see the point
    sigma2            given, or sum w f^2 / (m - 3 P_u) over the P_u points of status 1 and their m present scalars
    status            -1 fewer than two views or a NaN in X;  -2 a pivot of the scaled factor whose square is below 1e-12

The derivatives are analytic and written independently of csrc/mcba_tricov_math.h: the chain rule through d(x, y)/dX_c and the closed form of
dR/dr_k (Gallego & Yezzi 2015, eq. III.7; [e_k]x at r = 0) instead of the right Jacobian.  tests/test_tricov_cpu.py holds them to central
differences of project5.

Metric and bound (per point, cond = cond_2 of the scaled H, T = |G| |Sigma_cc| |G|^T):
    detection term    max_ij |got - ref|_ij / sqrt(ref_ii ref_jj)  <=  BOUND_FACTOR cond EPS
    calibration term  |got - ref|_ij                               <=  BOUND_FACTOR cond EPS sqrt(T_ii T_jj)
T because a real Sigma_cc is strongly correlated and G Sigma G^T cancels: an error measured against the result alone would punish correct
arithmetic.  The blocks are compared at a given sigma (SIGMA); the pooled sigma2 is compared on its own, to 1e-12 relative, on the cases with
detection noise and at least 33 points (POOLED_CASES): its terms f^2 carry the cancellation of detection - projection, eps |u| / |f| ~ 1e-13 each,
which 64 cond eps does not model, and at noise-free detections sigma2 is rounding noise (1e-26) with no digits to agree on.

BOUND_FACTOR.  Linear loss: the project's 64 (covariance_oracle.BOUND_FACTOR), confirmed on the CPU: the g++ build of the kernels' header meets it
on every case held to it at 0.15 of the bound or less (calibration term 0.146 on "six"; detection term 0.109 on "three"), and two float64 host formulations of this oracle differ by at most 0.066 of it.  Robust losses:
the weights w = rho'((f / f_scale)^2) inherit the cancellation in f = detection - projection (|u| ~ 1e3 against |f| ~ 1: a last-place change of
the projection moves w by ~1e-13), so two correct float64 evaluations of H differ by more than 64 cond eps whatever the 3 x 3 arithmetic does: the
g++ build is at 3.05 times that on "outlier_cauchy" (1.87 on "outlier_soft_l1").  For these the factor is 25 x the measured host spread, as
the project's rule for this case says: the two host formulations of this oracle (`uncertainty(formulation="cholesky")`: keypoint_scenes.rodrigues,
Horner form of the radial polynomial, Cholesky of the scaled H; `formulation="lu"`: the coefficient form of the rotation, the polynomial term by
term, numpy's LU inverse of the unscaled H; G and the products formed from each) differ over CASES by at most HOST_SPREAD = 1.25 in units of
64 cond eps (measured 1.24 on "outlier_cauchy", 0.69 on "outlier_soft_l1"; detection term; calibration term 0.48 / 0.38), hence
ROBUST_BOUND_FACTOR = 25 x 1.25 x 64 = 2000.  Only where that cancellation reaches the weights: the two cases of the "outlier" scene (and any
call of `uncertainty` with a robust loss that does not say otherwise).  "c24_p33" (huber at 0.3 px noise and f_scale 1: z < 1, so w = 1 exactly)
and "c3_p17" (arctan at residual-free detections: w' = 0 there) are held to 64 like the linear cases; the host formulations differ by less than
0.07 x 64 cond eps on them.  The wide cases (WIDE_CASES, 29 to 64 cameras at 0.3 px noise) follow the same rule: soft_l1, cauchy and arctan have
weights off 1 at every detection and host spreads of 0.52, 2.33 and 0.59 x 64 cond eps (detection term; calibration term 0.07 / 0.13 / 0.05), so
they are ROBUST_CASES and held to the same 2000 -- not to 25 x 2.33 x 64, which would be wider: the factor the "outlier" cases fixed stays.  So is
"c30_p21" (huber): 2 of its 886 scalars lie beyond the knee (|f| up to 1.05), where w = z^-1/2 carries the cancellation like any other robust
weight; the two host formulations happen to agree there (0.04), the g++ build of the kernels' header does not (G off by 7.9e-14 of its largest
entry, 3.8 x 64 cond eps).  "c64_p6" (linear) spreads by 0.03 and is held to 64.
tests/test_tricov_cpu.py prints the spread per case; neither factor was tuned against a GPU."""
import functools

import numpy as np
import scipy.linalg

import keypoint_scenes as ks
from test_triangulate_cpu import scene

EPS = 2.2e-16
BOUND_FACTOR = 64.0
HOST_SPREAD = 1.25   # two float64 host formulations on the robust cases, in units of BOUND_FACTOR cond EPS (module docstring)
ROBUST_BOUND_FACTOR = 25 * HOST_SPREAD * BOUND_FACTOR
PIVOT2_MIN = 1e-12
SIGMA = 0.3   # the detection noise the cases are run with where the bound is applied (see the module docstring)
LOSS_NAMES = ("linear", "soft_l1", "huber", "cauchy", "arctan")


LDS_LIMIT = 160 * 1024   # the opt-in LDS of a gfx950 workgroup


def cal_lds(n, G):
    """bytes of LDS k_tricov_cal asks for (csrc/mcba_tricov.hip, tricov_cal_lds): R = 3 G rows of the stacked G matrices at stride KP + 2, the
    staging buffer of diag_blocks (a 32 x 80 chunk of Sigma, later Z as R x 66), H^-1 and the two output terms (6 each) per point"""
    KP, R = (n + 31) // 32 * 32, 3 * G
    return 8 * (R * (KP + 2) + max(32 * 80, R * 66) + G * 6 * 3)


def expected_group(C, force=0):
    """points per workgroup of k_tricov_cal at C cameras: 16 if its LDS fits, else 10, else 5; `force` (MCBA_TRICOV_G) wins if it fits"""
    n = 12 * C
    if force in (5, 10, 16) and cal_lds(n, force) <= LDS_LIMIT:
        return force
    return next((G for G in (16, 10, 5) if cal_lds(n, G) <= LDS_LIMIT), 0)


def rho1(z, loss):
    """rho'(z)"""
    if loss == "linear":
        return np.ones_like(z)
    if loss == "soft_l1":
        return 1 / np.sqrt(1 + z)
    if loss == "huber":
        return np.where(z <= 1, 1.0, 1 / np.sqrt(np.maximum(z, 1e-300)))
    if loss == "cauchy":
        return 1 / (1 + z)
    return 1 / (1 + z * z)


def skew(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0.0]])


def rotation_derivatives(r):
    """dR/dr_k, k = 0 .. 2 (Gallego & Yezzi): (r_k [r]x + [r x (I - R) e_k]x) R / |r|^2; [e_k]x at r = 0"""
    r = np.asarray(r, dtype=np.float64)
    th2 = r @ r
    if th2 == 0:
        return [skew(e) for e in np.eye(3)]
    R = ks.rodrigues(r)
    return [(r[k] * skew(r) + skew(np.cross(r, (np.eye(3) - R)[:, k]))) @ R / th2 for k in range(3)]


def rodrigues_coefficients(r):
    """R = I + (sin t / t) [r]x + ((1 - cos t) / t^2) [r]x^2: the same rotation as keypoint_scenes.rodrigues, other roundings"""
    r = np.asarray(r, dtype=np.float64)
    th = np.linalg.norm(r)
    if th == 0:
        return np.eye(3)
    K = skew(r)
    return np.eye(3) + (np.sin(th) / th) * K + ((1 - np.cos(th)) / (th * th)) * (K @ K)


def camera_rows(X, theta, d5, second=False):
    """projection (P, 2), A (P, 2, 3), B (P, 2, 12) of one camera at the points X (P, 3).  second: the same mathematics with the rotation from
    rodrigues_coefficients and the radial polynomial written out term by term (the second host formulation)"""
    fx, fy, cx, cy, k1, k2 = theta[:6]
    p1, p2, k3 = d5[2], d5[3], d5[4]
    R = rodrigues_coefficients(theta[6:9]) if second else ks.rodrigues(theta[6:9])
    Xc = X @ R.T + theta[9:12]
    z = Xc[:, 2]
    x, y = Xc[:, 0] / z, Xc[:, 1] / z
    r2 = x * x + y * y
    rad = 1 + k1 * r2 + k2 * r2 * r2 + k3 * r2 * r2 * r2 if second else 1 + r2 * (k1 + r2 * (k2 + r2 * k3))
    drad = k1 + r2 * (2 * k2 + 3 * k3 * r2)
    xd = x * rad + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    yd = y * rad + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    uv = np.stack([fx * xd + cx, fy * yd + cy], axis=-1)
    D = np.empty((len(X), 2, 2))   # d(xd, yd)/d(x, y)
    D[:, 0, 0] = rad + 2 * x * x * drad + 2 * p1 * y + 6 * p2 * x
    D[:, 0, 1] = D[:, 1, 0] = 2 * x * y * drad + 2 * p1 * x + 2 * p2 * y
    D[:, 1, 1] = rad + 2 * y * y * drad + 6 * p1 * y + 2 * p2 * x
    N = np.zeros((len(X), 2, 3))   # d(x, y)/dX_c
    N[:, 0, 0] = N[:, 1, 1] = 1 / z
    N[:, 0, 2] = -x / z
    N[:, 1, 2] = -y / z
    Pm = np.array([fx, fy])[None, :, None] * (D @ N)   # d(u, v)/dX_c
    A = Pm @ R
    B = np.zeros((len(X), 2, 12))
    B[:, 0, 0], B[:, 1, 1] = xd, yd
    B[:, 0, 2] = B[:, 1, 3] = 1.0
    B[:, 0, 4], B[:, 1, 4] = fx * x * r2, fy * y * r2
    B[:, 0, 5], B[:, 1, 5] = fx * x * r2 * r2, fy * y * r2 * r2
    for k, dR in enumerate(rotation_derivatives(theta[6:9])):
        B[:, :, 6 + k] = np.einsum("pij,pj->pi", Pm, X @ dR.T)
    B[:, :, 9:] = Pm
    return uv, A, B


def camera_blocks(ext, intr):
    """theta (C, 12) and dist5 (C, 5) from the extrinsics and (K, dist) pairs the public functions take"""
    C = len(ext)
    theta, d5 = np.zeros((C, 12)), np.zeros((C, 5))
    for c in range(C):
        K, d = intr[c]
        d = np.r_[np.ravel(d), np.zeros(5)][:5]
        theta[c] = np.r_[K[0, 0], K[1, 1], K[0, 2], K[1, 2], d[0], d[1], ext[c]]
        d5[c] = d
    return theta, d5


def linearise(points, uvs, ext, intr, loss, f_scale, second=False):
    """seen (C, P), f (C, P, 2), w (C, P, 2) (zero where unseen), A (C, P, 2, 3), B (C, P, 2, 12)"""
    theta, d5 = camera_blocks(ext, intr)
    X = np.asarray(points, dtype=np.float64)
    uv = np.stack([np.asarray(u, dtype=np.float64) for u in uvs])
    seen = ~np.isnan(uv).any(-1)
    Xs = np.where(np.isnan(X), 0.0, X)
    rows = [camera_rows(Xs, theta[c], d5[c], second) for c in range(len(ext))]
    f = np.where(seen[..., None], uv - np.stack([r[0] for r in rows]), 0.0)
    w = rho1((f / f_scale) ** 2, loss) * seen[..., None]
    return seen, f, w, np.stack([r[1] for r in rows]), np.stack([r[2] for r in rows])


def uncertainty(points, uvs, ext, intr, camera_covariance=None, sigma=None, loss="linear", f_scale=1.0, formulation="cholesky"):
    """dict: detection (P, 3, 3), calibration (P, 3, 3) or None, G (P, 3, 12 C), status, views, sigma2, n_residuals, n_free, n_unusable, n_degenerate,
    cond (P,), T (P, 3, 3) or None, bound (P,).  formulation "cholesky" is the definition; "lu" (numpy's inverse of the unscaled H) is the second
    host formulation the spread is measured with."""
    X = np.asarray(points, dtype=np.float64)
    P, C = len(X), len(ext)
    seen, f, w, A, B = linearise(X, uvs, ext, intr, loss, f_scale, second=formulation != "cholesky")
    views = seen.sum(0).astype(np.int32)
    H = np.einsum("cpki,cpk,cpkj->pij", A, w, A)
    status = np.where((views >= 2) & ~np.isnan(X).any(1), 1, -1).astype(np.int32)
    Hi, cond = np.full((P, 3, 3), np.nan), np.full(P, np.nan)
    for p in np.flatnonzero(status == 1):
        d = np.diagonal(H[p])
        if not (d > 0).all():
            status[p] = -2
            continue
        s = 1 / np.sqrt(d)
        Hs = H[p] * np.outer(s, s)
        try:
            L = scipy.linalg.cholesky(Hs, lower=True)
        except np.linalg.LinAlgError:
            status[p] = -2
            continue
        if (np.diagonal(L) ** 2 < PIVOT2_MIN).any():
            status[p] = -2
            continue
        cond[p] = np.linalg.cond(Hs)
        Hi[p] = scipy.linalg.cho_solve((L, True), np.eye(3)) * np.outer(s, s) if formulation == "cholesky" else np.linalg.inv(H[p])
        Hi[p] = 0.5 * (Hi[p] + Hi[p].T)
    ok = status == 1
    m, nfree = int(2 * views[ok].sum()), int(3 * ok.sum())
    if sigma is None:
        sigma2 = float((w * f * f)[:, ok].sum() / (m - nfree)) if m > nfree else float("nan")
    else:
        sigma2 = float(sigma) ** 2
    G = np.einsum("pij,cpkj,cpk,cpkl->picl", np.where(ok[:, None, None], Hi, 0.0), A, w, B).reshape(P, 3, 12 * C)
    G[~ok] = np.nan
    cal = T = None
    if camera_covariance is not None:
        S = np.asarray(camera_covariance, dtype=np.float64)
        cal = np.einsum("pia,ab,pjb->pij", G, S, G)
        cal = 0.5 * (cal + cal.transpose(0, 2, 1))
        T = np.einsum("pia,ab,pjb->pij", np.abs(G), np.abs(S), np.abs(G))
    return dict(detection=sigma2 * Hi, calibration=cal, G=G, status=status, views=views, sigma2=sigma2, n_residuals=m, n_free=nfree, n_unusable=int((status == -1).sum()),
                n_degenerate=int((status == -2).sum()), cond=cond, T=T, bound=(BOUND_FACTOR if loss == "linear" else ROBUST_BOUND_FACTOR) * cond * EPS)


def detection_error(got, ref):
    """per point: max_ij |got - ref|_ij / sqrt(ref_ii ref_jj), over the points where ref is finite (NaN elsewhere)"""
    d = np.sqrt(np.diagonal(ref, axis1=1, axis2=2))
    with np.errstate(invalid="ignore"):
        return (np.abs(got - ref) / (d[:, :, None] * d[:, None, :])).max(axis=(1, 2))


def calibration_error(got, ref, T):
    """per point: max_ij |got - ref|_ij / sqrt(T_ii T_jj); where T is zero (no camera that sees the point has a variance) only the exact value
    passes: 0 for equal entries, inf otherwise"""
    d = np.sqrt(np.diagonal(T, axis1=1, axis2=2))
    num, den = np.abs(got - ref), d[:, :, None] * d[:, None, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(den > 0, num / den, np.where(num == 0, 0.0, np.where(np.isnan(num), np.nan, np.inf))).max(axis=(1, 2))


def random_covariance(C, seed=0):
    """a dense random positive semi-definite (12 C, 12 C) camera covariance at the scales of a real one (pixels, 1e-3 distortion, milliradians,
    half a millimetre), every pair of parameters correlated"""
    rng = np.random.default_rng(1000 + seed)
    n = 12 * C
    M = rng.normal(size=(n, n + 4))
    s = np.tile(np.r_[1.0, 1.0, 0.7, 0.7, 1e-3, 2e-3, 1e-3, 1e-3, 1e-3, 0.5, 0.5, 0.8], C)
    S = (M @ M.T) / (n + 4) * np.outer(s, s)
    return 0.5 * (S + S.T)


def refine(points, uvs, ext, intr, loss, f_scale, iterations=30):
    """the minimiser of each point's robust cost near `points`: IRLS Gauss-Newton steps on the host, kept only while the cost does not rise"""
    X = np.array(points, dtype=np.float64)
    cost = ks.robust_cost(X, uvs, ext, intr, loss, f_scale)
    for _ in range(iterations):
        seen, f, w, A, _ = linearise(X, uvs, ext, intr, loss, f_scale)
        H = np.einsum("cpki,cpk,cpkj->pij", A, w, A)
        g = np.einsum("cpki,cpk,cpk->pi", A, w, f)
        good = seen.sum(0) >= 2
        step = np.zeros_like(X)
        step[good] = np.linalg.solve(H[good] + 1e-12 * np.eye(3), g[good][..., None])[..., 0]
        trial = ks.robust_cost(X + step, uvs, ext, intr, loss, f_scale)
        better = good & (trial <= cost)
        X[better] += step[better]
        cost[better] = trial[better]
    return X


# name -> (scene: a key of keypoint_scenes.SCENES or (C, P, seed, noise, p_unseen), loss, f_scale, refined)
CASES = {
    "c2_p1": ((2, 1, 41, 0.3, 0.0), "linear", 1.0, True),
    "three": ("three", "linear", 1.0, True),
    "three_exact": ((3, 200, 13, 0.0, 0.25), "linear", 1.0, False),
    "six": ("six", "linear", 1.0, True),
    "outlier_soft_l1": ("outlier", "soft_l1", 2.0, True),
    "outlier_cauchy": ("outlier", "cauchy", 2.0, True),
    "twelve": ("twelve", "linear", 1.0, True),
    "c24_p33": ((24, 33, 52, 0.3, 0.3), "huber", 1.0, True),
    "c3_p65": ((3, 65, 61, 0.3, 0.0), "linear", 1.0, True),
    "c3_p17": ((3, 17, 62, 0.0, 0.1), "arctan", 1.0, False),
    # ---- wide rigs: the natural groups of k_tricov_cal (expected_group) and the panel loop of diag_blocks up to its twelve panels
    "c29_p17": ((29, 17, 71, 0.3, 0.3), "soft_l1", 1.0, True),   # the last natural G = 16; P one past a group
    "c30_p21": ((30, 21, 72, 0.3, 0.3), "huber", 1.0, True),     # the first natural G = 10; P two groups + 1
    "c48_p11": ((48, 11, 73, 0.3, 0.4), "cauchy", 1.0, True),    # the last natural G = 10
    "c49_p11": ((49, 11, 74, 0.3, 0.4), "arctan", 1.0, True),    # the first natural G = 5
    "c64_p6": ((64, 6, 75, 0.3, 0.5), "linear", 1.0, True),      # the cap: n = 768 = ld, twelve panels; P one past a group of 5
}
WIDE_CASES = ("c29_p17", "c30_p21", "c48_p11", "c49_p11", "c64_p6")
# the cases held to ROBUST_BOUND_FACTOR: a robust loss whose weights are off 1 at detections that carry residuals (module docstring)
ROBUST_CASES = ("outlier_soft_l1", "outlier_cauchy", "c29_p17", "c30_p21", "c48_p11", "c49_p11")
# where the pooled sigma2 is compared to 1e-12 relative (module docstring)
POOLED_CASES = ("three", "six", "outlier_soft_l1", "outlier_cauchy", "twelve", "c24_p33", "c3_p65")


@functools.lru_cache(maxsize=None)
def case(name):
    """(inputs, oracle result with the random camera covariance and sigma = SIGMA) of one case, computed once and shared: treat both as read-only.
    inputs: points, uvs, ext, intr, loss, f_scale, camera_covariance.  The result also holds pooled_sigma2, what sigma=None estimates."""
    sc, loss, f_scale, refined = CASES[name]
    uvs, ext, intr, X = ks.make(sc) if isinstance(sc, str) else scene(C=sc[0], P=sc[1], seed=sc[2], noise=sc[3], p_unseen=sc[4])
    pts = refine(X, uvs, ext, intr, loss, f_scale) if refined else X.copy()
    S = random_covariance(len(ext), seed=len(name))
    inputs = dict(points=pts, uvs=uvs, ext=ext, intr=intr, loss=loss, f_scale=f_scale, camera_covariance=S)
    o = uncertainty(pts, uvs, ext, intr, camera_covariance=S, sigma=SIGMA, loss=loss, f_scale=f_scale)
    if name not in ROBUST_CASES:
        o["bound"] = BOUND_FACTOR * o["cond"] * EPS
    o["pooled_sigma2"] = uncertainty(pts, uvs, ext, intr, loss=loss, f_scale=f_scale)["sigma2"]
    return inputs, o


def formulation_spread(name):
    """(detection, calibration) spread between the two host formulations over the case's usable points, in units of BOUND_FACTOR cond EPS"""
    i, o = case(name)
    o2 = uncertainty(i["points"], i["uvs"], i["ext"], i["intr"], camera_covariance=i["camera_covariance"], sigma=SIGMA, loss=i["loss"], f_scale=i["f_scale"], formulation="lu")
    ok = o["status"] == 1
    unit = BOUND_FACTOR * o["cond"][ok] * EPS
    return (float((detection_error(o2["detection"], o["detection"])[ok] / unit).max()), float((calibration_error(o2["calibration"], o["calibration"], o["T"])[ok] / unit).max()))


def check_against_oracle(name, got, o, with_cov=True):
    """the figures of one case (got: a dict with this module's keys), printed, then the bound; shared by the host build's tests and the GPU tier"""
    ok = o["status"] == 1
    assert np.array_equal(got["status"], o["status"]) and np.array_equal(got["views"], o["views"])
    e_det = detection_error(got["detection"], o["detection"])
    worst = float((e_det[ok] / o["bound"][ok]).max()) if ok.any() else 0.0
    line = f"{name}: usable {ok.sum()} / {len(ok)} cond {np.nanmin(o['cond']):.3g} .. {np.nanmax(o['cond']):.3g}  detection term {np.nanmax(e_det):.3g} = {worst:.3g} of the bound"
    worst_cal = 0.0
    if with_cov:
        e_cal = calibration_error(got["calibration"], o["calibration"], o["T"])
        worst_cal = float((e_cal[ok] / o["bound"][ok]).max()) if ok.any() else 0.0
        line += f"  calibration term {np.nanmax(e_cal):.3g} = {worst_cal:.3g} of the bound"
    print(line + f"  sigma2 {got['sigma2']:.17g} (oracle {o['sigma2']:.17g})")
    assert np.isnan(got["detection"][~ok]).all() and np.isfinite(got["detection"][ok]).all()
    assert worst <= 1.0 and worst_cal <= 1.0
    assert (got["n_residuals"], got["n_free"], got["n_unusable"], got["n_degenerate"]) == (o["n_residuals"], o["n_free"], o["n_unusable"], o["n_degenerate"])
    assert got["sigma2"] == o["sigma2"]
    return worst, worst_cal


def check_pooled(name, pooled, given, o):
    """sigma=None against the same call with sigma given: the pooled sigma2 to 1e-12 of the oracle's (its terms f^2 carry the cancellation of
    detection - projection, eps |u| / |f| ~ 1e-13 each: not the 64 cond eps of the blocks), the same counts, and a detection term that is the given
    one rescaled"""
    print(f"{name}: pooled sigma2 {pooled['sigma2']:.17g} (oracle {o['pooled_sigma2']:.17g}, {abs(pooled['sigma2'] - o['pooled_sigma2']) / o['pooled_sigma2']:.3g} relative)")
    assert abs(pooled["sigma2"] - o["pooled_sigma2"]) <= 1e-12 * o["pooled_sigma2"]
    assert (pooled["n_residuals"], pooled["n_free"], pooled["n_unusable"], pooled["n_degenerate"]) == (o["n_residuals"], o["n_free"], o["n_unusable"], o["n_degenerate"])
    ok = o["status"] == 1
    want = given["detection"][ok] * (pooled["sigma2"] / given["sigma2"])
    assert np.abs(pooled["detection"][ok] - want).max() <= 4 * EPS * np.abs(want).max()
    if given["calibration"] is not None:
        assert np.array_equal(pooled["calibration"], given["calibration"], equal_nan=True)
