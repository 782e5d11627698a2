"""Numpy + scipy statement of refine_extrinsics: free-point bundle adjustment of the camera extrinsics on raw keypoint
detections, the checker of the host build (tests/test_hostcheck_kpba.py) and of the GPU tier (tests/test_gpu_kpba.py).

    minimise 0.5 f_scale^2 sum rho((f / f_scale)^2),  f = detection - keypoint_scenes.project5(X_p; extrinsics_c, K_c, dist_c)
over the free extrinsics and the used points (at least two views, a finite start), intrinsics fixed.  Gauge (`held_mask`): all six scalars of
`gauge_camera`; one scalar of `scale_camera` (default: the camera whose centre is farthest from the gauge camera's), the component of its
translation along which d = -R_j (c_j - c_0) is largest in magnitude -- scaling the rig about c_0 moves t_j along d; a camera no used point sees is
held whole.  Afterwards camera centres and points are rescaled about c_0 so that |c_j - c_0| is a given baseline (`rescale`; by default the start's).

`solve` is scipy.optimize.least_squares with method="trf", tr_solver="exact", jac="3-point", x_scale="jac", ftol = xtol = 1e-15, gtol = 1e-12.

Two starts of one case differ in their own baselines by millimetres (the translations are perturbed), so the two-start spread is taken after both
optima are rescaled to the FIRST start's baseline: what is compared is the optimum's shape, the one thing the data determine.

Bound of the Schur system (`check_schur`).  S = U - sum_p W_p H_p^-1 W_p^T is a difference of positive semi-definite matrices of the size of
U = sum B^T B, and each subtracted term passes through the inverse of a 3 x 3 block: an entry's error is bounded, as tests/tricov_oracle.py derives
for G Sigma G^T, by k cond eps times the uncancelled magnitude, here
    |S_got - S_ref|_ij <= BOUND_FACTOR cond EPS sqrt(U_ii U_jj),     |rhs_got - rhs_ref|_i <= BOUND_FACTOR cond EPS sqrt(U_ii) |f|_2
with cond the largest cond_2 of the Jacobi-scaled H_p over the used points and BOUND_FACTOR the project's 64 (by Cauchy-Schwarz
|g_c|_i <= sqrt(U_ii) |f|_2 and the same for W H^-1 g_p).  Neither factor comes from the code under test."""
import os

import numpy as np

import keypoint_scenes as ks
import tricov_oracle as tco
from test_triangulate_cpu import scene

EPS = 2.2e-16
BOUND_FACTOR = 64.0
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kpba.npz")
TWO_START_RULE = 1e-7   # a case is pinned to 1e-6 only if its own two starts agree to 1e-7 relative
# name -> (scene, loss, points kept: the first so many, None = all).  "c24": 24 cameras x 60 points, "c2": 2 cameras x 8 points
# (tests/test_triangulate_cpu.scene); "six_pN": "six" cut to N points, one short of, at and one past a group of 16, 32 and 64 points
CASES = {"three": ("three", "linear", None), "six": ("six", "linear", None), "twelve": ("twelve", "linear", None), "outlier": ("outlier", "soft_l1", None),
         "outlier_huber": ("outlier", "huber", None), "c24": ("c24", "linear", None), "c2": ("c2", "linear", None)}
TRUNCATED = tuple(f"six_p{n}" for n in (15, 16, 17, 31, 32, 33, 63, 64, 65))
CASES.update({name: ("six", "linear", int(name[5:])) for name in TRUNCATED})
EXTRA_SCENES = {"c24": dict(C=24, P=60, seed=41, noise=0.3, p_unseen=0.5), "c2": dict(C=2, P=8, seed=43, noise=0.3, p_unseen=0.0)}
START_SEEDS = (2001, 2002)


def make_scene(name, keep=None):
    uvs, ext, intr, X = scene(**EXTRA_SCENES[name]) if name in EXTRA_SCENES else ks.make(name)
    return [u[:keep] for u in uvs], ext, intr, X[:keep]


def perturbed_start(ext, X, gauge_camera, seed):
    """extrinsics of the non-gauge cameras + N(0, 5e-3 rad), N(0, 2 mm); points + N(0, 1 mm)"""
    rng = np.random.default_rng(seed)
    e = np.array(ext, dtype=np.float64)
    d = np.concatenate([rng.normal(0, 5e-3, (len(e), 3)), rng.normal(0, 2.0, (len(e), 3))], axis=1)
    d[gauge_camera] = 0.0
    return e + d, np.asarray(X, dtype=np.float64) + rng.normal(0, 1.0, np.shape(X))


def centres(ext):
    return np.stack([-ks.rodrigues(e[:3]).T @ e[3:] for e in np.asarray(ext, dtype=np.float64)])


def default_scale_camera(ext, gauge_camera):
    c = centres(ext)
    return int(np.argmax(np.linalg.norm(c - c[gauge_camera], axis=1)))


def used_points(uvs, points):
    seen = ~np.isnan(np.stack(uvs)).any(-1)
    return (seen.sum(0) >= 2) & np.isfinite(points).all(-1), seen


def held_mask(ext, uvs, points, gauge_camera=0, scale_camera=None):
    """(held (C, 6) bool, scale_camera)"""
    ext = np.asarray(ext, dtype=np.float64)
    if scale_camera is None:
        scale_camera = default_scale_camera(ext, gauge_camera)
    held = np.zeros((len(ext), 6), dtype=bool)
    held[gauge_camera] = True
    c = centres(ext)
    d = -ks.rodrigues(ext[scale_camera][:3]) @ (c[scale_camera] - c[gauge_camera])
    held[scale_camera, 3 + int(np.argmax(np.abs(d)))] = True
    used, seen = used_points(uvs, points)
    held[~(seen & used[None]).any(1)] = True
    return held, scale_camera


def residual_vector(ext, X, uvs, intr, used, seen):
    """the present scalars of the used points, camera-major"""
    out = []
    for c in range(len(ext)):
        sel = used & seen[c]
        out.append((np.asarray(uvs[c])[sel] - ks.project5(X[sel], ext[c], *intr[c])).ravel())
    return np.concatenate(out)


def cost_of(ext, X, uvs, intr, loss, f_scale=1.0):
    used, seen = used_points(uvs, X)
    f = residual_vector(np.asarray(ext), np.asarray(X), uvs, intr, used, seen)
    return 0.5 * f_scale ** 2 * ks.rho((f / f_scale) ** 2, loss).sum()


def rescale(ext, X, gauge_camera, scale_camera, baseline):
    """centres and points about c_0 by baseline / |c_j - c_0|: every projection is unchanged.  Returns (ext, X, factor)"""
    ext = np.array(ext, dtype=np.float64)
    c = centres(ext)
    c0 = c[gauge_camera]
    s = baseline / np.linalg.norm(c[scale_camera] - c0)
    for k in range(len(ext)):
        ext[k, 3:] = -ks.rodrigues(ext[k, :3]) @ (c0 + s * (c[k] - c0))
    return ext, c0 + s * (np.asarray(X) - c0), s


def baseline_of(ext, gauge_camera, scale_camera):
    c = centres(ext)
    return float(np.linalg.norm(c[scale_camera] - c[gauge_camera]))


def solve(uvs, ext0, intr, pts0, loss="linear", f_scale=1.0, gauge_camera=0, scale_camera=None, baseline=None, max_nfev=200):
    """dict(extrinsics, points (NaN rows where unused), cost, held, scale_camera, used, scipy=the OptimizeResult)"""
    from scipy.optimize import least_squares

    ext0, pts0 = np.asarray(ext0, dtype=np.float64), np.asarray(pts0, dtype=np.float64)
    held, scale_camera = held_mask(ext0, uvs, pts0, gauge_camera, scale_camera)
    used, seen = used_points(uvs, pts0)
    free = ~held
    nf = int(free.sum())

    def unpack(x):
        e = ext0.copy()
        e[free] = x[:nf]
        X = pts0.copy()
        X[used] = x[nf:].reshape(-1, 3)
        return e, X

    def fun(x):
        e, X = unpack(x)
        return residual_vector(e, X, uvs, intr, used, seen)

    r = least_squares(fun, np.r_[ext0[free], pts0[used].ravel()], method="trf", tr_solver="exact", jac="3-point", x_scale="jac", ftol=1e-15, xtol=1e-15, gtol=1e-12, loss=loss, f_scale=f_scale,
                      max_nfev=max_nfev)
    e, X = unpack(r.x)
    e, X, s = rescale(e, X, gauge_camera, scale_camera, baseline_of(ext0, gauge_camera, scale_camera) if baseline is None else baseline)
    X[~used] = np.nan
    return dict(extrinsics=e, points=X, cost=cost_of(e, np.where(used[:, None], X, pts0), uvs, intr, loss, f_scale), held=held, scale_camera=scale_camera, used=used, scale=s, scipy=r)


def relative_spread(a, b):
    """max |a - b| / max(1, |a|) over the finite entries"""
    a, b = np.asarray(a), np.asarray(b)
    ok = np.isfinite(a) & np.isfinite(b)
    return float((np.abs(a - b)[ok] / np.maximum(1.0, np.abs(a)[ok])).max()) if ok.any() else 0.0


_golden = None


def golden():
    global _golden
    if _golden is None:
        _golden = dict(np.load(GOLDEN, allow_pickle=False))
    return _golden


def pinned_cases():
    g = golden()
    return [n for n in CASES if f"{n}/extrinsics" in g and bool(g[f"{n}/pinned"])]


def case(name):
    """the inputs (scene and first start) and the stored optimum of a case"""
    g = golden()
    sc, loss, keep = CASES[name]
    uvs, ext, intr, X = make_scene(sc, keep)
    return dict(uvs=uvs, intr=intr, loss=loss, ext0=g[f"{name}/ext0"], pts0=g[f"{name}/pts0"]), \
        dict(extrinsics=g[f"{name}/extrinsics"], points=g[f"{name}/points"], cost=float(g[f"{name}/cost"]), held=g[f"{name}/held"], spread_ext=float(g[f"{name}/spread_ext"]),
             spread_pts=float(g[f"{name}/spread_pts"]), scale_camera=int(g[f"{name}/scale_camera"]))


def check_result(name, ext, pts, cost, o):
    """the three bars of a pinned case; prints each figure before it asserts"""
    used = np.isfinite(o["points"]).all(-1)
    e_err = (np.abs(ext - o["extrinsics"]) / np.maximum(1.0, np.abs(o["extrinsics"]))).max()
    p_err = (np.abs(pts[used] - o["points"][used]) / np.maximum(1.0, np.abs(o["points"][used]))).max()
    p_abs = np.abs(pts[used] - o["points"][used]).max()
    p_bar_abs = 10 * o["spread_pts"]
    print(f"{name}: cost {cost:.15g} golden {o['cost']:.15g} ratio-1 {cost / o['cost'] - 1:.3g}; extrinsics {e_err:.3g} (bar 1e-6); points rel {p_err:.3g} abs {p_abs:.3g} (bars 1e-6 rel, {p_bar_abs:.3g} abs)")
    assert np.array_equal(np.isnan(pts).any(-1), ~used)
    assert cost <= o["cost"] * (1 + 1e-10)
    assert e_err <= 1e-6
    assert p_err <= 1e-6 or p_abs <= p_bar_abs


# ---------------------------------------------------------------- the dense Schur system (linear loss), for the Jacobian check
def dense_system(uvs, ext, intr, X, held):
    """Analytic J (tricov_oracle.camera_rows) of the residuals over (free camera scalars | used points); returns S, rhs at lambda = 0 over the free
    camera scalars, U's diagonal, |f|_2 and the largest cond_2 of the scaled point blocks"""
    ext, X = np.asarray(ext, dtype=np.float64), np.asarray(X, dtype=np.float64)
    used, seen = used_points(uvs, X)
    C = len(ext)
    theta, d5 = tco.camera_blocks(ext, intr)
    pu = np.flatnonzero(used)
    rows_c, rows_p, Bs, As, fs = [], [], [], [], []
    for c in range(C):
        uv, A, B = tco.camera_rows(X[pu], theta[c], d5[c])
        sel = seen[c][pu]
        for k in np.flatnonzero(sel):
            rows_c.append(c); rows_p.append(k); As.append(A[k]); Bs.append(B[k][:, 6:]); fs.append(np.asarray(uvs[c])[pu[k]] - uv[k])
    m = len(rows_c)
    Jc, Jp, f = np.zeros((2 * m, 6 * C)), np.zeros((2 * m, 3 * len(pu))), np.concatenate(fs)
    for i in range(m):
        Jc[2 * i:2 * i + 2, 6 * rows_c[i]:6 * rows_c[i] + 6] = -Bs[i]
        Jp[2 * i:2 * i + 2, 3 * rows_p[i]:3 * rows_p[i] + 3] = -As[i]
    free = ~np.asarray(held).ravel()
    Jc = Jc[:, free]
    U, W, H = Jc.T @ Jc, Jc.T @ Jp, Jp.T @ Jp
    gc, gp = Jc.T @ f, Jp.T @ f
    Hi = np.zeros_like(H)
    cond = 1.0
    for k in range(len(pu)):
        blk = H[3 * k:3 * k + 3, 3 * k:3 * k + 3]
        d = 1 / np.sqrt(np.diagonal(blk))
        cond = max(cond, np.linalg.cond(blk * np.outer(d, d)))
        Hi[3 * k:3 * k + 3, 3 * k:3 * k + 3] = np.linalg.inv(blk)
    return dict(S=U - W @ Hi @ W.T, rhs=-gc + W @ Hi @ gp, Udiag=np.diagonal(U).copy(), fnorm=float(np.linalg.norm(f)), cond=float(cond), free=free)


def check_schur(name, S, rhs, d):
    bS = BOUND_FACTOR * d["cond"] * EPS * np.sqrt(np.outer(d["Udiag"], d["Udiag"]))
    br = BOUND_FACTOR * d["cond"] * EPS * np.sqrt(d["Udiag"]) * d["fnorm"]
    rS, rr = (np.abs(S - d["S"]) / bS).max(), (np.abs(rhs - d["rhs"]) / br).max()
    print(f"{name}: cond {d['cond']:.3g}; S error / bound {rS:.3g}; rhs error / bound {rr:.3g}")
    assert rS <= 1 and rr <= 1
