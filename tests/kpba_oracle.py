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
    |S_got - S_ref|_ij <= BOUND_FACTOR cond EPS sqrt(U_ii U_jj)
    |rhs_got - rhs_ref|_i <= BOUND_FACTOR EPS sqrt(U_ii) (cond |f|_2 + max|detection| sqrt(n_scalars))
with cond the largest cond_2 of the Jacobi-scaled H_p over the used points and BOUND_FACTOR the project's 64 (by Cauchy-Schwarz
|g_c|_i <= sqrt(U_ii) |f|_2 and the same for W H^-1 g_p).  The second term of the right-hand side's bound is the rounding of every residual
f = detection - projection, which happens at the magnitude of the detection (eps max|detection| per scalar, not eps |f|), carried through the
same Cauchy-Schwarz step over the n_scalars present scalars; without it the bound is not met piece by piece (g_c and W H^-1 g_p each on its own)
where |f| is small against the pixel coordinates and the points are few ("c2": 8 points, |f|_2 about 1).  Neither factor comes from the code
under test.

`block_system` states one evaluation block by block in O(P C), for every loss, f_scale, damping and held bits, accumulated in np.longdouble; its
checkers (`check_block`, `check_step`) hold the host build (tests/test_hostcheck_kpba.py) and the kernels (tests/test_gpu_kpba_system.py) to
    U, Y Y^T (each entry)      BOUND_FACTOR cond EPS sqrt(U_ii U_jj)
    g_c, sum Y z (each entry)  the right-hand side's bound above
    cost                       BOUND_FACTOR EPS (cost + |f|_2 max|detection| sqrt(n_scalars))
    max |g_p|                  BOUND_FACTOR EPS max_p,i sum_k |A_ki| (|f_k| + max|detection|)
    dX_p, coordinate j         BOUND_FACTOR cond_p EPS d_j (|D g_p|_2 + |D q_p|_2 + max|detection| sqrt(2 views_p)), D = diag(H_p)^-1/2; the trial point
                               X + dX adds 4 EPS |X_pj| (the rounding of the sum)
    sum X^2                    n_used EPS relative (positive terms: any order of summation)
    sum dX^2                   the same, plus the bounds of dX carried through the squares
    trial cost                 the cost's bound, against `cost_of` at the trial points that came back (the cost evaluation apart from the step)
A status -2 point (a zero on the diagonal of H_p with two views and a finite start) is stated but exercised nowhere: no input was found that
reaches it without also being status -1."""
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
    maxdet = max(float(np.abs(np.asarray(uvs[c])[used & seen[c]]).max()) for c in range(C) if (used & seen[c]).any())
    return dict(S=U - W @ Hi @ W.T, rhs=-gc + W @ Hi @ gp, Udiag=np.diagonal(U).copy(), fnorm=float(np.linalg.norm(f)), cond=float(cond), free=free, maxdet=maxdet, n_scalars=len(f))


def check_schur(name, S, rhs, d):
    """the bounds of the module docstring; the right-hand side's carries the rounding of the residuals at pixel magnitude"""
    bS = BOUND_FACTOR * d["cond"] * EPS * np.sqrt(np.outer(d["Udiag"], d["Udiag"]))
    br = BOUND_FACTOR * EPS * np.sqrt(d["Udiag"]) * (d["cond"] * d["fnorm"] + d["maxdet"] * np.sqrt(d["n_scalars"]))
    rS, rr = (np.abs(S - d["S"]) / bS).max(), (np.abs(rhs - d["rhs"]) / br).max()
    print(f"{name}: cond {d['cond']:.3g}; S error / bound {rS:.3g}; rhs error / bound {rr:.3g}")
    assert rS <= 1 and rr <= 1


# ---------------------------------------------------------------- one evaluation, block by block (every loss, damping and held bits)
LOSS_NAMES = ("linear", "soft_l1", "huber", "cauchy", "arctan")
LD = np.longdouble


def loss_terms(f, loss, f_scale):
    """rho(z), rho'(z) and the curvature weight max(max(rho' + 2 rho'' z, eps), 0.1 rho') at z = (f / f_scale)^2, restated (not the library's)"""
    z = (f / LD(f_scale)) ** 2
    one = np.ones_like(z)
    if loss == "linear":
        r0, r1, r2 = z, one, 0 * z
    elif loss == "soft_l1":
        t = 1 + z
        r0, r1, r2 = 2 * (np.sqrt(t) - 1), 1 / np.sqrt(t), -0.5 / (t * np.sqrt(t))
    elif loss == "huber":
        small, zs = z <= 1, np.maximum(z, 1)
        r0, r1, r2 = np.where(small, z, 2 * np.sqrt(zs) - 1), np.where(small, one, 1 / np.sqrt(zs)), np.where(small, 0 * z, -0.5 / (zs * np.sqrt(zs)))
    elif loss == "cauchy":
        r0, r1, r2 = np.log1p(z), 1 / (1 + z), -1 / (1 + z) ** 2
    elif loss == "arctan":
        r0, r1, r2 = np.arctan(z), 1 / (1 + z * z), -2 * z / (1 + z * z) ** 2
    else:
        raise ValueError(loss)
    return r0, r1, np.maximum(np.maximum(r1 + 2 * r2 * z, LD(np.finfo(np.float64).eps)), 0.1 * r1)


def _inv3(M):
    """inverse of the symmetric (n, 3, 3) M by cofactors, in M's precision"""
    a, b, c, d, e, f = M[:, 0, 0], M[:, 0, 1], M[:, 0, 2], M[:, 1, 1], M[:, 1, 2], M[:, 2, 2]
    c00, c01, c02, c11, c12, c22 = d * f - e * e, c * e - b * f, b * e - c * d, a * f - c * c, b * c - a * e, a * d - b * b
    det = a * c00 + b * c01 + c * c02
    return np.stack([np.stack([c00, c01, c02], -1), np.stack([c01, c11, c12], -1), np.stack([c02, c12, c22], -1)], -2) / det[:, None, None]


def block_system(uvs, ext, intr, X, held, loss="linear", f_scale=1.0, lam=0.0, step=None, chunk=4096):
    """One evaluation at (ext, X), vectorised over the points and accumulated in np.longdouble, O(P C):
        U (6 C, 6 C) block diagonal, gc (6 C), YY = sum_p W_p (H_p + lam diag H_p)^-1 W_p^T, Yz = sum_p W_p (H_p + lam diag H_p)^-1 g_p
        (rows of W of a held scalar zeroed; U and gc are not), cost, count (present scalars), gmax = max |g_p|, status (P,),
        cond (used points: cond_2 of the Jacobi-scaled H_p), fnorm = |f|_2, maxdet = max |detection|, gmax_bound.
    held: (C, 6) bool.  step = (ext_trial, dtheta (C, 6)): also dX (P, 3; zero where unused), dX_bound (P, 3), trial = X + dX (unused rows as
    they are), sum_dX2, sum_X2, sum_dX2_bound, sum_X2_bound, ext_trial."""
    ext, X = np.asarray(ext, dtype=np.float64), np.asarray(X, dtype=np.float64)
    uv = np.stack([np.asarray(u, dtype=np.float64) for u in uvs])
    C, P = uv.shape[:2]
    free = ~np.asarray(held, dtype=bool).reshape(C, 6)
    seen = ~np.isnan(uv).any(-1)
    cand = (seen.sum(0) >= 2) & np.isfinite(X).all(-1)
    theta, d5 = tco.camera_blocks(ext, intr)
    pc = np.flatnonzero(cand)
    rows = []
    H = np.zeros((len(pc), 3, 3), LD)
    for c in range(C):
        proj, A, B = tco.camera_rows(X[pc], theta[c], d5[c])
        sel = seen[c][pc]
        f = np.where(sel[:, None], uv[c][pc] - proj, 0.0).astype(LD)
        r0, r1, w = loss_terms(f, loss, f_scale)
        m = sel[:, None].astype(LD)
        rows.append((A.astype(LD), B[:, :, 6:].astype(LD), f, r0 * m, r1 * m, w * m, sel))
        H += np.einsum("nki,nk,nkj->nij", rows[-1][0], rows[-1][5], rows[-1][0])
    ok = (np.diagonal(H, axis1=1, axis2=2) > 0).all(-1)
    status = np.full(P, -1, np.int32)
    status[pc] = np.where(ok, 1, -2)
    pu = pc[ok]
    n = len(pu)
    H = H[ok]
    g, gb, W = np.zeros((n, 3), LD), np.zeros((n, 3), LD), np.zeros((n, C, 6, 3), LD)
    U, gc = np.zeros((6 * C, 6 * C), LD), np.zeros(6 * C, LD)
    cost, f2, views, maxdet = LD(0), LD(0), np.zeros(n, np.int64), 0.0
    for c in range(C):
        A, B, f, r0, r1, w, sel = (a[ok] for a in rows[c])
        if sel.any():
            maxdet = max(maxdet, float(np.abs(uv[c][pu][sel]).max()))
        views += sel
        g -= np.einsum("nki,nk->ni", A, r1 * f)
        W[:, c] = np.einsum("nka,nk,nki->nai", B, w, A)
        U[6 * c:6 * c + 6, 6 * c:6 * c + 6] = np.einsum("nka,nk,nkb->ab", B, w, B)
        gc[6 * c:6 * c + 6] = -np.einsum("nka,nk->a", B, r1 * f)
        cost += (LD(0.5) * LD(f_scale) ** 2 * r0).sum()
        f2 += (f * f).sum()
    for c in range(C):   # (max |detection| is known only now)
        A, _, f, _, _, _, sel = (a[ok] for a in rows[c])
        gb += np.einsum("nki,nk->ni", np.abs(A), (np.abs(f) + maxdet) * sel[:, None])
    del rows
    d = 1 / np.sqrt(np.diagonal(H, axis1=1, axis2=2))
    Hs = H * d[:, :, None] * d[:, None, :]
    cond = np.linalg.cond(Hs.astype(np.float64)) if n else np.zeros(0)
    Hi = _inv3(Hs + LD(lam) * np.eye(3, dtype=LD)) * d[:, :, None] * d[:, None, :]
    Wf = (W * free[None, :, :, None]).reshape(n, 6 * C, 3)
    YY, Yz = np.zeros((6 * C, 6 * C), LD), np.zeros(6 * C, LD)
    for s in range(0, n, chunk):
        T = np.einsum("nai,nij->naj", Wf[s:s + chunk], Hi[s:s + chunk])
        YY += np.einsum("naj,nbj->ab", T, Wf[s:s + chunk])
        Yz += np.einsum("naj,nj->a", T, g[s:s + chunk])
    fnorm, count = float(np.sqrt(f2)), int(2 * views.sum())
    out = dict(U=U.astype(np.float64), gc=gc.astype(np.float64), YY=YY.astype(np.float64), Yz=Yz.astype(np.float64), cost=float(cost), count=count,
               gmax=float(np.abs(g).max()) if n else 0.0, gmax_bound=BOUND_FACTOR * EPS * float(gb.max()) if n else 0.0, status=status, used=status == 1, cond=cond,
               fnorm=fnorm, maxdet=maxdet, free=free, views=views)
    if step is not None:
        ext_trial, dth = np.asarray(step[0], dtype=np.float64), np.asarray(step[1], dtype=np.float64).reshape(C, 6).astype(LD)
        q = np.einsum("ncai,ca->ni", W, dth)
        dX = -np.einsum("nij,nj->ni", Hi, g + q)
        bound = BOUND_FACTOR * cond[:, None] * EPS * d * (np.linalg.norm(d * g, axis=1) + np.linalg.norm(d * q, axis=1) + maxdet * np.sqrt(2.0 * views))[:, None]
        full_dX, full_b = np.zeros((P, 3)), np.zeros((P, 3))
        full_dX[pu], full_b[pu] = dX.astype(np.float64), bound.astype(np.float64)
        trial = X.copy()
        trial[pu] = (X[pu].astype(LD) + dX).astype(np.float64)
        sum_dX2, sum_X2 = float((dX * dX).sum()), float((X[pu].astype(LD) ** 2).sum())
        out.update(dX=full_dX, dX_bound=full_b, trial=trial, sum_dX2=sum_dX2, sum_X2=sum_X2, sum_X2_bound=n * EPS * sum_X2,
                   sum_dX2_bound=n * EPS * sum_dX2 + float((2 * np.abs(dX) * bound + bound * bound).sum()), ext_trial=ext_trial)
    return out


def cost_bound(cost, fnorm, maxdet, count):
    return BOUND_FACTOR * EPS * (cost + fnorm * maxdet * np.sqrt(count))


def cost_with_bound(ext, X, uvs, intr, loss, f_scale=1.0):
    """(cost_of, its bound: BOUND_FACTOR EPS (cost + |f|_2 max|detection| sqrt(n_scalars)))"""
    ext, X = np.asarray(ext, dtype=np.float64), np.asarray(X, dtype=np.float64)
    used, seen = used_points(uvs, X)
    f = residual_vector(ext, X, uvs, intr, used, seen)
    maxdet = max(float(np.abs(np.asarray(uvs[c])[used & seen[c]]).max()) for c in range(len(ext)) if (used & seen[c]).any())
    ref = cost_of(ext, X, uvs, intr, loss, f_scale)
    return ref, cost_bound(ref, float(np.linalg.norm(f)), maxdet, len(f))


def unpack_acc(acc):
    """(C, 33) -> U (6 C, 6 C) block diagonal, gc (6 C), Yz (6 C)"""
    C = len(acc)
    U, tri = np.zeros((6 * C, 6 * C)), np.tril_indices(6)
    for c in range(C):
        blk = np.zeros((6, 6))
        blk[tri] = acc[c, :21]
        U[6 * c:6 * c + 6, 6 * c:6 * c + 6] = blk + np.tril(blk, -1).T
    return U, acc[:, 21:27].ravel().copy(), acc[:, 27:33].ravel().copy()


def _ratio(err, bound):
    """max err / bound; where the bound is zero only an exact value passes"""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    if err.size == 0:
        return 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf)).max())


def check_block(name, got, o):
    """got: YY (NP, NP), acc (C, 33), cost, count, gmax, tail, point_status of one evaluation (geometry.refine_extrinsics_system's keys; the host
    build's likewise), o: block_system's.  Exact: the statuses and the count, the fourth trailing scalar, zero padding, zero rows and columns
    of held scalars (and their Yz), every tile above the diagonal bit for bit the transpose of its mirror.  Bounded: the module docstring's.
    Prints the ratios before it asserts and returns them."""
    C = len(got["acc"])
    n6 = 6 * C
    YY = np.asarray(got["YY"])
    U, gc, Yz = unpack_acc(np.asarray(got["acc"]))
    cond = float(o["cond"].max()) if len(o["cond"]) else 1.0
    Ud = np.sqrt(np.diagonal(o["U"]))
    bM = BOUND_FACTOR * cond * EPS * np.outer(Ud, Ud)
    bv = BOUND_FACTOR * EPS * Ud * (cond * o["fnorm"] + o["maxdet"] * np.sqrt(o["count"]))
    tiles = np.arange(len(YY)) // 16
    diag_tiles = (tiles[:, None] == tiles[None, :])[:n6, :n6]
    r = dict(U=_ratio(np.abs(U - o["U"]), bM), YY=_ratio(np.abs(YY[:n6, :n6] - o["YY"]), bM), gc=_ratio(np.abs(gc - o["gc"]), bv), Yz=_ratio(np.abs(Yz - o["Yz"]), bv),
             cost=_ratio(abs(got["cost"] - o["cost"]), cost_bound(o["cost"], o["fnorm"], o["maxdet"], o["count"])), gmax=_ratio(abs(got["gmax"] - o["gmax"]), o["gmax_bound"]),
             symmetry=_ratio(np.abs(YY[:n6, :n6] - YY[:n6, :n6].T) * diag_tiles, bM))
    print(f"{name}: used {int(o['used'].sum())} / {len(o['used'])} cond {cond:.3g} |f| {o['fnorm']:.3g}; error / bound: " + " ".join(f"{k} {v:.3g}" for k, v in r.items()))
    assert np.array_equal(got["point_status"], o["status"]) and got["count"] == o["count"] and got["tail"] == 0.0
    assert (YY[n6:] == 0.0).all() and (YY[:, n6:] == 0.0).all()
    upper = tiles[:, None] < tiles[None, :]
    assert np.array_equal(YY[upper], YY.T[upper])
    heldf = ~o["free"].ravel()
    assert (YY[:n6][heldf] == 0.0).all() and (YY[:, :n6][:, heldf] == 0.0).all() and (Yz[heldf] == 0.0).all()
    assert all(v <= 1 for v in r.values()), r
    return r


def check_step(name, trial, step4, o, X, uvs, intr, loss, f_scale):
    """trial (P, 3) and step4 = trial cost, sum dX^2, 0, sum X^2 of one back-substitution against block_system(step=...)'s; the trial cost against
    cost_of at the trial points that came back, under ext_trial.  Prints the ratios before it asserts and returns them."""
    X, trial = np.asarray(X, dtype=np.float64), np.asarray(trial)
    used = o["used"]
    ref, ref_bound = cost_with_bound(o["ext_trial"], trial, uvs, intr, loss, f_scale)
    r = dict(dX=_ratio(np.abs(trial[used] - o["trial"][used]), o["dX_bound"][used] + 4 * EPS * np.abs(X[used])), sum_dX2=_ratio(abs(step4[1] - o["sum_dX2"]), o["sum_dX2_bound"]),
             sum_X2=_ratio(abs(step4[3] - o["sum_X2"]), o["sum_X2_bound"]), trial_cost=_ratio(abs(step4[0] - ref), ref_bound))
    print(f"{name}: step |dX| max {np.abs(o['dX']).max():.3g}; trial cost {step4[0]:.15g} (cost_of {ref:.15g}); error / bound: " + " ".join(f"{k} {v:.3g}" for k, v in r.items()))
    assert np.array_equal(trial[~used], X[~used], equal_nan=True) and step4[2] == 0.0
    assert all(v <= 1 for v in r.values()), r
    return r


# ---------------------------------------------------------------- the inputs of the one-evaluation tests (host tier and GPU tier alike)
# name -> dict(C, P, seed, p_unseen | scene="outlier"; loss, f_scale, lam; edit).  Built at test time from the seeded scene() and perturbed_start.
# edit "gap": every point of the second chunk of 256 starts NaN (a chunk with no usable point between two that have some); "last": only
# the last point of the first chunk and the one point of the second are usable; "held": the gauge camera at 63, one scale bit, camera 2 at
# 0b101010, camera 3 without detections and at 63.
CAMERA_COUNTS = (2, 3, 6, 8, 10, 11, 16, 24)
GROUP_EDGES = (15, 16, 17, 31, 32, 33, 63, 64, 65)
SYSTEM_INPUTS = {f"c{C}": dict(C=C, P=70, seed=100 + C, p_unseen=0.4) for C in CAMERA_COUNTS}
SYSTEM_INPUTS.update({f"g6_p{n}": dict(C=6, P=n, seed=200 + n, p_unseen=0.4) for n in GROUP_EDGES})
SYSTEM_INPUTS.update({f"p{n}": dict(C=3, P=n, seed=300, p_unseen=0.25) for n in (255, 256, 257)})
SYSTEM_INPUTS.update({"p600_gap": dict(C=3, P=600, seed=301, p_unseen=0.25, edit="gap"), "p257_last": dict(C=3, P=257, seed=302, p_unseen=0.0, edit="last"),
                      "held": dict(C=6, P=70, seed=303, p_unseen=0.4, edit="held", loss="soft_l1", f_scale=1.5, lam=1e-2)})
# 512 and 513 chunks: the last shape without the grid stride of k_kpba_reduce and k_kpba_step and the first with it.  The seeds are ones with
# which the last point is a used one (system_case asserts it): the one point of chunk 513 must take part, or a pass that never reaches it shows nowhere
SYSTEM_INPUTS.update({f"big3_p{n}": dict(C=3, P=n, seed=304, p_unseen=0.25) for n in (131072, 131073)})
SYSTEM_INPUTS.update({f"big2_p{n}": dict(C=2, P=n, seed=306, p_unseen=0.2, loss="soft_l1", f_scale=1.5) for n in (131072, 131073)})
LOSS_GRID = [(loss, fs, lam) for loss in LOSS_NAMES for fs in (1.0, 1.5, 3.0) for lam in (0.0, 1e-4, 1.0)]
SYSTEM_INPUTS.update({f"outlier_{loss}_{fs}_{lam}": dict(scene="outlier", loss=loss, f_scale=fs, lam=lam) for loss, fs, lam in LOSS_GRID})
BIG = tuple(n for n in SYSTEM_INPUTS if n.startswith("big"))
PIECES = ("U", "YY", "gc", "Yz", "cost", "gmax", "symmetry", "dX", "sum_dX2", "sum_X2", "trial_cost")

_system_cache = {}


def system_case(name):
    """(inputs, oracle) of one input of SYSTEM_INPUTS, computed once and shared: treat both as read-only.  inputs: uvs, ext0, intr, pts0, held
    (C, 6) bool, loss, f_scale, lam, step = (ext_trial, dtheta)."""
    if name in _system_cache:
        return _system_cache[name]
    sp = SYSTEM_INPUTS[name]
    if sp.get("scene"):
        uvs, ext, intr, X = ks.make(sp["scene"])
        seed = 31
    else:
        uvs, ext, intr, X = scene(C=sp["C"], P=sp["P"], seed=sp["seed"], noise=0.3, p_unseen=sp["p_unseen"])
        seed = sp["seed"]
    uvs = [np.array(u) for u in uvs]
    ext0, pts0 = perturbed_start(ext, X, 0, 5000 + seed)
    edit = sp.get("edit")
    if edit == "gap":
        pts0[256:512] = np.nan
    elif edit == "last":
        pts0[:255] = np.nan
    elif edit == "held":
        uvs[3][:] = np.nan
    held, scale_camera = held_mask(ext0, uvs, pts0, scale_camera=1 if edit == "held" else None)
    if edit == "held":
        held[2] = [False, True, False, True, False, True]   # 0b101010
        assert held[0].all() and held[3].all() and held[1].sum() == 1
    rng = np.random.default_rng(7000 + seed)
    dtheta = np.concatenate([rng.normal(0, 1e-3, (len(ext0), 3)), rng.normal(0, 0.5, (len(ext0), 3))], axis=1) * ~held
    i = dict(uvs=uvs, ext0=ext0, intr=intr, pts0=pts0, held=held, loss=sp.get("loss", "linear"), f_scale=sp.get("f_scale", 1.0), lam=sp.get("lam", 1e-4), step=(ext0 + dtheta, dtheta))
    o = block_system(uvs, ext0, intr, pts0, held, loss=i["loss"], f_scale=i["f_scale"], lam=i["lam"], step=i["step"])
    assert name not in BIG or o["used"][-1]
    if len(_system_cache) >= 8 or name in BIG:   # (the big ones hold hundreds of megabytes: one at a time)
        _system_cache.clear()
    _system_cache[name] = (i, o)
    return i, o


def held_bits(held):
    return np.ascontiguousarray((np.asarray(held, dtype=np.int32) << np.arange(6, dtype=np.int32)).sum(1), dtype=np.int32)


def note_worst(worst, r):
    for k, v in r.items():
        worst[k] = max(worst.get(k, 0.0), v)


def worst_line(title, worst):
    return f"{title}: worst error / bound per piece: " + " ".join(f"{k} {worst.get(k, 0.0):.3g}" for k in PIECES)
