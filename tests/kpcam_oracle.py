"""Numpy + scipy statement of refine_cameras: tests/kpba_oracle.py with the intrinsics among the unknowns.  The checker
of the host build (tests/test_hostcheck_kpcam.py) and of the GPU tier (tests/test_gpu_kpcam_system.py, tests/test_gpu_kpcam.py).

    minimise 0.5 f_scale^2 sum rho((f / f_scale)^2) + 0.5 sum ((theta - theta_0) / std)^2
over the free scalars of theta_c = (fx fy cx cy k1 k2 | rotation vector | translation) and the used points; p1, p2, k3 are constants; the second
sum runs over the free intrinsic scalars with a finite std and never passes through the loss.  Gauge: kpba_oracle.held_mask on the extrinsics
(columns 6 .. 11 of `held12`); the intrinsic columns are held where `free` (C, 6) is False; a camera no used point sees is held whole.

`solve12` is scipy.optimize.least_squares with kpba_oracle.solve's settings, the prior as extra residual rows (theta - theta_0) / std: with a
prior only the linear loss is stated (scipy would put the prior rows through the loss).

`block_system12` is kpba_oracle.block_system with all 12 columns of tricov_oracle.camera_rows (the six intrinsic ones restated in np.longdouble:
`intrinsic_columns`), accumulated in np.longdouble; `check_block12` and
`check_step12` hold an evaluation to the same bound formulas -- they are relative to sqrt(U_ii U_jj), which carries the very different scales
of fx (a derivative of order x' ~ 0.1) and k2 (of order f r^5): nothing about them changes with the number of columns.  Detection weights
enter `block_system12` as sqrt(w) folded into f, A and B (SURVEY 8f-13's one sentence)."""
import os

import numpy as np

import keypoint_scenes as ks
import kpba_oracle as ko
import tricov_oracle as tco
from kpba_oracle import BOUND_FACTOR, EPS, LD, _inv3, _ratio, cost_bound, loss_terms

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kpcam.npz")
GROUPS = {"focal": (0, 1), "principal": (2, 3), "distortion": (4, 5)}
ALL_GROUPS = ("focal", "principal", "distortion")
# name -> (scene, loss, free groups, prior).  The prior: std = (0.5 % of fx, 0.5 % of fy, 2 px, 2 px, 0.005, 0.005) about the start's intrinsics
CASES = {"three_focal": ("three", "linear", ("focal",), False), "six_focal": ("six", "linear", ("focal",), False), "outlier_focal": ("outlier", "soft_l1", ("focal",), False),
         "three_all": ("three", "linear", ALL_GROUPS, False), "six_all": ("six", "linear", ALL_GROUPS, False),
         "three_prior": ("three", "linear", ALL_GROUPS, True), "six_prior": ("six", "linear", ALL_GROUPS, True)}
# stored without a pin whatever their two starts give: without a prior the full set is determined so weakly that its spread straddles the rule
NEVER_PINNED = ("three_all", "six_all")
NOMINAL_SEED = 3001   # the nominal intrinsics of a prior case: the scene's own + N(0, std), the same for both starts (theta_0 is the input)


def free_mask(C, groups):
    free = np.zeros((C, 6), dtype=bool)
    for g in groups:
        free[:, GROUPS[g]] = True
    return free


def theta6_of(intr):
    """(C, 6): fx fy cx cy k1 k2"""
    return np.array([[K[0, 0], K[1, 1], K[0, 2], K[1, 2], *(np.r_[np.ravel(d), 0, 0][:2])] for K, d in intr], dtype=np.float64)


def intr_of(theta6, intr):
    """the (K, dist) list with fx fy cx cy k1 k2 from theta6, everything else as in intr"""
    out = []
    for t, (K, d) in zip(np.asarray(theta6), intr):
        K2 = np.array(K, dtype=np.float64)
        K2[0, 0], K2[1, 1], K2[0, 2], K2[1, 2] = t[:4]
        d2 = np.array(np.ravel(d), dtype=np.float64)
        if d2.size < 2:
            d2 = np.r_[d2, np.zeros(2 - d2.size)]
        d2[:2] = t[4:6]
        out.append((K2, d2))
    return out


def prior_std_of(theta6):
    t = np.asarray(theta6)
    return np.stack([0.005 * t[:, 0], 0.005 * t[:, 1], np.full(len(t), 2.0), np.full(len(t), 2.0), np.full(len(t), 0.005), np.full(len(t), 0.005)], axis=1)


def perturbed_intrinsics(theta6, free, seed):
    """free scalars + N(0, 1 % of fx, fy; 3 px; 0.01)"""
    rng = np.random.default_rng(seed + 50000)
    t = np.asarray(theta6, dtype=np.float64)
    sig = np.stack([0.01 * t[:, 0], 0.01 * t[:, 1], np.full(len(t), 3.0), np.full(len(t), 3.0), np.full(len(t), 0.01), np.full(len(t), 0.01)], axis=1)
    return t + rng.normal(0, 1, t.shape) * sig * free


def case_inputs(name, seed):
    """the scene and one seeded start of a case: dict(uvs, intr (scene), ext0, pts0, theta0 (C, 6), free (C, 6), prior_std (C, 6) or None, loss)"""
    sc, loss, groups, prior = CASES[name]
    uvs, ext, intr, X = ko.make_scene(sc)
    free = free_mask(len(ext), groups)
    e0, p0 = ko.perturbed_start(ext, X, 0, seed)
    t6 = theta6_of(intr)
    if prior:
        std = prior_std_of(t6)
        t0 = t6 + np.random.default_rng(NOMINAL_SEED).normal(0, 1, t6.shape) * std
    else:
        std, t0 = None, perturbed_intrinsics(t6, free, seed)
    return dict(uvs=uvs, intr=intr, ext0=e0, pts0=p0, theta0=t0, free=free, prior_std=std, loss=loss)


def held12_of(ext0, uvs, pts0, free, gauge_camera=0, scale_camera=None):
    """(held (C, 12) bool, scale_camera)"""
    h6, scale_camera = ko.held_mask(ext0, uvs, pts0, gauge_camera, scale_camera)
    held = np.concatenate([~np.asarray(free, dtype=bool), h6], axis=1)
    used, seen = ko.used_points(uvs, pts0)
    held[~(seen & used[None]).any(1)] = True
    return held, scale_camera


def prior_cost(theta6, theta0, std, held12):
    if std is None:
        return 0.0
    on = ~np.asarray(held12)[:, :6] & np.isfinite(std)
    return float(0.5 * (((np.asarray(theta6) - theta0) / std)[on] ** 2).sum())


def solve12(uvs, ext0, intr, theta0, pts0, free, prior_std=None, loss="linear", f_scale=1.0, gauge_camera=0, scale_camera=None, baseline=None, max_nfev=200):
    """dict(extrinsics, theta6 (the intrinsic scalars), points (NaN rows where unused), cost (prior included), prior_cost, held (C, 12),
    scale_camera, used, scipy).  intr: the (K, dist) list that supplies p1, p2, k3; theta0 (C, 6): the start of the intrinsic scalars and the centre of the prior."""
    from scipy.optimize import least_squares

    if prior_std is not None and loss != "linear":
        raise ValueError("with a prior only the linear loss is stated: scipy would put the prior rows through the loss")
    ext0, pts0, theta0 = np.asarray(ext0, dtype=np.float64), np.asarray(pts0, dtype=np.float64), np.asarray(theta0, dtype=np.float64)
    held, scale_camera = held12_of(ext0, uvs, pts0, free, gauge_camera, scale_camera)
    used, seen = ko.used_points(uvs, pts0)
    fr = ~held
    nf = int(fr.sum())
    th0 = np.concatenate([theta0, ext0], axis=1)
    pr = None if prior_std is None else fr[:, :6] & np.isfinite(prior_std)

    def unpack(x):
        th = th0.copy()
        th[fr] = x[:nf]
        X = pts0.copy()
        X[used] = x[nf:].reshape(-1, 3)
        return th, X

    def fun(x):
        th, X = unpack(x)
        f = ko.residual_vector(th[:, 6:], X, uvs, intr_of(th[:, :6], intr), used, seen)
        return f if pr is None else np.r_[f, ((th[:, :6] - theta0) / prior_std)[pr]]

    r = least_squares(fun, np.r_[th0[fr], pts0[used].ravel()], method="trf", tr_solver="exact", jac="3-point", x_scale="jac", ftol=1e-15, xtol=1e-15, gtol=1e-12, loss=loss, f_scale=f_scale,
                      max_nfev=max_nfev)
    th, X = unpack(r.x)
    e, X, s = ko.rescale(th[:, 6:], X, gauge_camera, scale_camera, ko.baseline_of(ext0, gauge_camera, scale_camera) if baseline is None else baseline)
    X[~used] = np.nan
    pc = prior_cost(th[:, :6], theta0, prior_std, held)
    cost = ko.cost_of(e, np.where(used[:, None], X, pts0), uvs, intr_of(th[:, :6], intr), loss, f_scale) + pc
    return dict(extrinsics=e, theta6=th[:, :6].copy(), points=X, cost=cost, prior_cost=pc, held=held, scale_camera=scale_camera, used=used, scale=s, scipy=r)


_golden = None


def golden():
    global _golden
    if _golden is None:
        _golden = dict(np.load(GOLDEN, allow_pickle=False))
    return _golden


def stored_cases(pinned=None):
    g = golden()
    return [n for n in CASES if f"{n}/extrinsics" in g and (pinned is None or bool(g[f"{n}/pinned"]) == pinned)]


def case(name):
    """the inputs (scene and first start) and the stored optimum of a case"""
    g = golden()
    i = case_inputs(name, ko.START_SEEDS[0])
    i.update(ext0=g[f"{name}/ext0"], pts0=g[f"{name}/pts0"], theta0=g[f"{name}/theta0"], free=g[f"{name}/free"])   # (the start as stored)
    keys = ("extrinsics", "theta6", "points", "held")
    o = {k: g[f"{name}/{k}"] for k in keys}
    o.update(cost=float(g[f"{name}/cost"]), prior_cost=float(g[f"{name}/prior_cost"]), scale_camera=int(g[f"{name}/scale_camera"]), spread_ext=float(g[f"{name}/spread_ext"]),
             spread_intr=float(g[f"{name}/spread_intr"]), spread_pts=float(g[f"{name}/spread_pts"]), pinned=bool(g[f"{name}/pinned"]))
    return i, o


def check_result12(name, ext, theta6, pts, cost, o):
    """A pinned case: kpba_oracle.check_result's bars, and the intrinsics to the extrinsics' bar.  An unpinned one: cost <= golden (1 + 1e-6) only."""
    i_err = ko.relative_spread(o["theta6"], theta6)
    print(f"{name}: intrinsics {i_err:.3g} (bar 1e-6 where pinned); pinned {o['pinned']}")
    if not o["pinned"]:
        print(f"{name}: cost {cost:.15g} golden {o['cost']:.15g} ratio-1 {cost / o['cost'] - 1:.3g} (bar 1e-6)")
        assert cost <= o["cost"] * (1 + 1e-6)
        return
    ko.check_result(name, ext, pts, cost, o)
    assert i_err <= 1e-6


# ---------------------------------------------------------------- one evaluation, block by block
def rodrigues_ld(r):
    """keypoint_scenes.rodrigues in np.longdouble"""
    r = np.asarray(r).astype(LD)
    th = np.sqrt((r * r).sum())
    if th == 0:
        return np.eye(3, dtype=LD)
    k = r / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]], dtype=LD)
    return np.eye(3, dtype=LD) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def intrinsic_columns(X, theta, d5):
    """columns 0 .. 5 of B (fx fy cx cy k1 k2) in np.longdouble, the rotation included: (P, 2, 6).  The k1 and k2 columns are f x r^2 and f x r^4:
    monomials of degree 3 and 5 in the normalised coordinates, which carry the cancellation of R X + t three and five times over.  A float64
    rotation matrix is itself a few ulp off (keypoint_scenes.rodrigues: |R R^T - I| = 3 ulp), and one ulp of R moves the k2 diagonal of U by tens
    of ulp: stated in float64 the reference's own error would be of the size of the bound (measured on "g6_p16": 25 eps per half ulp of R,
    bound 122 eps)."""
    th, d = np.asarray(theta).astype(LD), np.asarray(d5).astype(LD)
    Xc = np.asarray(X).astype(LD) @ rodrigues_ld(theta[6:9]).T + th[9:12]
    x, y = Xc[:, 0] / Xc[:, 2], Xc[:, 1] / Xc[:, 2]
    r2 = x * x + y * y
    rad = 1 + r2 * (th[4] + r2 * (th[5] + r2 * d[4]))
    B = np.zeros((len(Xc), 2, 6), LD)
    B[:, 0, 0] = x * rad + 2 * d[2] * x * y + d[3] * (r2 + 2 * x * x)
    B[:, 1, 1] = y * rad + d[2] * (r2 + 2 * y * y) + 2 * d[3] * x * y
    B[:, 0, 2] = B[:, 1, 3] = 1
    B[:, 0, 4], B[:, 1, 4] = th[0] * x * r2, th[1] * y * r2
    B[:, 0, 5], B[:, 1, 5] = th[0] * x * r2 * r2, th[1] * y * r2 * r2
    return B


def block_system12(uvs, ext, intr, X, held, loss="linear", f_scale=1.0, lam=0.0, step=None, weights=None, chunk=4096):
    """kpba_oracle.block_system with n = 12 scalars per camera: U (12 C, 12 C) block diagonal, gc, YY, Yz, cost, count, gmax, status, cond, fnorm,
    maxdet, gmax_bound, free (C, 12).  held: (C, 12) bool.  weights: None or (C, P): sqrt(w) folded into f, A and B; w = 0 or NaN is unseen.
    step = (cameras_trial (C, 12), dtheta (C, 12)): also dX, dX_bound, trial, sum_dX2, sum_X2 and their bounds, cameras_trial."""
    ext, X = np.asarray(ext, dtype=np.float64), np.asarray(X, dtype=np.float64)
    uv = np.stack([np.asarray(u, dtype=np.float64) for u in uvs])
    C, P = uv.shape[:2]
    n = 12
    free = ~np.asarray(held, dtype=bool).reshape(C, n)
    seen = ~np.isnan(uv).any(-1)
    sw = None
    if weights is not None:
        w_ = np.asarray(weights, dtype=np.float64)
        seen &= w_ > 0   # (NaN compares false)
        sw = np.sqrt(np.where(seen, w_, 0.0))
    cand = (seen.sum(0) >= 2) & np.isfinite(X).all(-1)
    theta, d5 = tco.camera_blocks(ext, intr)
    pc = np.flatnonzero(cand)
    rows = []
    H = np.zeros((len(pc), 3, 3), LD)
    for c in range(C):
        proj, A, B = tco.camera_rows(X[pc], theta[c], d5[c])
        B = B.astype(LD)
        B[:, :, :6] = intrinsic_columns(X[pc], theta[c], d5[c])
        sel = seen[c][pc]
        s = (np.ones(len(pc)) if sw is None else sw[c][pc]).astype(LD)
        f = np.where(sel[:, None], uv[c][pc] - proj, 0.0).astype(LD) * s[:, None]
        r0, r1, w = loss_terms(f, loss, f_scale)
        m = sel[:, None].astype(LD)
        rows.append((A.astype(LD) * s[:, None, None], B.astype(LD) * s[:, None, None], f, r0 * m, r1 * m, w * m, sel))
        H += np.einsum("nki,nk,nkj->nij", rows[-1][0], rows[-1][5], rows[-1][0])
    ok = (np.diagonal(H, axis1=1, axis2=2) > 0).all(-1)
    status = np.full(P, -1, np.int32)
    status[pc] = np.where(ok, 1, -2)
    pu = pc[ok]
    nu = len(pu)
    H = H[ok]
    g, gb, W = np.zeros((nu, 3), LD), np.zeros((nu, 3), LD), np.zeros((nu, C, n, 3), LD)
    U, gc = np.zeros((n * C, n * C), LD), np.zeros(n * C, LD)
    cost, f2, views, maxdet = LD(0), LD(0), np.zeros(nu, np.int64), 0.0
    for c in range(C):
        A, B, f, r0, r1, w, sel = (a[ok] for a in rows[c])
        if sel.any():
            maxdet = max(maxdet, float(np.abs(uv[c][pu][sel]).max()))
        views += sel
        g -= np.einsum("nki,nk->ni", A, r1 * f)
        W[:, c] = np.einsum("nka,nk,nki->nai", B, w, A)
        U[n * c:n * c + n, n * c:n * c + n] = np.einsum("nka,nk,nkb->ab", B, w, B)
        gc[n * c:n * c + n] = -np.einsum("nka,nk->a", B, r1 * f)
        cost += (LD(0.5) * LD(f_scale) ** 2 * r0).sum()
        f2 += (f * f).sum()
    for c in range(C):   # (max |detection| is known only now)
        A, _, f, _, _, _, sel = (a[ok] for a in rows[c])
        gb += np.einsum("nki,nk->ni", np.abs(A), (np.abs(f) + maxdet) * sel[:, None])
    del rows
    d = 1 / np.sqrt(np.diagonal(H, axis1=1, axis2=2))
    Hs = H * d[:, :, None] * d[:, None, :]
    cond = np.linalg.cond(Hs.astype(np.float64)) if nu else np.zeros(0)
    Hi = _inv3(Hs + LD(lam) * np.eye(3, dtype=LD)) * d[:, :, None] * d[:, None, :]
    Wf = (W * free[None, :, :, None]).reshape(nu, n * C, 3)
    YY, Yz = np.zeros((n * C, n * C), LD), np.zeros(n * C, LD)
    for s in range(0, nu, chunk):
        T = np.einsum("nai,nij->naj", Wf[s:s + chunk], Hi[s:s + chunk])
        YY += np.einsum("naj,nbj->ab", T, Wf[s:s + chunk])
        Yz += np.einsum("naj,nj->a", T, g[s:s + chunk])
    fnorm, count = float(np.sqrt(f2)), int(2 * views.sum())
    out = dict(U=U.astype(np.float64), gc=gc.astype(np.float64), YY=YY.astype(np.float64), Yz=Yz.astype(np.float64), cost=float(cost), count=count,
               gmax=float(np.abs(g).max()) if nu else 0.0, gmax_bound=BOUND_FACTOR * EPS * float(gb.max()) if nu else 0.0, status=status, used=status == 1, cond=cond,
               fnorm=fnorm, maxdet=maxdet, free=free, views=views)
    if step is not None:
        cam_trial, dth = np.asarray(step[0], dtype=np.float64), np.asarray(step[1], dtype=np.float64).reshape(C, n).astype(LD)
        q = np.einsum("ncai,ca->ni", W, dth)
        dX = -np.einsum("nij,nj->ni", Hi, g + q)
        bound = BOUND_FACTOR * cond[:, None] * EPS * d * (np.linalg.norm(d * g, axis=1) + np.linalg.norm(d * q, axis=1) + maxdet * np.sqrt(2.0 * views))[:, None]
        full_dX, full_b = np.zeros((P, 3)), np.zeros((P, 3))
        full_dX[pu], full_b[pu] = dX.astype(np.float64), bound.astype(np.float64)
        trial = X.copy()
        trial[pu] = (X[pu].astype(LD) + dX).astype(np.float64)
        sum_dX2, sum_X2 = float((dX * dX).sum()), float((X[pu].astype(LD) ** 2).sum())
        out.update(dX=full_dX, dX_bound=full_b, trial=trial, sum_dX2=sum_dX2, sum_X2=sum_X2, sum_X2_bound=nu * EPS * sum_X2,
                   sum_dX2_bound=nu * EPS * sum_dX2 + float((2 * np.abs(dX) * bound + bound * bound).sum()), cameras_trial=cam_trial)
    return out


def unpack_acc12(acc):
    """(C, 102) -> U (12 C, 12 C) block diagonal, gc (12 C), Yz (12 C)"""
    C = len(acc)
    U, tri = np.zeros((12 * C, 12 * C)), np.tril_indices(12)
    for c in range(C):
        blk = np.zeros((12, 12))
        blk[tri] = acc[c, :78]
        U[12 * c:12 * c + 12, 12 * c:12 * c + 12] = blk + np.tril(blk, -1).T
    return U, acc[:, 78:90].ravel().copy(), acc[:, 90:102].ravel().copy()


def check_block12(name, got, o):
    """kpba_oracle.check_block for 12 scalars per camera: got = YY (NP, NP), acc (C, 102), cost, count, gmax, tail, point_status.  Exact: statuses,
    count, the fourth trailing scalar, zero padding, zero rows and columns of held scalars (and their Yz), every tile above the diagonal bit for
    bit the transpose of its mirror.  Bounded: kpba_oracle's module docstring.  Prints the ratios before it asserts and returns them."""
    C = len(got["acc"])
    n12 = 12 * C
    YY = np.asarray(got["YY"])
    U, gc, Yz = unpack_acc12(np.asarray(got["acc"]))
    cond = float(o["cond"].max()) if len(o["cond"]) else 1.0
    Ud = np.sqrt(np.diagonal(o["U"]))
    bM = BOUND_FACTOR * cond * EPS * np.outer(Ud, Ud)
    bv = BOUND_FACTOR * EPS * Ud * (cond * o["fnorm"] + o["maxdet"] * np.sqrt(o["count"]))
    tiles = np.arange(len(YY)) // 16
    diag_tiles = (tiles[:, None] == tiles[None, :])[:n12, :n12]
    r = dict(U=_ratio(np.abs(U - o["U"]), bM), YY=_ratio(np.abs(YY[:n12, :n12] - o["YY"]), bM), gc=_ratio(np.abs(gc - o["gc"]), bv), Yz=_ratio(np.abs(Yz - o["Yz"]), bv),
             cost=_ratio(abs(got["cost"] - o["cost"]), cost_bound(o["cost"], o["fnorm"], o["maxdet"], o["count"])), gmax=_ratio(abs(got["gmax"] - o["gmax"]), o["gmax_bound"]),
             symmetry=_ratio(np.abs(YY[:n12, :n12] - YY[:n12, :n12].T) * diag_tiles, bM))
    print(f"{name}: used {int(o['used'].sum())} / {len(o['used'])} cond {cond:.3g} |f| {o['fnorm']:.3g}; error / bound: " + " ".join(f"{k} {v:.3g}" for k, v in r.items()))
    assert np.array_equal(got["point_status"], o["status"]) and got["count"] == o["count"] and got["tail"] == 0.0
    assert len(YY) == (n12 + 15) // 16 * 16
    assert (YY[n12:] == 0.0).all() and (YY[:, n12:] == 0.0).all()
    upper = tiles[:, None] < tiles[None, :]
    assert np.array_equal(YY[upper], YY.T[upper])
    heldf = ~o["free"].ravel()
    assert (YY[:n12][heldf] == 0.0).all() and (YY[:, :n12][:, heldf] == 0.0).all() and (Yz[heldf] == 0.0).all()
    assert all(v <= 1 for v in r.values()), r
    return r


def cost_with_bound12(cam12, X, uvs, intr, loss, f_scale=1.0, weights=None):
    """the cost at the cameras cam12 (C, 12) and its bound, from block_system12's own residuals (long double)"""
    cam12 = np.asarray(cam12, dtype=np.float64)
    o = block_system12(uvs, cam12[:, 6:], intr_of(cam12[:, :6], intr), X, np.ones((len(cam12), 12), bool), loss=loss, f_scale=f_scale, weights=weights)
    return o["cost"], cost_bound(o["cost"], o["fnorm"], o["maxdet"], o["count"])


def check_step12(name, trial, step4, o, X, uvs, intr, loss, f_scale, weights=None):
    """kpba_oracle.check_step against block_system12(step=...)'s; the trial cost against the cost at the trial points that came back, under cameras_trial"""
    X, trial = np.asarray(X, dtype=np.float64), np.asarray(trial)
    used = o["used"]
    ref, ref_bound = cost_with_bound12(o["cameras_trial"], trial, uvs, intr, loss, f_scale, weights)
    r = dict(dX=_ratio(np.abs(trial[used] - o["trial"][used]), o["dX_bound"][used] + 4 * EPS * np.abs(X[used])), sum_dX2=_ratio(abs(step4[1] - o["sum_dX2"]), o["sum_dX2_bound"]),
             sum_X2=_ratio(abs(step4[3] - o["sum_X2"]), o["sum_X2_bound"]), trial_cost=_ratio(abs(step4[0] - ref), ref_bound))
    print(f"{name}: step |dX| max {np.abs(o['dX']).max():.3g}; trial cost {step4[0]:.15g} (oracle {ref:.15g}); error / bound: " + " ".join(f"{k} {v:.3g}" for k, v in r.items()))
    assert np.array_equal(trial[~used], X[~used], equal_nan=True) and step4[2] == 0.0
    assert all(v <= 1 for v in r.values()), r
    return r


def held_bits12(held):
    return np.ascontiguousarray((np.asarray(held, dtype=np.int32) << np.arange(12, dtype=np.int32)).sum(1), dtype=np.int32)


# ---------------------------------------------------------------- the inputs of the one-evaluation tests (host tier and GPU tier alike)
# kpba_oracle.SYSTEM_INPUTS' recipe (seeded scene(), perturbed_start) with 12 held bits and a 12-column step.  edit "gap", "last" as there;
# "held": gauge camera 0xFC0, one scale bit, camera 2 at 0b101010101010, camera 3 without detections at 0xFFF; "intr_held": every intrinsic bit
# held; "fx": only fx free.  force: MCBA_KPCAM_G.
CAMERA_COUNTS = (2, 3, 4, 5, 6, 11, 12)
GROUP_EDGES = (15, 16, 17, 31, 32, 33, 63, 64, 65)
SYSTEM_INPUTS = {f"c{C}": dict(C=C, P=70, seed=100 + C, p_unseen=0.4) for C in CAMERA_COUNTS}
SYSTEM_INPUTS.update({f"g6_p{n}": dict(C=6, P=n, seed=200 + n, p_unseen=0.4) for n in GROUP_EDGES})
SYSTEM_INPUTS.update({f"p{n}": dict(C=3, P=n, seed=300, p_unseen=0.25) for n in (255, 256, 257)})
SYSTEM_INPUTS.update({"p600_gap": dict(C=3, P=600, seed=301, p_unseen=0.25, edit="gap"), "p257_last": dict(C=3, P=257, seed=302, p_unseen=0.0, edit="last"),
                      "held": dict(C=6, P=70, seed=303, p_unseen=0.4, edit="held", loss="soft_l1", f_scale=1.5, lam=1e-2),
                      "intr_held": dict(C=6, P=70, seed=303, p_unseen=0.4, edit="intr_held"), "fx": dict(C=6, P=70, seed=303, p_unseen=0.4, edit="fx")})
SYSTEM_INPUTS.update({f"big2_p{n}": dict(C=2, P=n, seed=306, p_unseen=0.2, loss="soft_l1", f_scale=1.5) for n in (131072, 131073)})
LOSS_GRID = ko.LOSS_GRID
SYSTEM_INPUTS.update({f"outlier_{loss}_{fs}_{lam}": dict(scene="outlier", loss=loss, f_scale=fs, lam=lam) for loss, fs, lam in LOSS_GRID})
BIG = tuple(n for n in SYSTEM_INPUTS if n.startswith("big"))
PIECES = ko.PIECES

_system_cache = {}


def system_case(name):
    """(inputs, oracle) of one input of SYSTEM_INPUTS, computed once and shared: treat both as read-only.  inputs: uvs, ext0, intr, pts0, held
    (C, 12) bool, loss, f_scale, lam, step = (cameras_trial (C, 12), dtheta (C, 12))."""
    if name in _system_cache:
        return _system_cache[name]
    sp = SYSTEM_INPUTS[name]
    if sp.get("scene"):
        uvs, ext, intr, X = ks.make(sp["scene"])
        seed = 31
    else:
        uvs, ext, intr, X = ko.scene(C=sp["C"], P=sp["P"], seed=sp["seed"], noise=0.3, p_unseen=sp["p_unseen"])
        seed = sp["seed"]
    uvs = [np.array(u) for u in uvs]
    ext0, pts0 = ko.perturbed_start(ext, X, 0, 5000 + seed)
    edit = sp.get("edit")
    if edit == "gap":
        pts0[256:512] = np.nan
    elif edit == "last":
        pts0[:255] = np.nan
    elif edit == "held":
        uvs[3][:] = np.nan
    C = len(ext0)
    free = np.ones((C, 6), dtype=bool)
    if edit == "intr_held":
        free[:] = False
    elif edit == "fx":
        free[:, 1:] = False
    held, scale_camera = held12_of(ext0, uvs, pts0, free, scale_camera=1 if edit == "held" else None)
    if edit == "held":
        held[2] = [False, True] * 6   # 0b101010101010
        assert held[0, 6:].all() and not held[0, :6].any() and held[3].all() and held[1].sum() == 1
    rng = np.random.default_rng(7000 + seed)
    t6 = theta6_of(intr)
    dtheta = np.concatenate([rng.normal(0, 1e-3, (C, 2)) * t6[:, :2], rng.normal(0, 0.5, (C, 2)), rng.normal(0, 1e-3, (C, 2)), rng.normal(0, 1e-3, (C, 3)), rng.normal(0, 0.5, (C, 3))], axis=1) * ~held
    cam0 = np.concatenate([t6, ext0], axis=1)
    i = dict(uvs=uvs, ext0=ext0, intr=intr, pts0=pts0, held=held, loss=sp.get("loss", "linear"), f_scale=sp.get("f_scale", 1.0), lam=sp.get("lam", 1e-4), step=(cam0 + dtheta, dtheta))
    o = block_system12(uvs, ext0, intr, pts0, held, loss=i["loss"], f_scale=i["f_scale"], lam=i["lam"], step=i["step"])
    assert name not in BIG or o["used"][-1]
    if len(_system_cache) >= 8 or name in BIG:   # (the big ones hold hundreds of megabytes: one at a time)
        _system_cache.clear()
    _system_cache[name] = (i, o)
    return i, o
