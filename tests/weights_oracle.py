"""Two independent statements of the per-detection weights of the keypoint estimators, built on the existing, unweighted
oracles (tests/tricov_oracle.py, tests/kpba_oracle.py), which stay as they are.  The definition: a detection of weight w enters every cost exactly
as if it and fx, fy, cx, cy of its camera had been multiplied by sqrt(w); w = 0 or NaN = the detection is unseen.

1. Virtual cameras (`virtual_rig`).  For weights drawn from a few levels, camera c becomes one virtual camera per positive level l: the same
   extrinsics and distortion, fx, fy, cx, cy and the detections times sqrt(l), NaN where the detection has another level.  The unweighted oracles
   then run on the virtual rig:
     refine_virtual        tricov_oracle.refine
     uncertainty_virtual   tricov_oracle.uncertainty; the camera covariance maps as T Sigma T^T, T = diag(sqrt(l) 1_4, 1_8) per virtual camera
     block_system_virtual  kpba_oracle.block_system; the physical system is the sum of the virtual system's blocks over the virtual cameras of each
                           physical camera (U_c, g_c, Y z, the tiles of Y Y^T), held bits and the step repeated per virtual camera; the point
                           blocks and the point steps are the same
     solve_virtual         kpba_oracle.solve's scipy call, the virtual cameras of one physical camera tied by construction of the parameter vector
2. Direct (`direct`).  sqrt(w) multiplied into f, A and B of tricov_oracle.linearise, the weights rho' then taken at the scaled residual.  Serves
   weights that are not on levels: `uncertainty_direct`, `refine_direct`, `robust_cost_direct`.

The bounds are the unweighted oracles' own, evaluated on the virtual or the direct problem: nothing here sets a tolerance."""
import contextlib

import numpy as np

import keypoint_scenes as ks
import kpba_oracle as ko
import tricov_oracle as tco
from test_triangulate_cpu import scene

LEVELS = (0.0, 0.25, 1.0, 4.0)


def draw_levels(C, P, seed, levels=LEVELS):
    """(C, P) weights drawn uniformly from the levels"""
    return np.random.default_rng(seed).choice(np.asarray(levels, dtype=np.float64), size=(C, P))


def positive(levels):
    return tuple(float(l) for l in levels if l > 0)


def masked(uvs, w):
    """the detections with NaN where the weight is not positive: what 'unseen' means"""
    uv = np.stack([np.asarray(u, dtype=np.float64) for u in uvs])
    return list(np.where((np.asarray(w) > 0)[:, :, None], uv, np.nan))


# ---------------------------------------------------------------- 1. virtual cameras
def virtual_rig(uvs, ext, intr, w, levels=LEVELS):
    """(v_uvs list, v_ext (V, 6), v_intr list, owner (V,), scale (V,)): V = C x the positive levels, virtual camera v = (camera owner[v], level
    scale[v]^2).  Every weight must be on a level (or NaN / 0)."""
    w = np.asarray(w, dtype=np.float64)
    pos = positive(levels)
    assert np.isin(w[w > 0], pos).all(), "weights off the levels: use the direct statement"
    v_uvs, v_ext, v_intr, owner, scale = [], [], [], [], []
    for c in range(len(ext)):
        K, d = intr[c]
        for l in pos:
            s = np.sqrt(l)
            Kv = np.array(K, dtype=np.float64)
            Kv[0, 0], Kv[1, 1], Kv[0, 2], Kv[1, 2] = s * K[0, 0], s * K[1, 1], s * K[0, 2], s * K[1, 2]
            v_uvs.append(np.where((w[c] == l)[:, None], s * np.asarray(uvs[c], dtype=np.float64), np.nan))
            v_ext.append(np.asarray(ext[c], dtype=np.float64))
            v_intr.append((Kv, np.array(d, dtype=np.float64)))
            owner.append(c)
            scale.append(s)
    return v_uvs, np.stack(v_ext), v_intr, np.asarray(owner), np.asarray(scale)


def virtual_covariance(S, owner, scale):
    """T Sigma T^T: the covariance of the virtual cameras' parameters theta_v = diag(s 1_4, 1_8) theta_owner(v)"""
    idx = (12 * owner[:, None] + np.arange(12)[None, :]).ravel()
    t = np.concatenate([np.r_[np.full(4, s), np.ones(8)] for s in scale])
    return np.asarray(S)[np.ix_(idx, idx)] * np.outer(t, t)


def refine_virtual(points, uvs, ext, intr, w, loss, f_scale, levels=LEVELS, iterations=30):
    vu, ve, vi, _, _ = virtual_rig(uvs, ext, intr, w, levels)
    return tco.refine(points, vu, ve, vi, loss, f_scale, iterations)


def uncertainty_virtual(points, uvs, ext, intr, w, camera_covariance=None, sigma=None, loss="linear", f_scale=1.0, levels=LEVELS):
    vu, ve, vi, owner, scale = virtual_rig(uvs, ext, intr, w, levels)
    S = None if camera_covariance is None else virtual_covariance(camera_covariance, owner, scale)
    return tco.uncertainty(points, vu, ve, vi, camera_covariance=S, sigma=sigma, loss=loss, f_scale=f_scale)


def fold(M, owner, C, axes):
    """sum the 6-blocks of the virtual cameras of each physical camera along the given axes"""
    M = np.asarray(M)
    for ax in axes:
        M = np.moveaxis(M, ax, 0)
        out = np.zeros((6 * C,) + M.shape[1:], M.dtype)
        for v, c in enumerate(owner):
            out[6 * c:6 * c + 6] += M[6 * v:6 * v + 6]
        M = np.moveaxis(out, 0, ax)
    return M


def block_system_virtual(uvs, ext, intr, X, held, w, loss="linear", f_scale=1.0, lam=0.0, step=None, levels=LEVELS):
    """kpba_oracle.block_system of the virtual rig, folded to the physical cameras: block_system's keys, U, gc, YY, Yz and free physical; cost,
    count, gmax, status, cond, fnorm, maxdet, views and the step are the virtual problem's as they are (they are the weighted problem's)"""
    vu, ve, vi, owner, _ = virtual_rig(uvs, ext, intr, w, levels)
    C = len(ext)
    held = np.asarray(held, dtype=bool).reshape(C, 6)
    vstep = None if step is None else (np.asarray(step[0])[owner], np.asarray(step[1]).reshape(C, 6)[owner])
    o = ko.block_system(vu, ve, vi, X, held[owner], loss=loss, f_scale=f_scale, lam=lam, step=vstep)
    o = dict(o)
    Uv = o["U"]
    U = np.zeros((6 * C, 6 * C))
    for v, c in enumerate(owner):   # (block diagonal in the virtual rig: the diagonal blocks alone)
        U[6 * c:6 * c + 6, 6 * c:6 * c + 6] += Uv[6 * v:6 * v + 6, 6 * v:6 * v + 6]
    o.update(U=U, gc=fold(o["gc"], owner, C, (0,)), Yz=fold(o["Yz"], owner, C, (0,)), YY=fold(o["YY"], owner, C, (0, 1)), free=~held)
    if step is not None:
        o["ext_trial"] = np.asarray(step[0], dtype=np.float64)
    return o


def cost_virtual(ext, X, uvs, intr, w, loss, f_scale=1.0, levels=LEVELS):
    """(kpba_oracle.cost_of on the virtual rig, its bound)"""
    vu, _, vi, owner, _ = virtual_rig(uvs, ext, intr, w, levels)
    return ko.cost_with_bound(np.asarray(ext)[owner], X, vu, vi, loss, f_scale)


def check_step_virtual(name, trial, step4, o, X, uvs, intr, w, loss, f_scale, levels=LEVELS):
    """kpba_oracle.check_step with the trial cost taken on the virtual rig"""
    vu, _, vi, owner, _ = virtual_rig(uvs, o["ext_trial"], intr, w, levels)
    ov = dict(o, ext_trial=np.asarray(o["ext_trial"])[owner])
    return ko.check_step(name, trial, step4, ov, X, vu, vi, loss, f_scale)


def solve_virtual(uvs, ext0, intr, pts0, w, loss="linear", f_scale=1.0, gauge_camera=0, scale_camera=None, baseline=None, max_nfev=200, levels=LEVELS):
    """kpba_oracle.solve's scipy call on the virtual rig; the parameter vector holds the free extrinsics of the physical cameras, every virtual
    camera reads its owner's: tied by construction.  The gauge (held_mask), the used points and the closing rescale are the physical rig's with
    the detections of weight 0 / NaN unseen.  Returns solve's dict (cost: the weighted one)."""
    from scipy.optimize import least_squares

    ext0, pts0 = np.asarray(ext0, dtype=np.float64), np.asarray(pts0, dtype=np.float64)
    seen_uvs = masked(uvs, w)
    held, scale_camera = ko.held_mask(ext0, seen_uvs, pts0, gauge_camera, scale_camera)
    used, _ = ko.used_points(seen_uvs, pts0)
    vu, _, vi, owner, _ = virtual_rig(uvs, ext0, intr, w, levels)
    vseen = ~np.isnan(np.stack(vu)).any(-1)
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
        return ko.residual_vector(e[owner], X, vu, vi, used, vseen)

    r = least_squares(fun, np.r_[ext0[free], pts0[used].ravel()], method="trf", tr_solver="exact", jac="3-point", x_scale="jac", ftol=1e-15, xtol=1e-15, gtol=1e-12, loss=loss, f_scale=f_scale,
                      max_nfev=max_nfev)
    e, X = unpack(r.x)
    e, X, s = ko.rescale(e, X, gauge_camera, scale_camera, ko.baseline_of(ext0, gauge_camera, scale_camera) if baseline is None else baseline)
    cost = ko.cost_of(e[owner], np.where(used[:, None], X, pts0), vu, vi, loss, f_scale)
    X[~used] = np.nan
    return dict(extrinsics=e, points=X, cost=cost, held=held, scale_camera=scale_camera, used=used, scale=s, scipy=r)


# ---------------------------------------------------------------- 2. direct
@contextlib.contextmanager
def direct(w):
    """inside: tricov_oracle.linearise is the weighted one -- sqrt(w) into f, A and B, rho' at the scaled residual, weight 0 / NaN unseen"""
    w = np.asarray(w, dtype=np.float64)
    sw = np.sqrt(np.where(w > 0, w, 0.0))
    plain = tco.linearise

    def linearise(points, uvs, ext, intr, loss, f_scale, second=False):
        seen, f, _, A, B = plain(points, masked(uvs, w), ext, intr, "linear", 1.0, second)
        f = f * sw[..., None]
        return seen, f, tco.rho1((f / f_scale) ** 2, loss) * seen[..., None], A * sw[..., None, None], B * sw[..., None, None]

    tco.linearise = linearise
    try:
        yield
    finally:
        tco.linearise = plain


def uncertainty_direct(points, uvs, ext, intr, w, **kw):
    with direct(w):
        return tco.uncertainty(points, uvs, ext, intr, **kw)


def robust_cost_direct(X, uvs, ext, intr, w, loss, f_scale=1.0):
    """(P,) keypoint_scenes.robust_cost of the weighted problem"""
    w = np.asarray(w, dtype=np.float64)
    f = np.stack([np.asarray(uvs[c]) - ks.project5(X, ext[c], *intr[c]) for c in range(len(ext))])
    seen = ~np.isnan(f).any(-1) & (w > 0)
    f = np.where(seen[..., None], f, 0.0) * np.sqrt(np.where(w > 0, w, 0.0))[..., None]
    return 0.5 * f_scale ** 2 * (ks.rho((f / f_scale) ** 2, loss) * seen[..., None]).sum(axis=(0, 2))


def refine_direct(points, uvs, ext, intr, w, loss, f_scale, iterations=30):
    """tricov_oracle.refine's iteration on the direct statement"""
    X = np.array(points, dtype=np.float64)
    cost = robust_cost_direct(X, uvs, ext, intr, w, loss, f_scale)
    with direct(w):
        for _ in range(iterations):
            seen, f, wt, A, _ = tco.linearise(X, uvs, ext, intr, loss, f_scale)
            H = np.einsum("cpki,cpk,cpkj->pij", A, wt, A)
            g = np.einsum("cpki,cpk,cpk->pi", A, wt, f)
            good = seen.sum(0) >= 2
            step = np.zeros_like(X)
            step[good] = np.linalg.solve(H[good] + 1e-12 * np.eye(3), g[good][..., None])[..., 0]
            trial = robust_cost_direct(X + step, uvs, ext, intr, w, loss, f_scale)
            better = good & (trial <= cost)
            X[better] += step[better]
            cost[better] = trial[better]
    return X


# ---------------------------------------------------------------- shared inputs
_cache = {}


def rig(C, P, seed, p_unseen, levels=LEVELS, noise=0.3, name=None):
    """(uvs list, ext, intr, truth, weights (C, P)) of a seeded scene() (or a scene of keypoint_scenes by name) with weights drawn from the levels;
    computed once and shared: read-only"""
    key = (C, P, seed, p_unseen, tuple(levels), noise, name)
    if key not in _cache:
        uvs, ext, intr, X = ks.make(name) if name else scene(C=C, P=P, seed=seed, noise=noise, p_unseen=p_unseen)
        uvs = [np.array(u) for u in uvs]
        _cache[key] = (uvs, np.asarray(ext), intr, X, draw_levels(len(ext), len(X), 9000 + seed, levels))
    return _cache[key]


# ---------------------------------------------------------------- the end-to-end golden (tests/golden/make_golden_kpba_weighted.py)
import os  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kpba_weighted.npz")
GOLDEN_CASES = {"six": ("six", "linear"), "outlier": ("outlier", "soft_l1")}   # name -> (scene of keypoint_scenes, loss), kpba_oracle.CASES' pairs
GOLDEN_WEIGHT_SEEDS = {"six": 9116, "outlier": 9131}
_golden = None


def golden_scene(name):
    """(uvs, ext, intr, truth, weights on LEVELS) of a golden case"""
    uvs, ext, intr, X = ks.make(GOLDEN_CASES[name][0])
    return uvs, ext, intr, X, draw_levels(len(ext), len(X), GOLDEN_WEIGHT_SEEDS[name])


def golden():
    global _golden
    if _golden is None:
        _golden = dict(np.load(GOLDEN, allow_pickle=False))
    return _golden


def pinned_cases():
    g = golden()
    return [n for n in GOLDEN_CASES if f"{n}/extrinsics" in g and bool(g[f"{n}/pinned"])]


def golden_case(name):
    """the inputs (scene, weights and first start) and the stored optimum of a pinned case, in kpba_oracle.case's keys"""
    g = golden()
    uvs, ext, intr, X, w = golden_scene(name)
    assert np.array_equal(w, g[f"{name}/weights"])
    return dict(uvs=uvs, intr=intr, loss=GOLDEN_CASES[name][1], weights=w, ext0=g[f"{name}/ext0"], pts0=g[f"{name}/pts0"]), \
        dict(extrinsics=g[f"{name}/extrinsics"], points=g[f"{name}/points"], cost=float(g[f"{name}/cost"]), held=g[f"{name}/held"], spread_ext=float(g[f"{name}/spread_ext"]),
             spread_pts=float(g[f"{name}/spread_pts"]), scale_camera=int(g[f"{name}/scale_camera"]))


# ---------------------------------------------------------------- the cases of the host tier (tests/test_hostcheck_weights.py) and the GPU tier (tests/test_gpu_weights*.py)
NO_ZERO = (0.25, 1.0, 4.0)
LOSS_NAMES = tco.LOSS_NAMES
# refinement.  name -> C, P, seed, p_unseen, levels (None: weights uniform in [0.1, 3], the direct statement), loss, f_scale.  2 cameras: no zero
# level and nothing unseen; 16 cameras: 48 virtual ones; 1, 255, 256, 257 points: around a workgroup of k_tri_refine
REFINE_CASES = {"c2_p257": (2, 257, 71, 0.0, NO_ZERO, "soft_l1", 1.0), "c6_p1": (6, 1, 72, 0.0, NO_ZERO, "linear", 1.0), "c6_p255": (6, 255, 73, 0.2, LEVELS, "linear", 1.0),
                "c6_p256": (6, 256, 74, 0.2, LEVELS, "soft_l1", 2.0), "c16_p33": (16, 33, 75, 0.3, LEVELS, "huber", 1.0), "direct_c6_p65": (6, 65, 76, 0.2, None, "soft_l1", 1.0)}
REFINE_CASES.update({f"c6_p257_{loss}": (6, 257, 77, 0.2, LEVELS, loss, 1.5) for loss in LOSS_NAMES})
# covariance.  17 and 33 points: one side of k_tricov_cal's 16-point groups each
TRICOV_CASES = {"c2_p17": (2, 17, 81, 0.0, NO_ZERO, "linear", 1.0), "c6_p33": (6, 33, 16, 0.2, LEVELS, "soft_l1", 1.0), "c6_p17": (6, 17, 82, 0.2, LEVELS, "cauchy", 2.0),
                "c16_p33": (16, 33, 83, 0.3, LEVELS, "linear", 1.0), "c3_p33": (3, 33, 84, 0.1, LEVELS, "huber", 1.0), "direct_c6_p33": (6, 33, 85, 0.2, None, "linear", 1.0)}
POOLED_CASES = ("c6_p33", "c16_p33", "c3_p33", "direct_c6_p33")   # 33 points with detection noise (tricov_oracle's rule for the pooled sigma2)


def draw_weights(C, P, seed, levels):
    if levels is None:
        return np.random.default_rng(9000 + seed).uniform(0.1, 3.0, (C, P))
    return draw_levels(C, P, 9000 + seed, levels)


def usable_fraction(uvs, w):
    seen = ~np.isnan(np.stack(uvs)).any(-1) & (np.asarray(w) > 0)
    return float((seen.sum(0) >= 2).mean())


def _scene(C, P, seed, p_unseen, levels):
    uvs, ext, intr, X = scene(C=C, P=P, seed=seed, noise=0.3, p_unseen=p_unseen)
    uvs = [np.array(u) for u in uvs]
    w = draw_weights(C, P, seed, levels)
    assert usable_fraction(uvs, w) >= 0.5, "fewer than half of the points are usable under the oracle"   # (a condition of every case)
    return uvs, np.asarray(ext), intr, X, w


def refine_case(name):
    """(inputs, oracle): inputs uvs, ext, intr, weights, start, loss, f_scale; oracle points (the minimiser from the start under the virtual or the
    direct statement; NaN where unusable), usable.  Computed once and shared: read-only."""
    key = ("refine", name)
    if key not in _cache:
        C, P, seed, p_unseen, levels, loss, f_scale = REFINE_CASES[name]
        uvs, ext, intr, X, w = _scene(C, P, seed, p_unseen, levels)
        start = X + np.random.default_rng(9500 + seed).normal(0, 0.3, X.shape)
        pts = refine_direct(start, uvs, ext, intr, w, loss, f_scale) if levels is None else refine_virtual(start, uvs, ext, intr, w, loss, f_scale, levels or LEVELS)
        usable = (~np.isnan(np.stack(uvs)).any(-1) & (w > 0)).sum(0) >= 2
        pts[~usable] = np.nan
        _cache[key] = (dict(uvs=uvs, ext=ext, intr=intr, weights=w, start=start, loss=loss, f_scale=f_scale, levels=levels), dict(points=pts, usable=usable))
    return _cache[key]


def tricov_case(name):
    """(inputs, oracle) in tricov_oracle.case's keys plus weights: the oracle with the random camera covariance at sigma = SIGMA, and pooled_sigma2"""
    key = ("tricov", name)
    if key not in _cache:
        C, P, seed, p_unseen, levels, loss, f_scale = TRICOV_CASES[name]
        uvs, ext, intr, X, w = _scene(C, P, seed, p_unseen, levels)
        S = tco.random_covariance(C, seed=seed)
        if levels is None:
            pts = refine_direct(X, uvs, ext, intr, w, loss, f_scale)
            unc = lambda **kw: uncertainty_direct(pts, uvs, ext, intr, w, loss=loss, f_scale=f_scale, **kw)   # noqa: E731
        else:
            pts = refine_virtual(X, uvs, ext, intr, w, loss, f_scale, levels)
            unc = lambda **kw: uncertainty_virtual(pts, uvs, ext, intr, w, loss=loss, f_scale=f_scale, levels=levels, **kw)   # noqa: E731
        o = unc(camera_covariance=S, sigma=tco.SIGMA)
        o["pooled_sigma2"] = unc()["sigma2"]
        assert (o["status"] == 1).mean() >= 0.5, "fewer than half of the points are usable under the oracle"
        _cache[key] = (dict(points=pts, uvs=uvs, ext=ext, intr=intr, weights=w, loss=loss, f_scale=f_scale, camera_covariance=S), o)
    return _cache[key]


# one evaluation of the extrinsics refinement.  name -> dict(C, P, seed, p_unseen | scene="outlier"; levels, loss, f_scale, lam, edit)
SYSTEM_CASES = {"c2_p70": dict(C=2, P=70, seed=91, p_unseen=0.0, levels=NO_ZERO), "c3_p257": dict(C=3, P=257, seed=92, p_unseen=0.1), "c11_p70": dict(C=11, P=70, seed=93, p_unseen=0.3),
                "c24_p70": dict(C=24, P=70, seed=94, p_unseen=0.3), "held": dict(C=6, P=70, seed=95, p_unseen=0.2, edit="held", loss="soft_l1", f_scale=1.5, lam=1e-2)}
SYSTEM_CASES.update({f"g6_p{n}": dict(C=6, P=n, seed=96, p_unseen=0.2) for n in (63, 64, 65)})
SYSTEM_CASES.update({f"outlier_{loss}_{lam}": dict(scene="outlier", loss=loss, f_scale=1.5, lam=lam) for loss in ("soft_l1", "cauchy") for lam in (0.0, 1e-4, 1.0)})


def system_case(name):
    """(inputs, oracle) as kpba_oracle.system_case builds them, with weights: inputs uvs, weights, ext0, intr, pts0, held (C, 6) bool, loss, f_scale,
    lam, step = (ext_trial, dtheta); oracle: block_system_virtual's"""
    key = ("system", name)
    if key not in _cache:
        sp = SYSTEM_CASES[name]
        levels = sp.get("levels", LEVELS)
        if sp.get("scene"):
            uvs, ext, intr, X = ks.make(sp["scene"])
            uvs, seed = [np.array(u) for u in uvs], 31
            w = draw_levels(len(ext), len(X), 9031, levels)
            assert usable_fraction(uvs, w) >= 0.5
        else:
            uvs, ext, intr, X, w = _scene(sp["C"], sp["P"], sp["seed"], sp["p_unseen"], levels)
            seed = sp["seed"]
        ext0, pts0 = ko.perturbed_start(ext, X, 0, 5000 + seed)
        edit = sp.get("edit")
        if edit == "held":
            w = w.copy()
            w[3] = 0.0   # a camera without a detection of positive weight
        held, _ = ko.held_mask(ext0, masked(uvs, w), pts0, scale_camera=1 if edit == "held" else None)
        if edit == "held":
            held[2] = [False, True, False, True, False, True]   # 0b101010
            assert held[0].all() and held[3].all() and held[1].sum() == 1
        rng = np.random.default_rng(7000 + seed)
        dtheta = np.concatenate([rng.normal(0, 1e-3, (len(ext0), 3)), rng.normal(0, 0.5, (len(ext0), 3))], axis=1) * ~held
        i = dict(uvs=uvs, weights=w, ext0=ext0, intr=intr, pts0=pts0, held=held, loss=sp.get("loss", "linear"), f_scale=sp.get("f_scale", 1.0), lam=sp.get("lam", 1e-4), step=(ext0 + dtheta, dtheta),
                 levels=levels)
        o = block_system_virtual(uvs, ext0, intr, pts0, held, w, loss=i["loss"], f_scale=i["f_scale"], lam=i["lam"], step=i["step"], levels=levels)
        assert o["used"].mean() >= 0.5, "fewer than half of the points are usable under the oracle"
        _cache[key] = (i, o)
    return _cache[key]


def check_system(name, i, o, got):
    """kpba_oracle.check_block and check_step of one weighted evaluation against the folded virtual system"""
    r = ko.check_block(name, got, o)
    r.update(check_step_virtual(name, got["trial_points"], got["step4"], o, i["pts0"], i["uvs"], i["intr"], i["weights"], i["loss"], i["f_scale"], i["levels"]))
    return r
