"""The reference of skeleton.refine_skeleton and skeleton.estimate_bone_lengths in numpy / scipy: per frame the data
term's H, g and cost from the analytic derivatives of tricov_oracle.linearise under the weighted statement of weights_oracle.direct (as
trajectory_refine_oracle does), the dense (3 n)^2 Gauss-Newton matrix of the frame's n active keypoints, a dense Levenberg-Marquardt loop with
the library's accept and stop rule, a scipy least_squares cross-check of the minimiser, the inverse of the dense matrix for the covariance, the
forest plan, the scenes and cases of the tests and the rules both tiers (host-check and GPU) are held to.

Per frame, over the positions x_k of its active keypoints:
    minimise 0.5 sum_k sum_{c sees k} f^2 [rho(ru^2 / f^2) + rho(rv^2 / f^2)] + 0.5 sum_{active bones} ((|x_k - x_p(k)| - L_k) / s_k)^2,
    (ru, rv) = sqrt(w) (detection - project5(x_k)) / pixel_std_c
A detection is seen when neither coordinate is NaN and its weight is positive and not NaN.  A keypoint is usable (2) with two views or more and
a finite start, single (1) with exactly one view and a finite start, otherwise out of the frame (-1) with its bones; a connected piece of what
is left without a usable keypoint is not fitted (-2).  H_k = sum A^T diag(cw) A with the curvature weight cw = max(rho' + 2 rho'' z, eps,
0.1 rho'); a bone with direction u adds u u^T / s^2 to both diagonal blocks and - u u^T / s^2 off the diagonal.

The loop (refine_point's): damping lam diag(M) from 1e-4; a trial x + d is accepted when the frame's objective is not larger (lam / 10, floor
1e-12), otherwise lam x 10; the frame stops when max|d| < xtol max|x| (accepted or not), when lam >= 1e12, or after max_iterations trials."""
import functools

import numpy as np

import keypoint_scenes as ks
import smoothing_cov_oracle as sco
import smoothing_oracle as so
import tricov_oracle as tco
import weights_oracle as wo
from test_triangulate_cpu import scene as rig_scene
from trajectory_refine_oracle import effective_weights

EPS = so.EPS
MACH_EPS = 2.220446049250313e-16
CURV_FLOOR = 0.1       # MCBA_CURV_FLOOR_TRIGGS
USABLE, SINGLE, OUT, NO_ANCHOR = 2, 1, -1, -2
CONVERGED, ITERATION_LIMIT, NOTHING = 1, 0, -1
LAM_START, LAM_FLOOR, LAM_STOP = 1e-4, 1e-12, 1e12
LOSSES = {"linear": 0, "soft_l1": 1, "huber": 2, "cauchy": 3, "arctan": 4}


# ---------------------------------------------------------------- the forest
def parents_of(bones, K):
    """(parent (K,), child (E,)): the walk from the lowest-numbered keypoint of each piece, neighbours in index order; ValueError for a cycle"""
    bones = np.asarray(bones, dtype=np.int64).reshape(-1, 2)
    parent, child, seen, used = np.full(K, -1), np.full(len(bones), -1), np.zeros(K, bool), np.zeros(len(bones), bool)
    for root in range(K):
        if seen[root]:
            continue
        seen[root] = True
        queue = [root]
        while queue:
            i = queue.pop(0)
            nb = sorted([(int(b[1] if b[0] == i else b[0]), e) for e, b in enumerate(bones) if i in b and not used[e]])
            for j, e in nb:
                used[e] = True
                if seen[j]:
                    raise ValueError("cycle")
                seen[j], parent[j], child[e] = True, i, j
                queue.append(j)
    return parent, child


def plan(parent):
    """dict(level (K,), order (K,), children (list of lists), levels): depth of every keypoint, the order by depth then index, child lists in index order"""
    K = len(parent)
    level = np.zeros(K, int)
    for k in range(K):
        j, d = k, 0
        while parent[j] >= 0:
            j, d = parent[j], d + 1
        level[k] = d
    order = sorted(range(K), key=lambda k: (level[k], k))
    return dict(level=level, order=np.array(order), children=[[k for k in range(K) if parent[k] == p] for p in range(K)], levels=int(level.max()) + 1)


def chain(K):
    return np.array([[k, k + 1] for k in range(K - 1)]).reshape(-1, 2)


def star(K):
    return np.array([[0, k] for k in range(1, K)]).reshape(-1, 2)


def random_tree(K, seed):
    rng = np.random.default_rng(seed)
    lab = rng.permutation(K)
    return np.array([[lab[k], lab[rng.integers(0, k)]] for k in range(1, K)]).reshape(-1, 2)


# ---------------------------------------------------------------- statuses
def classes(case):
    """(T, K) keypoint statuses and (T, K) views of a case from its detections, weights, start and bones"""
    uv, w = np.asarray(case["uvs"]), case["weff"]
    views = (~np.isnan(uv).any(-1) & (w > 0)).sum(0)
    fin = np.isfinite(case["start"]).all(-1)
    cls = np.where(~fin | (views == 0), OUT, np.where(views >= 2, USABLE, SINGLE))
    T, K = cls.shape
    for t in range(T):
        comp = np.arange(K)
        for a, b in case["bones"]:
            if cls[t, a] > 0 and cls[t, b] > 0:
                comp[comp == comp[b]] = comp[a]
        for c in np.unique(comp):
            m = (comp == c) & (cls[t] > 0)
            if m.any() and not (cls[t][m] == USABLE).any():
                cls[t][m] = NO_ANCHOR
    return cls.astype(np.int32), views


# ---------------------------------------------------------------- one frame
def rho(z, loss):
    return ks.rho(z, loss)


def curvature(z, rho1, loss):
    """max(rho' + 2 rho'' z, eps, CURV_FLOOR rho') per scalar"""
    if loss == "linear":
        return np.ones_like(z)
    if loss == "soft_l1":
        w2 = (1.0 + z) ** -1.5
    elif loss == "huber":
        w2 = np.where(z <= 1.0, 1.0, 0.0)
    elif loss == "cauchy":
        w2 = (1.0 - z) / (1.0 + z) ** 2
    else:
        w2 = 1.0 / (1.0 + z * z) - 4.0 * z * z / (1.0 + z * z) ** 2
    return np.maximum(np.maximum(w2, MACH_EPS), CURV_FLOOR * rho1)


def frame_data(x, t, case):
    """x (K, 3) -> dict(H (K, 3, 3), g, gabs (K, 3), cost (K,)) of the data term of frame t"""
    C = len(case["ext"])
    uv = [np.asarray(case["uvs"][c][t], dtype=np.float64) for c in range(C)]
    loss, fs = case["loss"], case["f_scale"]
    with wo.direct(case["weff"][:, t]), np.errstate(all="ignore"):
        seen, f, wt, A, _ = tco.linearise(np.asarray(x, dtype=np.float64), uv, case["ext"], case["intr"], loss, fs)
    z = (f / fs) ** 2
    cw = curvature(z, tco.rho1(z, loss), loss) * seen[..., None]
    terms = A * (wt * f)[..., None]
    # the gradient's scale: its terms in absolute value, the residual taken as the difference it is -- sw (|detection| + |projection|)
    sw = np.sqrt(np.where(case["weff"][:, t] > 0, case["weff"][:, t], 0.0))
    operands = np.where(seen[..., None], 2.0 * np.abs(np.nan_to_num(np.stack(uv))) * sw[..., None] + np.abs(f), 0.0)
    return dict(H=np.einsum("cpki,cpk,cpkj->pij", A, cw, A), g=-terms.sum(axis=(0, 2)), gabs=(np.abs(A) * (wt * operands)[..., None]).sum(axis=(0, 2)),
                cost=0.5 * fs ** 2 * (rho(z, loss) * seen[..., None]).sum(axis=(0, 2)))


def bone_terms(x, act, case):
    """the active bones of a frame at x: list of (child k, parent p, u (3,), r, 1 / s)"""
    out = []
    for k, p in enumerate(case["parent"]):
        if p >= 0 and act[k] and act[p]:
            e = x[k] - x[p]
            n = np.linalg.norm(e)
            out.append((k, int(p), e / n, (n - case["L"][k]) / case["s"][k], 1.0 / case["s"][k]))
    return out


def objective(x, t, act, case):
    d = frame_data(x, t, case)
    return float(d["cost"][act].sum()) + 0.5 * sum(b[3] ** 2 for b in bone_terms(x, act, case))


def dense_matrix(info, direction, act, case):
    """the Gauss-Newton matrix over the active keypoints idx from its diagonal blocks info (K, 3, 3) (bones included) and the bones' directions
    (K, 3) by child: (M (3 n, 3 n), idx)"""
    idx = np.flatnonzero(act)
    pos = {int(k): i for i, k in enumerate(idx)}
    M = np.zeros((3 * len(idx), 3 * len(idx)))
    for k in idx:
        i = pos[int(k)]
        M[3 * i:3 * i + 3, 3 * i:3 * i + 3] = info[k]
        p = case["parent"][k]
        if p >= 0 and act[p]:
            j, B = pos[int(p)], np.outer(direction[k], direction[k]) / case["s"][k] ** 2
            M[3 * i:3 * i + 3, 3 * j:3 * j + 3] = -B
            M[3 * j:3 * j + 3, 3 * i:3 * i + 3] = -B
    return M, idx


def damped_solve(M, G, lam):
    """(d, cond of the Jacobi-scaled damped matrix); d NaN where the solve fails"""
    A = M + lam * np.diag(np.diagonal(M))
    s = np.sqrt(np.diagonal(A))
    with np.errstate(all="ignore"):
        Ah = A / np.outer(s, s)
        try:
            d = np.linalg.solve(Ah, -G / s) / s
            cnd = float(np.linalg.cond(Ah))
        except np.linalg.LinAlgError:
            d, cnd = np.full(len(G), np.nan), np.inf
    return d, cnd


def evaluate(x, t, act, case, lam):
    """one frame at x (K, 3): dict(info (K, 3, 3), G, S, u (K, 3), r (K,), data, bone, M, idx, d (K, 3), cond, trial, dmax, xmax)"""
    K = len(x)
    dt = frame_data(x, t, case)
    info, G, S = dt["H"].copy(), dt["g"].copy(), dt["gabs"].copy()
    u, r = np.full((K, 3), np.nan), np.full(K, np.nan)
    bone = 0.0
    for k, p, uk, rk, isk in bone_terms(x, act, case):
        u[k], r[k] = uk, rk
        B = np.outer(uk, uk) * isk * isk
        info[k] += B
        info[p] += B
        G[k] += uk * rk * isk
        G[p] -= uk * rk * isk
        S[k] += np.abs(uk * rk * isk)
        S[p] += np.abs(uk * rk * isk)
        bone += 0.5 * rk * rk
    info[~act], G[~act] = np.nan, np.nan
    M, idx = dense_matrix(info, u, act, case)
    dv, cnd = damped_solve(M, G[idx].ravel(), lam)
    d = np.full((K, 3), np.nan)
    d[idx] = dv.reshape(-1, 3)
    xt = np.where(act[:, None], x + d, x)
    with np.errstate(all="ignore"):
        trial = objective(xt, t, act, case) if np.isfinite(dv).all() else np.nan
    return dict(info=info, G=G, S=S, u=u, r=r, data=float(dt["cost"][act].sum()), bone=bone, M=M, idx=idx, d=d, cond=cnd, trial=trial, dmax=float(np.abs(d[idx]).max()),
                xmax=float(np.abs(x[idx]).max()), xt=xt)


def lm(case, t, cls_t, max_iterations=50, xtol=1e-8):
    """the loop of one frame from case["start"][t]: dict(points (K, 3), status, n_iterations, cost, cost_start, history [(cost, dmax, threshold, accepted, margin)])"""
    K = case["start"].shape[1]
    act = cls_t > 0
    out = dict(points=np.full((K, 3), np.nan), status=NOTHING, n_iterations=0, cost=np.nan, cost_start=np.nan, history=[], max_iterations=max_iterations)
    if not act.any():
        return out
    x = np.array(case["start"][t], dtype=np.float64)
    cost = objective(x, t, act, case)
    out["cost_start"] = cost
    lam, status, it = LAM_START, ITERATION_LIMIT, 0
    while it < max_iterations:
        it += 1
        ev = evaluate(x, t, act, case, lam)
        small = ev["dmax"] < xtol * ev["xmax"]
        accept = bool(ev["trial"] <= cost)
        out["history"].append((ev["trial"] if accept else cost, ev["dmax"], xtol * ev["xmax"], accept, abs(ev["trial"] - cost) / max(cost, 1e-300)))
        if accept:
            x, cost, lam = ev["xt"], ev["trial"], max(0.1 * lam, LAM_FLOOR)
            if small:
                status = CONVERGED
                break
        else:
            lam *= 10.0
            if small or not lam < LAM_STOP:
                status = CONVERGED
                break
    x[~act] = np.nan
    out.update(points=x, status=status, n_iterations=it, cost=cost)
    return out


def decided(o):
    """the reference's count does not hinge on rounding: every step after which it went on is more than twice its threshold xtol max|x| and its
    accept-or-reject comparison is not at the objective's resolution (a relative gap above 1e-11), and it stopped at the iteration limit, at the
    damping limit or where the step is below half the threshold -- there the frame stops whether the step is accepted or not"""
    h = o["history"]
    if not h:
        return True
    go_on = all(dm > 2 * thr and margin > 1e-11 for _, dm, thr, _, margin in h[:-1])
    _, dm, thr, _, margin = h[-1]
    last = dm < thr / 2 or ((len(h) == o["max_iterations"] or dm > 2 * thr) and margin > 1e-11)
    return bool(go_on and last)


def scipy_minimiser(case, t, cls_t, x0):
    """the minimiser of a frame's objective by scipy least_squares from x0 (K, 3), linear loss only: (points (K, 3), cost)"""
    from scipy.optimize import least_squares
    assert case["loss"] == "linear"
    act = cls_t > 0
    idx = np.flatnonzero(act)
    C = len(case["ext"])
    sw = np.sqrt(np.where(case["weff"][:, t] > 0, case["weff"][:, t], 0.0))
    uv = np.stack([np.asarray(case["uvs"][c][t]) for c in range(C)])
    seen = ~np.isnan(uv).any(-1) & (sw > 0) & act[None]

    def residuals(v):
        x = np.array(case["start"][t])
        x[idx] = v.reshape(-1, 3)
        proj = np.stack([ks.project5(np.where(np.isfinite(x), x, 0.0), case["ext"][c], *case["intr"][c]) for c in range(C)])
        f = (np.where(seen[..., None], uv - proj, 0.0) * sw[..., None])[seen]
        return np.r_[f.ravel(), [b[3] for b in bone_terms(x, act, case)]]

    r = least_squares(residuals, x0[idx].ravel(), method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=2000)
    x = np.full_like(x0, np.nan)
    x[idx] = r.x.reshape(-1, 3)
    return x, float(r.cost)


def covariance_reference(M):
    """diag blocks (n, 3, 3) of the inverse of a dense Gauss-Newton matrix with the quantities of the section 8f-20 bar: s, cond, zmax"""
    n = len(M) // 3
    s = np.sqrt(np.diagonal(M))
    Ah = M / np.outer(s, s)
    Zh = np.linalg.inv(Ah)
    Zh = (Zh + Zh.T) / 2
    Z = (Zh / np.outer(s, s)).reshape(n, 3, n, 3)
    i = np.arange(n)
    return dict(diag=Z[i, :, i, :].copy(), lag=None, s=s, cond=float(np.linalg.cond(Ah)), zmax=float(np.abs(Zh).max()))


# ---------------------------------------------------------------- estimate_bone_lengths
def bone_lengths(points, bones):
    """(length (E,), std (E,), count (E,)): the exact nan-medians, distances as sqrt((dx dx + dy dy) + dz dz) in float64"""
    pts = np.asarray(points, dtype=np.float64)
    length, std, count = [], [], []
    for a, b in bones:
        e = pts[:, a] - pts[:, b]
        d = np.sqrt(e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1] + e[:, 2] * e[:, 2])
        n = int((~np.isnan(d)).sum())
        with np.errstate(all="ignore"):
            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                med = np.nanmedian(d) if n else np.nan
                mad = np.nanmedian(np.abs(d - med)) if n else np.nan
        length.append(med); std.append(1.4826 * mad); count.append(n)
    return np.array(length), np.array(std), np.array(count, dtype=np.int32)


# ---------------------------------------------------------------- scenes
def make_scene(C, T, bones, K, seed, noise=0.5, p_drop=0.2, bone_range=(8.0, 30.0), bone_jitter=0.5, spread=25.0, max_single=1, min_cos=0.5):
    """dict(uvs (C, T, K, 2), ext, intr, truth (T, K, 3), bones, bone_length): a rig of test_triangulate_cpu.scene; per frame the skeleton is laid out
    afresh through its cloud -- every bone its length (drawn once from bone_range) with N(0, bone_jitter^2) mm added, in a random direction --,
    detections with noise, a share p_drop dropped.  max_single: at most that many keypoints of a frame are left with exactly one view (the others get
    their second view back; None: no limit) -- frames with several single-view keypoints converge linearly, with a ratio up to 0.5, and belong to
    the one-evaluation tests, where convergence does not enter.  min_cos (with max_single): a keypoint stays single only where one of its bones
    makes an angle below acos(min_cos) with its ray -- where every bone is near perpendicular to the ray, the ray is near tangent to the spheres
    about the neighbours, the two solutions merge, the Gauss-Newton matrix is near singular along the ray and the loop crawls"""
    _, ext, intr, X = rig_scene(C=C, P=8, seed=seed)
    rng = np.random.default_rng(seed + 2000)
    parent, child = parents_of(bones, K)
    Lb = rng.uniform(*bone_range, len(child))
    L = np.zeros(K)
    L[child] = Lb
    truth = np.zeros((T, K, 3))
    for k in plan(parent)["order"]:
        if parent[k] < 0:
            truth[:, k] = X.mean(0) + rng.normal(0, spread, (T, 3))
        else:
            v = rng.normal(size=(T, 3))
            truth[:, k] = truth[:, parent[k]] + v / np.linalg.norm(v, axis=1, keepdims=True) * (L[k] + rng.normal(0, bone_jitter, T))[:, None]
    uv = np.stack([ks.project5(truth, ext[c], *intr[c]) for c in range(C)])
    uv += rng.normal(0, noise, uv.shape)
    drop = rng.uniform(size=(C, T, K)) < p_drop
    if max_single is not None and C >= 2:
        for t in range(T):
            kept = 0
            for k in np.flatnonzero((~drop[:, t]).sum(0) == 1):
                c = int(np.flatnonzero(~drop[:, t, k])[0])
                ray = truth[t, k] + ks.rodrigues(ext[c][:3]).T @ ext[c][3:]      # from the camera's centre - R^T t
                nb = [truth[t, k] - truth[t, b if a == k else a] for a, b in np.asarray(bones).reshape(-1, 2) if k in (a, b)]
                cos = max([abs(ray @ e) / np.linalg.norm(ray) / np.linalg.norm(e) for e in nb], default=0.0)
                if kept < max_single and cos >= min_cos:
                    kept += 1
                else:
                    drop[np.flatnonzero(drop[:, t, k])[0], t, k] = False
    uv[drop] = np.nan
    return dict(uvs=uv, ext=ext, intr=intr, truth=truth, bones=np.asarray(bones).reshape(-1, 2), bone_length=Lb)


def make_case(s, bone_std=0.5, pixel_std=0.5, loss="linear", f_scale=3.0, weights=None, start_noise=0.03, seed=0):
    """a scene with its parameters and a start (the truth with start_noise of white noise)"""
    C, T, K = s["uvs"].shape[:3]
    parent, child = parents_of(s["bones"], K)
    start = s["truth"] + np.random.default_rng(7000 + seed).normal(0, start_noise, s["truth"].shape)
    sb = np.broadcast_to(np.asarray(bone_std, dtype=np.float64), (len(child),))
    L, sk = np.ones(K), np.ones(K)
    L[child], sk[child] = s["bone_length"], sb
    return dict(s, bone_std=bone_std, pixel_std=pixel_std, loss=loss, f_scale=f_scale, weights=weights, start=start, weff=effective_weights(weights, pixel_std, C, T, K), parent=parent,
                child=child, L=L, s=sk)


def see(case, t, k, cams):
    """keypoint k of frame t is seen by exactly the cameras `cams`, noise-free where it was dropped"""
    for c in range(len(case["ext"])):
        if c in cams:
            if np.isnan(case["uvs"][c, t, k]).any():
                case["uvs"][c, t, k] = ks.project5(case["truth"][t, k], case["ext"][c], *case["intr"][c])
        else:
            case["uvs"][c, t, k] = np.nan


def best_camera(case, t, k):
    """the camera whose ray to keypoint k of frame t is closest to the direction of one of its bones (make_scene: min_cos)"""
    best, arg = -1.0, 0
    for c in range(len(case["ext"])):
        ray = case["truth"][t, k] + ks.rodrigues(case["ext"][c][:3]).T @ case["ext"][c][3:]
        for a, b in case["bones"]:
            if k in (a, b):
                e = case["truth"][t, a] - case["truth"][t, b]
                cos = abs(ray @ e) / np.linalg.norm(ray) / np.linalg.norm(e)
                if cos > best:
                    best, arg = cos, c
    return arg


def special_frames():
    """K = 7: 0 - 1 - 2 - 3 a chain with 4 and 5 on 1 and 6 on 3; 4 cameras, 6 frames, each with what its comment says"""
    bones = np.array([[0, 1], [1, 2], [2, 3], [1, 4], [1, 5], [3, 6]])
    c = make_case(make_scene(4, 6, bones, 7, seed=41, p_drop=0.0, **QUIET), loss="linear", seed=41)
    see(c, 0, 1, ())                      # frame 0: keypoint 1 unseen -- the tree splits into {0}, {2, 3, 6}, {4}, {5}
    see(c, 1, 2, ()); see(c, 1, 3, (0,)); see(c, 1, 6, (1,))   # frame 1: {3, 6} a piece of singles only (-2) behind the unseen 2
    see(c, 2, 6, (best_camera(c, 2, 6),)); see(c, 2, 4, (best_camera(c, 2, 4),))   # frame 2: single-view leaves
    see(c, 3, 1, (best_camera(c, 3, 1),))   # frame 3: a single-view inner node with usable children
    see(c, 4, 2, (0,)); see(c, 4, 3, (1,)); see(c, 4, 6, (2,))  # frame 4: three singles in a row behind usable keypoints (one evaluation only)
    c["start"][5, 5, 1] = np.nan          # frame 5: a NaN in the start of keypoint 5
    c["weff"] = effective_weights(c["weights"], c["pixel_std"], 4, 6, 7)
    return c


# The loop scenes (cases()): 0.05 px of detection noise, 0.05 mm of bone-length jitter and a start 0.03 mm from the truth.  With small residuals
# Gauss-Newton converges fast (steps of about 1e-1, 2e-4, 6e-7 mm against a threshold xtol max|x| of 7e-6 mm), so the oracle's stopping step seldom
# falls within a factor 2 of the threshold and decided() leaves out 13 of its 240 frames; at 0.5 px and a start 0.3 mm off, where the third step
# lands on the threshold, it left out 95.  The scenes with 0.5 px ("cauchy", "singles") are held to the one-evaluation rules
QUIET = dict(noise=0.05, bone_jitter=0.05)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> case: the smallest shapes at which the kernel can go wrong (computed once and shared: read-only).  K1: no bones; K2; K3 as a chain
    and as a star; K5: G = 51 frames per workgroup and one idle lane, T = 3 G + 1 = 154; K33: G = 7, 25 idle lanes; K64 as a chain (63 levels) and
    as a star, T = 3 G + 1 = 13; two pieces; C1: nothing usable; C2; C6 with weights on levels, per-camera pixel_std and huber; cauchy; singles:
    half the detections dropped, frames with several single-view keypoints; special: the frames of special_frames()"""
    out = {}
    out["K1"] = make_case(make_scene(3, 5, chain(1), 1, seed=51, **QUIET), seed=1)
    out["K2"] = make_case(make_scene(3, 5, chain(2), 2, seed=52, **QUIET), seed=2)
    out["K3_chain"] = make_case(make_scene(3, 5, chain(3), 3, seed=53, **QUIET), seed=3)
    out["K3_star"] = make_case(make_scene(3, 5, star(3), 3, seed=54, **QUIET), loss="soft_l1", f_scale=2.0, seed=4)
    out["K5"] = make_case(make_scene(4, 154, random_tree(5, 55), 5, seed=55, p_drop=0.25, **QUIET), seed=5)
    out["K33"] = make_case(make_scene(4, 8, random_tree(33, 56), 33, seed=56, p_drop=0.25, **QUIET), seed=6)
    out["K64_chain"] = make_case(make_scene(4, 13, chain(64), 64, seed=57, p_drop=0.25, **QUIET), seed=7)
    out["K64_star"] = make_case(make_scene(4, 13, star(64), 64, seed=58, p_drop=0.25, bone_range=(20.0, 40.0), **QUIET), seed=8)
    two = np.array([[0, 2], [2, 5], [1, 3], [3, 4], [3, 6]])
    out["two_pieces"] = make_case(make_scene(4, 9, two, 7, seed=59, p_drop=0.3, **QUIET), bone_std=np.array([0.5, 0.3, 1.0, 0.5, 0.5]), seed=9)
    out["C1"] = make_case(make_scene(1, 4, chain(3), 3, seed=60, p_drop=0.0, **QUIET), seed=10)
    out["C2"] = make_case(make_scene(2, 9, random_tree(6, 61), 6, seed=61, p_drop=0.2, **QUIET), seed=11)
    s = make_scene(6, 9, random_tree(12, 62), 12, seed=62, p_drop=0.35, **QUIET)
    w = wo.draw_levels(6, 9 * 12, 9062, (0.25, 1.0, 1.0, 4.0)).reshape(6, 9, 12)
    out["C6"] = make_case(s, pixel_std=np.array([0.5, 0.4, 0.6, 0.5, 0.45, 0.55]), loss="huber", weights=w, seed=12)
    out["cauchy"] = make_case(make_scene(4, 6, random_tree(8, 63), 8, seed=63, p_drop=0.2), loss="cauchy", f_scale=4.0, seed=13)
    out["singles"] = make_case(make_scene(4, 6, random_tree(8, 64), 8, seed=64, p_drop=0.5, max_single=None), seed=14)   # (one evaluation only)
    out["special"] = special_frames()
    return out


LOOP_CASES = ("K1", "K2", "K3_chain", "K3_star", "K5", "K33", "K64_chain", "K64_star", "two_pieces", "C1", "C2", "C6", "special")
SYSTEM_CASES = ("K1", "K2", "K3_chain", "K3_star", "K33", "K64_chain", "K64_star", "two_pieces", "C1", "C2", "C6", "cauchy", "singles", "special")
SPECIAL_LOOP_FRAMES = (0, 1, 2, 3, 5)   # (frame 4, three single-view keypoints in a row, converges slowly: covered by the one-evaluation tests)
SYSTEM_LAM = 1e-4


def loop_frames(name):
    T = cases()[name]["start"].shape[0]
    return SPECIAL_LOOP_FRAMES if name == "special" else tuple(range(T))


@functools.lru_cache(maxsize=None)
def statuses(name):
    return classes(cases()[name])[0]


@functools.lru_cache(maxsize=None)
def reference(name, max_iterations=50, xtol=1e-8):
    """per frame the oracle's loop of a case (None for the frames the loop tests leave out), computed once"""
    case, cls = cases()[name], statuses(name)
    return [lm(case, t, cls[t], max_iterations, xtol) if t in loop_frames(name) else None for t in range(len(cls))]


@functools.lru_cache(maxsize=None)
def system_reference(name, lam=SYSTEM_LAM):
    """per frame with something to fit the oracle's evaluation at the start of a case (None for the others), computed once"""
    case, cls = cases()[name], statuses(name)
    return [evaluate(np.array(case["start"][t]), t, cls[t] > 0, case, lam) if (cls[t] > 0).any() else None for t in range(len(cls))]


def by_child(plane, case):
    """(T, E, ...) per bone -> (T, K, ...) by the bone's child end, NaN for roots"""
    T, K = case["start"].shape[:2]
    out = np.full((T, K) + plane.shape[2:], np.nan)
    out[:, case["child"]] = plane
    return out


# ---------------------------------------------------------------- the rules of the host-check and GPU tiers
def check_system(name, got, lam=SYSTEM_LAM):
    """got: dict(information (T, K, 3, 3), gradient, step (T, K, 3), direction (T, K, 3) by child, data_cost, bone_cost, trial_cost (T), keypoint_status,
    frame_status).  The rules of trajectory_refine_oracle.check_system, per frame.  The gradient's scale is the largest S of the frame, S = per entry the
    sum of the absolute values of its terms with every residual taken as the difference it is, sw (|detection| + |projection|): the rounding of a
    projection, eps x 1000 px, enters every term of the data gradient whatever the residual's size, so a sum over |residual| alone understates what
    float64 can deliver where the residuals are small (the loop scenes: 0.05 px); the entries of a frame share their unit and their cameras"""
    case, cls = cases()[name], statuses(name)
    assert np.array_equal(got["keypoint_status"], cls), (name, got["keypoint_status"], cls)
    for t, ev in enumerate(system_reference(name, lam)):
        act = cls[t] > 0
        frame = [got[f][t] for f in ("data_cost", "bone_cost", "trial_cost")]
        assert np.isnan(got["information"][t][~act]).all() and np.isnan(got["gradient"][t][~act]).all() and np.isnan(got["step"][t][~act]).all(), (name, t)
        if ev is None:
            assert got["frame_status"][t] == NOTHING and all(np.isnan(f) for f in frame), (name, t)
            continue
        assert got["frame_status"][t] == CONVERGED, (name, t)
        H, G, d, u = got["information"][t], got["gradient"][t], got["step"][t], got["direction"][t]
        assert np.isfinite(H[act]).all() and np.isfinite(G[act]).all() and np.isfinite(d[act]).all() and all(np.isfinite(f) for f in frame), (name, t)
        has_bone = ~np.isnan(ev["u"]).any(-1)
        assert np.array_equal(~np.isnan(u).any(-1), has_bone), (name, t)
        eh = np.abs(H[act] - ev["info"][act]).max() / np.abs(ev["info"][act]).max()
        eg = np.abs(G[act] - ev["G"][act]).max() / ev["S"][act].max()
        eu = np.abs(u[has_bone] - ev["u"][has_bone]).max() if has_bone.any() else 0.0
        M, idx = dense_matrix(H, u, act, case)       # from the returned information, directions and gradient
        dref, cnd = damped_solve(M, G[idx].ravel(), lam)
        ed, bar_d = np.abs(d[idx].ravel() - dref).max(), so.BAR_K * EPS * cnd * np.abs(dref).max()
        cost = ev["data"] + ev["bone"]
        tol = 1e-9 * max(1.0, cost) + 100 * EPS * cnd * cost
        ec = max(abs(got["data_cost"][t] - ev["data"]), abs(got["bone_cost"][t] - ev["bone"]), abs(got["trial_cost"][t] - ev["trial"]))
        print(f"{name} frame {t}: information {eh:.3g} (bar 1e-12), gradient {eg:.3g} of max S (bar 1e-12), direction {eu:.3g} (bar 1e-12), step {ed:.3g} (bar {bar_d:.3g}, cond {cnd:.3g}), "
              f"costs {ec:.3g} (bar {tol:.3g})")
        assert eh <= 1e-12 and eg <= 1e-12 and eu <= 1e-12 and ed <= bar_d and ec <= tol, (name, t)


def check_loop(name, got, xtol=1e-8, history=None):
    """got: dict(points (T, K, 3), keypoint_status, frame_status, n_iterations, cost, cost_start, bone_residual (T, K) by child).  The rules of
    trajectory_refine_oracle.check_loop, per frame; history (the host-check tier has it): per frame the objective after every trial.
    Returns (frames left out as undecided, frames run)"""
    case, cls = cases()[name], statuses(name)
    assert np.array_equal(got["keypoint_status"], cls), (name, got["keypoint_status"], cls)
    left_out = ran = 0
    for t, o in enumerate(reference(name, xtol=xtol)):
        act = cls[t] > 0
        x, nit = got["points"][t], int(got["n_iterations"][t])
        assert np.isnan(x[~act]).all() and np.isfinite(x[act]).all(), (name, t)
        if not act.any():
            assert got["frame_status"][t] == NOTHING and nit == 0 and np.isnan(got["cost"][t]) and np.isnan(got["cost_start"][t]) and np.isnan(got["bone_residual"][t]).all(), (name, t)
            continue
        if o is None:
            continue
        ran += 1
        assert got["frame_status"][t] == CONVERGED and 1 <= nit < 50, (name, t, got["frame_status"][t], nit)
        assert got["cost"][t] <= got["cost_start"][t], (name, t)                      # exact: a step is taken only when the objective is not above
        if history is not None:
            h = np.r_[got["cost_start"][t], history[t][:nit]]
            assert (h[1:] <= h[:-1]).all() and h[-1] == got["cost"][t], (name, t, h)   # exact
        assert abs(got["cost_start"][t] - o["cost_start"]) <= 1e-9 * max(1.0, o["cost_start"]), (name, t)
        bt = {k: r for k, _, _, r, _ in bone_terms(x, act, case)}
        br = got["bone_residual"][t]
        assert np.array_equal(np.flatnonzero(~np.isnan(br)), sorted(bt)) and all(abs(br[k] - r) <= 1e-9 * max(1.0, abs(r)) for k, r in bt.items()), (name, t)
        move = evaluate(x, t, act, case, 0.0)["dmax"]
        print(f"{name} frame {t}: iterations {nit} (oracle {o['n_iterations']}), cost {got['cost'][t]:.12g} (oracle {o['cost']:.12g}), one more step {move:.3g}")
        assert move < 10 * xtol * np.abs(x[act]).max(), (name, t, move)
        if decided(o):
            assert nit == o["n_iterations"], (name, t, nit, o["n_iterations"])
        else:
            left_out += 1
    return left_out, ran


def check_covariance(name, got):
    """got: the loop's result with covariance, information (T, K, 3, 3) and direction (T, K, 3) by child: the section 8f-20 bar against the inverse of
    the dense matrix built from the returned information and directions"""
    case, cls = cases()[name], statuses(name)
    for t in range(len(cls)):
        act = cls[t] > 0
        assert np.isnan(got["covariance"][t][~act]).all(), (name, t)
        if not act.any():
            continue
        M, idx = dense_matrix(got["information"][t], got["direction"][t], act, case)
        ref = covariance_reference(M)
        err, bar = sco.scaled_error(got["covariance"][t][idx], None, ref), sco.bar_of(ref)
        print(f"{name} frame {t}: covariance {err:.3g} (bar {bar:.3g}, cond {ref['cond']:.3g})")
        assert err <= bar, (name, t, err, bar)
