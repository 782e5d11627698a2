"""The reference of skeleton.refine_skeleton_trajectories in numpy / scipy, built from trajectory_refine_oracle (the data
term, the penalty bands, the accept and stop rule) and skeleton_oracle (the forest, the bones' terms, the gradient's scale): the dense matrices A =
M + B, M and B and the gradient G of one evaluation, a dense solve, a dense Gauss-Newton with the library's accept and stop rule on the call's
objective, kappa = the largest eigenvalue of the pencil (A, M) -- what bounds the conjugate-gradient iteration the library preconditions with M --,
the scenes and cases of the tests and the rules of the host-check and GPU tiers.

One problem per call, unknowns x_{t,k} of the running tracks (trajectory_refine_oracle.counts), ordered (frame, running track, coordinate):
    minimise 0.5 sum_t sum_k sum_{c sees (t,k)} f^2 [rho(ru^2 / f^2) + rho(rv^2 / f^2)] + 0.5 sum_k a_k^-2 sum_t |x_{t-1,k} - 2 x_{t,k} + x_{t+1,k}|^2
             + 0.5 sum_t sum_{active bones (k, p)} ((|x_{t,k} - x_{t,p}| - L) / s)^2
A bone is active, in every frame, when both its tracks run.  Its Gauss-Newton term with u = (x_k - x_p) / |x_k - x_p| is + u u^T / s^2 on both
diagonal blocks and - u u^T / s^2 off them."""
import functools

import numpy as np

import keypoint_scenes as ks
import skeleton_oracle as sko
import smoothing_oracle as so
import tricov_oracle as tco
import trajectory_refine_oracle as tro
import weights_oracle as wo
from test_triangulate_cpu import scene as rig_scene

EPS = so.EPS
ALPHAS = tro.ALPHAS
STATUS_OK, STATUS_TOO_FEW, STATUS_PIVOT, STATUS_BAD_START = 1, -1, -2, -3
CG_TOL = 1e-10   # what the bars of the two tiers hold at


# ---------------------------------------------------------------- one evaluation
def running(case):
    """(n_usable, n_single, status (K,), run (K,) bool, apar (K,): the parent of every keypoint whose bone is active, -1 otherwise)"""
    nus, nsg, status = tro.counts(case)
    run = status == STATUS_OK
    par = np.asarray(case["parent"])
    apar = np.where(run & (par >= 0) & run[np.maximum(par, 0)], par, -1)
    return nus, nsg, status, run, apar


def data_terms(x, case):
    """trajectory_refine_oracle.data_terms with skeleton_oracle.frame_data's scale of the gradient: its terms in absolute value, the residual
    taken as the difference it is -- sw (|detection| + |projection|)"""
    C, T, K = case["weff"].shape
    P = T * K
    uv = [np.asarray(case["uvs"][c], dtype=np.float64).reshape(P, 2) for c in range(C)]
    weff = case["weff"].reshape(C, P)
    loss, fs = case["loss"], case["f_scale"]
    with wo.direct(weff), np.errstate(all="ignore"):
        seen, f, wt, A, _ = tco.linearise(np.asarray(x, dtype=np.float64).reshape(P, 3), uv, case["ext"], case["intr"], loss, fs)
    z = (f / fs) ** 2
    cw = tro.curvature(z, tco.rho1(z, loss), loss) * seen[..., None]
    terms = A * (wt * f)[..., None]
    sw = np.sqrt(np.where(weff > 0, weff, 0.0))
    operands = np.where(seen[..., None], 2.0 * np.abs(np.nan_to_num(np.stack(uv))) * sw[..., None] + np.abs(f), 0.0)
    return dict(H=np.einsum("cpki,cpk,cpkj->pij", A, cw, A).reshape(T, K, 3, 3), g=-terms.sum(axis=(0, 2)).reshape(T, K, 3),
                gabs=(np.abs(A) * (wt * operands)[..., None]).sum(axis=(0, 2)).reshape(T, K, 3), cost=(0.5 * fs ** 2 * (so.rho(loss, z) * seen[..., None]).sum(axis=(0, 2))).reshape(T, K))


def bones_at(x, case, apar):
    """(u (T, K, 3), r (T, K)) by child: NaN where the keypoint has no active bone"""
    T, K = x.shape[:2]
    u, r = np.full((T, K, 3), np.nan), np.full((T, K), np.nan)
    for k in np.flatnonzero(apar >= 0):
        e = x[:, k] - x[:, apar[k]]
        with np.errstate(all="ignore"):
            n = np.linalg.norm(e, axis=1)
            u[:, k], r[:, k] = e / n[:, None], (n - case["L"][k]) / case["s"][k]
    return u, r


def costs(x, case, run, apar):
    """(data, penalty, bone) of the call's objective at x (T, K, 3)"""
    d = data_terms(x, case)
    acc = np.broadcast_to(np.asarray(case["accel_std"], dtype=np.float64), (len(run),))
    pen = sum(tro.penalty_cost(x[:, k], acc[k]) for k in np.flatnonzero(run))
    _, r = bones_at(x, case, apar)
    return float(d["cost"][:, run].sum()), float(pen), 0.5 * float(np.nansum(r * r)) + (np.nan if np.isnan(r[:, apar >= 0]).any() else 0.0)


def objective(x, case, run, apar):
    return float(sum(costs(x, case, run, apar)))


def dense(H, u, case, run, apar):
    """(M, B) over the running tracks, unknowns ordered (frame, running track, coordinate): M = blockdiag(H) + a^-2 D2^T D2 (x) I3 per track from
    H (T, K, 3, 3), B the bones' terms from their directions u (T, K, 3) by child"""
    T, K = H.shape[:2]
    idx = np.flatnonzero(run)
    pos = {int(k): j for j, k in enumerate(idx)}
    nr = len(idx)
    ia2 = 1.0 / np.broadcast_to(np.asarray(case["accel_std"], dtype=np.float64), (K,))[idx] ** 2
    M = np.kron(tro.penalty_matrix(T), np.kron(np.diag(ia2), np.eye(3)))
    B = np.zeros_like(M)
    for t in range(T):
        for j, k in enumerate(idx):
            i = 3 * (t * nr + j)
            M[i:i + 3, i:i + 3] += H[t, k]
            if apar[k] >= 0:
                p = 3 * (t * nr + pos[int(apar[k])])
                b = np.outer(u[t, k], u[t, k]) / case["s"][k] ** 2
                B[i:i + 3, i:i + 3] += b
                B[p:p + 3, p:p + 3] += b
                B[i:i + 3, p:p + 3] -= b
                B[p:p + 3, i:i + 3] -= b
    return M, B


def scaled_solve(A, G, cond=True):
    """(d, cond of the Jacobi-scaled A -- NaN where it is not asked for: it costs more than the solve)"""
    s = np.sqrt(np.diagonal(A))
    Ah = A / np.outer(s, s)
    return np.linalg.solve(Ah, -G / s) / s, float(np.linalg.cond(Ah)) if cond else np.nan


def kappa(A, M):
    """the largest eigenvalue of the pencil (A, M)"""
    from scipy.linalg import cholesky, solve_triangular
    L = cholesky(M, lower=True)
    W = solve_triangular(L, solve_triangular(L, A, lower=True).T, lower=True)
    return float(np.linalg.eigvalsh((W + W.T) / 2).max())


def pcg_iterations(A, M, G, tols=(1e-2, 1e-4, 1e-8), cap=2000):
    """iterations of conjugate gradients on A d = -G preconditioned with M from d = 0 until sqrt(r^T z / r0^T z0) <= tol, per tol"""
    from scipy.linalg import cho_factor, cho_solve
    cf = cho_factor(M)
    d, r = np.zeros(len(G)), -G.copy()
    z = cho_solve(cf, r)
    p, rz = z.copy(), float(r @ z)
    rz0, out, it = rz, [], 0
    for tol in tols:
        while rz > tol * tol * rz0 and it < cap:
            Ap = A @ p
            al = rz / float(p @ Ap)
            d += al * p
            r -= al * Ap
            z = cho_solve(cf, r)
            rzn = float(r @ z)
            p = z + rzn / rz * p
            rz, it = rzn, it + 1
        out.append(it)
    return out


def evaluate(x, case, with_kappa=False):
    """the call at x (T, K, 3): dict(status.., H (T, K, 3, 3), G, S (T, K, 3: NaN off the running tracks), u, r, data, pen, bone, M, B, A, d (T, K, 3),
    cond, trial (4), dmax, xmax[, kappa])"""
    nus, nsg, status, run, apar = running(case)
    T, K = x.shape[:2]
    idx = np.flatnonzero(run)
    out = dict(n_usable=nus, n_single=nsg, status=status, run=run, apar=apar)
    if not run.any():
        return out
    dt = data_terms(x, case)
    acc = np.broadcast_to(np.asarray(case["accel_std"], dtype=np.float64), (K,))
    P = tro.penalty_matrix(T)
    G, S = np.full((T, K, 3), np.nan), np.full((T, K, 3), np.nan)
    for k in idx:
        G[:, k] = dt["g"][:, k] + (P @ x[:, k]) / acc[k] ** 2
        S[:, k] = dt["gabs"][:, k] + (np.abs(P) @ np.abs(x[:, k])) / acc[k] ** 2
    u, r = bones_at(x, case, apar)
    for k in np.flatnonzero(apar >= 0):
        gb = u[:, k] * (r[:, k] / case["s"][k])[:, None]
        G[:, k] += gb
        G[:, apar[k]] -= gb
        S[:, k] += np.abs(gb)
        S[:, apar[k]] += np.abs(gb)
    H = np.where(run[None, :, None, None], dt["H"], np.nan)
    M, B = dense(dt["H"], u, case, run, apar)
    A = M + B
    dv, cnd = scaled_solve(A, G[:, idx].ravel(), cond=with_kappa)
    d = np.zeros((T, K, 3))
    d[:, idx] = dv.reshape(T, len(idx), 3)
    data, pen, bone = costs(x, case, run, apar)
    out.update(H=H, G=G, S=S, u=u, r=r, data=data, pen=pen, bone=bone, M=M, B=B, A=A, d=d, cond=cnd, trial=np.array([objective(x + a * d, case, run, apar) for a in ALPHAS]),
               dmax=float(np.abs(dv).max()), xmax=float(np.abs(x[:, idx]).max()))
    if with_kappa:
        out["kappa"] = kappa(A, M)
    return out


def gauss_newton(case, max_iterations=30, xtol=1e-8, bones=True):
    """the dense loop of the call from case["start"]: dict(points, status, n_iterations, converged, cost, cost_start, history (n, 3), dmax, thresholds).
    bones=False: the same without the bone term (every track on its own: refine_trajectories' fit)"""
    if not bones:
        case = dict(case, parent=np.full(len(case["parent"]), -1))
    nus, nsg, status, run, apar = running(case)
    T, K = case["start"].shape[:2]
    out = dict(points=np.full((T, K, 3), np.nan), status=status, n_usable=nus, n_single=nsg, n_iterations=0, converged=False, cost=np.nan, cost_start=np.nan, history=np.zeros((0, 3)),
               dmax=[], thresholds=[], max_iterations=max_iterations, run=run, apar=apar)
    if not run.any():
        return out
    x = np.array(case["start"], dtype=np.float64)
    x[:, ~run] = 0.0
    hist = []
    for it in range(max_iterations):
        ev = evaluate(x, case)
        cur = ev["data"] + ev["pen"] + ev["bone"]
        if it == 0:
            out["cost_start"] = cur
        alpha, cost = 0.0, cur
        for a, c in zip(ALPHAS, ev["trial"]):
            if c <= cur:
                alpha, cost = a, float(c)
                break
        hist.append((cost, alpha * ev["dmax"], alpha))
        out["dmax"].append(ev["dmax"])
        out["thresholds"].append(xtol * ev["xmax"])
        x = x + alpha * ev["d"]
        small = alpha == 0.0 or alpha * ev["dmax"] < xtol * ev["xmax"]
        if small or it + 1 >= max_iterations:
            out["converged"] = bool(small)
            break
    x[:, ~run] = np.nan
    out.update(points=x, n_iterations=len(hist), cost=hist[-1][0], history=np.array(hist))
    return out


decided = tro.decided


def further_step(x, case):
    """how far one more dense Gauss-Newton step moves x: max |d|"""
    run = running(case)[3]
    return evaluate(np.where(run[None, :, None], x, 0.0), case)["dmax"]


# ---------------------------------------------------------------- scenes
def make_scene(C, T, bones, K, seed, noise=0.5, p_drop=0.2, bone_range=(8.0, 30.0), single=(), unseen=(), ends=0, outliers=0.0, outlier_size=40.0, min_cos=None):
    """dict(uvs (C, T, K, 2), ext, intr, truth (T, K, 3), bones, bone_length): a rig of test_triangulate_cpu.scene; every root a smooth track
    (smoothing_oracle.truth, three times as wide) through its cloud, every other keypoint at its bone's length from its parent in a direction that
    turns smoothly; detections with noise, a share p_drop dropped, a share `outliers` displaced.  single: (keypoint, a, b) -- frames a .. b - 1 of it
    seen by one camera only (min_cos: by the camera whose ray makes the smallest angle with one of its bones in the middle of the stretch, and the
    scene is refused -- None -- where that angle's cosine falls below min_cos inside the stretch); unseen: (keypoint, a, b) -- by nobody; ends: that
    many frames unseen at both ends"""
    _, ext, intr, X = rig_scene(C=C, P=8, seed=seed)
    rng = np.random.default_rng(seed + 3000)
    bones = np.asarray(bones, dtype=np.int64).reshape(-1, 2)
    parent, child = sko.parents_of(bones, K)
    Lb = rng.uniform(*bone_range, len(child))
    L = np.zeros(K)
    L[child] = Lb
    truth = np.zeros((T, K, 3))
    tt = np.arange(T)[:, None]
    for k in sko.plan(parent)["order"]:
        if parent[k] < 0:
            truth[:, k] = X.mean(0) + 3.0 * so.truth(T, 1, rng)[:, 0]
        else:
            n = rng.normal(size=(3, 3))
            v = n[0] + 0.6 * (n[1] * np.sin(2 * np.pi * tt / rng.uniform(80, 200) + rng.uniform(0, 6)) + n[2] * np.cos(2 * np.pi * tt / rng.uniform(80, 200)))
            truth[:, k] = truth[:, parent[k]] + L[k] * v / np.linalg.norm(v, axis=1, keepdims=True)
    uv = np.stack([ks.project5(truth, ext[c], *intr[c]) for c in range(C)])
    uv += rng.normal(0, noise, uv.shape)
    if outliers > 0:
        hit = rng.uniform(size=(C, T, K)) < outliers
        uv[hit] += rng.normal(0, outlier_size, (int(hit.sum()), 2))
    drop = rng.uniform(size=(C, T, K)) < p_drop

    def cosines(k, c, a, b):
        ray = truth[a:b, k] + ks.rodrigues(ext[c][:3]).T @ ext[c][3:]
        out = np.zeros(b - a)
        for i, j in bones:
            if k in (i, j):
                e = truth[a:b, i] - truth[a:b, j]
                out = np.maximum(out, np.abs((ray * e).sum(1)) / np.linalg.norm(ray, axis=1) / np.linalg.norm(e, axis=1))
        return out

    for k, a, b in single:
        cam = 0 if min_cos is None else int(np.argmax([cosines(k, c, (a + b) // 2, (a + b) // 2 + 1)[0] for c in range(C)]))
        if min_cos is not None and cosines(k, cam, a, b).min() < min_cos:
            return None
        drop[:, a:b, k] = True
        drop[cam, a:b, k] = False
    for k, a, b in unseen:
        drop[:, a:b, k] = True
    if ends:
        drop[:, :ends] = True
        drop[:, T - ends:] = True
    uv[drop] = np.nan
    return dict(uvs=uv, ext=ext, intr=intr, truth=truth, bones=bones, bone_length=Lb)


def make_case(s, accel_std=0.15, bone_std=0.5, pixel_std=0.5, loss="linear", f_scale=3.0, weights=None, segment=None, start_noise=0.3, seed=0, bone_length=None):
    """a scene with its parameters and a start (the truth with start_noise of white noise: every frame filled)"""
    C, T, K = s["uvs"].shape[:3]
    parent, child = sko.parents_of(s["bones"], K)
    start = s["truth"] + np.random.default_rng(9000 + seed).normal(0, start_noise, s["truth"].shape)
    Lb = s["bone_length"] if bone_length is None else bone_length
    L, sk = np.ones(K), np.ones(K)
    L[child], sk[child] = Lb, np.broadcast_to(np.asarray(bone_std, dtype=np.float64), (len(child),))
    return dict(s, bone_length=Lb, accel_std=accel_std, bone_std=bone_std, pixel_std=pixel_std, loss=loss, f_scale=f_scale, weights=weights, segment=segment, start=start,
                weff=tro.effective_weights(weights, pixel_std, C, T, K), parent=parent, child=child, L=L, s=sk)


def with_start_seed(build, seeds, max_iterations=30):
    """the first of `seeds` at which the dense loop of build(seed) is decided (its count does not hinge on rounding) and ends before the limit"""
    for seed in seeds:
        case = build(seed)
        o = gauss_newton(case, max_iterations)
        if decided(o) and o["converged"]:
            case["reference"] = o
            return case
    raise AssertionError("no decided start among the seeds")


@functools.lru_cache(maxsize=None)
def cases():
    """name -> case: the smallest shapes at which the kernels can go wrong (computed once and shared: read-only).
    T2: no penalty row; T3; K1: one track, no bone; T257: one frame past a 256-lane workgroup's frames, a chain of three, a one-camera stretch, an
    unseen gap, unseen ends, segment 3; T71_seg2: an odd T (the phantom frame) and several levels, five keypoints of which one has status -1 and one
    -3 -- their bones drop --, per-camera pixel_std, weights on levels, huber with outliers; K64_star: the keypoint cap and a node of degree 63;
    C64_T6: the camera cap; C2.  The start of every case is the first of its seeds at which decided() holds for the oracle itself"""
    out = {}
    out["T2"] = with_start_seed(lambda sd: make_case(make_scene(3, 2, sko.chain(2), 2, seed=31, p_drop=0.0), segment=2, seed=sd), (1, 11, 21))
    out["T3"] = with_start_seed(lambda sd: make_case(make_scene(3, 3, sko.chain(3), 3, seed=32, p_drop=0.0), segment=2, seed=sd), (2, 12, 22))
    out["K1"] = with_start_seed(lambda sd: make_case(make_scene(3, 40, np.zeros((0, 2), int), 1, seed=33, p_drop=0.1, single=((0, 10, 20),)), segment=None, seed=sd), (3, 13, 23))
    out["T257"] = with_start_seed(lambda sd: make_case(make_scene(3, 257, sko.chain(3), 3, seed=44, p_drop=0.15, single=((1, 100, 140),), unseen=((2, 200, 210),), ends=3), loss="soft_l1",
                                                       f_scale=2.0, segment=3, seed=sd), (14, 4, 24))

    def t71(sd):
        s = make_scene(4, 71, np.array([[0, 1], [0, 2], [2, 3], [2, 4]]), 5, seed=35, p_drop=0.2, single=((2, 30, 45),), unseen=((4, 50, 56),), ends=1, outliers=0.05)
        s["uvs"][:, :, 1] = np.nan                  # track 1: one usable frame, a few single ones
        for c in range(4):
            s["uvs"][c, 7, 1] = ks.project5(s["truth"][7, 1], s["ext"][c], *s["intr"][c])
        s["uvs"][0, 20:25, 1] = ks.project5(s["truth"][20:25, 1], s["ext"][0], *s["intr"][0])
        w = wo.draw_levels(4, 71 * 5, 9035, (0.25, 1.0, 1.0, 4.0)).reshape(4, 71, 5)
        c = make_case(s, accel_std=np.array([0.15, 0.15, 0.05, 0.15, 0.5]), pixel_std=np.array([0.5, 0.4, 0.6, 0.5]), loss="huber", weights=w, segment=2, seed=sd)
        c["start"][11, 3, 2] = np.nan               # track 3: a NaN in its start
        return c

    out["T71_seg2"] = with_start_seed(t71, (5, 15, 25))
    out["K64_star"] = with_start_seed(lambda sd: make_case(make_scene(3, 4, sko.star(64), 64, seed=36, p_drop=0.1), segment=2, seed=sd), (6, 16, 26))
    out["C64_T6"] = with_start_seed(lambda sd: make_case(make_scene(64, 6, sko.chain(3), 3, seed=37, p_drop=0.5), loss="soft_l1", segment=2, seed=sd), (7, 17, 27))
    out["C2"] = with_start_seed(lambda sd: make_case(make_scene(2, 40, sko.chain(2), 2, seed=38, p_drop=0.1), segment=None, seed=sd), (8, 18, 28))
    return out


@functools.lru_cache(maxsize=None)
def reference(name, max_iterations=30, xtol=1e-8):
    """the dense loop of a case (at the defaults: the one its start was chosen by)"""
    if (max_iterations, xtol) == (30, 1e-8):
        return cases()[name]["reference"]
    return gauss_newton(cases()[name], max_iterations, xtol)


@functools.lru_cache(maxsize=None)
def system_reference(name):
    case = cases()[name]
    run = running(case)[3]
    return evaluate(np.where(run[None, :, None], case["start"], 0.0), case, with_kappa=True)


def by_child(plane, case):
    return sko.by_child(plane, case)


# ---------------------------------------------------------------- the rules of the host-check and GPU tiers
def a_norm(A, v):
    return float(np.sqrt(max(v @ (A @ v), 0.0)))


def check_system(name, got, cg_tol=CG_TOL):
    """got: dict(information (T, K, 3, 3), gradient, step (T, K, 3), direction (T, K, 3) by child, cg_iterations, cg_residual, data_cost, penalty_cost,
    bone_cost, trial_costs (4), status, n_usable, n_single), computed at cg_tol.  Information within 1e-12 of the largest entry; per frame the
    gradient within 1e-12 of the frame's largest S (section 8f-22's scale); directions within 1e-12; the step against the dense solve d* of the
    system rebuilt from the returned information, directions and gradient: |d - d*|_A <= (2 cg_tol sqrt(kappa) + 100 eps kappa_A) |d*|_A -- A >= M
    gives |e|_A <= |r|_{M^-1} <= cg_tol sqrt(kappa) |d*|_A, the factor 2 and the eps term pay for the recurrence's drift --; the costs within section
    8f-21's bar"""
    case, ev = cases()[name], system_reference(name)
    run, apar = ev["run"], ev["apar"]
    assert np.array_equal(got["status"], ev["status"]) and np.array_equal(got["n_usable"], ev["n_usable"]) and np.array_equal(got["n_single"], ev["n_single"]), (name, got["status"], ev["status"])
    H, G, d, u = got["information"], got["gradient"], got["step"], got["direction"]
    assert np.isnan(H[:, ~run]).all() and np.isnan(G[:, ~run]).all() and np.isnan(d[:, ~run]).all(), name
    assert np.isfinite(H[:, run]).all() and np.isfinite(G[:, run]).all() and np.isfinite(d[:, run]).all(), name
    has = apar >= 0
    assert np.isnan(u[:, ~has]).all() and np.isfinite(u[:, has]).all(), name
    eh = np.abs(H[:, run] - ev["H"][:, run]).max() / np.abs(ev["H"][:, run]).max()
    eg = (np.abs(G[:, run] - ev["G"][:, run]).max(axis=(1, 2)) / ev["S"][:, run].max(axis=(1, 2))).max()
    eu = np.abs(u[:, has] - ev["u"][:, has]).max() if has.any() else 0.0
    M, B = dense(H, u, case, run, apar)       # from the returned information, directions and gradient
    A = M + B
    dref, cnd = scaled_solve(A, G[:, run].ravel())
    ed = a_norm(A, d[:, run].ravel() - dref) / a_norm(A, dref)
    bar_d = 2 * cg_tol * np.sqrt(ev["kappa"]) + 100 * EPS * cnd
    cost = ev["data"] + ev["pen"] + ev["bone"]
    tol = 1e-9 * max(1.0, cost) + 100 * EPS * cnd * cost
    et = np.abs(got["trial_costs"] - ev["trial"]).max()
    ec = max(abs(got["data_cost"] - ev["data"]), abs(got["penalty_cost"] - ev["pen"]), abs(got["bone_cost"] - ev["bone"]))
    print(f"{name}: information {eh:.3g} (bar 1e-12), gradient {eg:.3g} of max S (bar 1e-12), direction {eu:.3g} (bar 1e-12), step {ed:.3g} in the A norm (bar {bar_d:.3g}, kappa "
          f"{ev['kappa']:.3g}, cond {cnd:.3g}), CG iterations {got['cg_iterations']} to {got['cg_residual']:.3g}, costs {max(et, ec):.3g} (bar {tol:.3g})")
    assert eh <= 1e-12 and eg <= 1e-12 and eu <= 1e-12 and ed <= bar_d and et <= tol and ec <= tol, name
    assert got["cg_residual"] <= cg_tol or got["cg_iterations"] >= 200, name
    return ev


def check_loop(name, got, xtol=1e-8):
    """got: dict(points, information, status, n_usable, n_single, converged, n_iterations, cost, cost_start, history (n, 4), bone_residual, direction
    (T, K[, 3]) by child), computed at CG_TOL.  The history never rises, one further dense step moves less than 10 xtol max|x|, n_iterations is the
    oracle's, statuses and counts exact"""
    case, o = cases()[name], reference(name, xtol=xtol)
    run, apar = o["run"], o["apar"]
    assert np.array_equal(got["status"], o["status"]) and np.array_equal(got["n_usable"], o["n_usable"]) and np.array_equal(got["n_single"], o["n_single"]), (name, got["status"], o["status"])
    x, nit, h = got["points"], int(got["n_iterations"]), got["history"]
    assert np.isnan(x[:, ~run]).all() and np.isnan(got["information"][:, ~run]).all() and np.isfinite(x[:, run]).all() and np.isfinite(got["information"][:, run]).all(), name
    has = apar >= 0
    assert np.isnan(got["bone_residual"][:, ~has]).all() and np.isfinite(got["bone_residual"][:, has]).all() and np.isnan(got["direction"][:, ~has]).all(), name
    assert len(h) == nit and np.isfinite(h).all() and got["cost"] == h[-1, 0] and h[0, 0] <= got["cost_start"], name
    assert (h[1:, 0] <= h[:-1, 0]).all(), (name, h[:, 0])   # exact: a step is taken only when the objective, evaluated the same way, is not above
    u, r = bones_at(np.where(run[None, :, None], x, 0.0), case, apar)
    if has.any():
        assert np.abs(got["bone_residual"][:, has] - r[:, has]).max() <= 1e-9 * max(1.0, np.abs(r[:, has]).max()) and np.abs(got["direction"][:, has] - u[:, has]).max() <= 1e-12, name
    move = further_step(x, case)
    print(f"{name}: iterations {nit} (oracle {o['n_iterations']}), cost {h[-1, 0]:.12g} (oracle {o['cost']:.12g}), alphas {h[:, 2]}, CG iterations {h[:, 3]}, one more step {move:.3g}")
    assert move < 10 * xtol * np.abs(x[:, run]).max(), (name, move)
    assert decided(o), name      # (the seeds are chosen so)
    assert nit == o["n_iterations"] and bool(got["converged"]) == o["converged"], (name, nit, o["n_iterations"])


def check_resolve(name, got):
    """got: dict(resolve (2, T, K, 3), information, status) of one evaluation: M z = -G by the elimination and back-substitution, and -- after the
    right-hand-side halves of every stored record and every level's solution were overwritten with NaN -- by the re-solve from the stored factors
    and the same back-substitution: within 4 eps cond max|z| per track"""
    case = cases()[name]
    K = case["start"].shape[1]
    fresh, again = got["resolve"]
    assert (got["status"] == STATUS_OK).any(), name
    for k in np.flatnonzero(got["status"] == STATUS_OK):
        cnd = so.cond(dict(A=tro.dense_matrix(got["information"][:, k], np.broadcast_to(case["accel_std"], (K,))[k])))
        err, bar = np.abs(again[:, k] - fresh[:, k]).max(), so.BAR_K * EPS * cnd * np.abs(fresh[:, k]).max()
        print(f"{name} track {k}: re-solve against the fresh elimination {err:.3g} (bar {bar:.3g}, cond {cnd:.3g})")
        assert np.isfinite(fresh[:, k]).all() and np.isfinite(again[:, k]).all() and err <= bar, (name, k, err, bar)


RESOLVE_CASES = ("T71_seg2", "T257", "T2", "T3")


def check_one_track(got):
    """K1 (one track, no bone: A = M) at one evaluation: the recurrence ends after one iteration; its step is the dense solve of the track's own
    system (trajectory_refine_oracle) to 4 eps cond max|d|, and the residual the re-solve leaves is within 4 eps cond"""
    case = cases()["K1"]
    A = tro.dense_matrix(got["information"][:, 0], case["accel_std"])
    dref = np.linalg.solve(A, -got["gradient"][:, 0].ravel()).reshape(-1, 3)
    cnd = so.cond(dict(A=A))
    err, bar = np.abs(got["step"][:, 0] - dref).max(), so.BAR_K * EPS * cnd * np.abs(dref).max()
    print(f"K1: step against the track's dense solve {err:.3g} (bar {bar:.3g}, cond {cnd:.3g}), residual after the re-solve {got['cg_residual']:.3g}")
    assert got["cg_iterations"] == 1 and err <= bar and got["cg_residual"] <= so.BAR_K * EPS * cnd


def coincident_case():
    """T3 with keypoint 1 of frame 1 started on its parent: a bone of zero length has a finite residual and no direction, so the objective at the
    start is not finite and every running track is -3"""
    case = dict(cases()["T3"])
    case["start"] = np.array(case["start"])
    case["start"][1, 1] = case["start"][1, 0]
    return case


def check_coincident(loop, system):
    """loop, system: the two calls' results on coincident_case() (planes by child)"""
    nus, nsg, _ = tro.counts(cases()["T3"])
    for got in (loop, system):
        assert (got["status"] == STATUS_BAD_START).all() and np.array_equal(got["n_usable"], nus) and np.array_equal(got["n_single"], nsg)
        assert np.isnan(got["information"]).all() and np.isnan(got["direction"]).all()
    assert np.isnan(loop["points"]).all() and np.isnan(loop["bone_residual"]).all() and np.isnan(loop["cost"]) and np.isnan(loop["cost_start"])
    assert loop["n_iterations"] == 0 and len(loop["history"]) == 0 and not loop["converged"]
    assert np.isnan(system["gradient"]).all() and np.isnan(system["step"]).all() and np.isnan(system["trial_costs"]).all()
    assert all(np.isnan(system[f]) for f in ("data_cost", "penalty_cost", "bone_cost", "cg_residual")) and system["cg_iterations"] == 0


# ---------------------------------------------------------------- what the fit gains
def gain_scene(seed):
    """4 cameras, 200 frames, a tree of 6 keypoints with bones of 8 to 30 mm, given lengths off by N(0, 0.5^2) mm, bone_std 0.5, accel_std 0.15, 0.5 px
    noise, 20 % dropped; one-camera stretches of 40 frames on two keypoints and an unseen gap of 20 on a third, every stretch's bone within 60
    degrees of its ray (None where the scene's geometry does not give that)"""
    s = make_scene(4, 200, sko.random_tree(6, seed), 6, seed=seed, noise=0.5, p_drop=0.2, single=((1, 40, 80), (4, 110, 150)), unseen=((2, 90, 110),), min_cos=0.5)
    if s is None:
        return None
    given = s["bone_length"] + np.random.default_rng(seed + 77).normal(0, 0.5, len(s["bone_length"]))
    return make_case(s, accel_std=0.15, bone_std=0.5, pixel_std=0.5, bone_length=given, seed=seed)


GAIN_STRETCHES = ((1, 40, 80), (4, 110, 150), (2, 90, 110))


def gain(case, max_iterations=30):
    """RMS error against the truth of the joint fit and of the fit without bones: dict(joint, plain: {"all": .., (k, a, b): ..})"""
    out = {}
    for name, bones in (("joint", True), ("plain", False)):
        o = gauss_newton(case, max_iterations, bones=bones)
        err = np.linalg.norm(o["points"] - case["truth"], axis=2)
        out[name] = {"all": float(np.sqrt(np.mean(err ** 2)))}
        for k, a, b in GAIN_STRETCHES:
            out[name][(k, a, b)] = float(np.sqrt(np.mean(err[a:b, k] ** 2)))
    return out


# ---------------------------------------------------------------- the budget
def chunk_doubles(T, K, C, segment):
    """device doubles (and ints, counted as doubles) the call needs (mcba_skeltraj_math.h: skeltraj_chunk_doubles)"""
    blocks = (T * K + 255) // 256
    plan_doubles = ((2 + 64 * 4 + 65) * 4 + 7) // 8 + 64 * 3   # (SkPlan: 323 ints, padded, and 192 doubles)
    return T * K * (3 * C + 31) + K * 8 + plan_doubles + 10 * (blocks + 1) + 8 + 2 + so.level_doubles(T, segment or so.SEGMENT_DEFAULT, K, so.X_EXTRA)
