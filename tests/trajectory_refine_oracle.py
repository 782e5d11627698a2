"""The reference of trajectory.refine_trajectories in numpy / scipy: per track the data term's H, g and cost from the
analytic derivatives of tricov_oracle.linearise under the weighted statement of weights_oracle.direct, the penalty bands and the dense system
of smoothing_oracle, a dense Gauss-Newton with the library's accept and stop rule, the two-stage chain it is compared with, the scenes and
cases of the tests.

Per track, frames t = 0 .. T-1:
    minimise 0.5 sum_t sum_{c sees (t,k)} f^2 [rho(ru^2 / f^2) + rho(rv^2 / f^2)] + 0.5 / a^2 sum_{t=1}^{T-2} |x_{t-1} - 2 x_t + x_{t+1}|^2,
    (ru, rv) = sqrt(w) (detection - project5(x_t)) / pixel_std_c
A detection is seen when neither coordinate is NaN and its weight is positive and not NaN; a frame is usable with two views or more, single with
exactly one.  H_t = sum A^T diag(cw) A with the curvature weight cw = max(rho' + 2 rho'' z, eps, 0.1 rho') of the library's other keypoint
estimators (z = r^2 / f^2 per scalar), g_t = -sum A^T rho' r, G = g + a^-2 (D2^T D2 x).

The loop: at x the objective `cur`, the step d of (blockdiag(H) + a^-2 D2^T D2 (x) I3) d = -G, the objective at x + alpha d for alpha = 1, 1/2, 1/4,
1/8; the largest alpha whose objective is <= cur is taken (none: alpha = 0 and the track stops); the track stops when alpha max|d| < xtol max|x|
or after max_iterations."""
import functools

import numpy as np

import keypoint_scenes as ks
import smoothing_cov_oracle as sco
import smoothing_oracle as so
import tricov_oracle as tco
import weights_oracle as wo
from test_triangulate_cpu import scene as rig_scene

EPS = so.EPS
ALPHAS = (1.0, 0.5, 0.25, 0.125)
STATUS_OK, STATUS_TOO_FEW, STATUS_PIVOT, STATUS_BAD_START = 1, -1, -2, -3
CURV_FLOOR = 0.1       # MCBA_CURV_FLOOR_TRIGGS
MACH_EPS = 2.220446049250313e-16


def effective_weights(weights, pixel_std, C, T, K):
    """(C, T, K): w / pixel_std^2 -- what multiplies the squared pixel residual; NaN and 0 stay (unseen)"""
    w = np.ones((C, T, K)) if weights is None else np.asarray(weights, dtype=np.float64)
    ps = np.broadcast_to(np.asarray(pixel_std, dtype=np.float64), (C,))
    return w / (ps * ps)[:, None, None]


def curvature(z, rho1, loss):
    """max(rho' + 2 rho'' z, eps, CURV_FLOOR rho') per scalar"""
    if loss == "linear":
        return np.ones_like(z)
    if loss == "soft_l1":
        w2 = (1.0 + z) ** -1.5
    else:
        w2 = np.where(z <= 1.0, 1.0, 0.0)
    return np.maximum(np.maximum(w2, MACH_EPS), CURV_FLOOR * rho1)


def penalty_matrix(T):
    """D2^T D2 of T frames, dense, from smoothing_oracle.penalty_bands"""
    dg, o1, o2 = so.penalty_bands(T)
    M = np.diag(dg)
    if T > 1:
        M += np.diag(o1[:T - 1], 1) + np.diag(o1[:T - 1], -1)
    if T > 2:
        M += np.diag(o2[:T - 2], 2) + np.diag(o2[:T - 2], -2)
    return M


def data_terms(x, uvs, ext, intr, weff, loss, f_scale):
    """x (T, K, 3), uvs (C, T, K, 2), weff (C, T, K) -> dict(H (T, K, 3, 3), g, gabs (T, K, 3: the gradient of the data term and the sum of
    the absolute values of its terms), cost (T, K), views (T, K))"""
    C, T, K = weff.shape
    P = T * K
    uv = [np.asarray(uvs[c], dtype=np.float64).reshape(P, 2) for c in range(C)]
    with wo.direct(weff.reshape(C, P)):
        seen, f, wt, A, _ = tco.linearise(np.asarray(x, dtype=np.float64).reshape(P, 3), uv, ext, intr, loss, f_scale)
    z = (f / f_scale) ** 2
    cw = curvature(z, tco.rho1(z, loss), loss) * seen[..., None]
    H = np.einsum("cpki,cpk,cpkj->pij", A, cw, A)
    terms = A * (wt * f)[..., None]
    cost = 0.5 * f_scale ** 2 * (so.rho(loss, z) * seen[..., None]).sum(axis=(0, 2))
    return dict(H=H.reshape(T, K, 3, 3), g=-terms.sum(axis=(0, 2)).reshape(T, K, 3), gabs=np.abs(terms).sum(axis=(0, 2)).reshape(T, K, 3), cost=cost.reshape(T, K),
                views=seen.sum(0).reshape(T, K))


def penalty_cost(x, accel_std):
    """one track x (T, 3)"""
    return 0.5 / float(accel_std) ** 2 * float(np.sum((x[:-2] - 2.0 * x[1:-1] + x[2:]) ** 2)) if len(x) >= 3 else 0.0


def track_inputs(case, k):
    """the case restricted to track k (K = 1)"""
    C, T, K = case["weff"].shape
    return dict(case, uvs=case["uvs"][:, :, k:k + 1], weff=case["weff"][:, :, k:k + 1], accel_std=float(np.broadcast_to(case["accel_std"], (K,))[k]))


def objective(x, tc):
    """one track: x (T, 3), tc = track_inputs(..)"""
    d = data_terms(x[:, None], tc["uvs"], tc["ext"], tc["intr"], tc["weff"], tc["loss"], tc["f_scale"])
    return float(d["cost"].sum()) + penalty_cost(x, tc["accel_std"])


def evaluate(x, tc):
    """one track at x (T, 3): dict(H (T, 3, 3), G, S (T, 3), data, pen, A (dense), d (T, 3), cond, trial (4), dmax, xmax)"""
    T = len(x)
    d = data_terms(x[:, None], tc["uvs"], tc["ext"], tc["intr"], tc["weff"], tc["loss"], tc["f_scale"])
    ia2 = 1.0 / tc["accel_std"] ** 2
    M = penalty_matrix(T)
    G = d["g"][:, 0] + ia2 * (M @ x)
    S = d["gabs"][:, 0] + ia2 * (np.abs(M) @ np.abs(x))
    A = dense_matrix(d["H"][:, 0], tc["accel_std"])
    step = np.linalg.solve(A, -G.ravel()).reshape(T, 3)
    out = dict(H=d["H"][:, 0], G=G, S=S, data=float(d["cost"].sum()), pen=penalty_cost(x, tc["accel_std"]), A=A, d=step, dmax=float(np.abs(step).max()), xmax=float(np.abs(x).max()))
    out["trial"] = np.array([objective(x + a * step, tc) for a in ALPHAS])
    return out


def dense_matrix(H, accel_std):
    """blockdiag(H_t) + a^-2 D2^T D2 (x) I3 of one track; H (T, 3, 3)"""
    T = len(H)
    A = np.kron(penalty_matrix(T), np.eye(3)) / float(accel_std) ** 2
    for t in range(T):
        A[3 * t:3 * t + 3, 3 * t:3 * t + 3] += H[t]
    return A


def counts(case):
    """(n_usable (K,), n_single (K,), status (K,)) of a case from its detections, weights and start"""
    uv, w = np.asarray(case["uvs"]), case["weff"]
    seen = ~np.isnan(uv).any(-1) & (w > 0)
    views = seen.sum(0)
    nus, nsg = (views >= 2).sum(0), (views == 1).sum(0)
    bad = ~np.isfinite(case["start"]).all(axis=(0, 2))
    return nus.astype(np.int32), nsg.astype(np.int32), np.where(nus < 2, STATUS_TOO_FEW, np.where(bad, STATUS_BAD_START, STATUS_OK)).astype(np.int32)


def gauss_newton(case, k, max_iterations=30, xtol=1e-8):
    """one track of a case from case["start"]: dict(points, status, n_iterations, cost, history (n, 3), dmax (n,), thresholds (n,))"""
    nus, nsg, status = counts(case)
    T = case["start"].shape[0]
    out = dict(points=np.full((T, 3), np.nan), status=int(status[k]), n_usable=int(nus[k]), n_single=int(nsg[k]), n_iterations=0, cost=np.nan, history=np.zeros((0, 3)), dmax=[], thresholds=[])
    if status[k] != STATUS_OK:
        return out
    tc = track_inputs(case, k)
    x = np.array(case["start"][:, k], dtype=np.float64)
    hist = []
    for it in range(max_iterations):
        ev = evaluate(x, tc)
        cur = ev["data"] + ev["pen"]
        alpha, cost = 0.0, cur
        for a, c in zip(ALPHAS, ev["trial"]):
            if c <= cur:
                alpha, cost = a, float(c)
                break
        hist.append((cost, alpha * ev["dmax"], alpha))
        out["dmax"].append(ev["dmax"])
        out["thresholds"].append(xtol * ev["xmax"])
        x = x + alpha * ev["d"]
        if alpha == 0.0 or it + 1 >= max_iterations or alpha * ev["dmax"] < xtol * ev["xmax"]:
            break
    out.update(points=x, n_iterations=len(hist), cost=hist[-1][0], history=np.array(hist), max_iterations=max_iterations)
    return out


def decided(o):
    """the reference's count does not hinge on rounding: every step after which it went on is more than twice its threshold xtol max|x|, and
    it stopped at the iteration limit or where the full step max|d| is below half the threshold -- there every alpha stops the track, the
    alpha = 0 of an objective that can no longer be told apart included (that choice is made at the objective's resolution)"""
    st, thr, dmax = o["history"][:, 1], np.array(o["thresholds"]), np.array(o["dmax"])
    return bool((st[:-1] > 2 * thr[:-1]).all() and (len(st) == o["max_iterations"] or dmax[-1] < thr[-1] / 2))


def further_step(x, case, k):
    """how far one more Gauss-Newton step of the oracle moves x (one track): max |d|"""
    return evaluate(x, track_inputs(case, k))["dmax"]


def covariance_reference(A, T):
    """smoothing_cov_oracle.reference's quantities of a dense Gauss-Newton matrix: diag, lag, s, cond, zmax"""
    s = np.sqrt(np.diagonal(A))
    Ah = A / np.outer(s, s)
    Zh = np.linalg.inv(Ah)
    Zh = (Zh + Zh.T) / 2
    diag, lag = sco.band_of(Zh / np.outer(s, s), T)
    return dict(diag=diag, lag=lag, s=s, cond=float(np.linalg.cond(Ah)), zmax=float(np.abs(Zh).max()))


# ---------------------------------------------------------------- the two-stage chain: per-frame fits, then smoothing_oracle.smooth
def two_stage(case):
    """(points (T, K, 3), list of smoothing_oracle.irls results): every frame two cameras see is fitted on its own (from the truth, to the
    minimiser of its robust cost), its covariance is the inverse of its H, and smoothing_oracle.smooth fills and smooths the tracks"""
    C, T, K = case["weff"].shape
    P = T * K
    uv = [np.asarray(case["uvs"][c]).reshape(P, 2) for c in range(C)]
    w = case["weff"].reshape(C, P)
    X = wo.refine_direct(case["truth"].reshape(P, 3), uv, case["ext"], case["intr"], w, case["loss"], case["f_scale"]).reshape(T, K, 3)
    d = data_terms(X, case["uvs"], case["ext"], case["intr"], case["weff"], case["loss"], case["f_scale"])
    pts, cov = np.full((T, K, 3), np.nan), np.full((T, K, 3, 3), np.nan)
    ok = d["views"] >= 2
    pts[ok] = X[ok]
    cov[ok] = np.linalg.inv(d["H"][ok])
    res = so.smooth(pts, cov, case["accel_std"], loss=case["loss"], f_scale=3.0)
    return np.stack([r["points"] for r in res], axis=1), res


# ---------------------------------------------------------------- scenes
def make_scene(C, T, K, seed, noise=0.5, p_drop=0.2, single=None, unseen=None, ends=0, outliers=0.0, outlier_size=40.0):
    """dict(uvs (C, T, K, 2), ext, intr, truth (T, K, 3)): a rig of test_triangulate_cpu.scene, smooth tracks (smoothing_oracle.truth, three
    times as wide) through its cloud, detections with noise; a share p_drop dropped, a share `outliers` displaced by N(0, outlier_size^2) px;
    single = (a, b): frames a .. b - 1 seen by camera 0 only; unseen = (a, b): by nobody; ends: that many frames unseen at both ends"""
    _, ext, intr, X = rig_scene(C=C, P=8, seed=seed)
    rng = np.random.default_rng(seed + 1000)
    truth = X.mean(0) + 3.0 * so.truth(T, K, rng)
    uv = np.stack([ks.project5(truth, ext[c], *intr[c]) for c in range(C)])
    uv += rng.normal(0, noise, uv.shape)
    if outliers > 0:
        hit = rng.uniform(size=(C, T, K)) < outliers
        uv[hit] += rng.normal(0, outlier_size, (int(hit.sum()), 2))
    drop = rng.uniform(size=(C, T, K)) < p_drop
    if single:
        drop[1:, single[0]:single[1]] = True
        drop[0, single[0]:single[1]] = False
    if unseen:
        drop[:, unseen[0]:unseen[1]] = True
    if ends:
        drop[:, :ends] = True
        drop[:, T - ends:] = True
    uv[drop] = np.nan
    return dict(uvs=uv, ext=ext, intr=intr, truth=truth)


def make_case(s, accel_std=0.15, pixel_std=0.5, loss="linear", f_scale=3.0, weights=None, segment=None, start_noise=0.3, seed=0):
    """a scene with its parameters and a start (the truth with start_noise of white noise: every frame filled)"""
    C, T, K = s["uvs"].shape[:3]
    start = s["truth"] + np.random.default_rng(5000 + seed).normal(0, start_noise, s["truth"].shape)
    return dict(s, accel_std=accel_std, pixel_std=pixel_std, loss=loss, f_scale=f_scale, weights=weights, segment=segment, start=start, weff=effective_weights(weights, pixel_std, C, T, K))


def stretch_scene():
    """the one-camera stretch: 4 cameras, 200 frames, 0.5 px noise, 20 % of the detections dropped, frames 80 .. 119 seen by camera 0 only"""
    return make_case(make_scene(4, 200, 1, seed=11, noise=0.5, p_drop=0.2, single=(80, 120)), loss="linear")


def outlier_scene():
    """the same with 10 % of the detections displaced by N(0, 40^2) px and the huber loss"""
    return make_case(make_scene(4, 200, 1, seed=11, noise=0.5, p_drop=0.2, single=(80, 120), outliers=0.10), loss="huber")


@functools.lru_cache(maxsize=None)
def cases():
    """name -> case: the smallest shapes at which the kernels can go wrong (computed once and shared: read-only).
    T2: no penalty row; T3; T257: one frame past a 256-frame evaluation workgroup, a 40-frame single-camera stretch, a 10-frame unseen gap,
    unseen frames at both ends; T333_seg2: five levels and the phantom frame, five tracks, per-camera pixel_std, weights on levels, outliers
    under huber, one track with a single usable frame (-1), one with a NaN in its start (-3); C2; C64_T6: the camera cap.  The seeds of the
    starts are the first of 4, 14, 24 (6, 16, 26) at which decided() holds for every running track of the reference itself"""
    out = {}
    out["T2"] = make_case(make_scene(3, 2, 1, seed=21, p_drop=0.0), segment=2, seed=1)
    out["T3"] = make_case(make_scene(3, 3, 1, seed=22, p_drop=0.0), segment=2, seed=2)
    out["T257"] = make_case(make_scene(3, 257, 1, seed=23, p_drop=0.15, single=(100, 140), unseen=(200, 210), ends=3), loss="soft_l1", f_scale=2.0, segment=3, seed=3)
    s = make_scene(4, 333, 5, seed=24, p_drop=0.2, single=(150, 190), unseen=(40, 50), ends=2, outliers=0.05)
    s["uvs"][:, :, 1] = np.nan                  # track 1: one usable frame, a few single ones
    for c in range(4):
        s["uvs"][c, 7, 1] = ks.project5(s["truth"][7, 1], s["ext"][c], *s["intr"][c])
    s["uvs"][0, 20:25, 1] = ks.project5(s["truth"][20:25, 1], s["ext"][0], *s["intr"][0])
    w = wo.draw_levels(4, 333 * 5, 9024, (0.25, 1.0, 1.0, 4.0)).reshape(4, 333, 5)
    c = make_case(s, accel_std=np.array([0.15, 0.15, 0.05, 0.15, 0.5]), pixel_std=np.array([0.5, 0.4, 0.6, 0.5]), loss="huber", weights=w, segment=2, seed=14)
    c["start"][11, 3, 2] = np.nan               # track 3: a NaN in its start
    out["T333_seg2"] = c
    out["C2"] = make_case(make_scene(2, 40, 1, seed=25, p_drop=0.1), segment=None, seed=5)
    out["C64_T6"] = make_case(make_scene(64, 6, 5, seed=26, p_drop=0.5), loss="soft_l1", segment=2, seed=16)
    return out


@functools.lru_cache(maxsize=None)
def reference(name, max_iterations=30, xtol=1e-8):
    """per track the oracle's loop of a case, computed once"""
    case = cases()[name]
    return [gauss_newton(case, k, max_iterations, xtol) for k in range(case["start"].shape[1])]


@functools.lru_cache(maxsize=None)
def system_reference(name):
    """per running track the oracle's evaluation at the start of a case (None for the others), computed once"""
    case = cases()[name]
    status = counts(case)[2]
    return [evaluate(case["start"][:, k], track_inputs(case, k)) if status[k] == STATUS_OK else None for k in range(case["start"].shape[1])]


# ---------------------------------------------------------------- the rules of the host-check and GPU tiers
def check_system(name, got):
    """got: dict(information (T, K, 3, 3), gradient, step (T, K, 3), data_cost, penalty_cost (K), trial_costs (K, 4), status, n_usable, n_single)"""
    case = cases()[name]
    nus, nsg, status = counts(case)
    assert np.array_equal(got["status"], status) and np.array_equal(got["n_usable"], nus) and np.array_equal(got["n_single"], nsg), (name, got["status"], status)
    for k, ev in enumerate(system_reference(name)):
        fields = [got[f][:, k] for f in ("information", "gradient", "step")] + [got[f][k] for f in ("data_cost", "penalty_cost", "trial_costs")]
        if ev is None:
            assert all(np.isnan(f).all() for f in fields), (name, k)
            continue
        assert all(np.isfinite(f).all() for f in fields), (name, k)
        H, G, d = got["information"][:, k], got["gradient"][:, k], got["step"][:, k]
        eh = np.abs(H - ev["H"]).max() / np.abs(ev["H"]).max()
        eg = (np.abs(G - ev["G"]) / ev["S"]).max()
        A = dense_matrix(H, np.broadcast_to(case["accel_std"], (len(status),))[k])   # from the returned information and gradient
        dref = np.linalg.solve(A, -G.ravel()).reshape(-1, 3)
        cnd = so.cond(dict(A=A))
        ed, bar_d = np.abs(d - dref).max(), so.BAR_K * EPS * cnd * np.abs(dref).max()
        cost = ev["data"] + ev["pen"]
        tol = 1e-9 * max(1.0, cost) + 100 * EPS * cnd * cost
        et = np.abs(got["trial_costs"][k] - ev["trial"]).max()
        ec = max(abs(got["data_cost"][k] - ev["data"]), abs(got["penalty_cost"][k] - ev["pen"]))
        print(f"{name} track {k}: information {eh:.3g} (bar 1e-12), gradient {eg:.3g} of S (bar 1e-12), step {ed:.3g} (bar {bar_d:.3g}, cond {cnd:.3g}), costs {max(et, ec):.3g} (bar {tol:.3g})")
        assert eh <= 1e-12 and eg <= 1e-12 and ed <= bar_d and et <= tol and ec <= tol, (name, k)


def check_loop(name, got, xtol=1e-8):
    """got: dict(points, information, status, n_usable, n_single, n_iterations, cost, history (n, K, 3)).  Returns (tracks left out as undecided, tracks run)"""
    case = cases()[name]
    nus, nsg, status = counts(case)
    assert np.array_equal(got["status"], status) and np.array_equal(got["n_usable"], nus) and np.array_equal(got["n_single"], nsg), (name, got["status"], status)
    left_out = ran = 0
    for k, o in enumerate(reference(name, xtol=xtol)):
        x, nit = got["points"][:, k], int(got["n_iterations"][k])
        if o["status"] != STATUS_OK:
            assert np.isnan(x).all() and np.isnan(got["information"][:, k]).all() and np.isnan(got["cost"][k]) and nit == 0 and np.isnan(got["history"][:, k]).all(), (name, k)
            continue
        ran += 1
        h = got["history"][:nit, k]
        assert np.isfinite(x).all() and np.isfinite(h).all() and np.isnan(got["history"][nit:, k]).all() and got["cost"][k] == h[-1, 0], (name, k)
        assert (h[1:, 0] <= h[:-1, 0]).all(), (name, k, h[:, 0])   # exact: a step is taken only when the objective, evaluated the same way, is not above
        move = further_step(x, case, k)
        print(f"{name} track {k}: iterations {nit} (oracle {o['n_iterations']}), cost {h[-1, 0]:.12g} (oracle {o['cost']:.12g}), alphas {h[:, 2]}, one more step {move:.3g}")
        assert move < 10 * xtol * np.abs(x).max(), (name, k, move)
        if decided(o):
            assert nit == o["n_iterations"], (name, k, nit, o["n_iterations"])
        else:
            left_out += 1
    return left_out, ran


def check_covariance(name, got):
    """got: the loop's result with covariance (T, K, 3, 3) and lag_covariance (T - 1, K, 3, 3): the section 8f-20 bar against the inverse of the
    dense matrix built from the returned information"""
    case = cases()[name]
    K = case["start"].shape[1]
    T = case["start"].shape[0]
    for k in range(K):
        if got["status"][k] != STATUS_OK:
            assert np.isnan(got["covariance"][:, k]).all() and np.isnan(got["lag_covariance"][:, k]).all()
            continue
        ref = covariance_reference(dense_matrix(got["information"][:, k], np.broadcast_to(case["accel_std"], (K,))[k]), T)
        err, bar = sco.scaled_error(got["covariance"][:, k], got["lag_covariance"][:, k], ref), sco.bar_of(ref)
        print(f"{name} track {k}: covariance {err:.3g} (bar {bar:.3g}, cond {ref['cond']:.3g})")
        assert err <= bar, (name, k, err, bar)


# ---------------------------------------------------------------- the chunk rule
def chunk_doubles(T, K, C, segment, cov=False, lag=False):
    """device doubles (and ints, counted as doubles) one chunk of K tracks needs: the detection and weight planes count (3 C per frame)"""
    return T * K * (3 * C + 15 + (6 if cov else 0) + (9 if lag else 0)) + K * (8 + 9) + 9 * ((T + 255) // 256) * K + so.level_doubles(T, segment, K, so.ZC_EXTRA if cov else so.X_EXTRA)


def expected_chunks(T, K, C, segment, budget_mb, cov=False, lag=False):
    """(tracks_per_chunk, chunks, device_bytes, levels) of refine_trajectories under a budget of budget_mb MiB"""
    segment = segment or so.SEGMENT_DEFAULT
    per_track = float(chunk_doubles(T, 1, C, segment, cov, lag)) * 8
    Kc = int(min(float(K), max(1.0, np.floor(budget_mb * 1048576.0 / per_track))))
    return Kc, (K + Kc - 1) // Kc, chunk_doubles(T, Kc, C, segment, cov, lag) * 8, len(so.plan(T, segment, Kc))
