"""The reference of trajectory.smooth_trajectories in numpy / scipy: per track the block-pentadiagonal normal equations,
dense and banded, solved by scipy.linalg.solveh_banded; the IRLS loop with the library's start, stopping rule and loss formulas; the objective;
the condition number the linear bar is scaled by; the scenes of the tests.

Per track, frames t = 0 .. T-1:  minimise 0.5 f^2 sum_t rho(d_t^2 / f^2) + 0.5 / a^2 sum_{t=1}^{T-2} |x_{t-1} - 2 x_t + x_{t+1}|^2,
d_t^2 = (x_t - p_t)^T Sigma_t^-1 (x_t - p_t).  A frame is usable when p_t and Sigma_t are finite, Sigma_t is positive definite (every pivot of
its Jacobi-scaled Cholesky factor has a square >= 1e-12) and its inverse is finite.

The loop: weights start at 1 (or weights_in) on usable frames; solve number it = 0, 1, .. gives x, then d^2, the objective and the step
max |x - x_old| (infinite for it = 0), then the weights rho'(d^2 / f^2); it stops after the solve when the loss is linear, when it + 1 ==
max_iterations, or when it >= 1 and step < xtol max |x|.

The linear bar (per track): max |x - x_oracle| <= BAR_K eps cond max |x_oracle|, cond = cond(system) of the Jacobi-scaled dense matrix."""
import numpy as np
import scipy.linalg

EPS = np.finfo(np.float64).eps
BAR_K = 4.0
PIVOT2_MIN = 1e-12
LOSSES = {"linear": 0, "soft_l1": 1, "huber": 2}
STATUS_OK, STATUS_TOO_FEW, STATUS_PIVOT = 1, -1, -2


def rho(loss, z):
    z = np.asarray(z, dtype=np.float64)
    if loss == "linear":
        return z.copy()
    if loss == "soft_l1":
        return 2.0 * (np.sqrt(1.0 + z) - 1.0)
    if loss == "huber":
        return np.where(z <= 1.0, z, 2.0 * np.sqrt(np.maximum(z, 1.0)) - 1.0)
    raise ValueError(loss)


def drho(loss, z):
    z = np.asarray(z, dtype=np.float64)
    if loss == "linear":
        return np.ones_like(z)
    if loss == "soft_l1":
        return 1.0 / np.sqrt(1.0 + z)
    if loss == "huber":
        return np.where(z <= 1.0, 1.0, 1.0 / np.sqrt(np.maximum(z, 1.0)))
    raise ValueError(loss)


def prepare(points, cov):
    """points (T, 3), cov (T, 3, 3) -> usable (T,), Sigma^-1 (T, 3, 3; zero where unusable), p (zero where unusable)"""
    points, cov = np.asarray(points, dtype=np.float64), np.asarray(cov, dtype=np.float64)
    T = len(points)
    usable, winv = np.zeros(T, bool), np.zeros((T, 3, 3))
    for t in range(T):
        S = cov[t]
        if not (np.isfinite(points[t]).all() and np.isfinite(S).all() and (np.diagonal(S) > 0).all()):
            continue
        d = 1.0 / np.sqrt(np.diagonal(S))
        A = S * np.outer(d, d)
        A[np.arange(3), np.arange(3)] = 1.0
        l10, l20 = A[1, 0], A[2, 0]
        p1 = 1.0 - l10 * l10
        if not p1 >= PIVOT2_MIN:
            continue
        l21 = (A[2, 1] - l20 * l10) / np.sqrt(p1)
        p2 = 1.0 - l20 * l20 - l21 * l21
        if not p2 >= PIVOT2_MIN:
            continue
        Wi = np.linalg.inv((A + A.T) / 2) * np.outer(d, d)
        if np.isfinite(Wi).all():
            usable[t], winv[t] = True, (Wi + Wi.T) / 2
    return usable, winv, np.where(usable[:, None], points, 0.0)


def penalty_bands(T):
    """D2^T D2 of T frames: its diagonal, first and second off-diagonal (entries (t, t + 1), (t, t + 2)), length T each"""
    v = np.zeros(T + 3)
    if T >= 3:
        v[2:T] = 1.0   # v[r + 1] = 1 for the centres r = 1 .. T - 2
    t = np.arange(T)
    return v[t + 2] + 4.0 * v[t + 1] + v[t], -2.0 * (v[t + 1] + v[t + 2]), v[t + 2]


def system(points, cov, accel_std, weights=None, dense=True):
    """One track: dict(ab = the upper banded form (9, 3 T) for solveh_banded, b, A (dense, on request), usable, winv)"""
    usable, winv, p = prepare(points, cov)
    T = len(p)
    w = np.where(usable, 1.0 if weights is None else np.asarray(weights, dtype=np.float64), 0.0)
    W = winv * w[:, None, None]
    ia2 = 1.0 / float(accel_std) ** 2
    dg, o1, o2 = penalty_bands(T)
    ab = np.zeros((9, 3 * T))
    for a in range(3):
        for b in range(a, 3):
            ab[8 + a - b, b::3] = W[:, a, b]
        ab[8, a::3] += ia2 * dg
        if T > 1:
            ab[5, 3 + a::3] = ia2 * o1[:T - 1]
        if T > 2:
            ab[2, 6 + a::3] = ia2 * o2[:T - 2]
    rhs = np.einsum("tab,tb->ta", W, p).ravel()
    out = dict(ab=ab, b=rhs, usable=usable, winv=winv, p=p, w=w)
    if dense:
        A = np.zeros((3 * T, 3 * T))
        for t in range(T):
            A[3 * t:3 * t + 3, 3 * t:3 * t + 3] = W[t]
        if T >= 3:
            D2 = np.zeros((T - 2, T))
            for r in range(T - 2):
                D2[r, r:r + 3] = (1.0, -2.0, 1.0)
            A += ia2 * np.kron(D2.T @ D2, np.eye(3))
        out["A"] = A
    return out


def banded_to_dense(ab):
    n = ab.shape[1]
    A = np.zeros((n, n))
    for k in range(9):
        off = 8 - k
        i = np.arange(n - off)
        A[i, i + off] = ab[k, off:]
        A[i + off, i] = ab[k, off:]
    return A


def solve(sysd):
    return scipy.linalg.solveh_banded(sysd["ab"], sysd["b"], lower=False).reshape(-1, 3)


def cond(sysd):
    """condition number of the Jacobi-scaled dense matrix"""
    A = sysd["A"] if "A" in sysd else banded_to_dense(sysd["ab"])
    d = 1.0 / np.sqrt(np.diagonal(A))
    return float(np.linalg.cond(A * np.outer(d, d)))


def mahalanobis2(x, sysd):
    d = x - sysd["p"]
    return np.where(sysd["usable"], np.einsum("ta,tab,tb->t", d, sysd["winv"], d), np.nan)


def objective(x, points, cov, accel_std, loss="linear", f_scale=3.0):
    usable, winv, p = prepare(points, cov)
    d = x - p
    d2 = np.einsum("ta,tab,tb->t", d, winv, d)[usable]
    f2 = float(f_scale) ** 2
    pen = np.sum((x[:-2] - 2.0 * x[1:-1] + x[2:]) ** 2) if len(x) >= 3 else 0.0
    return 0.5 * f2 * np.sum(rho(loss, d2 / f2)) + 0.5 / float(accel_std) ** 2 * pen


def irls(points, cov, accel_std, loss="linear", f_scale=3.0, weights_in=None, max_iterations=50, xtol=1e-8):
    """One track.  dict(points, weights, mahalanobis2, status, n_usable, n_iterations, cost, history (n_iterations, 2), last_step, last_xmax)"""
    points, cov = np.asarray(points, dtype=np.float64), np.asarray(cov, dtype=np.float64)
    T = len(points)
    usable = prepare(points, cov)[0]
    nus = int(usable.sum())
    out = dict(points=np.full((T, 3), np.nan), weights=np.zeros(T), mahalanobis2=np.full(T, np.nan), status=STATUS_OK, n_usable=nus, n_iterations=0, cost=np.nan, history=np.zeros((0, 2)),
               last_step=np.inf, last_xmax=np.nan)
    if nus < 2:
        out["status"] = STATUS_TOO_FEW
        return out
    w = None if weights_in is None else np.asarray(weights_in, dtype=np.float64)
    f2 = float(f_scale) ** 2
    hist, xold = [], None
    for it in range(max_iterations):
        s = system(points, cov, accel_std, w, dense=False)
        x = solve(s)
        d2 = mahalanobis2(x, s)
        step = np.inf if it == 0 else float(np.abs(x - xold).max())
        xmax = float(np.abs(x).max())
        hist.append((objective(x, points, cov, accel_std, loss, f_scale), step))
        w = np.where(usable, drho(loss, np.where(usable, d2, 0.0) / f2), 0.0)
        out.update(n_iterations=it + 1, last_step=step, last_xmax=xmax)
        if loss == "linear" or it + 1 >= max_iterations or (it >= 1 and step < xtol * xmax):
            break
        xold = x
    out.update(points=x, weights=w, mahalanobis2=d2, cost=hist[-1][0], history=np.array(hist))
    return out


def smooth(points, cov, accel_std, **kw):
    """every track of (T, K, 3), (T, K, 3, 3): a list of irls() results; weights_in (T, K) if given"""
    points, cov = np.asarray(points, dtype=np.float64), np.asarray(cov, dtype=np.float64)
    K = points.shape[1]
    acc = np.broadcast_to(np.asarray(accel_std, dtype=np.float64), (K,))
    win = kw.pop("weights_in", None)
    return [irls(points[:, k], cov[:, k], acc[k], weights_in=None if win is None else np.asarray(win)[:, k], **kw) for k in range(K)]


def linear_bar(x, x_ref, cnd):
    """(largest error, the bar) of one track"""
    return float(np.abs(x - x_ref).max()), BAR_K * EPS * cnd * float(np.abs(x_ref).max())


# ---------------------------------------------------------------- scenes
def truth(T, K, rng):
    """smooth tracks: a few sinusoids per coordinate, amplitudes of order 10"""
    t = np.arange(T)[:, None, None]
    x = np.zeros((T, K, 3))
    for _ in range(3):
        x = x + rng.uniform(2.0, 6.0, (1, K, 3)) * np.sin(t * rng.uniform(0.01, 0.08, (1, K, 3)) + rng.uniform(0, 6.28, (1, K, 3)))
    return x + rng.uniform(-5, 5, (1, K, 3))


def random_cov(T, K, rng, sigma=0.05, ratio=5.0):
    """anisotropic covariances: standard deviations sigma .. ratio sigma along random axes"""
    A = rng.standard_normal((T, K, 3, 3))
    Q = np.linalg.qr(A)[0]
    s = sigma * rng.uniform(1.0, ratio, (T, K, 3))
    cov = np.einsum("tkab,tkb,tkcb->tkac", Q, s * s, Q)
    return (cov + cov.transpose(0, 1, 3, 2)) / 2


def scene(T, K=1, seed=0, sigma=0.05, ratio=5.0, gaps=(), outliers=0.0, outlier_size=20.0):
    """dict(truth, points, cov, clean (T, K) bool): noise drawn from cov; gaps = [(a, b)] frames made NaN in every track; a share `outliers`
    of the frames of every track displaced by outlier_size in a random direction"""
    rng = np.random.default_rng(seed)
    x = truth(T, K, rng)
    cov = random_cov(T, K, rng, sigma, ratio)
    L = np.linalg.cholesky(cov)
    pts = x + np.einsum("tkab,tkb->tka", L, rng.standard_normal((T, K, 3)))
    clean = np.ones((T, K), bool)
    if outliers > 0:
        for k in range(K):
            idx = rng.choice(T, int(round(outliers * T)), replace=False)
            d = rng.standard_normal((len(idx), 3))
            pts[idx, k] += outlier_size * d / np.linalg.norm(d, axis=1, keepdims=True)
            clean[idx, k] = False
    for a, b in gaps:
        pts[a:b] = np.nan
        clean[a:b] = False
    return dict(truth=x, points=pts, cov=cov, clean=clean)


def outlier_scene():
    """the robust scene: 120 frames, one track, noise of standard deviation 0.66 per coordinate (isotropic), 10 % of the frames displaced by 40;
    seed 7, accel_std 0.05"""
    s = scene(120, 1, seed=7, sigma=0.66, ratio=1.0, outliers=0.10, outlier_size=40.0)
    s["accel_std"] = 0.05
    return s


# ---------------------------------------------------------------- the cases of the host-check and GPU tiers, and what they are held to
def pack6(cov):
    """(.., 3, 3) -> (.., 6) packed 00 01 02 11 12 22"""
    cov = np.asarray(cov, dtype=np.float64)
    return np.ascontiguousarray(np.stack([cov[..., 0, 0], cov[..., 0, 1], cov[..., 0, 2], cov[..., 1, 1], cov[..., 1, 2], cov[..., 2, 2]], axis=-1))


def linear_cases():
    """name -> dict(points (T, K, 3), cov (T, K, 3, 3), accel_std, segment): the smallest shapes at which the elimination can go wrong"""
    cases = {}

    def add(name, s, accel_std, segment):
        cases[name] = dict(points=s["points"], cov=s["cov"], accel_std=accel_std, segment=segment)

    for T in (1, 2, 3, 4, 5):   # odd and phantom, chains shorter than one segment
        add(f"T{T}", scene(T, 1, seed=T), 0.1, 2)
    for seg in (2, 3):          # super-frame counts around the segment: an empty last interior, the last block a separator
        for S in (seg, seg + 1, seg + 2, 2 * seg + 1, 2 * seg + 2):
            add(f"S{S}_seg{seg}", scene(2 * S, 1, seed=10 * seg + S), 0.1, seg)
            add(f"S{S}_odd_seg{seg}", scene(2 * S - 1, 1, seed=100 + 10 * seg + S), 0.1, seg)
    add("T333_seg3", scene(333, 1, seed=3), 0.05, 3)
    add("T333_seg2", scene(333, 1, seed=3), 0.05, 2)    # five levels
    gaps = [(0, 5), (20, 33), (38, 41)]                 # a whole segment and both its separators unusable, both ends missing
    add("gaps_seg2", scene(41, 1, seed=4, gaps=gaps), 0.1, 2)
    add("gaps_seg3", scene(41, 2, seed=5, gaps=gaps), 0.1, 3)
    s = scene(30, 1, seed=6)                            # a covariance that is not positive definite, a NaN covariance: both missing
    s["cov"][7, 0] = np.diag([1.0, 1.0, -1.0]) * 1e-3
    s["cov"][8, 0] = np.array([[1.0, 1.0, 0.0], [1.0, 1.0, 0.0], [0.0, 0.0, 1.0]]) * 1e-3
    s["cov"][15, 0, 1, 1] = np.nan
    add("bad_cov", s, 0.1, 2)
    s = scene(24, 3, seed=8)                            # a track with one usable frame between two good ones
    s["points"][1:, 1] = np.nan
    add("one_usable", s, 0.1, 2)
    add("three_accel", scene(50, 3, seed=9), np.array([0.01, 0.1, 1.0]), 3)
    for e in (-3, -1, 1, 3):                            # accel_std from 1e-3 to 1e3 times the detection noise
        add(f"accel_1e{e}", scene(60, 1, seed=20 + e, sigma=0.05, ratio=2.0), 0.05 * 10.0 ** e, 3)
    add("T400_default", scene(400, 2, seed=11, gaps=[(100, 140)]), 0.05, None)
    add("T400_seg2", scene(400, 2, seed=11, gaps=[(100, 140)]), 0.05, 2)
    return cases


_ref_cache = {}


def linear_reference(name, case):
    """per track (oracle result, cond) of a linear case, computed once"""
    if name not in _ref_cache:
        K = case["points"].shape[1]
        acc = np.broadcast_to(np.asarray(case["accel_std"], dtype=np.float64), (K,))
        refs = []
        for k in range(K):
            o = irls(case["points"][:, k], case["cov"][:, k], acc[k], loss="linear")
            c = cond(system(case["points"][:, k], case["cov"][:, k], acc[k])) if o["status"] == STATUS_OK else np.nan
            refs.append((o, c))
        _ref_cache[name] = refs
    return _ref_cache[name]


def check_linear(name, case, got):
    """got: dict(points (T, K, 3), weights, mahalanobis2 (T, K), status, n_usable, n_iterations (K)).  Returns the largest error / (eps cond max|x|)"""
    worst = 0.0
    for k, (o, c) in enumerate(linear_reference(name, case)):
        assert got["status"][k] == o["status"] and got["n_usable"][k] == o["n_usable"], (name, k, got["status"][k], o["status"], got["n_usable"][k], o["n_usable"])
        if o["status"] != STATUS_OK:
            assert np.isnan(got["points"][:, k]).all() and got["n_iterations"][k] == 0
            continue
        assert got["n_iterations"][k] == 1 and np.isfinite(got["points"][:, k]).all()
        err, bar = linear_bar(got["points"][:, k], o["points"], c)
        ratio = err / (bar / BAR_K)
        worst = max(worst, ratio)
        print(f"{name} track {k}: cond {c:.3g} err {err:.3g} bar {bar:.3g} ratio to eps cond max|x| {ratio:.3g}")
        assert err <= bar, (name, k, err, bar)
        us = prepare(case["points"][:, k], case["cov"][:, k])[0]
        assert np.array_equal(np.isnan(got["mahalanobis2"][:, k]), ~us) and (got["weights"][~us, k] == 0).all() and (got["weights"][us, k] == 1).all()
        assert np.allclose(got["mahalanobis2"][us, k], o["mahalanobis2"][us], rtol=0, atol=1e-6 * max(1.0, np.nanmax(o["mahalanobis2"])) + 100 * EPS * c)
    return worst


def robust_cases():
    """name -> dict(points, cov, accel_std, loss, f_scale, segment): two tracks with noise 0.3 .. 0.9, 8 % of the frames displaced by 15, per seed
    the loss (soft_l1 for an even seed), the length 90 + 7 (seed mod 10) and a gap [30, 36) when the seed is a multiple of 3; and the outlier
    scene.  The seeds are those of 31 .. 74 at which decided() holds for both tracks of the reference itself (13 of 44 do)."""
    cases = {}
    for seed, seg in ((33, 2), (34, 3), (36, None), (43, 2), (62, 3), (72, None)):
        loss = ("soft_l1", "huber")[seed % 2]
        s = scene(90 + 7 * (seed % 10), 2, seed=seed, sigma=0.3, ratio=3.0, outliers=0.08, outlier_size=15.0, gaps=[(30, 36)] if seed % 3 == 0 else [])
        cases[f"{loss}_{seed}"] = dict(points=s["points"], cov=s["cov"], accel_std=0.08, loss=loss, f_scale=3.0, segment=seg)
    o = outlier_scene()
    for loss in ("soft_l1", "huber"):
        cases[f"outlier_{loss}"] = dict(points=o["points"], cov=o["cov"], accel_std=o["accel_std"], loss=loss, f_scale=3.0, segment=2)
    return cases


def robust_reference(name, case, xtol=1e-8, max_iterations=50):
    key = ("robust", name)
    if key not in _ref_cache:
        K = case["points"].shape[1]
        _ref_cache[key] = [irls(case["points"][:, k], case["cov"][:, k], case["accel_std"], loss=case["loss"], f_scale=case["f_scale"], xtol=xtol, max_iterations=max_iterations) for k in range(K)]
    return _ref_cache[key]


def further_step(x, case, k):
    """how far one more IRLS solve moves x (one track): max |x' - x|"""
    pts, cov = case["points"][:, k], case["cov"][:, k]
    s0 = system(pts, cov, case["accel_std"], None, dense=False)
    d2 = mahalanobis2(x, s0)
    w = np.where(s0["usable"], drho(case["loss"], np.where(s0["usable"], d2, 0.0) / case["f_scale"] ** 2), 0.0)
    return float(np.abs(solve(system(pts, cov, case["accel_std"], w, dense=False)) - x).max())


def decided(o, xtol=1e-8):
    """the reference's stopping step is not within a factor 2 of the threshold xtol max |x|, nor the step before it within 1 % of it (a build
    whose steps agree with the reference's to far better than that then stops at the same solve): status and counts are comparable"""
    thr, st = xtol * o["last_xmax"], o["history"][:, 1]
    return not (thr / 2 <= st[-1] <= 2 * thr) and not (len(st) > 1 and thr / 1.01 <= st[-2] <= 1.01 * thr)


def check_robust(name, case, got, xtol=1e-8):
    """got: the result dict with history (max_iterations, K, 2).  Returns the number of tracks left out as undecided"""
    left_out = 0
    f2 = case["f_scale"] ** 2
    for k, o in enumerate(robust_reference(name, case, xtol)):
        x, nit = got["points"][:, k], int(got["n_iterations"][k])
        assert got["status"][k] == STATUS_OK and np.isfinite(x).all()
        s0 = system(case["points"][:, k], case["cov"][:, k], case["accel_std"], got["weights"][:, k])
        cnd = cond(s0)
        us = s0["usable"]
        h = got["history"][:nit, k]
        print(f"{name} track {k}: iterations {nit} (oracle {o['n_iterations']}), cost {h[-1, 0]:.10g} (oracle {o['cost']:.10g}), last step {h[-1, 1]:.3g}, cond {cnd:.3g}")
        assert np.isfinite(h).all() or (np.isinf(h[0, 1]) and np.isfinite(h[1:]).all() and np.isfinite(h[:, 0]).all())
        assert np.isnan(got["history"][nit:, k]).all()
        assert (h[1:, 0] <= h[:-1, 0] * (1.0 + BAR_K * EPS * cnd)).all(), (name, k, h[:, 0])
        assert np.allclose(got["weights"][us, k], drho(case["loss"], got["mahalanobis2"][us, k] / f2), rtol=1e-12, atol=0) and (got["weights"][~us, k] == 0).all()
        assert np.isnan(got["mahalanobis2"][~us, k]).all()
        move = further_step(x, case, k)
        assert move < 10 * xtol * np.abs(x).max(), (name, k, move)
        if decided(o, xtol):
            assert nit == o["n_iterations"] and got["n_usable"][k] == o["n_usable"], (name, k, nit, o["n_iterations"])
        else:
            left_out += 1
    return left_out


# ---------------------------------------------------------------- the level plan and the chunk rule of both trajectory calls
SEGMENT_DEFAULT, MAX_LEVELS = 16, 40
FAC, SEP, X_EXTRA, ZC_EXTRA = 63, 90, 6, 57   # doubles per node: factors; separator planes (levels >= 1); then the solution or the Zd | Zs planes


def plan(T, segment, K):
    """the levels of T frames and K tracks: a list of (n, m, nq, NS), or None past MAX_LEVELS"""
    n, levels = (T + 1) // 2, []
    while True:
        if len(levels) == MAX_LEVELS:
            return None
        m = n if n <= segment + 1 else segment
        nq = (n - 1) // (m + 1) + 1
        levels.append((n, m, nq, (m + 1) * nq * K))
        if m == n:
            return levels
        n //= m + 1


def level_doubles(T, segment, K, extra):
    """the level storage of one chunk: per level NS (FAC + (SEP + extra from level 1 on))"""
    return sum(NS * (FAC + (SEP + extra if l else 0)) for l, (_, _, _, NS) in enumerate(plan(T, segment, K) or []))


def check_carve(levels, extra, offs, total):
    """offs (3 per level: the starts of fac, sep and the extra plane in doubles, -1 for none) tile [0, total) in that order, level after level,
    without gap or overlap: level 0 has fac alone"""
    cur = 0
    for l, (_, _, _, NS) in enumerate(levels):
        fac, sep, aux = (int(v) for v in offs[3 * l:3 * l + 3])
        assert fac == cur, (l, fac, cur)
        cur += NS * FAC
        if l == 0:
            assert sep == -1 and aux == -1
            continue
        assert sep == cur and aux == cur + NS * SEP, (l, sep, aux, cur)
        cur += NS * (SEP + extra)
    assert cur == total, (cur, total)


def chunk_doubles(T, K, segment, kind, lag=False):
    """device doubles (and ints, counted as doubles) one chunk of K tracks needs; kind: "smooth" or "cov" """
    if kind == "smooth":
        return T * K * 24 + K * 8 + 4 * ((T + 255) // 256) * K + level_doubles(T, segment, K, X_EXTRA)
    assert kind == "cov"
    return T * K * (20 + 6 + (9 if lag else 0)) + K * 4 + level_doubles(T, segment, K, ZC_EXTRA)


def expected_chunks(T, K, segment, budget_mb, kind, lag=False):
    """(tracks_per_chunk, chunks, device_bytes, levels) of smooth_trajectories (kind "smooth") or trajectory_uncertainty ("cov") under a
    budget of budget_mb MiB: as many tracks per chunk as fit, at least one, at most K; device_bytes is what the widest chunk takes"""
    segment = segment or SEGMENT_DEFAULT
    per_track = float(chunk_doubles(T, 1, segment, kind, lag)) * 8
    Kc = int(min(float(K), max(1.0, np.floor(budget_mb * 1048576.0 / per_track))))
    return Kc, (K + Kc - 1) // Kc, chunk_doubles(T, Kc, segment, kind, lag) * 8, len(plan(T, segment, Kc))
