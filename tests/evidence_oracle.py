"""The reference of trajectory.trajectory_evidence and trajectory.estimate_accel_std in numpy / scipy over
smoothing_oracle.system.  Per track, with A(a) = blockdiag(w_t Sigma_t^-1) + a^-2 (D2^T D2 (x) I3) and x = A^-1 b,

    N(a) = sum_t w_t d_t^2(x) + a^-2 sum_t |x_{t-1} - 2 x_t + x_{t+1}|^2 + log det A(a) + 6 (T - 2) log a.

Two routes to it: terms_dense (float64: slogdet of the Jacobi-scaled dense matrix plus sum log A_ii) and terms_banded (np.longdouble: a banded
Cholesky factorisation written out here).  The search rule of the C call is mirrored in estimate(); Track.neg2 is the fast float64 evaluation
it uses (scipy's banded Cholesky).

The bars (BAR_K = 4, EPS = 2^-52), per track unless said:
  log det    4 EPS (3 T cond + S), cond of the Jacobi-scaled matrix, S = sum |log A_ii| + sum |2 log l_ii| of the reference's factor: a computed
             Cholesky factor is exact for A + dA, |dA| <~ EPS |A|, and d log det = tr(A^-1 dA);
  data, penalty   the cost bar of section 8f-21 for each, on its own term: 1e-9 max(1, c) + 100 EPS cond c, c = the term;
  N          their sum plus 4 EPS |6 (T - 2) log a|;
  estimate   |log a - log a_oracle| <= rtol + sqrt(4 b / kappa_oracle), b the bar of the unit's N at the estimate: the last bracket is narrower
             than rtol and an error b in N moves a minimum of curvature kappa by at most sqrt(4 b / kappa);
  log_std    kappa is off by at most 4 b / 0.04 through the second difference; log_std = sqrt(2 / kappa) is propagated through that interval;
  N at the estimate   the unit's sum of neg2_log_evidence within b of the oracle's objective at its own estimate.
decided(): the grid argmin counts as decided when the runner-up lies more than twice b above it."""
import numpy as np
import scipy.linalg

import smoothing_oracle as so

EPS, BAR_K = so.EPS, so.BAR_K
INVPHI = 0.6180339887498949
CURV_H = 0.2
LD = np.longdouble


# ---------------------------------------------------------------- one evaluation, two routes
def _terms(x, s, ia2):
    """data, penalty of a solution x (T, 3) in its own precision"""
    d = x - s["p"].astype(x.dtype)
    W = (s["winv"] * s["w"][:, None, None]).astype(x.dtype)
    data = np.einsum("ta,tab,tb->", d, W, d) if x.dtype == np.float64 else sum(d[t] @ (W[t] @ d[t]) for t in range(len(d)))
    sd = x[:-2] - 2 * x[1:-1] + x[2:]
    return data, ia2 * (sd * sd).sum()


def terms_dense(points, cov, a, weights=None):
    """float64, dense: dict(N, data, penalty, log_det, cond, S)"""
    s = so.system(points, cov, a, weights)
    A, T = s["A"], len(s["p"])
    dg = np.diagonal(A)
    j = 1.0 / np.sqrt(dg)
    As = A * np.outer(j, j)
    sign, lds = np.linalg.slogdet(As)
    assert sign > 0
    log_det = lds + np.log(dg).sum()
    x = np.linalg.solve(As, s["b"] * j) * j
    data, pen = _terms(x.reshape(-1, 3), s, 1.0 / float(a) ** 2)
    return dict(N=data + pen + log_det + 6.0 * (T - 2) * np.log(a), data=data, penalty=pen, log_det=log_det, cond=float(np.linalg.cond(As)))


def banded_cholesky_ld(ab):
    """ab: the upper banded form (9, n) of smoothing_oracle.system -> L (n, 9) in np.longdouble, L[i, 8 - (i - j)] = l_ij"""
    n = ab.shape[1]
    L = np.zeros((n, 9), LD)
    abl = ab.astype(LD)
    for i in range(n):
        for j in range(max(0, i - 8), i + 1):
            k0 = max(0, i - 8)
            v = abl[8 - (i - j), i] - (L[i, 8 - (i - k0):8 - (i - j)] * L[j, 8 - (j - k0):8]).sum()
            L[i, 8 - (i - j)] = np.sqrt(v) if i == j else v / L[j, 8]
    return L


def terms_banded(points, cov, a, weights=None):
    """np.longdouble, banded: dict(N, data, penalty, log_det, S) as floats"""
    s = so.system(points, cov, a, weights, dense=False)
    T, n = len(s["p"]), 3 * len(s["p"])
    L = banded_cholesky_ld(s["ab"])
    y = np.zeros(n, LD)
    b = s["b"].astype(LD)
    for i in range(n):
        k0 = max(0, i - 8)
        y[i] = (b[i] - (L[i, 8 - (i - k0):8] * y[k0:i]).sum()) / L[i, 8]
    x = np.zeros(n, LD)
    for i in range(n - 1, -1, -1):
        k1 = min(n - 1, i + 8)
        acc = y[i]
        for r in range(i + 1, k1 + 1):
            acc -= L[r, 8 - (r - i)] * x[r]
        x[i] = acc / L[i, 8]
    ia2 = LD(1.0) / (LD(float(a)) * LD(float(a)))
    data, pen = _terms(x.reshape(-1, 3), s, ia2)
    ll = 2 * np.log(L[:, 8])
    log_det = ll.sum()
    S = float(np.abs(np.log(s["ab"][8])).sum() + np.abs(ll).sum())
    return dict(N=float(data + pen + log_det + 6 * (T - 2) * np.log(LD(float(a)))), data=float(data), penalty=float(pen), log_det=float(log_det), S=S)


def bars(T, a, ref, cnd, S):
    """the bars of one evaluation of one track: dict(log_det, data, penalty, N)"""
    ld = BAR_K * EPS * (3 * T * cnd + S)
    cost = {f: 1e-9 * max(1.0, ref[f]) + 100 * EPS * cnd * ref[f] for f in ("data", "penalty")}
    return dict(log_det=ld, N=ld + cost["data"] + cost["penalty"] + BAR_K * EPS * abs(6.0 * (T - 2) * np.log(a)), **cost)


_ref_cache = {}


def reference(key, points, cov, a, weights=None):
    """the reference of one track at one a, computed once per key: the np.longdouble route, cond of the dense one, the bars"""
    if key not in _ref_cache:
        r = terms_banded(points, cov, a, weights)
        d = terms_dense(points, cov, a, weights)
        r["cond"], r["dense"] = d["cond"], d
        r["bars"] = bars(len(points), a, r, r["cond"], r["S"])
        _ref_cache[key] = r
    return _ref_cache[key]


# ---------------------------------------------------------------- the fast evaluation and the search rule
class Track:
    """one track prepared once: neg2(a) in float64 by scipy's banded Cholesky"""

    def __init__(self, points, cov, weights=None):
        self.points, self.cov, self.weights = points, cov, weights
        s1 = so.system(points, cov, 1.0, weights, dense=False)
        self.T = T = len(points)
        W = s1["winv"] * s1["w"][:, None, None]
        dg, o1, o2 = so.penalty_bands(T)
        self.dat, self.pen = np.zeros((9, 3 * T)), np.zeros((9, 3 * T))   # the two parts of smoothing_oracle.system's ab
        for a in range(3):
            for b in range(a, 3):
                self.dat[8 + a - b, b::3] = W[:, a, b]
            self.pen[8, a::3] = dg
            self.pen[5, 3 + a::3] = o1[:T - 1]
            self.pen[2, 6 + a::3] = o2[:T - 2]
        assert np.array_equal(self.dat + self.pen, s1["ab"])
        self.s = s1
        self.n_usable = int(s1["usable"].sum())
        self.runs = self.n_usable >= 2

    def neg2(self, a):
        ia2 = 1.0 / float(a) ** 2
        ab = self.dat + ia2 * self.pen
        try:
            c = scipy.linalg.cholesky_banded(ab, lower=False)
        except np.linalg.LinAlgError:
            return np.nan
        x = scipy.linalg.cho_solve_banded((c, False), self.s["b"]).reshape(-1, 3)
        data, pen = _terms(x, self.s, ia2)
        return float(data + pen + 2.0 * np.log(c[8]).sum() + 6.0 * (self.T - 2) * np.log(a))


def make_grid(lo, hi, G):
    ul, du = np.log(lo), (np.log(hi) - np.log(lo)) / (G - 1)
    g = np.exp(ul + np.arange(G) * du)
    g[0], g[-1] = lo, hi
    return g


def rounds(lo, hi, G, rtol):
    w, r = 2.0 * (np.log(hi) - np.log(lo)) / (G - 1), 0
    while not w < rtol and r < 200:
        w *= INVPHI
        r += 1
    return r


def search_unit(f, lo, hi, G, rtol, grid):
    """the rule for one unit with objective f(a) (NaN = +inf): dict(a, u, log_std, edge, all_nan, g_star, obj_grid, obj, kappa, evaluate)"""
    inf = np.inf

    def F(a):
        v = f(a)
        return v if v == v else inf

    ul, du = np.log(lo), (np.log(hi) - np.log(lo)) / (G - 1)
    og = np.array([F(a) for a in grid])
    out = dict(obj_grid=og, log_std=np.nan, edge=0, all_nan=False, kappa=np.nan)
    gs = int(np.argmin(og))   # (the first on a tie)
    out["g_star"] = gs
    if not og[gs] < inf:
        out.update(all_nan=True, a=np.nan, u=np.nan, obj=np.nan)
        return out
    if gs in (0, G - 1):
        out.update(edge=-1 if gs == 0 else 1, a=lo if gs == 0 else hi, u=ul + gs * du, obj=og[gs])
        return out
    ub, fb, ab_ = ul + gs * du, og[gs], grid[gs]
    a, b = ul + (gs - 1) * du, ul + (gs + 1) * du
    c, d = b - INVPHI * (b - a), a + INVPHI * (b - a)

    def ev(u):
        nonlocal ub, fb, ab_
        v = F(np.exp(u))
        if v < fb:
            ub, fb, ab_ = u, v, np.exp(u)
        return v

    fc = ev(c)
    fd = ev(d)
    for _ in range(rounds(lo, hi, G, rtol)):
        if fc < fd:
            b, d, fd = d, c, fc
            c = b - INVPHI * (b - a)
            fc = ev(c)
        else:
            a, c, fc = c, d, fd
            d = a + INVPHI * (b - a)
            fd = ev(d)
    fp, fm = F(np.exp(ub + CURV_H)), F(np.exp(ub - CURV_H))
    kappa = (fp - 2.0 * fb + fm) / (CURV_H * CURV_H)
    out.update(a=ab_, u=ub, obj=fb, kappa=kappa, log_std=np.sqrt(2.0 / kappa) if kappa > 0 and np.isfinite(kappa) else np.nan)
    return out


def units_of(pool, K):
    """pool (None, "all" or (K,) labels) -> the unit of every track"""
    if pool is None:
        return np.arange(K)
    if isinstance(pool, str):
        return np.zeros(K, int)
    return np.unique(np.asarray(pool), return_inverse=True)[1].reshape(K)


def estimate(points, cov, accel_range, n_grid=17, rtol=1e-3, weights=None, pool=None, grid=None):
    """every track of (T, K, 3), (T, K, 3, 3): dict(accel_std, log_std, edge, status (K), grid, n_evaluations, units: unit -> (tracks, search_unit
    result), tracks: the Track of every track).  grid: the C call's own, where given"""
    points, cov = np.asarray(points, dtype=np.float64), np.asarray(cov, dtype=np.float64)
    T, K = points.shape[:2]
    lo, hi = accel_range
    grid = make_grid(lo, hi, n_grid) if grid is None else np.asarray(grid)
    tracks = [Track(points[:, k], cov[:, k], None if weights is None else np.asarray(weights)[:, k]) for k in range(K)]
    unit = units_of(pool, K)
    out = dict(accel_std=np.full(K, np.nan), log_std=np.full(K, np.nan), edge=np.zeros(K, int), status=np.array([so.STATUS_OK if t.runs else so.STATUS_TOO_FEW for t in tracks]),
               n_usable=np.array([t.n_usable for t in tracks]), grid=grid, n_evaluations=n_grid + 2 + rounds(lo, hi, n_grid, rtol) + 2, units={}, tracks=tracks)
    for u in np.unique(unit):
        mem = [k for k in range(K) if unit[k] == u and tracks[k].runs]
        if not mem:
            continue

        def f(a, mem=mem):
            s = 0.0
            for k in mem:
                s += tracks[k].neg2(a)
            return s

        r = search_unit(f, lo, hi, n_grid, rtol, grid)
        out["units"][int(u)] = (mem, r)
        for k in mem:
            out["accel_std"][k], out["log_std"][k], out["edge"][k] = r["a"], r["log_std"], r["edge"]
            if r["all_nan"]:
                out["status"][k] = so.STATUS_PIVOT
    return out


def unit_bar(key, points, cov, mem, a, weights=None):
    """b: the bar of a unit's objective at a: the sum of its tracks' N bars"""
    return sum(reference((key, k, float(a)), points[:, k], cov[:, k], a, None if weights is None else np.asarray(weights)[:, k])["bars"]["N"] for k in mem)


def decided(r, b):
    """the grid argmin of a unit: the runner-up lies more than twice the bar above it"""
    og = np.sort(r["obj_grid"])
    return bool(og[1] - og[0] > 2.0 * b)


def estimate_bars(r, b, rtol):
    """(bar of log a, (lowest, highest) log_std allowed) of a unit with the search result r and N bar b"""
    if r["edge"] or r["all_nan"] or not r["kappa"] > 0:
        return 0.0, (np.nan, np.nan)
    dk = 4.0 * b / (CURV_H * CURV_H)
    hi = np.sqrt(2.0 / (r["kappa"] - dk)) if r["kappa"] - dk > 0 else np.inf
    return rtol + np.sqrt(4.0 * b / r["kappa"]), (np.sqrt(2.0 / (r["kappa"] + dk)), hi)


# ---------------------------------------------------------------- scenes
def matched_scene(T, K, a, seed, sigma=0.05, ratio=5.0, gap=None):
    """tracks whose second differences are drawn as N(0, a^2) per coordinate, anisotropic covariances, noise drawn from them; gap = (t0, t1) NaN"""
    rng = np.random.default_rng(seed)
    x = np.zeros((T, K, 3))
    x[0] = rng.uniform(-5, 5, (K, 3))
    x[1] = x[0] + rng.normal(0, 0.1, (K, 3))
    for t in range(2, T):
        x[t] = 2 * x[t - 1] - x[t - 2] + a * rng.standard_normal((K, 3))
    cov = so.random_cov(T, K, rng, sigma, ratio)
    pts = x + np.einsum("tkab,tkb->tka", np.linalg.cholesky(cov), rng.standard_normal((T, K, 3)))
    if gap:
        pts[gap[0]:gap[1]] = np.nan
    return dict(truth=x, points=pts, cov=cov)


def linear_scene(T, seed, sigma=0.05):
    """one track exactly linear in time plus noise: the evidence falls towards a = 0 and the minimum lies on the lower edge"""
    rng = np.random.default_rng(seed)
    x = (rng.uniform(-5, 5, (1, 1, 3)) + np.arange(T)[:, None, None] * rng.uniform(-0.2, 0.2, (1, 1, 3)))
    cov = so.random_cov(T, 1, rng, sigma, 2.0)
    return dict(points=x + np.einsum("tkab,tkb->tka", np.linalg.cholesky(cov), rng.standard_normal((T, 1, 3))), cov=cov)


A_TRUE = 0.1
RANGE = (0.005, 2.0)
EVAL_AT = (0.005, 0.1, 2.0)   # three values of a spanning the grid


def cases():
    """name -> dict(points (T, K, 3), cov, segment, weights or None): the shapes of the host-check and GPU tiers.  blocks n = ceil(T / 2)"""
    out = {}

    def add(name, s, segment=2, weights=None):
        out[name] = dict(points=s["points"], cov=s["cov"], segment=segment, weights=weights)

    for T in (3, 4, 7, 11, 12, 13):   # one level and a phantom frame; n = 2; a second segment of one block; n = 6: the last segment is empty; n = 7
        add(f"T{T}", matched_scene(T, 1, A_TRUE, seed=T))
    add("T257_seg3", matched_scene(257, 1, A_TRUE, seed=257), segment=3)   # several levels
    s = matched_scene(71, 5, A_TRUE, seed=71, gap=(30, 37))
    s["points"][1:, 3] = np.nan                                           # a track with a single usable frame
    w = np.ones((71, 5))
    w[np.random.default_rng(5).random((71, 5)) < 0.15] = 0.0
    w[10:14, 1] = 0.5
    add("T71_K5", s, weights=w)
    s = matched_scene(9, 67, A_TRUE, seed=67)                             # crosses a wavefront; tracks 30 and 31 do not run: `list` is not dense
    s["points"][:, 30] = np.nan                                           # no usable frame
    s["points"][1:, 31] = np.nan                                          # one
    s["points"][2:, 32] = np.nan                                          # two: the fewest with which a track runs
    add("K67", s)
    return out


def check_evaluation(name, case, a, got):
    """got: dict(neg2_log_evidence, data, penalty, log_det, status, n_usable (K)) at accel_std a.  Returns the largest fraction of a bar"""
    pts, cov, w = case["points"], case["cov"], case["weights"]
    T, K = pts.shape[:2]
    worst = 0.0
    for k in range(K):
        wk = None if w is None else w[:, k]
        nus = int(so.prepare(pts[:, k], cov[:, k])[0].sum())
        assert got["n_usable"][k] == nus, (name, k)
        if nus < 2:
            assert got["status"][k] == so.STATUS_TOO_FEW and all(np.isnan(got[f][k]) for f in ("neg2_log_evidence", "data", "penalty", "log_det")), (name, k)
            continue
        assert got["status"][k] == so.STATUS_OK, (name, k, got["status"][k])
        r = reference((name, k, float(a)), pts[:, k], cov[:, k], a, wk)
        for f, bar in (("log_det", r["bars"]["log_det"]), ("data", r["bars"]["data"]), ("penalty", r["bars"]["penalty"]), ("neg2_log_evidence", r["bars"]["N"])):
            ref = r["N"] if f == "neg2_log_evidence" else r[f]
            err = abs(got[f][k] - ref)
            worst = max(worst, err / bar)
            assert np.isfinite(got[f][k]) and err <= bar, (name, k, a, f, got[f][k], ref, err, bar)
    return worst


def check_estimate(name, case, got, accel_range, n_grid, rtol, pool=None):
    """got: dict(accel_std, log_std, edge, status, n_usable, neg2_log_evidence (K), grid, neg2_log_evidence_grid (G, K), n_evaluations).  Returns (undecided units,
    units, the largest fraction of the bar of log a, of the log_std interval)"""
    pts, cov, w = case["points"], case["cov"], case["weights"]
    o = estimate(pts, cov, accel_range, n_grid, rtol, w, pool, grid=got["grid"])
    assert np.allclose(got["grid"], make_grid(accel_range[0], accel_range[1], n_grid), rtol=4 * EPS, atol=0)
    assert got["n_evaluations"] == o["n_evaluations"], (got["n_evaluations"], o["n_evaluations"])
    assert np.array_equal(got["status"], o["status"]) and np.array_equal(got["n_usable"], o["n_usable"]), (name, got["status"], o["status"])
    undecided, worst_a, worst_s = 0, 0.0, 0.0
    for u, (mem, r) in o["units"].items():
        b = unit_bar(name, pts, cov, mem, r["a"], w)
        if not decided(r, b):
            undecided += 1
            continue
        gobj = np.where(np.isnan(got["neg2_log_evidence_grid"][:, mem]), np.inf, got["neg2_log_evidence_grid"][:, mem]).sum(axis=1)
        assert int(np.argmin(gobj)) == r["g_star"], (name, u)
        for k in mem:
            assert got["edge"][k] == r["edge"], (name, k)
            assert got["accel_std"][k] == got["accel_std"][mem[0]] and (got["log_std"][k] == got["log_std"][mem[0]] or np.isnan(got["log_std"][mem[0]]))
        en = abs(got["neg2_log_evidence"][mem].sum() - r["obj"])
        assert en <= b, (name, u, en, b)
        if r["edge"]:
            assert got["accel_std"][mem[0]] == accel_range[0 if r["edge"] < 0 else 1] and np.isnan(got["log_std"][mem[0]])
            continue
        du, (slo, shi) = estimate_bars(r, b, rtol)
        ea = abs(np.log(got["accel_std"][mem[0]]) - np.log(r["a"]))
        worst_a = max(worst_a, ea / du)
        assert ea <= du, (name, u, ea, du)
        ls = got["log_std"][mem[0]]
        print(f"{name} unit {u}: a {got['accel_std'][mem[0]]:.6g} (oracle {r['a']:.6g}, bar of log a {du:.3g}), log_std {ls:.6g} (oracle {r['log_std']:.6g}, allowed {slo:.6g} .. {shi:.6g})")
        assert slo <= ls <= shi, (name, u, ls, slo, shi)
        worst_s = max(worst_s, abs(ls - r["log_std"]) / max(r["log_std"] - slo, min(shi, 1e300) - r["log_std"]))
    return undecided, len(o["units"]), worst_a, worst_s
