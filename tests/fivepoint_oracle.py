"""Numpy statement of the five-point hypothesis generator of the two-view RANSAC, the checker of the host build
(tests/test_hostcheck_fivepoint.py) and of the GPU tier (tests/test_gpu_fivepoint.py).  Prepare, score, winner and vote are
tests/twoview_oracle.py's; only the generator is new.

Stages, each a function here:
  null_space    the 5 x 9 matrix of rows kron([x_b, 1], [x_a, 1]) (np.linalg.svd): sigma, and the orthonormal basis of its null space turned
                inside the subspace into the canonical one -- W, Z, Y, X = Gram-Schmidt of the subspace's coordinates of the entries E33, E32,
                E31, E23, each with a positive pivot -- so that the roots (which depend on the basis) have an order both sides can agree on
  constraints   E = x X + y Y + z Z + W; det E and the nine entries of 2 E E^T E - tr(E E^T) E as a 10 x 20 matrix over the monomials of
                degree <= 3, in either monomial order
  roots         route "action": Gauss-Jordan on the cubic block in degree-lex order, the 10 x 10 action matrix of multiplication by x
                on (x^2, xy, xz, y^2, yz, z^2, x, y, z, 1), np.linalg.eig; a real eigenvalue's eigenvector is the solution
                route "poly":   Nister's order, rows x^2 z - z x^2, y^2 z - z y^2, xyz - z xy give B(z) (x, y, 1)^T = 0 with entries of degree
                3, 3, 4; det B is the degree-10 polynomial in z (np.roots); (x, y) from the largest cross product of B(z)'s rows; Gauss-Newton
                on the ten cubics themselves (polish); a second pass with x for the hidden variable, the union of the two (roots_poly says why)
  candidates    per real solution E projected onto singular values (1, 1, 0), |E|_F = sqrt 2, sign-canonical; ascending z
  compaction    the live slots of the (H, 10) table in index order

A candidate is comparable when cond(cubic block) x kappa <= 1e8 (kappa = 1 / |y^H x| of its eigenvalue of the action matrix), no complex pair
of its sample has |imag| < 1e-6 max(1, |root|) (such a sample's real-root count is undecided: it is left out whole) and the sample is not void.
Tolerance of E, per entry: K5 EPS (cond x kappa + sigma_1 / sigma_5).  K5 is 8 x the worst multiple of EPS (cond kappa + sigma_1 / sigma_5)
between the two routes over the comparable candidates of the test cases ("thin3" and "thin6" pairs (0, 1) and (1, 2), "three" pair (0, 1); 64 and
512 samples, seed 0), and at least 64.  Measured (tests/test_fivepoint_oracle_cpu.py prints it): worst multiple 528.3 ("thin6" (0, 1), 512 samples;
the others 0.94 to 147), so K5 = 8 x 529 = 4232.  The multiple is that large because the bound's first term is a first-order statement about ONE
eigenvalue of the action matrix, and the eigenvector -- which is what gives y and z -- can be worse conditioned than it; the comparable
candidates left out are at most 0.13 % of a case (3 of 2380, "thin3" (1, 2), 512 samples), none of them by a near-real pair."""
import numpy as np

import keypoint_scenes as ks
import thin_scenes as ts
import twoview_oracle as tvo

EPS = tvo.EPS
K5_MEASURED = 529.0             # the worst multiple between the two routes (module docstring; test_fivepoint_oracle_cpu.test_case_rules prints it)
K5 = max(64.0, 8 * K5_MEASURED)
COND_KAPPA_MAX = 1e8
NEAR_REAL = 1e-6
SLOTS = 10
# the floors of csrc/mcba_fivepoint_math.h (FP_RANK_MIN, FP_PIVOT_MIN), restated: a sample below either is void
RANK_MIN, PIVOT_MIN = 1e-7, 1e-9

# exponents (a, b, c) of x^a y^b z^c
NISTER = [(3, 0, 0), (0, 3, 0), (2, 1, 0), (1, 2, 0), (2, 0, 1), (2, 0, 0), (0, 2, 1), (0, 2, 0), (1, 1, 1), (1, 1, 0),
          (1, 0, 2), (1, 0, 1), (1, 0, 0), (0, 1, 2), (0, 1, 1), (0, 1, 0), (0, 0, 3), (0, 0, 2), (0, 0, 1), (0, 0, 0)]
DEGLEX = [(3, 0, 0), (2, 1, 0), (2, 0, 1), (1, 2, 0), (1, 1, 1), (1, 0, 2), (0, 3, 0), (0, 2, 1), (0, 1, 2), (0, 0, 3),
          (2, 0, 0), (1, 1, 0), (1, 0, 1), (0, 2, 0), (0, 1, 1), (0, 0, 2), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]


def draw_samples(M, H, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.choice(M, 5, replace=False) for _ in range(H)]).astype(np.int32)


def pair_of(name, a=0, b=1):
    """twoview_oracle.pair_of over the thin scenes as well"""
    if name in ts.SCENES:
        uvs, _, intr, _ = ts.make(name)
        idx = tvo.common_points(np.asarray(uvs[a]), np.asarray(uvs[b]))
        return np.ascontiguousarray(uvs[a][idx]), np.ascontiguousarray(uvs[b][idx]), intr[a], intr[b], idx, ts.make(name)
    return tvo.pair_of(name, a, b)


def true_essential(sc, a, b):
    """the essential matrix of the scene's own extrinsics, |E|_F = sqrt 2"""
    ext = sc[1]
    Ra, Rb = ks.rodrigues(ext[a][:3]), ks.rodrigues(ext[b][:3])
    R = Rb @ Ra.T
    t = ext[b][3:] - R @ ext[a][3:]
    E = tvo.skew(t / np.linalg.norm(t)) @ R
    return E * np.sqrt(2.0) / np.linalg.norm(E)


def dE(E, E_true):
    E = np.asarray(E).reshape(3, 3)
    E = E * np.sqrt(2.0) / np.linalg.norm(E)
    return min(np.linalg.norm(E - E_true), np.linalg.norm(E + E_true))


# ---------------------------------------------------------------- null space
def epipolar_rows(xa, xb):
    a, b = np.c_[xa, np.ones(len(xa))], np.c_[xb, np.ones(len(xb))]
    return (b[:, :, None] * a[:, None, :]).reshape(len(a), 9)


def canonical_basis(N):
    """N (4, 9) orthonormal rows -> (X, Y, Z, W) (4, 9): the same subspace; W, Z, Y, X from columns 8, 7, 6, 5 by Gram-Schmidt"""
    C = N[:, [8, 7, 6, 5]]
    Q, R = np.linalg.qr(C)
    Q = Q * np.where(np.diag(R) < 0, -1.0, 1.0)
    B = Q.T @ N            # rows W, Z, Y, X
    return B[::-1]


def null_space(xa, xb):
    """(basis (4, 9): rows X, Y, Z, W; sigma (5,)) of five correspondences in normalised coordinates"""
    A = epipolar_rows(np.asarray(xa, dtype=np.float64), np.asarray(xb, dtype=np.float64))
    if not np.isfinite(A).all():
        return np.full((4, 9), np.nan), np.zeros(5)
    _, s, Vt = np.linalg.svd(A, full_matrices=True)
    if not s[4] > 0:
        return np.full((4, 9), np.nan), s
    return canonical_basis(Vt[5:]), s


# ---------------------------------------------------------------- constraints
# Polynomials in the homogeneous variables (x, y, z, 1) = 0 .. 3: a linear one is 4 numbers, a quadratic one 10 (the pairs i <= j), a cubic one 20
# (the triples, held in NISTER's order).  The index tables come from the exponents, not from a listing.
_PAIRS = [(i, j) for i in range(4) for j in range(i, 4)]
_Q2 = np.array([[_PAIRS.index((min(i, j), max(i, j))) for j in range(4)] for i in range(4)])
_T3 = np.array([[NISTER.index(tuple([i, j, v].count(k) for k in range(3))) for v in range(4)] for i, j in _PAIRS])
_TO_DEGLEX = np.array([NISTER.index(e) for e in DEGLEX])
_SWAP_XZ = np.array([NISTER.index((c, b, a)) for a, b, c in NISTER])


def _mul11(a, b):
    return np.bincount(_Q2.ravel(), weights=np.outer(a, b).ravel(), minlength=10)


def _mul21(a, b):
    return np.bincount(_T3.ravel(), weights=np.outer(a, b).ravel(), minlength=20)


_cm_cache = {}


def constraint_matrix(basis, order):
    """the ten cubics -- det E first, then 2 E E^T E - tr(E E^T) E row-major -- as a (10, 20) matrix over the monomials in `order`"""
    key = np.asarray(basis).tobytes()
    if key not in _cm_cache:
        if len(_cm_cache) > 4096:
            _cm_cache.clear()
        E = np.asarray(basis).T.reshape(3, 3, 4)
        G = np.array([[sum(_mul11(E[i, k], E[j, k]) for k in range(3)) for j in range(3)] for i in range(3)])
        L = 2.0 * G
        for i in range(3):
            L[i, i] -= G[0, 0] + G[1, 1] + G[2, 2]
        rows = [_mul21(_mul11(E[0, 1], E[1, 2]) - _mul11(E[0, 2], E[1, 1]), E[2, 0]) + _mul21(_mul11(E[0, 2], E[1, 0]) - _mul11(E[0, 0], E[1, 2]), E[2, 1])
                + _mul21(_mul11(E[0, 0], E[1, 1]) - _mul11(E[0, 1], E[1, 0]), E[2, 2])]
        rows += [sum(_mul21(L[i, k], E[k, j]) for k in range(3)) for i in range(3) for j in range(3)]
        _cm_cache[key] = np.array(rows)
    M = _cm_cache[key]
    return M if order is NISTER else M[:, _TO_DEGLEX]


# ---------------------------------------------------------------- roots
def roots_action(basis):
    """dict(xyz (n, 3) of the real solutions in ascending z, kappa (n), cond, near_real: a complex pair that close to the axis, pivot_ok)"""
    M = constraint_matrix(basis, DEGLEX)
    cond = np.linalg.cond(M[:, :10])
    if not np.isfinite(cond) or cond > 1e15:
        return dict(xyz=np.zeros((0, 3)), kappa=np.zeros(0), cond=np.inf, near_real=True)
    B = np.linalg.solve(M[:, :10], M[:, 10:])
    A = np.zeros((10, 10))
    A[:6] = -B[:6]
    A[6, 0] = A[7, 1] = A[8, 2] = A[9, 6] = 1.0
    w, V = np.linalg.eig(A)
    Vi = np.linalg.inv(V)
    kap = np.linalg.norm(Vi, axis=1) * np.linalg.norm(V, axis=0)
    real = w.imag == 0
    near = bool((np.abs(w.imag[~real]) < NEAR_REAL * np.maximum(1.0, np.abs(w[~real]))).any())
    v = V[:, real].real
    xyz = (v[6:9] / v[9]).T
    k = kap[real]
    o = np.argsort(xyz[:, 2], kind="stable")
    return dict(xyz=xyz[o], kappa=k[o], cond=float(cond), near_real=near)


def gauss_jordan(M):
    """(the reduced matrix, the smallest |pivot| over the largest |entry| of the cubic block as it came): partial pivoting, as the header does it"""
    M = np.array(M, dtype=np.float64)
    mx, worst = np.abs(M[:, :10]).max(), np.inf
    for k in range(10):
        p = k + int(np.argmax(np.abs(M[k:, k])))
        M[[k, p]] = M[[p, k]]
        worst = min(worst, abs(M[k, k]))
        M[k] /= M[k, k]
        for r in range(10):
            if r != k:
                M[r] -= M[r, k] * M[k]
    return M, (worst / mx if mx > 0 and np.isfinite(mx) and np.isfinite(worst) else 0.0)


def nister_polys(basis):
    """B (3, 3) of coefficient arrays, highest power first: rows (x^2z) - z (x^2), (y^2z) - z (y^2), (xyz) - z (xy) of the reduced matrix"""
    R = gauss_jordan(constraint_matrix(basis, NISTER))[0][:, 10:]      # rows e .. j are 4 .. 9
    B = []
    for r in (4, 6, 8):
        e, f = R[r], R[r + 1]
        bx = np.array([-f[0], e[0] - f[1], e[1] - f[2], e[2]])
        by = np.array([-f[3], e[3] - f[4], e[4] - f[5], e[5]])
        b1 = np.array([-f[6], e[6] - f[7], e[7] - f[8], e[8] - f[9], e[9]])
        B.append((bx, by, b1))
    return B


def _roots_hidden(basis):
    """the real solutions by the degree-10 polynomial in the third coordinate of this basis, polished: [(xyz, relative residual)]"""
    B = nister_polys(basis)
    p1 = np.polysub(np.polymul(B[0][1], B[1][2]), np.polymul(B[0][2], B[1][1]))
    p2 = np.polysub(np.polymul(B[0][2], B[1][0]), np.polymul(B[0][0], B[1][2]))
    p3 = np.polysub(np.polymul(B[0][0], B[1][1]), np.polymul(B[0][1], B[1][0]))
    det = np.polyadd(np.polyadd(np.polymul(p1, B[2][0]), np.polymul(p2, B[2][1])), np.polymul(p3, B[2][2]))
    r = np.roots(det)
    z = np.sort(r[r.imag == 0].real)
    d = np.polyder(det)
    for _ in range(3):           # Newton on the polynomial itself: np.roots is backward stable for the companion matrix, not for the roots
        z = z - np.polyval(det, z) / np.polyval(d, z)
    M = constraint_matrix(basis, NISTER)
    out = []
    for zk in np.sort(z):        # the null vector of B(z): the largest of the three cross products of its rows
        Bz = np.array([[np.polyval(B[i][j], zk) for j in range(3)] for i in range(3)])
        n = max((np.cross(Bz[i], Bz[j]) for i, j in ((0, 1), (0, 2), (1, 2))), key=lambda c: c @ c)
        with np.errstate(all="ignore"):
            out.append(polish(M, NISTER, [n[0] / n[2], n[1] / n[2], zk]))
    return out


def roots_poly(basis):
    """xyz (n, 3) of the real solutions in ascending z: the union of two passes, the hidden variable z, then x (X and Z exchanged) -- solutions
    whose z nearly coincide are a cluster of roots of the one polynomial and far apart in the other.  A polished point counts when its residual is
    below RESIDUAL_MAX of the magnitude of the cubics' terms; two are the same solution within SAME (1 + the largest coordinate)."""
    sols = []
    for p in (0, 1):
        bp = basis if p == 0 else basis[[2, 1, 0, 3]]
        if p == 1 and gauss_jordan(constraint_matrix(bp, NISTER))[1] < PIVOT_MIN:
            continue
        for v, rel in _roots_hidden(bp):
            v = v if p == 0 else v[[2, 1, 0]]
            if not rel <= RESIDUAL_MAX or not np.isfinite(v).all():
                continue
            if any(np.abs(v - s).max() <= SAME * (1 + np.abs(s).max()) for s in sols) or len(sols) == SLOTS:
                continue
            sols.append(v)
    sols.sort(key=lambda v: v[2])
    return np.array(sols).reshape(len(sols), 3)


RESIDUAL_MAX, SAME = 1e-6, 1e-6
POLISH_STEPS = 6


def polish(M, order, xyz, steps=POLISH_STEPS):
    """(xyz, residual over the magnitude of the terms): Gauss-Newton on the ten cubics themselves from a root of the univariate polynomial -- two
    solutions with nearly the same z are an ill-conditioned pair of roots of that polynomial and a well-conditioned pair of solutions of the system"""
    ex = np.array(order)

    def at(v):
        pw = np.stack([v ** 0, v, v ** 2, v ** 3])                  # (4, 3): powers of x, y, z
        dp = np.stack([0 * v, v ** 0, 2 * v, 3 * v ** 2])
        m = pw[ex[:, 0], 0] * pw[ex[:, 1], 1] * pw[ex[:, 2], 2]
        J = np.stack([dp[ex[:, 0], 0] * pw[ex[:, 1], 1] * pw[ex[:, 2], 2], pw[ex[:, 0], 0] * dp[ex[:, 1], 1] * pw[ex[:, 2], 2], pw[ex[:, 0], 0] * pw[ex[:, 1], 1] * dp[ex[:, 2], 2]], axis=1)
        return M @ J, M @ m

    v = np.array(xyz, dtype=np.float64)
    A, r = at(v)
    for _ in range(steps):           # a step that does not lower the residual is not taken, and nothing moves after it
        with np.errstate(all="ignore"):
            try:
                w = v - np.linalg.solve(A.T @ A, A.T @ r)
            except np.linalg.LinAlgError:
                break
            A2, r2 = at(w)
        if not r2 @ r2 < r @ r:
            break
        v, A, r = w, A2, r2
    pw = np.stack([v ** 0, v, v ** 2, v ** 3])
    mag = np.abs(M * (pw[ex[:, 0], 0] * pw[ex[:, 1], 1] * pw[ex[:, 2], 2])).sum(1)
    return v, float(np.sqrt((r @ r) / (mag @ mag)))


# ---------------------------------------------------------------- candidates
def essential_of(basis, xyz):
    e = xyz[0] * basis[0] + xyz[1] * basis[1] + xyz[2] * basis[2] + basis[3]
    U, s, Vt = np.linalg.svd(e.reshape(3, 3))
    return tvo.canonical_sign(U @ np.diag([1.0, 1.0, 0.0]) @ Vt).ravel()


def candidates(xa, xb, route="action"):
    """dict(E (n, 9) in ascending z, comparable (n) bool, tol (n), void, undecided, sigma_ratio, cond) of one sample"""
    basis, s = null_space(xa, xb)
    out = dict(E=np.zeros((0, 9)), comparable=np.zeros(0, bool), tol=np.zeros(0), void=True, undecided=False, sigma_ratio=0.0, pivot=0.0, cond=np.inf, z=np.zeros(0))
    if not np.isfinite(basis).all():
        return out
    out["sigma_ratio"] = float(s[4] / s[0])
    if out["sigma_ratio"] < RANK_MIN:
        return out
    ra = roots_action(basis)
    out["pivot"] = gauss_jordan(constraint_matrix(basis, NISTER))[1]
    if out["pivot"] < PIVOT_MIN:
        return out
    if not np.isfinite(ra["cond"]):      # the degree-lex cubic block is singular: no action matrix; the polynomial's roots stand in, nothing is comparable
        route, ra = "poly", dict(ra, xyz=np.zeros((0, 3)), kappa=np.zeros(0))
    xyz = ra["xyz"] if route == "action" else roots_poly(basis)
    n = len(xyz)
    ck = ra["cond"] * ra["kappa"]
    out.update(void=False, undecided=ra["near_real"] or len(ra["xyz"]) != n, cond=ra["cond"], z=xyz[:, 2])
    out["E"] = np.array([essential_of(basis, r) for r in xyz]).reshape(n, 9)
    if len(ra["xyz"]) == n:
        out["comparable"] = (ck <= COND_KAPPA_MAX) & (not out["undecided"])
        out["tol"] = K5 * EPS * (ck + s[0] / s[4])
    else:
        out["comparable"], out["tol"] = np.zeros(n, bool), np.full(n, np.inf)
    return out


def hypotheses(prep, samples, route="action"):
    """per sample the candidates() dict, and the packed table: dict(per_sample, E (n, 9), status (n) = 1, slot_of (n) = 10 sample + slot, ill (n), tol (n))"""
    per = [candidates(prep["na"][s], prep["nb"][s], route) for s in samples]
    E = np.concatenate([c["E"] for c in per]) if per else np.zeros((0, 9))
    slot_of = np.concatenate([SLOTS * h + np.arange(len(c["E"])) for h, c in enumerate(per)]).astype(np.int64)
    ill = np.concatenate([~c["comparable"] for c in per])
    tol = np.concatenate([c["tol"] for c in per])
    return dict(per_sample=per, E=E, status=np.ones(len(E), np.int32), slot_of=slot_of, ill=ill, tol=tol, gap_A=np.ones(len(E)), gap_E=np.ones(len(E)))


def compaction(status10):
    """the live slots of an (H, 10) status table in index order: the map packed index -> 10 sample + slot"""
    return np.flatnonzero(np.asarray(status10).ravel() == 1)


def route_multiple(prep, samples):
    """(worst |E_action - E_poly| over EPS (cond kappa + sigma_1 / sigma_5) among the comparable candidates, their number, the real candidates)"""
    worst, n_cmp, n_all = 0.0, 0, 0
    for s in samples:
        a, b = candidates(prep["na"][s], prep["nb"][s], "action"), candidates(prep["na"][s], prep["nb"][s], "poly")
        n_all += len(a["E"])
        if a["void"] or a["undecided"] or len(a["E"]) != len(b["E"]):
            continue
        ok = a["comparable"]
        n_cmp += int(ok.sum())
        if ok.any():
            worst = max(worst, float((np.abs(a["E"] - b["E"]).max(1)[ok] / (a["tol"][ok] / K5)).max()))
    return worst, n_cmp, n_all


# ---------------------------------------------------------------- the whole generator + twoview_oracle's stages
def two_view5(uv_a, uv_b, intr_a, intr_b, samples, threshold, iterations=5):
    """twoview_oracle.two_view with the five-point generator: the same keys; hyp is hypotheses()'s packed table, winner an index into it,
    sample and slot the winner's place in the (H, 10) table"""
    prep = tvo.prepare(uv_a, uv_b, intr_a, intr_b, iterations)
    hyp = hypotheses(prep, samples)
    if len(hyp["E"]) == 0:
        return dict(prep=prep, hyp=hyp, winner=0, comparable=False, n_inliers=0)
    sc = tvo.score(hyp["E"], hyp["status"], prep, intr_a, intr_b, threshold)
    w, comparable = tvo.winner_comparable(sc, hyp)
    out = dict(prep=prep, hyp=hyp, score=sc, winner=w, comparable=comparable, inliers=sc["inlier"][w], n_inliers=int(sc["count"][w]), cost=float(sc["cost"][w]),
               sample=int(hyp["slot_of"][w] // SLOTS), slot=int(hyp["slot_of"][w] % SLOTS))
    v = tvo.vote(hyp["E"][w], prep, sc["inlier"][w])
    out.update(vote=v, rt12=v["Rt"][v["best"]], points=v["points"], n_in_front=int(v["in_front"][v["best"]]))
    return out


# ---------------------------------------------------------------- the checker the host tier and the GPU tier share
def check_candidates(label, E10, status10, o):
    """E10 (H, 10, 9) and status10 (H, 10) of a generator against hypotheses(): every comparable oracle candidate has exactly one live candidate of
    its sample within the bound, in the same order; every live candidate lies within the bound of some oracle root of its sample; live slots are
    the leading ones; an undecided sample is left out whole.  Prints the worst error / tolerance and what was left out before it asserts."""
    per = o["hyp"]["per_sample"]
    E10, status10 = np.asarray(E10).reshape(len(per), SLOTS, 9), np.asarray(status10).reshape(len(per), SLOTS)
    worst, n_cmp, n_real, n_out = 0.0, 0, 0, 0
    for h, c in enumerate(per):
        live = status10[h] == 1
        n = int(live.sum())
        assert live[:n].all() and np.isnan(E10[h][~live]).all() and (status10[h][~live] == -1).all(), h
        n_real += len(c["E"])
        if c["void"]:
            assert n == 0, h
            continue
        if c["undecided"]:
            n_out += len(c["E"])
            continue
        d = np.abs(E10[h][:n, None, :] - c["E"][None, :, :]).max(2) if n else np.zeros((0, len(c["E"])))     # (kernel, oracle)
        within = d <= c["tol"][None, :]
        last = -1
        for i in np.flatnonzero(c["comparable"]):
            hit = np.flatnonzero(within[:, i])
            assert len(hit) == 1 and hit[0] > last, (h, i, d[:, i], c["tol"][i])
            last = hit[0]
            worst = max(worst, d[hit[0], i] / c["tol"][i])
            n_cmp += 1
        n_out += int((~c["comparable"]).sum())
        loose = np.maximum(c["tol"], 1e-6)           # a root that is not comparable still has to be there
        assert ((d <= loose[None, :]).any(1)).all() and n <= len(c["E"]), (h, d)
    print(f"{label}: {n_real} real candidates, {n_cmp} compared, {n_out} left out; E error / tolerance {worst:.3g}")
    assert n_out <= 0.05 * max(n_real, 1)
    assert worst <= 1
