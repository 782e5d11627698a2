"""The reference of trajectory.trajectory_uncertainty in numpy, on the system, the scenes and the cases of
tests/smoothing_oracle.py: per track Z = A^-1 of exactly the smoother's matrix A = blockdiag(w_t Sigma_t^-1) + a^-2 (D2^T D2 (x) I3), of which
the library returns Z_tt (every frame, unusable ones included) and on request Z_{t,t+1}.

Reference: Zhat = inv(Ahat), Ahat the Jacobi-scaled dense matrix, unscaled afterwards.  A second route checks it: a banded Cholesky
factorisation and the band of the inverse in np.longdouble.

The bar (per track, over all entries of Z_tt and, where asked, Z_{t,t+1}) is the linear solve's own bar applied to the unit right-hand sides in
Jacobi-scaled units:  |zhat - zhat_ref| <= BAR_K eps cond(Ahat) max|zhat_ref|,  zhat_ab = Z_ab sqrt(A_aa A_bb).  The largest entry of an SPD
inverse is on its diagonal, so the maximum over the compared entries is the maximum of the matrix.

selinv_transcription() is the library's recursion in numpy (6 x 6 super-frame blocks, separators, every level), for the CPU tier."""
import numpy as np

import smoothing_oracle as so

EPS, BAR_K = so.EPS, so.BAR_K
ROUTES_AGREE = 0.25   # of the bar: the two reference routes


def band_of(Z, T):
    """(Z_tt (T, 3, 3), Z_{t,t+1} (T - 1, 3, 3)) of a dense (3 T, 3 T) matrix"""
    B = Z.reshape(T, 3, T, 3)
    t = np.arange(T)
    return B[t, :, t, :].copy(), B[t[:-1], :, t[1:], :].copy()


def reference(points, cov, accel_std, weights=None):
    """One track: dict(diag (T, 3, 3), lag (T - 1, 3, 3), s (3 T,) = sqrt(diag A), cond, zmax = max|zhat_ref|, A, usable)"""
    sysd = so.system(points, cov, accel_std, weights)
    A = sysd["A"]
    T = len(points)
    s = np.sqrt(np.diagonal(A))
    Ah = A / np.outer(s, s)
    Zh = np.linalg.inv(Ah)
    Zh = (Zh + Zh.T) / 2
    diag, lag = band_of(Zh / np.outer(s, s), T)
    return dict(diag=diag, lag=lag, s=s, cond=float(np.linalg.cond(Ah)), zmax=float(np.abs(Zh).max()), A=A, usable=sysd["usable"])


def longdouble_band(A):
    """the second route: (Z_tt, Z_{t,t+1}) of inv(A) from a banded Cholesky factor of the Jacobi-scaled matrix, all in np.longdouble"""
    n = len(A)
    T, bw = n // 3, 8
    s = np.sqrt(np.diagonal(A).astype(np.longdouble))
    Ah = A.astype(np.longdouble) / np.outer(s, s)
    L = np.zeros((n, n), np.longdouble)
    for j in range(n):
        lo, hi = max(0, j - bw), min(n, j + bw + 1)
        L[j, j] = np.sqrt(Ah[j, j] - np.dot(L[j, lo:j], L[j, lo:j]))
        L[j + 1:hi, j] = (Ah[j + 1:hi, j] - L[j + 1:hi, lo:j] @ L[j, lo:j]) / L[j, j]
    X = np.zeros((n, n), np.longdouble)   # L^-1, row by row
    for i in range(n):
        lo = max(0, i - bw)
        X[i] = -(L[i, lo:i] @ X[lo:i])
        X[i, i] += 1.0
        X[i] /= L[i, i]
    Zb = np.zeros((n, n), np.longdouble)  # the band of X^T X, offsets 0 .. 5
    for o in range(6):
        d = (X[:, :n - o] * X[:, o:]).sum(axis=0)
        i = np.arange(n - o)
        Zb[i, i + o] = d
        Zb[i + o, i] = d
    Zb = Zb / np.outer(s, s)
    return band_of(Zb, T)


def scaled_error(got_diag, got_lag, ref):
    """the largest |zhat - zhat_ref| over Z_tt and (got_lag not None) Z_{t,t+1}"""
    T = len(ref["diag"])
    s = ref["s"].reshape(T, 3)
    err = float(np.abs((got_diag - ref["diag"]) * (s[:, :, None] * s[:, None, :])).max())
    if got_lag is not None and T > 1:
        err = max(err, float(np.abs((got_lag - ref["lag"]) * (s[:-1, :, None] * s[1:, None, :])).max()))
    return err


def bar_of(ref):
    return BAR_K * EPS * ref["cond"] * ref["zmax"]


_ref_cache = {}


def case_reference(name, case, weights=None):
    """per track the reference of a case (None for a track with fewer than two usable frames), computed once.  weights: (T, K) or None"""
    key = (name, None if weights is None else weights.tobytes())
    if key not in _ref_cache:
        K = case["points"].shape[1]
        acc = np.broadcast_to(np.asarray(case["accel_std"], dtype=np.float64), (K,))
        refs = []
        for k in range(K):
            us = so.prepare(case["points"][:, k], case["cov"][:, k])[0]
            refs.append(reference(case["points"][:, k], case["cov"][:, k], acc[k], None if weights is None else weights[:, k]) if us.sum() >= 2 else None)
        _ref_cache[key] = refs
    return _ref_cache[key]


def check_case(name, case, got, weights=None):
    """got: dict(covariance (T, K, 3, 3), lag_covariance (T - 1, K, 3, 3) or None, status, n_usable (K)).  Asserts the bar per track, statuses and
    NaN rows; returns the largest error / (eps cond max|zhat|)"""
    worst = 0.0
    for k, ref in enumerate(case_reference(name, case, weights)):
        us = so.prepare(case["points"][:, k], case["cov"][:, k])[0]
        assert got["n_usable"][k] == us.sum(), (name, k, got["n_usable"][k], us.sum())
        lag = None if got["lag_covariance"] is None else got["lag_covariance"][:, k]
        if ref is None:
            assert got["status"][k] == so.STATUS_TOO_FEW and np.isnan(got["covariance"][:, k]).all() and (lag is None or np.isnan(lag).all()), (name, k)
            continue
        assert got["status"][k] == so.STATUS_OK and np.isfinite(got["covariance"][:, k]).all() and (lag is None or np.isfinite(lag).all()), (name, k, got["status"][k])
        assert np.array_equal(got["covariance"][:, k], got["covariance"][:, k].transpose(0, 2, 1))
        err, bar = scaled_error(got["covariance"][:, k], lag, ref), bar_of(ref)
        ratio = err / (bar / BAR_K)
        worst = max(worst, ratio)
        print(f"{name} track {k}: cond {ref['cond']:.3g} err {err:.3g} bar {bar:.3g} ratio to eps cond max|zhat| {ratio:.3g}")
        assert err <= bar, (name, k, err, bar)
    return worst


# ---------------------------------------------------------------- the library's recursion in numpy
def blocks_of(A, T):
    """the 6 x 6 super-frame blocks of a dense (3 T, 3 T) system: D (n), E (n; E[j] couples block j to j - 1); an odd T gets the phantom frame"""
    n = (T + 1) // 2
    M = np.eye(6 * n)
    M[:3 * T, :3 * T] = A
    D = [M[6 * j:6 * j + 6, 6 * j:6 * j + 6].copy() for j in range(n)]
    E = [np.zeros((6, 6))] + [M[6 * j:6 * j + 6, 6 * j - 6:6 * j].copy() for j in range(1, n)]
    return D, E


def selinv_chain(D, E, segment):
    """Zd (n), Zs (n; Zs[j] = Z_{j,j-1}, Zs[0] None) of the block-tridiagonal chain D, E: one level of the elimination, the level above by
    recursion, then  Z_il = -P Z_ll - Q Z_nl,  Z_in = -P Z_nl^T - Q Z_nn,  Z_ii = D'^-1 - Z_il P^T - Z_in Q^T  from the right separator leftwards"""
    n = len(D)
    m = n if n <= segment + 1 else segment
    nq = 1 if m == n else n // (m + 1) + 1
    Dinv, P, Q = [None] * n, [None] * n, [None] * n
    nup = 0 if m == n else n // (m + 1)
    base, cl, Eup = [None] * nup, [np.zeros((6, 6)) for _ in range(nup)], [np.zeros((6, 6)) for _ in range(nup)]
    for q in range(nq):
        j0 = q * (m + 1)
        ln = min(m, n - j0)
        if ln <= 0:
            continue
        hasL = q > 0
        Dc, G = D[j0].copy(), (E[j0].copy() if hasL else np.zeros((6, 6)))
        for i in range(ln):
            j = j0 + i
            Dinv[j] = np.linalg.inv(Dc)
            Dinv[j] = (Dinv[j] + Dinv[j].T) / 2
            P[j] = Dinv[j] @ G
            if hasL:
                cl[q - 1] -= G.T @ P[j]
            if j + 1 < n:
                Q[j] = Dinv[j] @ E[j + 1].T
                Dc = D[j + 1] - E[j + 1] @ Q[j]
                G = -E[j + 1] @ P[j]
                if i + 1 == ln:
                    base[q], Eup[q] = Dc, G
    Zd, Zs = [None] * n, [None] * n
    if nup:
        Zdu, Zsu = selinv_chain([(base[q] + cl[q] + (base[q] + cl[q]).T) / 2 for q in range(nup)], Eup, segment)
    for q in range(nq):
        j0 = q * (m + 1)
        ln = min(m, n - j0)
        if ln <= 0:
            continue
        hasL, hasR = q > 0, j0 + m < n
        Zll = Zdu[q - 1] if hasL else None
        Znn = Zdu[q] if hasR else None
        Znl = Zsu[q] if hasL and hasR else np.zeros((6, 6))
        if hasR:
            Zd[j0 + m] = Znn
        for i in range(ln - 1, -1, -1):
            j = j0 + i
            hasN = j + 1 < n
            Zil, Zin = np.zeros((6, 6)), np.zeros((6, 6))
            if hasL:
                Zil -= P[j] @ Zll
                if hasN:
                    Zin -= P[j] @ Znl.T
            if hasN:
                if hasL:
                    Zil -= Q[j] @ Znl
                Zin -= Q[j] @ Znn
                Zs[j + 1] = Zin.T
            if i == 0 and hasL:
                Zs[j] = Zil
            S = Dinv[j].copy()
            if hasL:
                S -= Zil @ P[j].T
            if hasN:
                S -= Zin @ Q[j].T
            Zd[j] = (S + S.T) / 2
            Znn, Znl = Zd[j], Zil
    return Zd, Zs


def selinv_transcription(A, T, segment):
    """(Z_tt (T, 3, 3), Z_{t,t+1} (T - 1, 3, 3)) by the recursion, written out as level 0 of the library writes them"""
    Zd, Zs = selinv_chain(*blocks_of(A, T), segment)
    diag, lag = np.full((T, 3, 3), np.nan), np.full((max(T - 1, 0), 3, 3), np.nan)
    for j, S in enumerate(Zd):
        for f in range(2):
            if 2 * j + f < T:
                diag[2 * j + f] = S[3 * f:3 * f + 3, 3 * f:3 * f + 3]
        if 2 * j + 1 < T:
            lag[2 * j] = S[0:3, 3:6]
        if j >= 1:
            lag[2 * j - 1] = Zs[j][0:3, 3:6].T
    return diag, lag
