"""Consensus triangulation in numpy: the definition of SURVEY.md section 8f-9, written without the library, for tests/test_hostcheck_consensus.py
(the g++ build of csrc/mcba_consensus_math.h) and tests/test_gpu_consensus.py (the kernels through the public function).

Per point: every camera pair (i < j, in the order (0,1), (0,2), ..., (1,2), ...) that both see it gives a hypothesis, the two-view DLT point of
the detections undistorted with `undistort_iterations` rounds; camera c, if it sees the point, is an inlier of hypothesis k iff the point is in
front of it and the raw detection is within `threshold` px of the five-coefficient projection; cost_k = sum of e^2 (inlier) or threshold^2; the
lowest cost wins, an exact tie goes to the lowest k; the point is refitted on the winner's inliers by plain Gauss-Newton (linear loss) until the
step is below 1e-12 mm.  Besides, per point: the second-lowest cost and min |e_c - threshold| over the winner's cameras, for the ambiguity rule."""
import functools

import numpy as np

import keypoint_scenes as ks
from oracle import triangulate_oracle as tri

REL_GAP, THRESHOLD_GAP, MAX_AMBIGUOUS = 1e-6, 1e-6, 0.01   # the ambiguity rule: see decided()


def pairs(C):
    return [(i, j) for i in range(C) for j in range(i + 1, C)]


def _camera_arrays(ext, intr):
    R = np.stack([ks.rodrigues(e[:3]) for e in ext])
    t = np.stack([np.asarray(e[3:], dtype=np.float64) for e in ext])
    K = np.stack([np.asarray(k, dtype=np.float64) for k, _ in intr])
    d = np.stack([np.r_[np.ravel(dd), np.zeros(5)][:5] for _, dd in intr])
    return R, t, K, d


def _project_all(X, cams):
    """keypoint_scenes.project5 for every camera at once (a scene of 64 cameras has 2 016 hypotheses to score): X (n, 3) -> uv (C, n, 2), z (C, n)."""
    R, t, K, d = cams
    Xc = np.einsum("cij,nj->cni", R, X) + t[:, None, :]
    x, y = Xc[..., 0] / Xc[..., 2], Xc[..., 1] / Xc[..., 2]
    d = d[:, None, :]
    r2 = x * x + y * y
    rad = 1 + r2 * (d[..., 0] + r2 * (d[..., 1] + r2 * d[..., 4]))
    xd = x * rad + 2 * d[..., 2] * x * y + d[..., 3] * (r2 + 2 * x * x)
    yd = y * rad + d[..., 2] * (r2 + 2 * y * y) + 2 * d[..., 3] * x * y
    return np.stack([K[:, 0, 0, None] * xd + K[:, 0, 2, None], K[:, 1, 1, None] * yd + K[:, 1, 2, None]], axis=-1), Xc[..., 2]


def _residuals(X, U, ext, intr):
    """(C, P, 2) detection - projection."""
    return np.stack([U[c] - ks.project5(X, ext[c], *intr[c]) for c in range(len(ext))])


def triangulate_pair(P1, P2, uv1, uv2):
    """oracle/triangulate_oracle.triangulate_pair's system (the rows x P[2] - P[0], y P[2] - P[1] of both views) and its smallest right singular
    vector, polished.  The system's fourth column is 1e2 .. 1e3 times longer than the others (singular values 8e5 .. 7e-2 on the scenes here),
    and LAPACK's SVD returns that vector with an error of up to 8e-11 mm in the point -- 1.5e-9 relative in a cost, above the 1e-9 these tests
    hold a cost to -- where a 60-digit SVD of the same doubles and the one-sided Jacobi of csrc/mcba_geom_math.h agree to 1e-13 mm.  So the
    triplet (sigma, u, v) from LAPACK is refined by Newton's method on A v = sigma u, A^T u = sigma v, v.v = 1, with the residuals evaluated
    in extended precision (np.longdouble); three steps bring it to the 60-digit result's 1e-13 mm."""
    n = len(uv1)
    A = np.empty((n, 4, 4))
    A[:, 0] = uv1[:, 0:1] * P1[2] - P1[0]
    A[:, 1] = uv1[:, 1:2] * P1[2] - P1[1]
    A[:, 2] = uv2[:, 0:1] * P2[2] - P2[0]
    A[:, 3] = uv2[:, 1:2] * P2[2] - P2[1]
    Uu, S, Vh = np.linalg.svd(A)
    x = Vh[:, 3].copy()
    simple = S[:, 2] > 1e-8 * S[:, 0]          # (two views of one and the same camera: a two-dimensional null space, nothing to polish)
    if simple.any():
        x[simple] = _polish(A[simple], Uu[simple][:, :, 3], S[simple][:, 3], x[simple])
    return x[:, :3] / x[:, 3:]


def _polish(A, u, sg, v):
    n = len(A)
    L = np.longdouble
    Al, u, v, sg = A.astype(L), u.astype(L), v.astype(L), sg.astype(L)
    M = np.zeros((n, 9, 9))
    M[:, :4, 4:8] = A
    M[:, 4:8, :4] = A.transpose(0, 2, 1)
    for _ in range(3):
        r = np.concatenate([(Al * v[:, None, :]).sum(2) - sg[:, None] * u, (Al * u[:, :, None]).sum(1) - sg[:, None] * v, ((v * v).sum(1, keepdims=True) - 1) / 2], axis=1)
        d = np.arange(8)
        M[:, d, d] = -np.asarray(sg, dtype=np.float64)[:, None]
        M[:, :4, 8], M[:, 4:8, 8], M[:, 8, 4:8] = -np.asarray(u, dtype=np.float64), -np.asarray(v, dtype=np.float64), np.asarray(v, dtype=np.float64)
        step = np.linalg.solve(M, -np.asarray(r, dtype=np.float64)[..., None])[..., 0]
        u, v, sg = u + step[:, :4], v + step[:, 4:8], sg + step[:, 8]
    return np.asarray(v / np.sqrt((v * v).sum(1, keepdims=True)), dtype=np.float64)


def refit(X0, U, ext, intr, inl, max_iterations=100):
    """Gauss-Newton per point on the inlier views (inl (C, P) bool), central-difference Jacobian; a point stops when its step is below 1e-12."""
    X = X0.copy()
    live = inl.sum(0) >= 2
    h = 1e-4
    for _ in range(max_iterations):
        if not live.any():
            break
        idx = np.flatnonzero(live)
        Xl, Ul, w = X[idx], U[:, idx], inl[:, idx]
        r = np.where(w[..., None], _residuals(Xl, Ul, ext, intr), 0.0)                       # (C, n, 2)
        J = np.empty(r.shape + (3,))
        for a in range(3):
            e = np.zeros(3)
            e[a] = h
            J[..., a] = -(_residuals(Xl + e, Ul, ext, intr) - _residuals(Xl - e, Ul, ext, intr)) / (2 * h)   # d projection / dX
        J = np.where(w[..., None, None], J, 0.0)
        H = np.einsum("cnka,cnkb->nab", J, J)
        g = np.einsum("cnka,cnk->na", J, r)
        step = np.linalg.solve(H, g[..., None])[..., 0]
        X[idx] = Xl + step
        live[idx[np.abs(step).max(1) < 1e-12]] = False
    return X


def consensus(uvs, ext, intr, threshold, min_views=2, undistort_iterations=5, max_iterations=100):
    """dict: points (P, 3), inliers (C, P), pair (P, 2), status (P), hypothesis_cost, second_cost (inf where there is one hypothesis), threshold_gap
    (min |e_c - threshold| over the cameras that see the point, at the winner), hypothesis (P, 3) (the winner's X), n_hypotheses (P)."""
    U = np.stack([np.asarray(u, dtype=np.float64) for u in uvs])
    C, P = U.shape[:2]
    seen = ~np.isnan(U).any(-1)
    und = [tri.undistort_points(U[c], intr[c][0], intr[c][1], undistort_iterations) for c in range(C)]
    Ps = [tri.projection_matrix(ext[c], intr[c][0]) for c in range(C)]
    cams = _camera_arrays(ext, intr)
    pr = pairs(C)
    NP = len(pr)
    cost = np.full((NP, P), np.inf)
    Xh = np.full((NP, P, 3), np.nan)
    inl = np.zeros((NP, C, P), bool)
    err = np.full((NP, C, P), np.nan)
    with np.errstate(all="ignore"):
        for k, (i, j) in enumerate(pr):
            both = seen[i] & seen[j]
            if not both.any():
                continue
            idx = np.flatnonzero(both)
            X = triangulate_pair(Ps[i], Ps[j], und[i][idx], und[j][idx])
            keep = np.isfinite(X).all(1) & (np.abs(X) < 1e300).all(1)
            idx, X = idx[keep], X[keep]
            uv, z = _project_all(X, cams)
            e = np.linalg.norm(U[:, idx] - uv, axis=-1)                                    # (C, n), NaN where unseen
            s = seen[:, idx]
            good = s & (z > 0) & (e <= threshold)
            cost[k, idx] = np.where(good, e * e, np.where(s, threshold ** 2, 0.0)).sum(0)
            Xh[k, idx], inl[k][:, idx], err[k][:, idx] = X, good, e
    n_hyp = np.isfinite(cost).sum(0)
    win = np.argmin(cost, axis=0)                                                          # (the first of equal minima: the lowest k)
    ar = np.arange(P)
    some = n_hyp > 0
    best = cost[win, ar]
    second = np.sort(cost, axis=0)[1] if NP > 1 else np.full(P, np.inf)
    mask = inl[win, :, ar].T & some
    with np.errstate(invalid="ignore"):
        gap = np.nanmin(np.where(seen, np.abs(err[win, :, ar].T - threshold), np.nan), axis=0, initial=np.inf)
    pair = np.where(some[:, None], np.array(pr)[win], -1)
    n_in = mask.sum(0)
    status = np.where(~some, -1, np.where(n_in < min_views, -2, 1))
    hyp = np.where(some[:, None], Xh[win, ar], np.nan)
    pts = np.full((P, 3), np.nan)
    fit = status == 1
    if fit.any():
        f = np.flatnonzero(fit)
        pts[f] = refit(hyp[f], U[:, f], ext, intr, mask[:, f], max_iterations)
    return dict(points=pts, inliers=mask, pair=pair, status=status, hypothesis_cost=np.where(some, best, np.nan), second_cost=second, threshold_gap=gap, hypothesis=hyp, n_hypotheses=n_hyp,
                n_inliers=n_in, seen=seen)


def decided(o):
    """(P,) bool: the points whose mask and pair a correct implementation must reproduce.  Left out only: the two lowest costs closer than 1e-6
    relative, or one of the winner's errors within 1e-6 px of the threshold; never more than 1 % of the points with a hypothesis."""
    some = o["n_hypotheses"] > 0
    with np.errstate(invalid="ignore"):
        tie = some & (o["second_cost"] - o["hypothesis_cost"] <= REL_GAP * o["hypothesis_cost"])
    near = some & (o["threshold_gap"] <= THRESHOLD_GAP)
    out = tie | near
    assert out.sum() <= MAX_AMBIGUOUS * max(1, some.sum()), f"{out.sum()} of {some.sum()} points are ambiguous"
    return ~out


def compare(got, o, gate_mm, label=""):
    """The comparisons of both tiers.  got: dict with points, inliers (C, P), n_inliers, pair, hypothesis_cost, status.  On the decided points
    mask, pair and status are equal; the winning cost to rtol 1e-9; the points to gate_mm.  Returns the decided points."""
    ok = decided(o)
    some = o["n_hypotheses"] > 0
    assert np.array_equal(got["inliers"][:, ok], o["inliers"][:, ok]), label
    assert np.array_equal(got["pair"][ok], o["pair"][ok]), label
    assert np.array_equal(got["status"][ok], o["status"][ok]), label          # (1 = converged: a refit that ends at its iteration limit, 0, fails here)
    assert np.array_equal(got["n_inliers"], got["inliers"].sum(0)), label
    rel = np.abs(got["hypothesis_cost"] - o["hypothesis_cost"])[ok & some] / o["hypothesis_cost"][ok & some]
    fit = ok & (o["status"] == 1)
    diff = np.abs(got["points"] - o["points"])[fit].max() if fit.any() else 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        gap = np.where(some, (o["second_cost"] - o["hypothesis_cost"]) / o["hypothesis_cost"], np.inf).min(initial=np.inf)
    print(f"{label}: {ok.sum()} of {len(ok)} points compared ({some.sum()} with a hypothesis), {int((~o['inliers'] & o['seen'])[:, some].sum())} detections outside the masks; "
          f"max |dX| {diff:.3e} mm, max relative cost difference {rel.max(initial=0.0):.2e}; oracle: smallest relative cost gap {gap:.2e}, "
          f"smallest |e - threshold| {o['threshold_gap'][some].min(initial=np.inf):.2e} px")
    np.testing.assert_allclose(got["hypothesis_cost"][ok & some], o["hypothesis_cost"][ok & some], rtol=1e-9, atol=0, err_msg=label)
    assert np.isnan(got["hypothesis_cost"][~some]).all() and not got["inliers"][:, ~some].any() and np.all(got["pair"][~some] == -1), label
    assert np.array_equal(np.isnan(got["points"]).any(1)[ok], ~fit[ok]), label
    assert diff <= gate_mm, label
    return ok


# launch boundaries of csrc/mcba_consensus.hip: (cameras, points)
BOUNDARY_CASES = [(2, 65),     # a single hypothesis per point
                  (8, 257),    # last camera count of the lane form; a workgroup boundary
                  (9, 130),    # first camera count of the wavefront form
                  (64, 5)]     # 2 016 pairs over 64 lanes; a partly filled last workgroup


def boundary_case(C, P):
    """(uvs, ext, intr): C five-coefficient cameras around a cloud of P points, 0.4 px noise, 30 % of the detections unseen (10 % with two
    cameras), and on a quarter of the points one seen detection displaced by N(0, 40^2) px."""
    rng = np.random.default_rng(1000 * C + P)
    ext = np.c_[rng.normal(0, 0.25, (C, 3)), rng.normal(0, 40, (C, 2)), rng.uniform(800, 1200, C)]
    intr = []
    for c in range(C):
        K = np.array([[rng.uniform(900, 1300), 0, rng.uniform(600, 700)], [0, rng.uniform(900, 1300), rng.uniform(450, 550)], [0, 0, 1.0]])
        intr.append((K, np.array([rng.normal(0, 0.08), rng.normal(0, 0.03), rng.normal(0, 1.5e-3), rng.normal(0, 1.5e-3), rng.normal(0, 0.01)])))
    X = rng.normal(0, 70, (P, 3))
    U = np.stack([ks.project5(X, ext[c], *intr[c]) for c in range(C)]) + rng.normal(0, 0.4, (C, P, 2))
    U[rng.uniform(size=(C, P)) < (0.1 if C == 2 else 0.3)] = np.nan
    for p in rng.choice(P, size=max(1, P // 4), replace=False):
        cams = np.flatnonzero(~np.isnan(U[:, p]).any(-1))
        if cams.size:
            U[rng.choice(cams), p] += rng.normal(0, 40, 2)
    return list(U), ext, intr


@functools.lru_cache(maxsize=None)
def boundary_oracle(C, P, threshold=2.5):
    uvs, ext, intr = boundary_case(C, P)
    return uvs, ext, intr, consensus(uvs, ext, intr, threshold)


@functools.lru_cache(maxsize=None)
def scene_oracle(name, threshold):
    """The oracle on a scene of tests/keypoint_scenes.py, computed once per process; treat the result as read-only."""
    uvs, ext, intr, X = ks.make(name)
    return uvs, ext, intr, X, consensus(uvs, ext, intr, threshold)


def duplicated_camera_scene():
    """scene(C=4, P=50, seed=45, noise=0.3) with camera 0 repeated as camera 1, detections included: the pairs (0, k) and (1, k) tie exactly."""
    from test_triangulate_cpu import scene

    uvs, ext, intr, X = scene(C=4, P=50, seed=45, noise=0.3)
    uvs, ext, intr = list(uvs), np.array(ext), list(intr)
    uvs[1], ext[1], intr[1] = uvs[0].copy(), ext[0], intr[0]
    return uvs, ext, intr, X


def twin_pair(pair):
    """The exact-tie twin of a pair in the duplicated-camera scene: camera 0 <-> camera 1 (a pair of both has none)."""
    i, j = int(pair[0]), int(pair[1])
    if (i, j) == (0, 1) or i > 1:
        return (i, j)
    return (1 - i, j)
