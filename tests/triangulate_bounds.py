"""A conditioning-scaled bar for `triangulate()` (csrc/mcba_triangulate.hip: k_triangulate<2..8>, k_triangulate_wave), the scenes it is held to and
the launch regimes of the wave kernel.  The checker of tests/test_triangulate_bounds_cpu.py (no GPU: the bar itself and the host build of the kernels'
text), of tests/test_gpu_triangulate_regimes.py (the GPU tier) and, beside their older gates, of tests/test_gpu_triangulate.py and of the two
triangulation tests of tests/test_hostcheck_math.py.

The bar.  `triangulate()` is the per-coordinate nan-median over the camera pairs of the two-view DLT points.  For pair k of one point let v_k be the
DLT point of the float64 route of oracle/triangulate_oracle.py and sigma_1 >= .. >= sigma_4 the singular values of its 4 x 4 system.  The null vector
of that system moves by (perturbation) / (sigma_3 - sigma_4), a backward-stable route perturbs the system by a few EPS sigma_1, so

    t_k = K_TRI  EPS  sigma_1 / (sigma_3 - sigma_4)  max(1, |v_k|_inf)

is the room a pair value gets, and because a median is monotone in every argument a kernel whose pair values all lie within t_k of v_k returns a
median inside

    [lo, hi] = [nanmedian_k (v_k - t_k), nanmedian_k (v_k + t_k)]           per coordinate.

`check` asserts exactly that (and the NaN pattern), on every point: the scenes are chosen so that no half-width exceeds 1e-9 max(1, |X|_inf)
(HALF_WIDTH_MAX, asserted on the CPU) and no point has to be left out.

K_TRI is measured against the reference, never against the kernel or its host build: it is 8 x the worst multiple of
EPS sigma_1 / (sigma_3 - sigma_4) max(1, |v|_inf) by which the LAPACK pair point departs from the 40-digit pair point of `exact_pairs` (mpmath:
Rodrigues, K [R | t], the fixed-count undistortion, mpmath.svd_r -- the whole route, so that the rounding of the projection matrices and of the
undistortion is in it), and at least 16.  Measured over 1276 pair-points, up to 100 drawn from the GPU cases of every regime below
(tests/test_triangulate_bounds_cpu.py::test_k_tri_is_measured_against_the_reference prints it): worst multiple 0.979 (37 and 42 cameras; the
other regimes 0.11 to 0.50), so K_TRI = 16, the floor.  The factor 8 is the usual margin over a two-route measurement (fivepoint_oracle.K5); the
kernel gets the remainder of the budget.

The regimes.  `launch_triangulate_wave` packs ppb = min(4, 65536 / slot) points (wavefronts) into a workgroup, slot = (3 C + 3 C (C - 1) / 2 + 2) 8
bytes of LDS per point; `wave_points_per_block` restates that and `regime_table()` derives, for 9 .. 64 cameras, the camera counts of every ppb
(4: 9 .. 36, 3: 37 .. 42, 2: 43 .. 51, 1: 52 .. 64).  `gpu_cases()` puts both ends of every row at the point counts around one workgroup
(1, ppb - 1, ppb, ppb + 1, 2 ppb + 1), every register kernel at one lane and around one 256-lane block, every number of views of a point from 0 to
C, and the undistortion at 0, 1, 5 and 20 rounds, with two coefficients and five, and past the model's valid radius."""
import functools
import itertools
from collections import namedtuple

import numpy as np

import multicam_calibration_amd as m
from oracle import triangulate_oracle as tri
from test_triangulate_cpu import scene

EPS = 2.0 ** -52
K_TRI_MEASURED = 0.98           # the worst multiple, LAPACK against mpmath (module docstring; test_k_tri_is_measured_against_the_reference prints it)
K_TRI = max(16.0, 8 * K_TRI_MEASURED)
HALF_WIDTH_MAX = 1e-9           # x max(1, |X|_inf): the widest enclosure a scene of this module may have, at any point
DIST5 = np.array([-0.25, 0.08, 2e-3, -1e-3, 0.01])   # k1 k2 p1 p2 k3: strong enough to matter (3 % at the image corners), mild enough to contract
GUARD_DIST = np.array([-0.5, 0.0, 0.0, 0.0, 0.0])    # valid to r = sqrt 2 (test_triangulate_cpu.test_oracle_undistort_icdist_guard's model)


# ---- the launch regimes of k_triangulate_wave
def wave_points_per_block(C):
    """launch_triangulate_wave's ppb for C cameras (0: the slot of one point does not fit)"""
    slot = (3 * C + 3 * (C * (C - 1) // 2) + 2) * 8
    return min(4, (64 * 1024) // slot)


def regime_table(lo=9, hi=64):
    """{ppb: (fewest cameras, most cameras)} over the wave kernel's camera counts"""
    table = {}
    for C in range(lo, hi + 1):
        ppb = wave_points_per_block(C)
        a, b = table.get(ppb, (C, C))
        table[ppb] = (min(a, C), max(b, C))
    return table


def wave_point_counts(ppb):
    """the point counts around one workgroup of ppb points: one point, one short of a workgroup, a full one, one more, two and one more"""
    return sorted({1, 2, 3} if ppb == 1 else {n for n in (1, ppb - 1, ppb, ppb + 1, 2 * ppb + 1) if n >= 1})


# ---- the float64 route, pair by pair
def _pairs(C):
    return list(itertools.combinations(range(C), 2))   # (0,1), (0,2), .., (1,2), ..: the oracle's and the wave kernel's order


def pair_points(uvs, ext, intr, iterations=5):
    """oracle/triangulate_oracle.py's route with the pairs kept apart: v (NP, P, 3) the DLT points, s (NP, P, 4) the singular values of their
    systems; NaN where one of the two cameras does not see the point."""
    C = len(ext)
    n = np.asarray(uvs[0]).shape[0]
    und = [tri.undistort_points(uv, K, d, iterations) for uv, (K, d) in zip(uvs, intr)]
    Ps = [tri.projection_matrix(e, K) for e, (K, _) in zip(ext, intr)]
    pr = _pairs(C)
    v = np.full((len(pr), n, 3), np.nan)
    s = np.full((len(pr), n, 4), np.nan)
    for k, (i, j) in enumerate(pr):
        seen = ~(np.isnan(und[i]).any(-1) | np.isnan(und[j]).any(-1))
        if not seen.any():
            continue
        A = np.empty((int(seen.sum()), 4, 4))   # (triangulate_pair's rows)
        A[:, 0] = und[i][seen, 0:1] * Ps[i][2] - Ps[i][0]
        A[:, 1] = und[i][seen, 1:2] * Ps[i][2] - Ps[i][1]
        A[:, 2] = und[j][seen, 0:1] * Ps[j][2] - Ps[j][0]
        A[:, 3] = und[j][seen, 1:2] * Ps[j][2] - Ps[j][1]
        _, sv, vt = np.linalg.svd(A)
        v[k, seen] = vt[:, 3, :3] / vt[:, 3, 3:]
        s[k, seen] = sv
    return v, s


def pair_unit(v, s):
    """EPS sigma_1 / (sigma_3 - sigma_4) max(1, |v|_inf) per pair-point, (NP, P): what K_TRI multiplies"""
    return EPS * s[..., 0] / (s[..., 2] - s[..., 3]) * np.maximum(1.0, np.abs(v).max(-1))


def nanmedian_rows(x):
    """np.nanmedian over the pairs with the oracle's rule for a point no pair sees (a NaN row), quietly"""
    out = np.full(x.shape[1:], np.nan)
    some = ~np.isnan(x).all((0, 2))
    if some.any():
        out[some] = np.nanmedian(x[:, some], axis=0)
    return out


def enclosure(uvs, ext, intr, iterations=5):
    """(lo, hi), both (P, 3): the interval of the module docstring; NaN rows where fewer than two cameras see the point"""
    v, s = pair_points(uvs, ext, intr, iterations)
    t = (K_TRI * pair_unit(v, s))[..., None]
    return nanmedian_rows(v - t), nanmedian_rows(v + t)


def half_width_ratio(lo, hi):
    """the largest half-width of the enclosure over max(1, |X|_inf) of its point (0.0 when no point is finite)"""
    ok = ~np.isnan(lo).any(1)
    if not ok.any():
        return 0.0
    mid, half = 0.5 * (lo[ok] + hi[ok]), 0.5 * (hi[ok] - lo[ok])
    return float((half.max(1) / np.maximum(1.0, np.abs(mid).max(1))).max())


def check(label, got, lo, hi):
    """got (P, 3) has the enclosure's NaN pattern and lies inside it on every finite row.  Prints, before it asserts, the worst position
    |got - mid| / half-width (1 = on the edge) and the largest half-width; returns the worst position.  (mid is the oracle's median only where
    the pair values lie further apart than their t_k differ, as on this module's noisy scenes; on a noise-free scene the interval is not centred
    on it and a position of 0.7 is no error: DESIGN.md section 8f-4.)"""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == lo.shape == hi.shape, (label, got.shape, lo.shape)
    ok = ~np.isnan(lo).any(1)
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    both = ok & ~np.isnan(got).any(1)
    worst = float((np.abs(got[both] - mid[both]) / half[both]).max()) if both.any() else 0.0
    widest = float(half[ok].max()) if ok.any() else 0.0
    print("%s: %d points (%d finite), worst position %.3g of the half-width, largest half-width %.3g (%.3g |X|)"
          % (label, len(lo), int(ok.sum()), worst, widest, half_width_ratio(lo, hi)))
    assert np.array_equal(np.isnan(got), np.isnan(lo)), (label, "NaN pattern")
    inside = (got[ok] >= lo[ok]) & (got[ok] <= hi[ok])
    assert inside.all(), (label, "outside the enclosure at", np.argwhere(~inside)[:5].tolist(), "worst position", worst)
    return worst


# ---- the same function in 40 digits
def _mp():
    import mpmath as mp

    mp.mp.dps = 40
    return mp


def _exact_undistort(mp, uv, K4, k, iterations, p):
    """detection p of one camera, undistorted (mpf pair), or None where it is unseen"""
    fx, fy, cx, cy = K4
    k1, k2, p1, p2, k3 = k
    u, w = uv[p]
    if np.isnan(u) or np.isnan(w):
        return None
    x0, y0 = (mp.mpf(float(u)) - cx) / fx, (mp.mpf(float(w)) - cy) / fy
    x, y = x0, y0
    for _ in range(iterations):
        r2 = x * x + y * y
        icdist = 1 / (1 + ((k3 * r2 + k2) * r2 + k1) * r2)
        if icdist < 0:   # the guard: the unrefined point, no further rounds
            return mp.mpf(float(u)), mp.mpf(float(w))
        dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        x, y = (x0 - dx) * icdist, (y0 - dy) * icdist
    return x * fx + cx, y * fy + cy


def _exact_cameras(mp, uvs, ext, intr, iterations):
    """per camera: the 3 x 4 projection K [R | t] and p -> the undistorted detection of point p (_exact_undistort), all mpf"""
    Ps, und = [], []
    for uv, e, (K, d) in zip(uvs, ext, intr):
        r = [mp.mpf(float(x)) for x in e[:3]]
        th = mp.sqrt(r[0] ** 2 + r[1] ** 2 + r[2] ** 2)
        S = mp.matrix([[0, -r[2], r[1]], [r[2], 0, -r[0]], [-r[1], r[0], 0]]) / (th if th > 0 else 1)
        R = mp.eye(3) + mp.sin(th) * S + (1 - mp.cos(th)) * (S * S)
        Rt = mp.matrix(3, 4)
        for a in range(3):
            for b in range(3):
                Rt[a, b] = R[a, b]
            Rt[a, 3] = mp.mpf(float(e[3 + a]))
        Ps.append(mp.matrix([[mp.mpf(float(x)) for x in row] for row in np.asarray(K, dtype=np.float64)]) * Rt)
        k = [mp.mpf(0)] * 5
        for a, x in enumerate(np.ravel(d)[:5]):
            k[a] = mp.mpf(float(x))
        k1, k2, p1, p2, k3 = k
        fx, fy, cx, cy = (mp.mpf(float(K[0][0])), mp.mpf(float(K[1][1])), mp.mpf(float(K[0][2])), mp.mpf(float(K[1][2])))
        und.append(functools.lru_cache(maxsize=None)(functools.partial(_exact_undistort, mp, np.asarray(uv, dtype=np.float64), (fx, fy, cx, cy), k, iterations)))
    return Ps, und


def exact_pairs(uvs, ext, intr, iterations=5, select=None):
    """The pair points of the whole route in 40 digits: an (NP, P) object array of 3-tuples of mpf, None where the pair does not see the point
    (or where the boolean mask `select`, (NP, P), leaves it out: about 5 ms per pair-point)."""
    mp = _mp()
    C = len(ext)
    n = np.asarray(uvs[0]).shape[0]
    Ps, und = _exact_cameras(mp, uvs, ext, intr, iterations)
    pr = _pairs(C)
    out = np.empty((len(pr), n), dtype=object)
    for k, (i, j) in enumerate(pr):
        for p in range(n):
            if select is not None and not select[k, p]:
                continue
            uv = {i: und[i](p), j: und[j](p)}
            if uv[i] is None or uv[j] is None:
                continue
            A = mp.matrix(4, 4)
            for row, (c, ax) in enumerate(((i, 0), (i, 1), (j, 0), (j, 1))):
                for col in range(4):
                    A[row, col] = uv[c][ax] * Ps[c][2, col] - Ps[c][ax, col]
            _, _, V = mp.svd_r(A)   # A = U diag(S) V, S descending: the null vector is V's last row
            out[k, p] = (V[3, 0] / V[3, 3], V[3, 1] / V[3, 3], V[3, 2] / V[3, 3])
    return out


def exact(uvs, ext, intr, iterations=5):
    """`triangulate()` in 40 digits, rounded to float64 at the end: (P, 3), NaN rows where fewer than two cameras see the point"""
    pairs = exact_pairs(uvs, ext, intr, iterations)
    n = pairs.shape[1]
    out = np.full((n, 3), np.nan)
    for p in range(n):
        kept = [x for x in pairs[:, p] if x is not None]
        for d in range(3):
            vals = sorted(x[d] for x in kept)
            if vals:
                out[p, d] = float((vals[(len(vals) - 1) // 2] + vals[len(vals) // 2]) / 2)
    return out


# ---- scenes
def project5(X, ext, intr):
    """(C, P, 2): the points through every camera, pinhole and the five-coefficient model"""
    out = []
    for e, (K, d) in zip(ext, intr):
        k1, k2, p1, p2, k3 = np.ravel(d)[:5]
        Xc = X @ tri.rodrigues(e[:3]).T + e[3:]
        a, b = Xc[:, 0] / Xc[:, 2], Xc[:, 1] / Xc[:, 2]
        r2 = a * a + b * b
        rad = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
        x = a * rad + 2 * p1 * a * b + p2 * (r2 + 2 * a * a)
        y = b * rad + p1 * (r2 + 2 * b * b) + 2 * p2 * a * b
        out.append(np.stack([K[0, 0] * x + K[0, 2], K[1, 1] * y + K[1, 2]], -1))
    return np.stack(out)


def bounds_scene(C, P, seed, noise=0.3, p_unseen=0.25, spread=60.0, dist=DIST5):
    """test_triangulate_cpu.scene's rig and cloud (the cloud `spread` wide instead of 60) seen through `dist` ((5,), or (C, 5) per camera) with
    `noise` px on every detection, so that the pair values differ and the rank of the median matters, and a share `p_unseen` of the detections
    missing.  Returns uvs (list of (P, 2)), ext (C, 6), intr [(K, dist5)], X (P, 3)."""
    _, ext, intr, X = scene(C=C, P=P, seed=seed)
    centre = m.synth._T(m.synth.make_problem(C, 2, seed=seed, noise=0.0)["true_poses"][0])[:3, 3]
    X = centre + (X - centre) * (spread / 60.0)
    dist = np.broadcast_to(np.asarray(dist, dtype=np.float64), (C, 5))
    intr = [(K, dist[c].copy()) for c, (K, _) in enumerate(intr)]
    rng = np.random.default_rng(seed + 11)
    uvs = project5(X, ext, intr) + rng.normal(0, noise, (C, P, 2))
    if p_unseen:
        uvs[rng.uniform(size=(C, P)) < p_unseen] = np.nan
    return list(uvs), ext, intr, X


def views_scene(C, seed):
    """C + 2 points: point m <= C is seen by m cameras (drawn), so the pair counts run 0, 0, 1, 3, 6, 10, .. -- odd and even, NaN rows for m < 2;
    the last point is seen by all but has ONE coordinate of one detection missing, which counts as that camera not seeing it."""
    uvs, ext, intr, X = bounds_scene(C, C + 2, seed, p_unseen=0.0)
    rng = np.random.default_rng(seed + 13)
    for mm in range(C + 1):
        for c in rng.permutation(C)[mm:]:
            uvs[c][mm] = np.nan
    uvs[int(rng.integers(C))][C + 1, int(rng.integers(2))] = np.nan
    return uvs, ext, intr, X


def guard_scene(C, seed):
    """6 points, all seen; camera 1 has the strong one-coefficient model, and two of its detections lie past that model's valid radius: point 0 at
    r = 2 (icdist < 0 at the first round), point 1 at r = 1.35 (the iterate leaves at the second) -- both come back unrefined and are triangulated
    as they stand"""
    dist = np.tile(DIST5, (C, 1))
    dist[1] = GUARD_DIST
    uvs, ext, intr, X = bounds_scene(C, 6, seed, p_unseen=0.0, dist=dist)
    K = intr[1][0]
    uvs[1][0] = K[0, 2] + K[0, 0] * 1.6, K[1, 2] + K[1, 1] * 1.2
    uvs[1][1] = K[0, 2] + K[0, 0] * 1.35, K[1, 2]
    return uvs, ext, intr, X


def teeth_scene():
    """4 cameras, 40 points towards the image corners (inside every image, 0.35 or more of a focal length off the axis in two cameras or more),
    every third point missing one view: 6 pairs (even) or 3 (odd).  The case the bar is shown to have teeth on."""
    uvs, ext, intr, X = bounds_scene(4, 600, seed=5, p_unseen=0.0, spread=200.0)
    uv = np.stack(uvs)
    clean = project5(X, ext, intr)
    inside = ((clean >= 0) & (clean <= np.array([1280.0, 1024.0]))).all((0, 2))
    r = np.stack([np.hypot((clean[c, :, 0] - K[0, 2]) / K[0, 0], (clean[c, :, 1] - K[1, 2]) / K[1, 1]) for c, (K, _) in enumerate(intr)])
    keep = np.flatnonzero(inside & ((r >= 0.35).sum(0) >= 2))[:40]
    assert len(keep) == 40
    uv = uv[:, keep].copy()
    for p in range(0, 40, 3):
        uv[p % 4, p] = np.nan
    return list(uv), ext, intr, X[keep]


Case = namedtuple("Case", "label regime uvs ext intr iterations direct")
# direct: None = through mc.triangulate; "null_dist" = the C entry point with dist5 = NULL (k1, k2 come from the camera block); "junk_block" = the
# C entry point with dist5 given and other numbers in the camera block's k1, k2 (dist5 is what counts)


@functools.lru_cache(maxsize=None)
def gpu_cases():
    """every case of tests/test_gpu_triangulate_regimes.py (and of the host build's pass over them), as a tuple of Case"""
    cases = []

    def add(label, regime, sc, iterations=5, direct=None):
        cases.append(Case(label, regime, sc[0], sc[1], sc[2], iterations, direct))

    for C in range(2, 9):     # one lane per point, 256 lanes per block: one lane, a block short of one, a full block, a block and one lane
        for P in (1, 255, 256, 257):
            add("C=%d P=%d" % (C, P), "register C=%d" % C, bounds_scene(C, P, seed=100 * C + P, p_unseen=0.25 if P > 1 else 0.0))
    for ppb, ends in sorted(regime_table().items(), reverse=True):
        for C in ends:
            for P in wave_point_counts(ppb):
                add("C=%d P=%d" % (C, P), "wave ppb=%d" % ppb, bounds_scene(C, P, seed=100 * C + P, p_unseen=(0.25 if C < 20 else 0.6) if P > 1 else 0.0))
    for C in (4, 8, 12):
        add("views C=%d" % C, "views", views_scene(C, seed=40 + C))
    for C in (3, 9):
        for it in (0, 1, 5, 20):
            add("rounds=%d C=%d" % (it, C), "undistortion", bounds_scene(C, 7, seed=60 + C), iterations=it)
        sc = scene(C=C, P=7, seed=70 + C, noise=0.3, p_unseen=0.2)   # (k1, k2, 0, 0, 0) per camera
        add("k1 k2 from the camera block C=%d" % C, "undistortion", sc, direct="null_dist")
        add("dist5 over the camera block C=%d" % C, "undistortion", bounds_scene(C, 7, seed=80 + C), direct="junk_block")
        add("past the valid radius C=%d" % C, "undistortion", guard_scene(C, seed=90 + C))
    return tuple(cases)


def regimes():
    return list(dict.fromkeys(c.regime for c in gpu_cases()))


@functools.lru_cache(maxsize=None)
def case_enclosure(label):
    c = next(c for c in gpu_cases() if c.label == label)
    return enclosure(c.uvs, c.ext, c.intr, c.iterations)
