"""Plain, high-precision statements of the three floor-plane entry points (csrc/mcba_flat.hip, include/mcba.h "floor-plane
alignment"), the checker of tests/test_flat_oracle_cpu.py (no GPU) and of tests/test_gpu_flat_kernels.py (one launch at a time).

    ransac_oracle     mcba_flat_ransac: per hypothesis z = a x + b y + c the residual r = z - (a x + b y + c) of every point in np.longdouble, the
                      inliers |r| <= thr (a NaN is never one), their count, and the nine moments X Y R XX XY YY XR YR RR of dx = x - sx, dy = y - sy, r.
    lattice_scene     an input on which count and moments have ONE right answer in any summation order (below); `lattice_answer` computes it in int64.
    transform_oracle  mcba_flat_order_stats: R p + t in np.longdouble, per-coordinate sums, NaN counts, the sorted values, the values at the ranks.
    floor_oracle      mcba_flat_floor_points: np.argmin / np.argmax over z and the gathered rows.

U = 2^-53 is the unit roundoff of double, EPS = 2 U, ULD the unit roundoff of np.longdouble.  No factor below comes from the code under test.

Rounding of r (`r_bound`).  The kernel evaluates z - (fma(y, b, x a) + c): four roundings, each of a quantity no larger than
S = |z| + |a x| + |b y| + |c| (to first order).  The numpy stand-in of tests/test_flatibration_cpu.py (`moments_numpy`) has no fma: five.  The oracle's own
evaluation rounds five times to ULD.  So, for either evaluation against the oracle,
    |r_got - r_ref| <= delta_r = 5 (U + ULD) S (1 + EPS).
The decision margin of a hypothesis is the smallest | |r| - thr | over the points whose r is finite.  Where margin_i > delta_r_i for EVERY point (`margin_excess`
> 0), no evaluation within delta_r can put a point on the other side of the threshold: the count and the mask must equal the oracle's exactly, and the
moments are sums over the same set.  tests/test_flat_oracle_cpu.py asserts this for every float scene the GPU tests use.

Bound of a moment (`moment_bound`), given equal inlier sets.  A moment is a sum of terms t_i, each a factor or a product of two of dx, dy, r.
  1. The terms.  dx = x - sx is rounded once: |dx_got - dx| <= e_x = (U + ULD) |dx|; likewise dy; r carries delta_r.  A product p q of factors with errors
     e_p, e_q is off by at most |p| e_q + |q| e_p + e_p e_q (its own rounding belongs to the fma that adds it: item 2).  Summed over the inliers this is
     `carry`; it is what takes the rounding of r through R, XR, YR and RR.
  2. The summation.  A sum formed by any tree in which a term passes through at most d additions is off by at most d U sum |t_i| to first order; the bound
     takes d EPS sum |t_i|, which covers the higher orders for every d in reach.  The kernel's tree is fixed: the 4 points of a lane (an fma each), the 6 steps of
     the xor butterfly, the 4 wavefronts of a block, ceil(nblk / 256) strided partials in k_ransac_finish (nblk = ceil(n / 1024) blocks), the 8 levels of
     its LDS tree:  d = 4 + 6 + 4 + ceil(nblk / 256) + 8  (`kernel_depth`).
  3. The oracle's own sums.  np.sum over a contiguous np.longdouble array is numpy's pairwise summation (blocks of at most 128 terms in 8 strands, then a
     binary tree); with the product's rounding that is fewer than ORACLE_DEPTH = 66 roundings per term for any n below 2^50:  ORACLE_DEPTH 2 ULD sum |t_i|.
    bound = (d EPS + ORACLE_DEPTH 2 ULD) sum |t_i| + carry.
`moments_numpy` sums with np.sum (pairwise) and BLAS dot products, whose trees are not the kernel's; the CPU tier holds it to the same bound with the kernel's d
and reports how much of it is used.

Lattice scenes.  Point coordinates and the shift are integers of magnitude below 2^10, a, b and thr are multiples of 1/8, c is an integer.  Then a x, b y, r,
dx, dy are multiples of 1/8 below 2^12, every term is a multiple of 1/64 below 2^22, and every partial sum of up to 2^20 terms is a multiple of 1/64 below
2^42: exactly representable, so every addition and every fma of every summation order is exact.  `lattice_answer` computes 8 r and the sums in int64.  Points
with r = +thr, r = -thr and |r| = thr + 1/8 are planted for every hypothesis (as many as n allows), so `<=` against `<` and a threshold off by one
unit of the lattice both change a count.

Transform (`transform_oracle`).  X = ((r0 x + r1 y) + r2 z) + t rounds at most six times (three products, three sums; fewer with fma), the sums at most
S = |r0 x| + |r1 y| + |r2 z| + |t| in size, the products r_k p_k once each; the oracle rounds six times to ULD:
    |X_got - X_ref| <= delta_i = 4 (U + 2 ULD) S_i (1 + EPS)       (u (|r0 x| + |r1 y| + |r2 z|) + 3 u S <= 4 u S).
An order statistic is 1-Lipschitz in the sup norm: if every element moves by at most delta_i, the k-th smallest moves by at most max_i delta_i (the k-th
smallest of v + e lies between the k-th smallest of v - max|e| and of v + max|e|).  So a returned order statistic is within max_i delta_i of the oracle's
value at that rank.  The sums: per block the 6 butterfly steps and the 4 wavefronts, then the host adds the nblk = ceil(n / 256) block sums in order:
    |sum_got - sum_ref| <= ((6 + 4 + nblk) EPS + ORACLE_DEPTH 2 ULD) sum |X_i| + sum delta_i     (`sum_bound`).
Whether r0 x + r1 y + r2 z + t is NaN depends on the inputs alone (a NaN operand, 0 * inf, inf - inf), not on the order or contraction of the finite
arithmetic, as long as nothing finite overflows: the NaN counts are exact.  They are taken from a double evaluation.
"""
import functools

import numpy as np

import flat_problem as fp

LD = np.longdouble
EPS = 2.0 ** -52
U = 2.0 ** -53
ULD = float(np.finfo(LD).eps) / 2
ORACLE_DEPTH = 66
MOMENTS = ("X", "Y", "R", "XX", "XY", "YY", "XR", "YR", "RR")
SCORE_POINTS, FLAT_THREADS = 1024, 256   # csrc/mcba_flat.hip: kScorePoints, kFlatThreads


def kernel_depth(n):
    nblk = -(-n // SCORE_POINTS)
    return 4 + 6 + 4 + -(-nblk // FLAT_THREADS) + 8


def r_bound(P, plane):
    """delta_r of every point for one hypothesis (np.longdouble; inf or NaN where the point is not finite)."""
    a, b, c = (LD(v) for v in plane)
    x, y, z = (np.asarray(P[:, k], dtype=LD) for k in range(3))
    with np.errstate(invalid="ignore"):
        return 5 * (U + ULD) * (1 + EPS) * (np.abs(z) + np.abs(a * x) + np.abs(b * y) + abs(c))


def ransac_oracle(P, planes, thr, shift):
    """dict: counts (H,) uint64, moments (H, 9) np.longdouble, mask (H, n) bool, abs_sums (H, 9) = sum |term|, carry (H, 9) = item 1 of the bound,
    margin (H,) = the smallest | |r| - thr | over the points with a finite r, margin_excess (H,) = the smallest (| |r| - thr | - delta_r) over them."""
    P = np.asarray(P, dtype=np.float64)
    planes = np.asarray(planes, dtype=np.float64).reshape(-1, 3)
    H, n = len(planes), len(P)
    x, y, z = (np.asarray(P[:, k], dtype=LD) for k in range(3))
    dx, dy = x - LD(shift[0]), y - LD(shift[1])
    out = dict(counts=np.zeros(H, dtype=np.uint64), moments=np.zeros((H, 9), dtype=LD), mask=np.zeros((H, n), dtype=bool), abs_sums=np.zeros((H, 9), dtype=LD),
               carry=np.zeros((H, 9), dtype=LD), margin=np.full(H, np.inf), margin_excess=np.full(H, np.inf))
    with np.errstate(invalid="ignore"):
        for h, (a, b, c) in enumerate(planes):
            r = z - (LD(a) * x + LD(b) * y + LD(c))
            dr = r_bound(P, planes[h])
            m = np.abs(r) <= LD(thr)   # (a comparison with NaN is False)
            fin = np.isfinite(r)
            if fin.any():
                gap = np.abs(np.abs(r[fin]) - LD(thr))
                out["margin"][h] = float(gap.min())
                out["margin_excess"][h] = float((gap - dr[fin]).min())
            u, v, w = dx[m], dy[m], r[m]
            eu, ev, ew = (U + ULD) * np.abs(u), (U + ULD) * np.abs(v), dr[m]
            factors = {"X": (u, eu), "Y": (v, ev), "R": (w, ew)}
            for k, name in enumerate(MOMENTS):
                if len(name) == 1:
                    t, e = factors[name]
                else:
                    (p, ep), (q, eq) = factors[name[0]], factors[name[1]]
                    t, e = p * q, np.abs(p) * eq + np.abs(q) * ep + ep * eq
                out["moments"][h, k], out["abs_sums"][h, k], out["carry"][h, k] = t.sum(), np.abs(t).sum(), e.sum()
            out["counts"][h], out["mask"][h] = m.sum(), m
    return out


def ratio(err, bound):
    """max of err / bound with 0 / 0 = 0 (an exact answer meets a bound of zero) and anything else over 0 = inf."""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.max(np.where(err == 0, 0.0, err / bound)))


def moment_bound(oracle, n, depth=None):
    """(H, 9) float64: the bound of the module docstring for a launch over n points."""
    d = kernel_depth(n) if depth is None else depth
    return np.asarray((d * EPS + ORACLE_DEPTH * 2 * ULD) * oracle["abs_sums"] + oracle["carry"], dtype=np.float64)


def moment_ratio(got, oracle, n):
    """max over the moments of |got - oracle| / bound."""
    return ratio(np.abs(np.asarray(got, dtype=LD) - oracle["moments"]), moment_bound(oracle, n))


# ------------------------------------------------------------------ scenes of the scoring tests
def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def lattice_scene(n, H, seed, shift=None, empty_last=False):
    """(P (n, 3), planes (H, 3), thr, shift (2,), planted): every quantity exact in double (module docstring).  planted: (point, hypothesis, 8 r) rows of
    the points put at r = +thr, r = -thr and |r| = thr + 1/8, every hypothesis first served with +thr, then -thr, then the near miss, while n lasts.
    empty_last: the last hypothesis lies far below every point (c = 3000 against |z| + |a x + b y| < 1800) and gets no planted point.  The arrays are shared: read-only."""
    rng = np.random.default_rng([n, H, seed])
    T8 = 20   # thr = 2.5
    A8 = 2 * rng.integers(-4, 4, H) + 1            # a = A8 / 8, odd A8: x can be chosen so that a x + b y has any fractional part
    B8 = rng.integers(-8, 9, H)
    C = rng.integers(-50, 51, H)
    x = rng.integers(-400, 401, n)
    y = rng.integers(-400, 401, n)
    hyp = rng.integers(0, H, n)
    z = (A8[hyp] * x + B8[hyp] * y) // 8 + C[hyp] + rng.integers(-4, 5, n)
    far = rng.uniform(size=n) < 0.25
    z[far] = rng.integers(-1000, 1001, int(far.sum()))
    live = H - 1 if empty_last else H
    if empty_last:
        C[H - 1] = 3000
    planted = []
    for j, p in enumerate(rng.permutation(n)[: 3 * live]):
        h, kind = j % live, j // live
        R8 = (T8, -T8, (T8 + 1) * (1 if h % 2 else -1))[kind]
        x[p] += int(np.flatnonzero((A8[h] * (x[p] + np.arange(8)) + B8[h] * y[p] + R8) % 8 == 0)[0])
        z[p] = (A8[h] * x[p] + B8[h] * y[p] + R8) // 8 + C[h]
        planted.append((p, h, R8))
    assert max(np.abs(x).max(), np.abs(y).max(), np.abs(z).max()) < 1024
    P = np.column_stack([x, y, z]).astype(np.float64)
    planes = np.column_stack([A8 / 8.0, B8 / 8.0, C.astype(np.float64)])
    sh = np.asarray(rng.integers(-100, 101, 2) if shift is None else shift, dtype=np.float64)
    return _frozen(P, planes) + (T8 / 8.0,) + _frozen(sh, np.array(planted, dtype=np.int64).reshape(-1, 3))


def lattice_answer(P, planes, thr, shift):
    """(counts (H,) uint64, moments (H, 9) float64, mask (H, n) bool) of a lattice scene in int64 arithmetic on 8 a, 8 b, 8 thr, 8 r."""
    Pi = np.asarray(P).astype(np.int64)
    assert np.array_equal(Pi, P)
    A8, B8 = np.rint(planes[:, 0] * 8).astype(np.int64), np.rint(planes[:, 1] * 8).astype(np.int64)
    C, T8, s = planes[:, 2].astype(np.int64), int(round(thr * 8)), np.asarray(shift).astype(np.int64)
    assert np.array_equal(A8 / 8.0, planes[:, 0]) and np.array_equal(B8 / 8.0, planes[:, 1]) and np.array_equal(C, planes[:, 2]) and T8 / 8.0 == thr and np.array_equal(s, shift)
    H = len(planes)
    counts, mom, mask = np.zeros(H, dtype=np.uint64), np.zeros((H, 9)), np.zeros((H, len(Pi)), dtype=bool)
    for h in range(H):
        R8 = 8 * Pi[:, 2] - (A8[h] * Pi[:, 0] + B8[h] * Pi[:, 1] + 8 * C[h])
        m = np.abs(R8) <= T8
        u, v, w = Pi[m, 0] - s[0], Pi[m, 1] - s[1], R8[m]
        sums = [u.sum(), v.sum(), w.sum(), (u * u).sum(), (u * v).sum(), (v * v).sum(), (u * w).sum(), (v * w).sum(), (w * w).sum()]
        assert max(abs(int(t)) for t in sums) < 2 ** 53
        mom[h] = np.array([float(t) for t in sums]) / [1, 1, 8, 1, 1, 1, 8, 8, 64]
        counts[h], mask[h] = m.sum(), m
    return counts, mom, mask


LATTICE_EDGES = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049)   # lane, wavefront, points-per-lane and block edges of k_ransac_score (H = 3)
LATTICE_STRIDED = (262144, 262145, 524289)                               # 256, 257, 513 partial blocks: k_ransac_finish's strided loop runs 1, 2, 3 times
LATTICE_TABLES = (1, 2, 127, 128)                                        # H at n = 4097: the LDS tables up to their declared limit
FAR_SHIFT = (509, -487)
THRESHOLD = fp.THRESHOLD
# (n, H, seed) of the float scenes of the scoring tests; MASK_N: H = 1 with the mask
FLOAT_SCENES = ((1025, 8, 31), (5000, 8, 32), (262145, 8, 33), (5000, 128, 34))
MASK_N = (255, 256, 257, 5000)
MASK_SEED = 35
NONFINITE_SCENE = (5000, 8, 36)


@functools.lru_cache(maxsize=None)
def float_scene(n, H, seed):
    """(P, planes, thr, shift): flat_problem.floor_points with 30 % outliers and H hypotheses of flatibration.hypotheses from seeded 3-point subsets; the
    shift is the first point's xy, as ransac_plane passes it.  Shared: read-only."""
    from multicam_calibration_amd import flatibration as fl

    P = np.ascontiguousarray(fp.floor_points(n, 0.3, seed))
    rng = np.random.default_rng([seed, H])
    idx = np.stack([rng.choice(n, 3, replace=False) for _ in range(H)])
    planes = np.ascontiguousarray(fl.hypotheses(P, idx))
    return _frozen(P, planes) + (THRESHOLD,) + _frozen(P[0, :2].copy())


@functools.lru_cache(maxsize=None)
def nonfinite_scene():
    """(P, planes, thr, shift, bad): the float scene NONFINITE_SCENE with a few points that hold NaN, +inf or -inf in one coordinate or in all, spread over
    lanes, wavefronts and blocks.  They are outliers of every hypothesis.  bad: their indices."""
    n, H, seed = NONFINITE_SCENE
    P0, planes, thr, shift = float_scene(n, H, seed)
    P = P0.copy()
    bad = np.array([1, 63, 64, 300, 1023, 1024, 2047, 4096, n - 1])
    vals = [np.nan, np.inf, -np.inf]
    for j, p in enumerate(bad):
        if j % 4 == 3:
            P[p] = vals[j % 3]
        else:
            P[p, j % 3] = vals[(j // 3) % 3]
    return _frozen(P) + (planes, thr, shift, bad)


@functools.lru_cache(maxsize=None)
def scene_oracle(kind, *key):
    """ransac_oracle of a scene of this module, computed once per process: kind 'float' (n, H, seed), 'nonfinite' (), 'removed' () = the non-finite scene
    without its bad points."""
    if kind == "float":
        P, planes, thr, shift = float_scene(*key)
    else:
        P, planes, thr, shift, bad = nonfinite_scene()
        if kind == "removed":
            P = np.delete(P, bad, axis=0)
    return ransac_oracle(P, planes, thr, shift)


# ------------------------------------------------------------------ transform and order statistics
TRANSFORM_N = (1, 255, 256, 257, 1001, 256 * 1025 + 17)


def rotation(rotvec):
    """Rodrigues' formula in double."""
    rv = np.asarray(rotvec, dtype=np.float64)
    th = np.linalg.norm(rv)
    k = rv / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def transforms():
    """name -> rt12: the rotation by 90 degrees about z with exact 0 and +-1 entries and no translation; a generic rotation with a translation of arena size
    whose three components differ."""
    quarter = np.array([0.0, -1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])
    generic = np.concatenate([rotation([0.3, -0.5, 0.8]).ravel(), [321.5, -188.25, 77.125]])
    return {"quarter": quarter, "generic": generic}


def eight_ranks(n):
    """All 8 ranks of one call, duplicates included: both ends twice, the 1st and 99th percentile's lower neighbours, the two middles."""
    return np.array([0, 0, (n - 1) // 100, (n - 1) // 2, n // 2, n - 1 - (n - 1) // 100, n - 1, n - 1], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def transform_points(n):
    """(n, 3) finite arena points with repeated x values and a signed zero (the scene of test_gpu_flatibration's order-statistics test, wider in y).  Read-only."""
    rng = np.random.default_rng([n, 77])
    P = rng.normal(size=(n, 3)) * [100.0, 60.0, 5.0]
    P[: n // 3, 0] = np.round(P[: n // 3, 0])
    if n > 2:
        P[1, 1] = -0.0
    return _frozen(np.ascontiguousarray(P))[0]


def nonfinite_points(n):
    """transform_points(n) with NaN and infinities of both signs in single coordinates and whole points, in the first, a middle and the last block."""
    P = transform_points(n).copy()
    for p, k, v in [(0, 0, np.nan), (3, 1, np.inf), (9, 0, np.inf), (5, 2, -np.inf), (n // 2, 0, np.inf), (n // 2 + 1, 0, -np.inf), (n // 2 + 2, 1, np.nan), (n - 2, 2, np.nan), (n - 1, 1, -np.inf)]:
        P[p, k] = v
    P[7] = [np.inf, np.inf, 1.0]
    P[n - 5] = [np.inf, -np.inf, np.nan]
    return P


def transform_oracle(P, rt12, ranks=()):
    """dict: xy (2, n) np.longdouble = the first two rows of R p + t, sums (2,), abs_sums (2,), delta (2, n) = the rounding bound of the double evaluation,
    nans (2,) uint64, sorted (list of two arrays: the non-NaN values in order), values (2, len(ranks)) = sorted[c][ranks]."""
    P = np.asarray(P, dtype=np.float64)
    rt = np.asarray(rt12, dtype=np.float64)
    x, y, z = (np.asarray(P[:, k], dtype=LD) for k in range(3))
    out = dict(xy=np.zeros((2, len(P)), dtype=LD), delta=np.zeros((2, len(P)), dtype=LD), nans=np.zeros(2, dtype=np.uint64), sorted=[])
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(2):
            r0, r1, r2, t = (LD(v) for v in (rt[3 * c], rt[3 * c + 1], rt[3 * c + 2], rt[9 + c]))
            out["xy"][c] = r0 * x + r1 * y + r2 * z + t
            out["delta"][c] = 4 * (U + 2 * ULD) * (1 + EPS) * (np.abs(r0 * x) + np.abs(r1 * y) + np.abs(r2 * z) + abs(t))
            dbl = rt[3 * c] * P[:, 0] + rt[3 * c + 1] * P[:, 1] + rt[3 * c + 2] * P[:, 2] + rt[9 + c]
            out["nans"][c] = np.isnan(dbl).sum()
            out["sorted"].append(np.sort(out["xy"][c][~np.isnan(out["xy"][c])]))
        out["sums"], out["abs_sums"] = out["xy"].sum(axis=1), np.abs(out["xy"]).sum(axis=1)
    rk = np.asarray(ranks, dtype=np.int64)
    out["values"] = np.stack([s[rk] if len(rk) and len(s) > rk.max(initial=0) else np.full(len(rk), np.nan, dtype=LD) for s in out["sorted"]])
    return out


def sum_bound(oracle, n):
    """(2,) float64: the bound of the module docstring on sums_out."""
    nblk = -(-n // FLAT_THREADS)
    return np.asarray(((6 + 4 + nblk) * EPS + ORACLE_DEPTH * 2 * ULD) * oracle["abs_sums"] + oracle["delta"].sum(axis=1), dtype=np.float64)


def order_bound(oracle):
    """(2,) float64: max_i delta_i per coordinate."""
    return np.asarray(oracle["delta"].max(axis=1), dtype=np.float64)


@functools.lru_cache(maxsize=None)
def transform_case(name, n):
    """(P, rt12, ranks, transform_oracle) of one case of the transform tests, computed once per process."""
    P, rt12, ranks = transform_points(n), transforms()[name], eight_ranks(n)
    return P, rt12, ranks, transform_oracle(P, rt12, ranks)


# ------------------------------------------------------------------ floor points
# (K, frames): K = 9 has row 27 and 227 frames per block, both odd, so blocks 1 and 3 start at an odd double and stage by the scalar branch -- with an odd
# count of doubles at F = 228, 455, 1000 and an even one at F = 229; K = 2047: one frame per block, every odd block unaligned; K = 2048: the limit; K = 682:
# 3 frames per block, even row
FLOOR_CASES = tuple((9, F) for F in (226, 227, 228, 229, 455, 1000)) + ((2047, 5), (2048, 3), (682, 7))


def frames_per_block(K):
    return min(FLAT_THREADS, 6144 // (3 * K))


def floor_oracle(kp, down):
    """(index (F,), rows (F, 3)): np.argmax / np.argmin of z per frame (first index on ties, the first NaN wins, an all-NaN frame gives 0) and that keypoint."""
    kp = np.asarray(kp, dtype=np.float64)
    ix = np.argmax(kp[:, :, 2], axis=1) if down else np.argmin(kp[:, :, 2], axis=1)
    return ix, kp[np.arange(len(kp)), ix]


def handmade_frames():
    """(8, 9, 3): the ties / first-NaN / all-NaN / signed-zero / infinity / leading-NaN frames of test_gpu_flatibration.py padded to 9 keypoints, and two frames
    whose LAST keypoint alone is the smallest (largest) z: the last double of a frame is the last double a block stages."""
    kp = np.zeros((8, 9, 3))
    kp[:, :, :2] = np.arange(18).reshape(9, 2) + 0.5
    pad = [2.5, 2.5, 2.5, 2.5, 2.5]
    kp[0, :, 2] = [3, 1, 1, 2] + pad
    kp[1, :, 2] = [3, np.nan, 0, np.nan] + pad
    kp[2, :, 2] = np.nan
    kp[3, :, 2] = [-0.0, 0.0, -1.0, -1.0] + [-0.5, 0.0, -0.0, -1.0, -0.25]
    kp[4, :, 2] = [np.inf, -np.inf, -np.inf, 5] + [np.inf, 1, 2, np.inf, -np.inf]
    kp[5, :, 2] = [np.nan, 1, 2, 3] + pad
    kp[6, :, 2] = [4, 3, 5, 3, 4, 6, 3, 4, -1234.5]
    kp[7, :, 2] = [4, 3, 5, 3, 4, 6, 3, 4, 4321.75]
    return kp


def handmade_keypoints(F, decisive):
    """(F, 9, 3): handmade_frames repeated, each repeat's xy moved (so that a row read from another repeat differs).  The last frame of every odd block of
    227 frames is frame `decisive` (6: its last keypoint is the smallest z, 7: the largest), so the last double that the scalar staging branch copies decides
    the answer; the even blocks end on other frames (frame 226 is the all-NaN one), so that whatever an earlier block left in LDS there is another value."""
    base = handmade_frames()
    kp = base[np.arange(F) % 8].copy()
    kp[:, :, :2] += (np.arange(F) // 8)[:, None, None] * 100.0
    fpb = frames_per_block(9)
    for b in range(1, -(-F // fpb), 2):
        last = min(F, (b + 1) * fpb) - 1
        kp[last, :, 2] = base[decisive, :, 2]
    return kp
