"""The five floor-plane kernels (csrc/mcba_flat.hip) held to the oracles of tests/flat_oracle.py one launch at a time, at their launch edges.  Every test calls
the C entry point itself through ops.call, as flatibration.py does, and compares what the launch wrote:

  mcba_flat_ransac       k_ransac_score / k_ransac_finish / k_ransac_mask: counts, the nine moments and the mask -- on lattice scenes with np.array_equal (one
                         right answer in any summation order) at the lane, wavefront, points-per-lane, block, strided-finish and LDS-table edges; on float scenes
                         counts exactly (tests/test_flat_oracle_cpu.py proves the decision margins) and every moment within its derived bound.
  mcba_flat_order_stats  k_flat_transform + the select: sums within the derived bound, order statistics within max_i delta_i, NaN counts exactly.
  mcba_flat_floor_points k_floor_points: index and row bit for bit where blocks take the scalar staging branch.
Each test that measures prints `ratio` = worst error / derived bound (tests/flat_oracle.py derives the bounds)."""
import numpy as np
import pytest

import flat_oracle as fo
import flat_problem as fp

pytestmark = pytest.mark.gpu
LD = np.longdouble


def gpu_ransac(P, planes, thr, shift, want_mask=False):
    """(counts (H,) uint64, moments (H, 9), mask (n,) uint8 or None) of one mcba_flat_ransac call; the outputs start as sentinels."""
    from multicam_calibration_amd import ops

    P, planes, shift = (np.ascontiguousarray(a, dtype=np.float64) for a in (P, planes, shift))
    n, H = len(P), len(planes)
    counts = np.full(H, 2 ** 63, dtype=np.uint64)
    mom = np.full((H, 9), np.nan)
    mask = np.full(n, 0xAA, dtype=np.uint8) if want_mask else None
    ops.call("mcba_flat_ransac", n, P.ctypes.data, H, planes.ctypes.data, float(thr), shift.ctypes.data, 0, counts.ctypes.data, mom.ctypes.data,
             None if mask is None else mask.ctypes.data, None)
    return counts, mom, mask


def gpu_order_stats(P, rt12, ranks):
    """(values (2, len(ranks)), sums (2,), nans (2,) uint64) of one mcba_flat_order_stats call."""
    from multicam_calibration_amd import ops

    P, rt12, ranks = np.ascontiguousarray(P, dtype=np.float64), np.ascontiguousarray(rt12, dtype=np.float64), np.ascontiguousarray(ranks, dtype=np.int64)
    values = np.full((2, max(len(ranks), 1)), np.nan)
    sums, nans = np.full(2, np.nan), np.full(2, 2 ** 63, dtype=np.uint64)
    ops.call("mcba_flat_order_stats", len(P), P.ctypes.data, rt12.ctypes.data, len(ranks), ranks.ctypes.data, 0, values.ctypes.data, sums.ctypes.data, nans.ctypes.data, None)
    return values[:, : len(ranks)], sums, nans


def gpu_floor_points(kp, down):
    """(index (F,) int32, rows (F, 3)) of one mcba_flat_floor_points call."""
    from multicam_calibration_amd import ops

    kp = np.ascontiguousarray(kp, dtype=np.float64)
    F, K = kp.shape[:2]
    out, idx = np.full((F, 3), -7.0), np.full(F, -1, dtype=np.int32)
    ops.call("mcba_flat_floor_points", F, K, kp.ctypes.data, int(down), 0, out.ctypes.data, idx.ctypes.data, None)
    return idx, out


# ---------------------------------------------------------------- a. scoring, lattice scenes: no tolerance
def check_lattice(n, H, shift=None, empty_last=False):
    P, planes, thr, sh, _ = fo.lattice_scene(n, H, 1, shift, empty_last)
    counts0, mom0, _ = fo.lattice_answer(P, planes, thr, sh)
    counts, mom, _ = gpu_ransac(P, planes, thr, sh)
    assert np.array_equal(counts, counts0), (counts, counts0)   # (the planted |r| == thr points are inliers, the |r| = thr + 1/8 ones are not)
    assert np.array_equal(mom, mom0), np.argwhere(mom != mom0)
    return counts, mom


@pytest.mark.parametrize("n", fo.LATTICE_EDGES)
def test_scoring_lattice_at_the_lane_wavefront_and_block_edges(n):
    check_lattice(n, 3)


@pytest.mark.parametrize("n", fo.LATTICE_STRIDED)
def test_scoring_lattice_through_the_strided_finish(n):
    """256, 257 and 513 partial blocks: lane 0 of k_ransac_finish sums 1, 2 and 3 partials before the LDS tree."""
    assert -(-n // fo.SCORE_POINTS) in (256, 257, 513)
    check_lattice(n, 3)


@pytest.mark.parametrize("H", fo.LATTICE_TABLES)
def test_scoring_lattice_with_the_lds_tables_at_their_limit(H):
    check_lattice(4097, H)


def test_scoring_hypothesis_without_an_inlier_is_all_zero():
    counts, mom = check_lattice(1025, 3, empty_last=True)
    assert counts[-1] == 0 and np.array_equal(mom[-1], np.zeros(9)) and counts[:-1].min() > 0


def test_scoring_sums_dx_not_x():
    """A shift near 2^9, well away from the data: the moments are those of x - sx, y - sy."""
    P, planes, thr, sh, _ = fo.lattice_scene(1025, 3, 1, fo.FAR_SHIFT)
    counts, mom = check_lattice(1025, 3, shift=fo.FAR_SHIFT)
    _, mom_x, _ = fo.lattice_answer(P, planes, thr, np.zeros(2))
    assert not np.array_equal(mom[:, 0], mom_x[:, 0]) and not np.array_equal(mom[:, 3], mom_x[:, 3])


# ---------------------------------------------------------------- b. scoring, float scenes: counts exact, moments within the derived bound
def check_float(P, planes, thr, shift, o, label):
    assert (o["margin_excess"] > 0).all()   # the precondition of exact counts (tests/test_flat_oracle_cpu.py), here for the planes as this host computed them
    counts, mom, _ = gpu_ransac(P, planes, thr, shift)
    assert np.array_equal(counts, o["counts"]), (counts, o["counts"])
    assert np.isfinite(mom).all()
    ratio = fo.moment_ratio(mom, o, len(P))
    print("gpu moments %s: ratio %.3g" % (label, ratio))
    assert ratio <= 1.0, np.argwhere(np.abs(mom.astype(LD) - o["moments"]) > fo.moment_bound(o, len(P)))
    return mom


@pytest.mark.parametrize("n,H,seed", fo.FLOAT_SCENES)
def test_scoring_float_scenes_against_the_oracle(n, H, seed):
    P, planes, thr, shift = fo.float_scene(n, H, seed)
    check_float(P, planes, thr, shift, fo.scene_oracle("float", n, H, seed), "n=%d H=%d" % (n, H))


def test_scoring_ignores_non_finite_points():
    """Points that hold NaN, +inf or -inf are outliers of every hypothesis and leave no trace in a moment: the launch over the scene with them and the launch
    over the scene without them both meet the oracle of the scene without them, and every value is finite."""
    P, planes, thr, shift, bad = fo.nonfinite_scene()
    o = fo.scene_oracle("removed")
    assert np.array_equal(fo.scene_oracle("nonfinite")["counts"], o["counts"])
    with_bad = check_float(P, planes, thr, shift, o, "non-finite points present")
    without = check_float(np.delete(P, bad, axis=0), planes, thr, shift, o, "non-finite points removed")
    # (the two launches differ in which lane holds which point, so in the order of summation: each is within the bound, together within twice)
    assert (np.abs(with_bad - without) <= 2 * fo.moment_bound(o, len(P))).all()


@pytest.mark.parametrize("n", fo.MASK_N)
def test_scoring_mask_float_scene(n):
    P, planes, thr, shift = fo.float_scene(n, 1, fo.MASK_SEED)
    o = fo.scene_oracle("float", n, 1, fo.MASK_SEED)
    assert (o["margin_excess"] > 0).all()
    counts, mom, mask = gpu_ransac(P, planes, thr, shift, want_mask=True)
    assert set(np.unique(mask)) <= {0, 1}
    assert np.array_equal(mask.astype(bool), o["mask"][0])
    assert int(mask.sum()) == int(counts[0]) == int(o["counts"][0])
    assert fo.moment_ratio(mom, o, n) <= 1.0


@pytest.mark.parametrize("n", fo.MASK_N)
def test_scoring_mask_lattice_scene_keeps_the_boundary_points(n):
    P, planes, thr, sh, planted = fo.lattice_scene(n, 1, 2)
    counts0, mom0, mask0 = fo.lattice_answer(P, planes, thr, sh)
    counts, mom, mask = gpu_ransac(P, planes, thr, sh, want_mask=True)
    assert np.array_equal(mask.astype(bool), mask0[0]) and np.array_equal(counts, counts0) and np.array_equal(mom, mom0)
    assert int(mask.sum()) == int(counts[0])
    on, near = planted[np.abs(planted[:, 2]) == 20, 0], planted[np.abs(planted[:, 2]) == 21, 0]
    assert len(on) == 2 and len(near) == 1 and mask[on].all() and not mask[near].any()


# ---------------------------------------------------------------- c. transform and order statistics
@pytest.mark.parametrize("name", ["quarter", "generic"])
@pytest.mark.parametrize("n", fo.TRANSFORM_N)
def test_transform_sums_and_order_statistics(name, n):
    P, rt12, ranks, o = fo.transform_case(name, n)
    values, sums, nans = gpu_order_stats(P, rt12, ranks)
    assert np.array_equal(nans, [0, 0])
    sum_ratio = fo.ratio(np.abs(sums.astype(LD) - o["sums"]), fo.sum_bound(o, n))
    order_ratio = fo.ratio(np.abs(values.astype(LD) - o["values"]), fo.order_bound(o)[:, None])
    print("gpu transform %s n=%d: ratio sums %.3g, order statistics %.3g" % (name, n, sum_ratio, order_ratio))
    assert sum_ratio <= 1.0 and order_ratio <= 1.0, (values, o["values"], sums, o["sums"])
    assert np.array_equal(values[:, 0], values[:, 1]) and np.array_equal(values[:, 6], values[:, 7])   # the duplicated ranks
    if name == "quarter":   # X = -y and Y = x exactly: the order statistics are the inputs' own bits
        assert np.array_equal(values[0], np.sort(-P[:, 1])[ranks]) and np.array_equal(values[1], np.sort(P[:, 0])[ranks])


@pytest.mark.parametrize("name", ["quarter", "generic"])
@pytest.mark.parametrize("n", [257, 1001])
def test_transform_nan_counts_per_coordinate(name, n):
    """NaN and infinities of both signs in the input: NaN-ness of r0 x + r1 y + r2 z + t does not depend on how it is evaluated, so the counts are exact."""
    P, rt12 = fo.nonfinite_points(n), fo.transforms()[name]
    o = fo.transform_oracle(P, rt12)
    ranks = np.arange(8, dtype=np.int64)   # (below the number of values either coordinate has left)
    assert n - int(o["nans"].max()) > 8
    _, sums, nans = gpu_order_stats(P, rt12, ranks)
    assert np.array_equal(nans, o["nans"]), (nans, o["nans"])
    assert np.isnan(sums).all()
    _, _, nans0 = gpu_order_stats(P, rt12, ranks[:0])
    assert np.array_equal(nans0, o["nans"])


# ---------------------------------------------------------------- d. floor points
@pytest.mark.parametrize("down", [False, True])
@pytest.mark.parametrize("K,F", fo.FLOOR_CASES)
def test_floor_points_where_blocks_start_unaligned(K, F, down):
    kp = fp.keypoints(F, K, seed=F + K)
    ix0, rows0 = fo.floor_oracle(kp, down)
    idx, rows = gpu_floor_points(kp, down)
    assert np.array_equal(idx, ix0), np.flatnonzero(idx != ix0)
    assert np.array_equal(rows.view(np.uint64), rows0.view(np.uint64))


@pytest.mark.parametrize("down", [False, True])
@pytest.mark.parametrize("F", [228, 229, 455, 1000])
def test_floor_points_hand_made_frames_in_odd_blocks(F, down):
    """Ties, first NaN, all NaN, signed zeros and infinities in every block, and at the end of every odd block a frame whose LAST keypoint decides."""
    kp = fo.handmade_keypoints(F, 7 if down else 6)
    ix0, rows0 = fo.floor_oracle(kp, down)
    idx, rows = gpu_floor_points(kp, down)
    assert np.array_equal(idx, ix0), np.flatnonzero(idx != ix0)
    assert np.array_equal(rows.view(np.uint64), rows0.view(np.uint64))
    assert idx[min(F, 454) - 1] == 8
