"""tests/flat_oracle.py proven without a GPU: the long-double statement of mcba_flat_ransac against the numpy stand-in of test_flatibration_cpu.py within
the derived bound and against int64 arithmetic exactly, the decision-margin precondition of every float scene the GPU tests use (under which the kernel's
counts must equal the oracle's), the sup-norm argument and the rounding bound of the transform, and the inputs of the floor-point tests.  Each test that
measures prints `ratio` = worst error / derived bound."""
import numpy as np
import pytest

import flat_oracle as fo
import flat_problem as fp
from test_flatibration_cpu import moments_numpy

LD = np.longdouble
FLOAT_KEYS = [("float",) + s for s in fo.FLOAT_SCENES] + [("float", n, 1, fo.MASK_SEED) for n in fo.MASK_N] + [("nonfinite",), ("removed",)]


@pytest.mark.parametrize("n,H,seed", fo.FLOAT_SCENES + tuple((n, 1, fo.MASK_SEED) for n in fo.MASK_N))
def test_oracle_agrees_with_the_numpy_stand_in(n, H, seed):
    P, planes, thr, shift = fo.float_scene(n, H, seed)
    o = fo.scene_oracle("float", n, H, seed)
    counts, mom, sh = moments_numpy(P, planes, thr)
    assert np.array_equal(sh, shift)
    assert np.array_equal(counts, o["counts"])
    ratio = fo.moment_ratio(mom, o, n)
    print("host moments n=%d H=%d: ratio %.3g" % (n, H, ratio))
    assert ratio <= 1.0
    assert o["counts"].max() > n // 8 or H == 1   # (some hypothesis lies along the floor: the sums are long)


def test_the_bound_notices_one_wrong_inlier():
    """A moment set that lacks ONE inlier (or holds one too many) is outside the bound in XX or YY: the bound is no wider than a single term."""
    n, H, seed = fo.FLOAT_SCENES[1]
    P, planes, thr, shift = fo.float_scene(n, H, seed)
    o = fo.scene_oracle("float", n, H, seed)
    h = int(np.argmax(o["counts"]))
    for p in (int(np.flatnonzero(o["mask"][h])[-1]), int(np.flatnonzero(~o["mask"][h])[0])):
        m = o["mask"][h].copy()
        m[p] = not m[p]
        dx, dy = P[m, 0] - shift[0], P[m, 1] - shift[1]
        bound = fo.moment_bound(o, n)[h]
        assert abs(LD(dx @ dx) - o["moments"][h, 3]) > bound[3] or abs(LD(dy @ dy) - o["moments"][h, 5]) > bound[5]


def lattice_cases():
    return [(n, 3, None, False) for n in fo.LATTICE_EDGES + fo.LATTICE_STRIDED] + [(4097, H, None, False) for H in fo.LATTICE_TABLES] + [(1025, 3, None, True), (1025, 3, fo.FAR_SHIFT, False)]


@pytest.mark.parametrize("n,H,shift,empty_last", lattice_cases())
def test_oracle_is_exact_on_the_lattice(n, H, shift, empty_last):
    P, planes, thr, sh, planted = fo.lattice_scene(n, H, 1, shift, empty_last)
    assert np.abs(P).max() < 2 ** 10 and np.abs(sh).max() < 2 ** 10 and np.array_equal(P, np.rint(P))
    counts, mom, mask = fo.lattice_answer(P, planes, thr, sh)
    o = fo.ransac_oracle(P, planes, thr, sh)
    assert np.array_equal(o["counts"], counts) and np.array_equal(o["mask"], mask)
    assert np.array_equal(o["moments"], mom.astype(LD))
    # the planted points sit where the scene says: r = +-thr inside, |r| = thr + 1/8 outside
    assert len(planted) == min(n, 3 * (H - empty_last))
    for p, h, R8 in planted:
        r = P[p, 2] - (planes[h, 0] * P[p, 0] + planes[h, 1] * P[p, 1] + planes[h, 2])
        assert r == R8 / 8.0 and mask[h, p] == (abs(R8) == 8 * thr)
    if n >= 3 * H:
        live = H - empty_last
        assert sorted(set(map(tuple, planted[:, 1:]))) == sorted((h, R8) for h in range(live) for R8 in (20, -20, 21 if h % 2 else -21))
    if empty_last:
        assert counts[-1] == 0 and not mom[-1].any() and counts[:-1].min() > 0
    if shift is not None:   # x itself summed instead of dx would be another number
        assert abs(mom[0, 0] - P[mask[0], 0].sum()) > 1000


@pytest.mark.parametrize("key", FLOAT_KEYS, ids=lambda k: "-".join(map(str, k)))
def test_decision_margin_exceeds_the_rounding_of_r(key):
    """No (point, hypothesis) pair of the float scenes lies within delta_r of the threshold, so the kernel's counts and mask must equal the oracle's."""
    o = fo.scene_oracle(*key)
    print("%s: smallest margin %.3g, smallest margin - delta_r %.3g" % (key, o["margin"].min(), o["margin_excess"].min()))
    assert (o["margin_excess"] > 0).all()


def test_non_finite_points_are_outliers_of_every_hypothesis():
    P, planes, thr, shift, bad = fo.nonfinite_scene()
    o, removed = fo.scene_oracle("nonfinite"), fo.scene_oracle("removed")
    assert not np.isfinite(P[bad]).all(axis=1).any() and not o["mask"][:, bad].any()
    assert np.array_equal(o["counts"], removed["counts"])
    assert np.isfinite(np.asarray(o["moments"], dtype=np.float64)).all()
    # the same inliers in the same order: the long-double sums differ by no more than their own summation error
    assert (np.abs(o["moments"] - removed["moments"]) <= fo.ORACLE_DEPTH * 2 * fo.ULD * o["abs_sums"]).all()


@pytest.mark.parametrize("name", ["quarter", "generic"])
@pytest.mark.parametrize("n", fo.TRANSFORM_N)
def test_transform_bounds_on_the_host(name, n):
    """The double evaluation of R p + t is within delta_i of the oracle point by point; the order statistics of the double values are within max delta_i
    (the sup-norm argument, also checked by moving the long-double values by +-delta_i); numpy's sums are within the sum bound."""
    P, rt12, ranks, o = fo.transform_case(name, n)
    R, t = rt12[:9].reshape(3, 3), rt12[9:]
    dbl = np.stack([R[c, 0] * P[:, 0] + R[c, 1] * P[:, 1] + R[c, 2] * P[:, 2] + t[c] for c in range(2)])
    point_ratio = fo.ratio(np.abs(dbl.astype(LD) - o["xy"]), o["delta"])
    ob, sb = fo.order_bound(o), fo.sum_bound(o, n)
    got = np.sort(dbl, axis=1)[:, ranks]
    order_ratio = fo.ratio(np.abs(got.astype(LD) - o["values"]), ob[:, None])
    sum_ratio = fo.ratio(np.abs(dbl.sum(axis=1).astype(LD) - o["sums"]), sb)
    print("host transform %s n=%d: ratio point %.3g, order statistics %.3g, sums %.3g" % (name, n, point_ratio, order_ratio, sum_ratio))
    assert point_ratio <= 1.0 and order_ratio <= 1.0 and sum_ratio <= 1.0
    assert np.array_equal(o["values"], np.stack([o["sorted"][c][ranks] for c in range(2)]))
    rng = np.random.default_rng(n)
    for sign in (np.ones((2, n)), -np.ones((2, n)), rng.choice([-1.0, 1.0], (2, n)), rng.uniform(-1, 1, (2, n))):
        moved = np.sort(o["xy"] + sign * o["delta"], axis=1)[:, ranks]
        # (the check's own long-double arithmetic rounds the moved value and the difference: 4 ULD of the largest value)
        assert (np.abs(moved - o["values"]) <= o["delta"].max(axis=1)[:, None] + 4 * fo.ULD * np.abs(o["xy"]).max()).all()


@pytest.mark.parametrize("name", ["quarter", "generic"])
def test_nan_counts_do_not_depend_on_the_evaluation(name):
    """NaN-ness of r0 x + r1 y + r2 z + t from three evaluations: the oracle's (double, left to right), long double, and a matrix product."""
    n = 1001
    P, rt12 = fo.nonfinite_points(n), fo.transforms()[name]
    o = fo.transform_oracle(P, rt12)
    with np.errstate(invalid="ignore"):
        mat = (P @ rt12[:9].reshape(3, 3).T + rt12[9:])[:, :2]
    assert np.array_equal(o["nans"], np.isnan(mat).sum(axis=0)) and np.array_equal(o["nans"], np.isnan(o["xy"]).sum(axis=1))
    assert o["nans"].min() >= 3 and (name == "generic" or o["nans"][0] != o["nans"][1])


def test_floor_oracle_and_the_floor_cases():
    """np.argmin / np.argmax semantics stated by hand on the hand-made frames, and the parities that put the floor-point cases on the scalar staging branch."""
    kp = fo.handmade_frames()
    up, rows = fo.floor_oracle(kp, False)
    down, _ = fo.floor_oracle(kp, True)
    assert list(up) == [1, 1, 0, 2, 1, 0, 8, 1] and list(down) == [0, 1, 0, 0, 0, 0, 5, 8]
    assert np.array_equal(rows[6], kp[6, 8]) and np.signbit(fo.floor_oracle(kp, True)[1][3, 2])   # (the first of the equal zeros is the negative one)
    assert fo.frames_per_block(9) == 227 and fo.frames_per_block(2047) == 1 and fo.frames_per_block(2048) == 1 and fo.frames_per_block(682) == 3
    odd_counts = set()
    for K, F in fo.FLOOR_CASES:
        fpb, row = fo.frames_per_block(K), 3 * K
        for b in range(-(-F // fpb)):
            if (b * fpb * row) % 2:   # an odd first double: the scalar branch
                odd_counts.add((K, ((min(F, (b + 1) * fpb) - b * fpb) * row) % 2))
    assert odd_counts == {(9, 0), (9, 1), (2047, 1)}
    for decisive, down_ in ((6, False), (7, True)):
        kp = fo.handmade_keypoints(1000, decisive)
        ix, _ = fo.floor_oracle(kp, down_)
        assert ix[453] == 8 and ix[907] == 8 and np.isnan(kp[226, :, 2]).all()
    kp = fp.keypoints(455, 9, seed=464)
    assert np.isnan(kp).any() and (np.sort(kp[:, :, 2], axis=1)[:, 0] == np.sort(kp[:, :, 2], axis=1)[:, 1]).any()   # NaN and ties are there
