"""Floor-plane alignment on the MI355X: get_floor_points bit-exact against numpy, flatibrate against the reference's goldens (same
n_trials, inlier mask and post-call global RNG state; transform within 1e-9), center_arena's order statistics bit-exact against numpy,
the tutorial chain, and run-to-run bitwise reproducibility of the scoring kernel."""
import numpy as np
import pytest

import flat_problem as fp

pytestmark = pytest.mark.gpu


def golden_state(z, name):
    s = z[f"{name}_state"]
    return s[:624].astype(np.uint32), int(s[624]), int(s[625]), float(z[f"{name}_gauss"])


def assert_state(z, name):
    key, pos, has_gauss, gauss = golden_state(z, name)
    st = np.random.get_state()
    assert np.array_equal(st[1], key) and st[2] == pos and st[3] == has_gauss and st[4] == gauss


@pytest.mark.parametrize("down", [False, True])
@pytest.mark.parametrize("F,K", [(1, 1), (7, 3), (1000, 12), (100003, 12), (5000, 31), (300, 700)])
def test_get_floor_points_is_numpy_bit_for_bit(F, K, down):
    import multicam_calibration_amd as m

    kp = fp.keypoints(F, K, seed=F + K)
    got, idx = m.get_floor_points(kp, z_points_down=down, return_index=True)
    ref_ix = np.argmax(kp[:, :, 2], axis=1) if down else np.argmin(kp[:, :, 2], axis=1)
    assert np.array_equal(idx, ref_ix)
    ref = kp[np.arange(F), ref_ix]
    assert np.array_equal(got.view(np.uint64), ref.view(np.uint64))


def test_get_floor_points_ties_nan_and_lists():
    import multicam_calibration_amd as m

    kp = np.zeros((6, 4, 3))
    kp[:, :, :2] = np.arange(8).reshape(4, 2)
    kp[0, :, 2] = [3, 1, 1, 2]             # tie: first index
    kp[1, :, 2] = [3, np.nan, 0, np.nan]   # the first NaN wins
    kp[2, :, 2] = np.nan                   # all NaN: index 0
    kp[3, :, 2] = [-0.0, 0.0, -1.0, -1.0]
    kp[4, :, 2] = [np.inf, -np.inf, -np.inf, 5]
    kp[5, :, 2] = [np.nan, 1, 2, 3]
    for down in (False, True):
        _, idx = m.get_floor_points([kp[:3], kp[3:]], z_points_down=down, return_index=True)
        assert np.array_equal(idx, (np.argmax if down else np.argmin)(kp[:, :, 2], axis=1))
    assert m.get_floor_points(kp.astype(np.float32)).dtype == np.float32


@pytest.mark.parametrize("name", list(fp.CASES))
def test_flatibrate_matches_the_reference(golden, name):
    import multicam_calibration_amd as m
    from multicam_calibration_amd import flatibration as fl

    z = golden("flatibration.npz")
    P = fp.case_points(name)
    gseed = fp.CASES[name][3]
    np.random.seed(gseed)
    (a, b, c), n_trials, stats = fl.ransac_plane(P, fp.THRESHOLD, return_stats=True)
    # a tie in inlier count decided by an R^2 difference below ~1e-12 could go the other way than numpy's pairwise sums: none here
    assert stats["tie_margin"] > 1e-10
    assert n_trials == int(z[f"{name}_n_trials"])
    assert_state(z, name)
    np.testing.assert_allclose([a, b, c], z[f"{name}_coef"], rtol=1e-9, atol=1e-9)
    np.random.seed(gseed)
    t, mask = m.flatibrate(P, residual_threshold=fp.THRESHOLD, return_inliers=True)
    assert np.array_equal(mask, z[f"{name}_inliers"])
    assert int(stats["counts"][stats["best"]]) == int(mask.sum())
    assert_state(z, name)
    np.testing.assert_allclose(t, z[f"{name}_transform"], rtol=1e-9, atol=1e-12 * np.abs(z[f"{name}_transform"]).max())


@pytest.mark.parametrize("name", ["n50", "n300", "n5000", "n100k"])
def test_center_arena_matches_the_reference(golden, name):
    import multicam_calibration_amd as m

    z = golden("flatibration.npz")
    P = fp.case_points(name)
    t = z[f"{name}_transform"]
    for method, kw in (("midrange", {}), ("mean", {}), ("median", {}), ("midrange5", dict(range_pctl=5))):
        got = m.center_arena(t, P, center_method=method.rstrip("5"), **kw)
        ref = z[f"{name}_center_{method}"]
        np.testing.assert_allclose(got, ref, rtol=1e-12, atol=1e-12 * np.abs(P).max())


@pytest.mark.parametrize("n", [1, 2, 3, 1000, 1001, 256 * 2049 + 17])
def test_order_statistics_are_numpys_bit_for_bit(n):
    from multicam_calibration_amd import flatibration as fl

    rng = np.random.default_rng(n)
    P = rng.normal(size=(n, 3)) * [100.0, 1e-3, 5.0]
    P[: n // 3, 0] = np.round(P[: n // 3, 0])  # repeated values
    if n > 2:
        P[1, 1] = -0.0
    for pctl in (0, 1, 2.5, 50):
        got = fl.arena_center(np.zeros(6), P, "midrange", pctl)
        ref = np.percentile(P[:, :2], [pctl, 100 - pctl], axis=0).mean(axis=0)
        assert np.array_equal(got, ref), (pctl, got, ref)
    assert np.array_equal(fl.arena_center(np.zeros(6), P, "median"), np.median(P[:, :2], axis=0))
    got, ref = fl.arena_center(np.zeros(6), P, "mean"), np.mean(P[:, :2], axis=0)
    assert np.all(np.abs(got - ref) <= 1e-12 * np.abs(P[:, :2]).max(axis=0)), (got, ref)


def test_center_arena_nan_is_nan():
    from multicam_calibration_amd import flatibration as fl

    P = fp.floor_points(1000, 0.2, 3)
    P[10, 1] = np.nan
    for method in ("midrange", "median", "mean"):
        got = fl.arena_center(np.zeros(6), P, method)
        # the reference maps the points by a 4 x 4 product with (x, y, z, 1), so a NaN in any coordinate reaches every transformed one
        pts = (np.c_[P, np.ones(len(P))] @ np.eye(4).T)[:, :2]
        ref = {"midrange": lambda v: np.percentile(v, [1, 99], axis=0).mean(axis=0), "median": lambda v: np.median(v, axis=0), "mean": lambda v: np.mean(v, axis=0)}[method](pts)
        assert np.isnan(ref).all() and np.isnan(got).all()


def test_tutorial_chain(golden):
    import multicam_calibration_amd as m

    z = golden("flatibration.npz")
    kp = -fp.keypoints(20000, 12, seed=21)
    fl_pts = m.get_floor_points(kp, z_points_down=True)
    fl_pts = fl_pts[np.isfinite(fl_pts).all(axis=1)]
    np.random.seed(8)
    t = m.flatibrate(fl_pts)
    t = m.center_arena(t, fl_pts, center_method="midrange")
    t = m.flip_z_axis(t)
    np.testing.assert_allclose(t, z["tutorial_transform"], rtol=1e-9, atol=1e-9)
    assert_state(z, "tutorial")


def test_scoring_is_bitwise_reproducible():
    from multicam_calibration_amd import flatibration as fl

    P = fp.floor_points(10**6, 0.6, 99)
    runs = []
    for _ in range(2):
        np.random.seed(1)
        plane, n_trials, stats = fl.ransac_plane(P, fp.THRESHOLD, forced_trials=100, return_stats=True)
        runs.append((np.asarray(plane), stats["counts"], stats["scores"]))
    assert n_trials == 100
    for x, y in zip(*runs):
        assert np.array_equal(np.asarray(x).view(np.uint64), np.asarray(y).view(np.uint64))
