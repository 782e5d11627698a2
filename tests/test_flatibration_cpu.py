"""Floor-plane alignment, CPU tier: the host half of flatibrate() (sklearn's subset draws, its sequential loop, its final fit) against
sklearn itself, the transform construction and flip_z_axis against the reference's goldens, and the loud error without a GPU.

The kernel's per-hypothesis outputs (inlier count + moments) are restated here in numpy as a test stand-in; the library itself has no
such path."""
import ctypes

import numpy as np
import pytest

import flat_problem as fp


def moments_numpy(P, planes, thr):
    """What mcba_flat_ransac returns, computed on the host (test stand-in)."""
    shift = P[0, :2]
    counts, mom = np.zeros(len(planes), dtype=np.uint64), np.zeros((len(planes), 9))
    for h, (a, b, c) in enumerate(planes):
        r = P[:, 2] - (P[:, 1] * b + P[:, 0] * a + c)
        m = np.abs(r) <= thr
        u, v, w = P[m, 0] - shift[0], P[m, 1] - shift[1], r[m]
        counts[h] = m.sum()
        mom[h] = [u.sum(), v.sum(), w.sum(), u @ u, u @ v, v @ v, u @ w, v @ w, w @ w]
    return counts, mom, shift


def host_ransac(P, thr):
    from multicam_calibration_amd import flatibration as fl

    idx, states = fl.draw_subsets(len(P))
    planes = fl.hypotheses(P, idx)
    counts, mom, shift = moments_numpy(P, planes, thr)
    best, n_trials, margin = fl.replay(counts, fl.r2_scores(planes, counts, mom), len(P))
    return fl.final_fit(planes[best], counts[best], mom[best], shift), n_trials, planes[best], states[n_trials], margin


@pytest.mark.parametrize("n,frac,seed", [(3, 0.0, 1), (4, 0.0, 2), (7, 0.3, 3), (50, 0.2, 4), (299, 0.5, 5), (300, 0.3, 6), (301, 0.6, 7), (2000, 0.65, 8),
                                         (5000, 0.1, 9)])
def test_draws_replay_and_final_fit_match_sklearn(n, frac, seed):
    pytest.importorskip("sklearn")
    from sklearn.linear_model import RANSACRegressor

    from multicam_calibration_amd import flatibration as fl

    P = fp.floor_points(n, frac, seed)
    np.random.seed(seed)
    r = RANSACRegressor(residual_threshold=fp.THRESHOLD).fit(P[:, :2], P[:, 2])
    after = np.random.get_state()
    np.random.seed(seed)
    (a, b, c), n_trials, plane, state, margin = host_ransac(P, fp.THRESHOLD)
    assert margin > 1e-10
    assert n_trials == r.n_trials_
    mask = np.abs(P[:, 2] - (P[:, 1] * plane[1] + P[:, 0] * plane[0] + plane[2])) <= fp.THRESHOLD
    assert np.array_equal(mask, r.inlier_mask_)
    np.testing.assert_allclose([a, b, c], np.r_[r.estimator_.coef_, r.estimator_.intercept_], rtol=1e-9, atol=1e-9)
    assert all(np.array_equal(x, y) for x, y in zip(state, after))


def test_subset_draws_are_sklearns():
    pytest.importorskip("sklearn")
    from sklearn.utils.random import sample_without_replacement

    from multicam_calibration_amd import flatibration as fl

    for n in (3, 4, 50, 299, 300, 301, 10**6):
        a, b = np.random.RandomState(n), np.random.RandomState(n)
        for _ in range(20):
            assert np.array_equal(fl.sample_subset(n, a), sample_without_replacement(n, 3, random_state=b))
        assert all(np.array_equal(x, y) for x, y in zip(a.get_state(), b.get_state()))


def test_draw_subsets_leaves_the_global_rng_alone():
    from multicam_calibration_amd import flatibration as fl

    np.random.seed(3)
    before = np.random.get_state()
    idx, states = fl.draw_subsets(1000)
    assert idx.shape == (100, 3) and len(states) == 101
    assert all(np.array_equal(x, y) for x, y in zip(before, np.random.get_state()))


def test_dynamic_max_trials_is_sklearns():
    pytest.importorskip("sklearn")
    from sklearn.linear_model._ransac import _dynamic_max_trials

    from multicam_calibration_amd import flatibration as fl

    for n_in, n in [(1, 10), (3, 3), (10, 100), (700, 1000), (999, 1000), (0, 5)]:
        assert fl.dynamic_max_trials(n_in, n) == _dynamic_max_trials(n_in, n, 3, 0.99)


def test_transform_construction_matches_the_reference(golden):
    from multicam_calibration_amd import flatibration as fl

    z = golden("flatibration.npz")
    for name in fp.CASES:
        t = fl.plane_transform(*z[f"{name}_coef"])
        np.testing.assert_allclose(t, z[f"{name}_transform"], rtol=1e-9, atol=1e-12)


def test_flip_z_axis_matches_the_reference(golden):
    import multicam_calibration_amd as m

    z = golden("flatibration.npz")
    for name in fp.CASES:
        np.testing.assert_allclose(m.flip_z_axis(z[f"{name}_transform"]), z[f"{name}_flip"], rtol=1e-9, atol=1e-12)


def test_percentile_interpolation_is_numpys():
    """center_arena's host half: the ranks it asks the device for and numpy's lerp of them, against np.percentile on sorted data."""
    from multicam_calibration_amd import flatibration as fl

    rng = np.random.default_rng(0)
    for n in (1, 2, 3, 10, 99, 100, 101, 1000, 12345):
        v = np.sort(rng.normal(size=n) * 100)
        for pctl in (0, 1, 2.5, 5, 33.3, 50):
            q = np.true_divide(np.asarray([pctl, 100 - pctl]), 100)
            prev, nxt, gamma = fl._percentile_ranks(n, q)
            got = fl._lerp(v[prev], v[nxt], gamma)
            assert np.array_equal(got, np.percentile(v, [pctl, 100 - pctl])), (n, pctl)


def test_library_does_not_import_sklearn():
    import subprocess
    import sys

    code = "import sys; import multicam_calibration_amd; assert 'sklearn' not in sys.modules"
    subprocess.check_call([sys.executable, "-c", code], cwd=fp.__file__.rsplit("/tests/", 1)[0])


def test_bad_input_is_a_value_error():
    import multicam_calibration_amd as m

    with pytest.raises(ValueError):
        m.flatibrate(np.zeros((2, 3)))
    P = fp.floor_points(50, 0.2, 1)
    P[3, 2] = np.nan
    with pytest.raises(ValueError):
        m.flatibrate(P)
    P[3, 2] = np.inf
    with pytest.raises(ValueError):
        m.flatibrate(P)
    with pytest.raises(ValueError, match="center_method should be 'midrange', 'mean', or 'median'"):
        m.center_arena(np.zeros(6), P, center_method="mode")


def test_no_gpu_is_a_loud_error():
    import multicam_calibration_amd as m
    from multicam_calibration_amd import ops

    n = ctypes.c_int()
    rc = ops.load_library().mcba_device_count(ctypes.byref(n))
    if rc == 0 and n.value > 0:
        pytest.skip("a GPU is visible here")
    np.random.seed(0)
    before = np.random.get_state()
    P = fp.floor_points(100, 0.2, 1)
    for call in (lambda: m.get_floor_points(fp.keypoints(10, 4, 0)), lambda: m.flatibrate(P), lambda: m.center_arena(np.zeros(6), P),
                 lambda: m.center_arena(np.zeros(6), P, center_method="mean")):
        with pytest.raises(ops.McbaError):
            call()
    assert all(np.array_equal(x, y) for x, y in zip(before, np.random.get_state()))
