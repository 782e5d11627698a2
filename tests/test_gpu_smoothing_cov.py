"""trajectory_uncertainty on the GPU, through the public calls, on the cases of the host-check tier (tests/test_hostcheck_smoothing_cov.py) and by
the same bar (tests/smoothing_cov_oracle.py): per track |zhat - zhat_ref| <= 4 eps cond max|zhat_ref| over Z_tt and Z_{t,t+1} in Jacobi-scaled
units, against the inverse of the dense matrix; identical bits from two calls, from any chunking and through smooth_trajectories(uncertainty=).
Largest observed error on MI355X: see DESIGN.md section 8f-20."""
import numpy as np
import pytest

import smoothing_cov_oracle as sc
import smoothing_oracle as so

pytestmark = pytest.mark.gpu
LINEAR, ROBUST = so.linear_cases(), so.robust_cases()
FIELDS = ("covariance", "std", "lag_covariance", "status", "n_usable")
SOLVE_FIELDS = ("points", "weights", "mahalanobis2", "status", "n_usable", "n_iterations", "history", "cost")


def run(case, lag=True, **kw):
    from multicam_calibration_amd import trajectory_uncertainty

    args = dict(accel_std=case["accel_std"], segment=case["segment"], lag=lag)
    args.update(kw)
    r = trajectory_uncertainty(case["points"], case["cov"], **args)
    return dict(covariance=r.covariance, std=r.std, lag_covariance=r.lag_covariance, status=r.status, n_usable=r.n_usable, info=r.info)


def same(a, b, fields=FIELDS):
    return all((a[f] is None and b[f] is None) or np.array_equal(a[f], b[f], equal_nan=True) for f in fields)


@pytest.mark.parametrize("name", sorted(LINEAR))
def test_covariance_meets_the_bar(name):
    case = LINEAR[name]
    got = run(case)
    worst = sc.check_case(name, case, got)
    print(f"{name}: levels {got['info']['levels']}, segment {got['info']['segment']}, largest error {worst:.3g} eps cond max|zhat|, kernels {got['info']['kernel_ms']:.3f} ms")
    T, K = case["points"].shape[:2]
    assert got["covariance"].shape == (T, K, 3, 3) and got["std"].shape == (T, K, 3) and got["lag_covariance"].shape == (T - 1, K, 3, 3)
    assert np.array_equal(got["std"], np.sqrt(np.diagonal(got["covariance"], axis1=2, axis2=3)), equal_nan=True)
    if name == "T333_seg2":
        assert got["info"]["levels"] == 5
    if name == "T400_default":   # frames 100 .. 139 missing: the middle of the gap is less certain than its edges
        tr = np.trace(got["covariance"], axis1=2, axis2=3)
        assert (tr[120] > tr[99]).all() and (tr[120] > tr[140]).all()


@pytest.mark.parametrize("name", sorted(ROBUST))
def test_covariance_at_given_weights_meets_the_bar(name):
    case = ROBUST[name]
    win = np.stack([o["weights"] for o in so.robust_reference(name, case)], axis=1)
    worst = sc.check_case(name, case, run(case, weights=win), weights=win)
    print(f"{name}: largest error {worst:.3g} eps cond max|zhat|")


def test_through_the_smoother_and_the_solve_unchanged():
    """uncertainty="lag" is trajectory_uncertainty at the returned weights, bit for bit; True leaves the lag plane out; and the solve itself is
    the same bits with and without"""
    from multicam_calibration_amd import smooth_trajectories, trajectory_uncertainty

    case = ROBUST["soft_l1_36"]
    kw = dict(accel_std=case["accel_std"], loss=case["loss"], f_scale=case["f_scale"], segment=case["segment"])
    plain = smooth_trajectories(case["points"], case["cov"], **kw)
    assert plain.covariance is None and plain.std is None and plain.lag_covariance is None
    again = smooth_trajectories(case["points"], case["cov"], uncertainty=False, **kw)
    both = smooth_trajectories(case["points"], case["cov"], uncertainty="lag", **kw)
    diag = smooth_trajectories(case["points"], case["cov"], uncertainty=True, **kw)
    for r in (again, both, diag):
        assert all(np.array_equal(getattr(plain, f), getattr(r, f), equal_nan=True) for f in SOLVE_FIELDS)
    u = trajectory_uncertainty(case["points"], case["cov"], accel_std=case["accel_std"], weights=plain.weights, lag=True, segment=case["segment"])
    assert (plain.weights < 0.5).any() and np.isfinite(u.covariance).all()
    assert np.array_equal(both.covariance, u.covariance) and np.array_equal(both.std, u.std) and np.array_equal(both.lag_covariance, u.lag_covariance)
    assert np.array_equal(diag.covariance, u.covariance) and np.array_equal(diag.std, u.std) and diag.lag_covariance is None
    for k, t in zip(*np.nonzero((plain.weights < 0.5).T)):   # a discounted frame is less certain than with its full weight
        break
    full = trajectory_uncertainty(case["points"], case["cov"], accel_std=case["accel_std"], segment=case["segment"])
    assert np.trace(u.covariance[t, k]) > np.trace(full.covariance[t, k])


def test_two_calls_return_the_same_bits():
    for name in ("T333_seg2", "gaps_seg3", "T400_default"):
        assert same(run(LINEAR[name]), run(LINEAR[name])), name


def test_chunks_over_tracks_return_the_same_bits(monkeypatch):
    case = LINEAR["T400_seg2"]
    big = dict(case, points=np.concatenate([case["points"]] * 3, axis=1)[:, :5].copy(), cov=np.concatenate([case["cov"]] * 3, axis=1)[:, :5].copy())
    big["points"][:, 3] = np.nan   # a track that is never launched, in the middle of a chunk
    whole = run(big)
    monkeypatch.setenv("MCBA_SMOOTH_BUDGET_MB", "0.5")
    parts = run(big)
    print(whole["info"], parts["info"])
    assert whole["info"]["chunks"] == 1 and parts["info"]["chunks"] >= 2 and parts["info"]["tracks_per_chunk"] < 5
    assert same(whole, parts)
    assert whole["status"][3] == -1 and np.isnan(whole["covariance"][:, 3]).all() and np.array_equal(whole["covariance"][:, 0], whole["covariance"][:, 2])
    assert np.array_equal(whole["lag_covariance"][:, 0], whole["lag_covariance"][:, 4]) and np.isfinite(whole["covariance"][:, [0, 1, 2, 4]]).all()


def test_a_chunk_in_which_no_track_is_launched(monkeypatch):
    """one track per chunk, the middle one without a usable frame: its chunk launches nothing"""
    s = so.scene(40, 3, seed=2)
    s["points"][:, 1] = np.nan
    case = dict(points=s["points"], cov=s["cov"], accel_std=0.1, segment=3)
    whole = run(case)
    monkeypatch.setenv("MCBA_SMOOTH_BUDGET_MB", "0.001")
    parts = run(case)
    print(whole["info"], parts["info"])
    assert whole["info"]["chunks"] == 1 and parts["info"]["chunks"] == 3 and parts["info"]["tracks_per_chunk"] == 1
    assert same(whole, parts)
    assert list(parts["status"]) == [1, -1, 1] and list(parts["n_usable"]) == [40, 0, 40]
    assert np.isnan(parts["covariance"][:, 1]).all() and np.isnan(parts["std"][:, 1]).all() and np.isnan(parts["lag_covariance"][:, 1]).all()
    assert np.isfinite(parts["covariance"][:, [0, 2]]).all() and np.isfinite(parts["lag_covariance"][:, [0, 2]]).all()


def test_long_tracks_default_segment_against_segment_two():
    """5000 frames x 7 tracks: the default segment against segment=2 within the sum of the two bars, the condition number and max|zhat| taken
    from the first 400 frames (the system is local: neither grows with the length of a stationary scene); that sub-case against the reference"""
    s = so.scene(5000, 7, seed=12, gaps=[(100, 140), (3000, 3001), (4990, 5000)])
    acc = np.linspace(0.03, 0.09, 7)
    case = dict(points=s["points"], cov=s["cov"], accel_std=acc, segment=None)
    sub = dict(points=s["points"][:400], cov=s["cov"][:400], accel_std=acc, segment=None)
    sc.check_case("T5000_sub400", sub, run(sub))
    a, b = run(case), run(case, segment=2)
    assert a["info"]["segment"] == 16 and b["info"]["segment"] == 2 and a["info"]["levels"] < b["info"]["levels"]
    for k, ref in enumerate(sc.case_reference("T5000_sub400", sub)):
        other = dict(diag=b["covariance"][:, k], lag=b["lag_covariance"][:, k], s=np.sqrt(so.system(s["points"][:, k], s["cov"][:, k], acc[k], dense=False)["ab"][8]))
        err, bar = sc.scaled_error(a["covariance"][:, k], a["lag_covariance"][:, k], other), 2 * sc.bar_of(ref)
        print(f"track {k}: cond {ref['cond']:.3g} default segment against segment 2: {err:.3g} (two bars {bar:.3g})")
        assert a["status"][k] == 1 and b["status"][k] == 1 and err <= bar
    assert np.array_equal(a["n_usable"], np.isfinite(s["points"][:, :, 0]).sum(axis=0))


def test_bad_tracks_are_nan_beside_an_unaffected_neighbour():
    """status -2 (an accel_std whose inverse square is finite but six times it is not), status -1 (one usable frame), and a good track between"""
    s = so.scene(40, 3, seed=2)
    s["points"][1:, 2] = np.nan
    case = dict(points=s["points"], cov=s["cov"], accel_std=np.array([1e-154, 0.1, 0.1]), segment=3)
    got = run(case)
    alone = run(dict(points=s["points"][:, 1:2], cov=s["cov"][:, 1:2], accel_std=0.1, segment=3))
    assert list(got["status"]) == [-2, 1, -1] and list(got["n_usable"]) == [40, 40, 1]
    for k in (0, 2):
        assert np.isnan(got["covariance"][:, k]).all() and np.isnan(got["std"][:, k]).all() and np.isnan(got["lag_covariance"][:, k]).all()
    assert np.array_equal(got["covariance"][:, 1], alone["covariance"][:, 0]) and np.array_equal(got["lag_covariance"][:, 1], alone["lag_covariance"][:, 0])


def test_without_lag_no_lag_plane_is_written():
    """lag=False: None in Python, and the C call with a NULL out_lag9 returns the same covariances and leaves a plane it was not given alone"""
    import ctypes

    from multicam_calibration_amd import ops

    case = LINEAR["gaps_seg3"]
    with_lag, without = run(case), run(case, lag=False)
    assert without["lag_covariance"] is None and np.array_equal(with_lag["covariance"], without["covariance"])
    pts, c6 = np.ascontiguousarray(case["points"]), so.pack6(case["cov"])
    T, K = pts.shape[:2]
    acc = np.full(K, case["accel_std"])
    oc, guard = np.full((T, K, 6), 7.0), np.full((T - 1, K, 9), 7.0)
    st, nu, info = np.zeros(K, np.int32), np.zeros(K, np.int32), np.zeros(8)
    ops.call("mcba_smooth_covariance", T, K, pts.ctypes.data, c6.ctypes.data, acc.ctypes.data, None, case["segment"], 0, oc.ctypes.data, None, st.ctypes.data, nu.ctypes.data, info.ctypes.data, None)
    assert (guard == 7.0).all() and (st == 1).all()
    i = np.array([[0, 1, 2], [1, 3, 4], [2, 4, 5]])
    assert np.array_equal(oc[..., i], with_lag["covariance"])
    assert info[6] < with_lag["info"]["device_bytes"]   # no lag plane on the device either
