"""smooth_trajectories on the GPU, through the public call, on the cases of the host-check tier (tests/test_hostcheck_smoothing.py) and by the same
rules (tests/smoothing_oracle.py): a linear solve -- loss="linear", or max_iterations=1 with the reference's converged weights -- within
4 eps cond max|x| of scipy's banded solve per track; the robust loop by its own definition; identical bits from two calls and from any chunking.
Largest observed error of a linear solve on MI355X: see DESIGN.md section 8f-19."""
import numpy as np
import pytest

import smoothing_oracle as so

pytestmark = pytest.mark.gpu
LINEAR, ROBUST = so.linear_cases(), so.robust_cases()
FIELDS = ("points", "weights", "mahalanobis2", "status", "n_usable", "n_iterations", "history", "cost")


def run(case, **kw):
    from multicam_calibration_amd import smooth_trajectories

    args = dict(accel_std=case["accel_std"], loss=case.get("loss", "linear"), f_scale=case.get("f_scale", 3.0), segment=case["segment"])
    args.update(kw)
    r = smooth_trajectories(case["points"], case["cov"], **args)
    return dict(points=r.points, weights=r.weights, mahalanobis2=r.mahalanobis2, status=r.status, n_usable=r.n_usable, n_iterations=r.n_iterations, history=r.history, cost=r.cost, info=r.info)


@pytest.mark.parametrize("name", sorted(LINEAR))
def test_linear_solve_meets_the_bar(name):
    case = LINEAR[name]
    got = run(case)
    worst = so.check_linear(name, case, got)
    print(f"{name}: levels {got['info']['levels']}, segment {got['info']['segment']}, largest error {worst:.3g} eps cond max|x|, kernels {got['info']['kernel_ms']:.3f} ms")
    for k, (o, c) in enumerate(so.linear_reference(name, case)):
        if o["status"] == 1:
            assert abs(got["cost"][k] - o["cost"]) <= 1e-9 * max(1.0, o["cost"]) + 100 * so.EPS * c * o["cost"]
        else:
            assert np.isnan(got["cost"][k])
    if name == "T333_seg2":
        assert got["info"]["levels"] == 5


@pytest.mark.parametrize("name", sorted(ROBUST))
def test_one_evaluation_with_converged_weights_meets_the_bar(name):
    case = ROBUST[name]
    win = np.stack([o["weights"] for o in so.robust_reference(name, case)], axis=1)
    got = run(case, weights_in=win, max_iterations=1)
    for k in range(win.shape[1]):
        s = so.system(case["points"][:, k], case["cov"][:, k], case["accel_std"], win[:, k])
        err, bar = so.linear_bar(got["points"][:, k], so.solve(s), so.cond(s))
        print(f"{name} track {k}: err {err:.3g} bar {bar:.3g} ratio {err / (bar / so.BAR_K):.3g}")
        assert err <= bar and got["n_iterations"][k] == 1 and got["status"][k] == 1


def test_robust_loop_and_identical_bits():
    left_out = total = 0
    for name, case in ROBUST.items():
        got = run(case)
        left_out += so.check_robust(name, case, got)
        total += case["points"].shape[1]
        again = run(case)
        assert all(np.array_equal(got[f], again[f], equal_nan=True) for f in FIELDS), name
    assert 10 * left_out <= total, (left_out, total)


def test_long_tracks_default_segment_against_segment_two():
    """5000 frames x 7 tracks: the default segment against segment=2 within the bar, the condition number taken from the first 400 frames (the
    system is local: the condition number of a stationary scene does not grow with its length); that sub-case itself against the reference"""
    s = so.scene(5000, 7, seed=12, gaps=[(100, 140), (3000, 3001), (4990, 5000)])
    case = dict(points=s["points"], cov=s["cov"], accel_std=np.linspace(0.03, 0.09, 7), segment=None)
    sub = dict(points=s["points"][:400], cov=s["cov"][:400], accel_std=case["accel_std"], segment=None)
    so.check_linear("T5000_sub400", sub, run(sub))
    a, b = run(case), run(case, segment=2)
    assert a["info"]["segment"] == 16 and b["info"]["segment"] == 2 and a["info"]["levels"] < b["info"]["levels"]
    for k, (o, c) in enumerate(so.linear_reference("T5000_sub400", sub)):
        err, bar = so.linear_bar(a["points"][:, k], b["points"][:, k], c)
        print(f"track {k}: cond {c:.3g} default segment against segment 2: {err:.3g} (bar {bar:.3g})")
        assert a["status"][k] == 1 and b["status"][k] == 1 and err <= bar
    assert np.array_equal(a["n_usable"], np.isfinite(s["points"][:, :, 0]).sum(axis=0))


def test_chunks_over_tracks_return_the_same_bits(monkeypatch):
    case = ROBUST["soft_l1_36"]
    big = dict(case, points=np.concatenate([case["points"]] * 3, axis=1)[:, :5], cov=np.concatenate([case["cov"]] * 3, axis=1)[:, :5])
    big["points"][:, 3] = np.nan   # a track that is never launched, in the middle of a chunk
    whole = run(big)
    monkeypatch.setenv("MCBA_SMOOTH_BUDGET_MB", "0.2")
    parts = run(big)
    print(whole["info"], parts["info"])
    assert whole["info"]["chunks"] == 1 and parts["info"]["chunks"] >= 2 and parts["info"]["tracks_per_chunk"] < 5
    assert all(np.array_equal(whole[f], parts[f], equal_nan=True) for f in FIELDS)
    assert whole["status"][3] == -1 and np.array_equal(whole["points"][:, 0], whole["points"][:, 2]) and whole["n_iterations"][0] != whole["n_iterations"][1]


def test_a_chunk_in_which_no_track_is_launched(monkeypatch):
    """one track per chunk, the middle one without a usable frame: its chunk launches nothing, beside two chunks whose IRLS loops run"""
    s = so.scene(40, 3, seed=2)
    s["points"][:, 1] = np.nan
    case = dict(points=s["points"], cov=s["cov"], accel_std=0.1, loss="soft_l1", f_scale=3.0, segment=3)
    whole = run(case)
    monkeypatch.setenv("MCBA_SMOOTH_BUDGET_MB", "0.001")
    parts = run(case)
    print(whole["info"], parts["info"], parts["n_iterations"])
    assert whole["info"]["chunks"] == 1 and parts["info"]["chunks"] == 3 and parts["info"]["tracks_per_chunk"] == 1
    assert all(np.array_equal(whole[f], parts[f], equal_nan=True) for f in FIELDS)
    assert list(parts["status"]) == [1, -1, 1] and (parts["n_iterations"][[0, 2]] > 1).all() and parts["n_iterations"][1] == 0
    assert np.isnan(parts["points"][:, 1]).all() and np.isnan(parts["mahalanobis2"][:, 1]).all() and np.isnan(parts["cost"][1]) and (parts["weights"][:, 1] == 0).all()
    assert np.isfinite(parts["points"][:, [0, 2]]).all()


def test_refused_pivot_and_isotropic_forms():
    s = so.scene(40, 2, seed=2)
    from multicam_calibration_amd import smooth_trajectories

    r = smooth_trajectories(s["points"], s["cov"], accel_std=np.array([1e-154, 0.1]), segment=3)
    assert r.status[0] == -2 and np.isnan(r.points[:, 0]).all() and np.isnan(r.cost[0]) and r.status[1] == 1 and np.isfinite(r.points[:, 1]).all()
    iso = [smooth_trajectories(s["points"], c, accel_std=0.1).points for c in (0.05, np.full(2, 0.05), np.full((40, 2), 0.05), np.broadcast_to(np.eye(3) * (0.05 * 0.05), (40, 2, 3, 3)))]
    assert all(np.array_equal(iso[0], x) for x in iso[1:])
