"""refine_skeleton_trajectories on the GPU (csrc/mcba_skeltraj.hip, k_smooth_resolve of csrc/mcba_smooth.hip, through
mcba_refine_skeleton_trajectories and mcba_refine_skeleton_trajectories_system) against tests/skeleton_trajectory_oracle.py, on its cases: T = 2 (no
penalty row), T = 3, K = 1 without a bone, T = 257 (a chain of three, segment 3: a one-camera stretch, an unseen gap, unseen ends), T = 71 with segment
2 (the phantom frame, several levels, a track of status -1 and one of status -3 whose bones drop, per-camera pixel_std, weights, huber), a star of 64
keypoints, C = 64 and C = 2.

One evaluation at cg_tol = 1e-10 (skeleton_trajectory_oracle.check_system): information within 1e-12 of the largest entry, the gradient within 1e-12
of the frame's largest sum of absolute terms, the step within (2 cg_tol sqrt(kappa) + 100 eps kappa_A) of the dense solve in the A norm, the costs
within section 8f-21's bar.  The loop (check_loop): the history never rises, one further dense step moves less than 10 xtol max|x|, n_iterations is
the oracle's on every case, statuses and counts exact.  K = 1 without a bone: the preconditioned recurrence must end after one iteration on
refine_trajectories_system's step.  The re-solve from the stored factors against a fresh elimination on the same right-hand side, within 4 eps cond
max|z| (T71_seg2, T257, T2, T3).  A bone of zero length at the start: status -3 on every running track.  Identical bits: two calls, weights=None against ones,
a zero or NaN weight against a NaN detection.  A budget too small: the error that names the knob."""
import numpy as np
import pytest

import skeleton_trajectory_oracle as sto
import smoothing_oracle as so
import trajectory_refine_oracle as tro

pytestmark = pytest.mark.gpu

CASES = sto.cases()
LOOP_FIELDS = ("points", "information", "status", "n_usable", "n_single", "converged", "n_iterations", "cost", "cost_start", "history", "bone_residual", "direction")
SYSTEM_FIELDS = ("information", "gradient", "step", "direction", "cg_iterations", "cg_residual", "data_cost", "penalty_cost", "bone_cost", "trial_costs", "status", "n_usable", "n_single")


def args(case, **kw):
    a = dict(accel_std=case["accel_std"], bones=case["bones"], bone_length=case["bone_length"], bone_std=case["bone_std"], pixel_std=case["pixel_std"], loss=case["loss"], f_scale=case["f_scale"],
             weights=case["weights"], segment=case["segment"], cg_tol=sto.CG_TOL)
    a.update(kw)
    return a


def by_child(r, case, fields):
    got = {f: getattr(r, f) for f in fields}
    assert np.array_equal(r.parent, case["parent"])
    for f in ("direction", "bone_residual"):
        if f in got:
            got[f] = sto.by_child(got[f], case)
    return got


def loop(case, uvs=None, **kw):
    from multicam_calibration_amd import refine_skeleton_trajectories

    r = refine_skeleton_trajectories(case["start"], case["uvs"] if uvs is None else uvs, case["ext"], case["intr"], **args(case, **kw))
    return r, by_child(r, case, LOOP_FIELDS)


def system(case, **kw):
    from multicam_calibration_amd import refine_skeleton_trajectories_system

    r = refine_skeleton_trajectories_system(case["start"], case["uvs"], case["ext"], case["intr"], **args(case, **kw))
    return r, by_child(r, case, SYSTEM_FIELDS)


def same_bits(a, b):
    return all(np.array_equal(a[f], b[f], equal_nan=True) for f in a)


@pytest.mark.parametrize("name", sorted(CASES))
def test_one_evaluation_against_the_oracle(name):
    r, got = system(CASES[name])
    sto.check_system(name, got)
    if name == "T71_seg2":
        assert r.info["levels"] == len(so.plan(71, 2, 5)) and r.info["segment"] == 2 and r.info["running_tracks"] == 3


@pytest.mark.parametrize("name", sorted(CASES))
def test_loop_against_the_oracle_and_two_calls_return_the_same_bits(name):
    r, got = loop(CASES[name])
    sto.check_loop(name, got)
    assert r.info["cg_iterations_total"] == int(r.history[:, 3].sum())
    assert same_bits(got, loop(CASES[name])[1]), name


def test_one_track_without_a_bone_is_one_iteration_on_the_trajectory_step():
    """K = 1, E = 0: A = M, so the recurrence ends after one iteration, and its step -- the elimination's solve scaled by alpha = r^T z / p^T A p,
    the re-solve entering the stopping test alone -- is refine_trajectories_system's to that call's own bar, 4 eps cond max|d|"""
    from multicam_calibration_amd import refine_trajectories_system

    case = CASES["K1"]
    r, got = system(case)
    t = refine_trajectories_system(case["start"], case["uvs"], case["ext"], case["intr"], accel_std=case["accel_std"], pixel_std=case["pixel_std"], loss=case["loss"], f_scale=case["f_scale"],
                                   weights=case["weights"], segment=case["segment"])
    assert r.cg_iterations == 1 and r.direction.shape == (40, 0, 3)
    assert np.array_equal(r.information, t.information) and np.array_equal(r.gradient, t.gradient)
    cnd = so.cond(dict(A=tro.dense_matrix(t.information[:, 0], case["accel_std"])))
    err, bar = np.abs(r.step - t.step).max(), so.BAR_K * sto.EPS * cnd * np.abs(t.step).max()
    print(f"K1: step against refine_trajectories_system {err:.3g} (bar {bar:.3g}, cond {cnd:.3g}), residual after the re-solve {r.cg_residual:.3g}")
    assert err <= bar and r.cg_residual <= so.BAR_K * sto.EPS * cnd
    sto.check_one_track(got)


@pytest.mark.parametrize("name", sto.RESOLVE_CASES)
def test_the_resolve_agrees_with_a_fresh_elimination(name):
    """k_smooth_resolve and the back-substitution against k_smooth_reduce (level 0 in its right-hand-side mode) and the back-substitution on the same
    right-hand side, the right-hand-side halves of every stored record overwritten with NaN in between: within 4 eps cond max|z| per track"""
    r, got = system(CASES[name], resolve_check=True)
    sto.check_resolve(name, dict(got, resolve=r.resolve_check))
    assert np.isnan(r.resolve_check[:, :, r.status != 1]).all()
    plain = system(CASES[name])[1]
    assert same_bits({f: got[f] for f in ("information", "gradient", "direction", "status")}, {f: plain[f] for f in ("information", "gradient", "direction", "status")})


def test_a_bone_of_zero_length_at_the_start_is_status_minus_three():
    case = sto.coincident_case()
    sto.check_coincident(loop(case)[1], system(case)[1])


def test_unit_weights_are_no_weights_and_an_unseen_weight_is_a_nan_detection():
    case = CASES["T71_seg2"]
    assert same_bits(loop(case, weights=None)[1], loop(case, weights=np.ones(case["uvs"].shape[:3]))[1])
    rng = np.random.default_rng(5)
    hit = rng.uniform(size=case["uvs"].shape[:3]) < 0.1
    w = np.array(case["weights"])
    w[hit] = np.where(rng.uniform(size=int(hit.sum())) < 0.5, 0.0, np.nan)
    uv = np.array(case["uvs"])
    uv[hit] = np.nan
    assert same_bits(loop(case, weights=w)[1], loop(case, uvs=uv)[1])


def test_a_call_over_the_budget_is_refused(monkeypatch):
    from multicam_calibration_amd import ops

    case = CASES["T257"]
    C, T, K = case["weff"].shape
    need = sto.chunk_doubles(T, K, C, case["segment"]) * 8 / 1048576.0
    monkeypatch.setenv("MCBA_SMOOTH_BUDGET_MB", repr(need * 0.999))
    with pytest.raises(ops.McbaError, match="MCBA_SMOOTH_BUDGET_MB"):
        loop(case)
    monkeypatch.setenv("MCBA_SMOOTH_BUDGET_MB", repr(need * 1.001))
    r, _ = loop(case, max_iterations=1)
    assert r.info["device_bytes"] == sto.chunk_doubles(T, K, C, case["segment"]) * 8 and r.n_iterations == 1
