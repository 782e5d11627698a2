"""The trajectory kernels on the GPU where the second stage of their reductions makes a second trip and where a chunk is wider than two
wavefronts, against tests/trajectory_scale_oracle.py (banded and matrix-free references; held to the dense oracles by
tests/test_trajectory_scale_oracle_cpu.py).

L: 66001 frames x 2 tracks -- 258 evaluation workgroups per track, so k_smooth_final, k_evidence_final and k_traj_final take their loop
`b < nblk; b += 256` twice on two lanes; 2065 elimination lanes per track at the default segment (k_evidence_final's lane loop makes nine
trips); four levels at the default segment, ten at segment 2.  1301 frames at segment 2: 329 lanes, six levels.  The skeleton scene: 9601
frames x 8 keypoints, 301 workgroups, so k_skt_scalars and k_skt_trial_final make the second trip; the scalars show in no returned plane, so
cg_iterations is held to a band around the oracle's own conjugate gradients (trajectory_scale_oracle.count_band).  W: 41 frames x 131 tracks at segment 3, the
lane map gid % nact, gid / nact over more than two wavefronts of tracks, with a `list` that shrinks as the IRLS loops of the tracks end.
Every test prints the largest fraction of each bar and the kernel time."""
import time

import numpy as np
import pytest

import evidence_oracle as eo
import skeleton_trajectory_oracle as sto
import smoothing_oracle as so
import trajectory_refine_oracle as tro
import trajectory_scale_oracle as tso

pytestmark = pytest.mark.gpu

SMOOTH_FIELDS = ("points", "weights", "mahalanobis2", "status", "n_usable", "n_iterations", "history", "cost")
EVIDENCE_FIELDS = ("neg2_log_evidence", "data", "penalty", "log_det")
REFINE_SYSTEM_FIELDS = ("information", "gradient", "step", "data_cost", "penalty_cost", "trial_costs", "status", "n_usable", "n_single")
REFINE_LOOP_FIELDS = ("points", "information", "status", "n_usable", "n_single", "n_iterations", "cost", "history")
SKELETON_SYSTEM_FIELDS = ("information", "gradient", "step", "direction", "cg_iterations", "cg_residual", "data_cost", "penalty_cost", "bone_cost", "trial_costs", "status", "n_usable", "n_single")
SKELETON_LOOP_FIELDS = ("points", "information", "status", "n_usable", "n_single", "converged", "n_iterations", "cost", "cost_start", "history", "bone_residual", "direction")


def smooth(case, **kw):
    from multicam_calibration_amd import smooth_trajectories

    args = dict(accel_std=case["accel_std"], loss=case.get("loss", "linear"), f_scale=case.get("f_scale", 3.0), segment=case.get("segment"))
    args.update(kw)
    r = smooth_trajectories(case["points"], case["cov"], **args)
    return dict({f: getattr(r, f) for f in SMOOTH_FIELDS}, info=r.info)


def same_bits(a, b, fields):
    return all(np.array_equal(a[f], b[f], equal_nan=True) for f in fields)


def refine_args(case, **kw):
    a = dict(accel_std=case["accel_std"], pixel_std=case["pixel_std"], loss=case["loss"], f_scale=case["f_scale"], weights=case["weights"], segment=case["segment"])
    a.update(kw)
    return a


def skeleton_args(case, **kw):
    a = dict(refine_args(case), bones=case["bones"], bone_length=case["bone_length"], bone_std=case["bone_std"], cg_tol=sto.CG_TOL)
    a.update(kw)
    return a


def skeleton_fields(r, case, fields):
    got = {f: getattr(r, f) for f in fields}
    assert np.array_equal(r.parent, case["parent"])
    for f in ("direction", "bone_residual"):
        if f in got:
            got[f] = sto.by_child(got[f], case)
    return got


# ---------------------------------------------------------------- L: the smoother
def test_linear_solve_on_long_tracks_at_both_segments_and_identical_bits():
    L = tso.long_scene()
    t0 = time.time()
    refs = tso.long_smooth_reference(False)
    t_ref = time.time() - t0
    for segment, levels in ((None, 4), (2, 10)):
        got = smooth(L, segment=segment)
        worst = tso.check_smooth(f"L segment {segment}", refs, L["accel_std"], got)
        assert got["info"]["levels"] == levels == len(so.plan(tso.T_LONG, segment or so.SEGMENT_DEFAULT, 2)) and got["info"]["chunks"] == 1
        assert (got["weights"][np.isfinite(L["points"][:, :, 0])] == 1).all()
        print(f"L segment {segment}: levels {levels}, the largest fraction of each bar {worst}, kernels {got['info']['kernel_ms']:.3f} ms")
        if segment is None:
            assert same_bits(got, smooth(L), SMOOTH_FIELDS)   # the two-trip sums are still in a fixed order
    print(f"reference: {t_ref:.1f} s")


def test_one_weighted_evaluation_on_long_tracks():
    L, w = tso.long_scene(), tso.long_weights()
    t0 = time.time()
    refs = tso.long_smooth_reference(True)
    t_ref = time.time() - t0
    got = smooth(L, loss="soft_l1", weights_in=w, max_iterations=1)
    worst = tso.check_smooth("L weighted", refs, L["accel_std"], got, loss="soft_l1")
    print(f"L weighted: the largest fraction of each bar {worst}, kernels {got['info']['kernel_ms']:.3f} ms; reference: {t_ref:.1f} s")


# ---------------------------------------------------------------- L and T = 1301: the evidence
def test_evidence_on_long_tracks():
    from multicam_calibration_amd import trajectory_evidence

    L = tso.long_scene()
    for a in eo.EVAL_AT:
        t0 = time.time()
        refs = tso.long_evidence_reference(a)
        t_ref = time.time() - t0
        r = trajectory_evidence(L["points"], L["cov"], accel_std=a)
        got = dict({f: getattr(r, f) for f in EVIDENCE_FIELDS}, status=r.status, n_usable=r.n_usable)
        worst = tso.check_evidence(f"L a = {a}", refs, got)
        assert r.info["levels"] == 4 and np.array_equal(r.n_usable, [tso.T_LONG - 52] * 2)
        print(f"L evidence a = {a}: the largest fraction of a bar {worst:.3g} (window cond {max(x['cond'] for x in refs):.3g}), kernels {r.info['kernel_ms']:.3f} ms, of which log-determinant "
              f"{r.info['log_det_ms']:.3f}; reference: {t_ref:.1f} s")


def test_evidence_at_1301_frames_segment_two_against_the_longdouble_route():
    from multicam_calibration_amd import trajectory_evidence

    case, a = tso.evidence_case(), eo.A_TRUE
    r = trajectory_evidence(case["points"], case["cov"], accel_std=a, segment=2)
    t0 = time.time()
    worst = eo.check_evaluation("T1301_seg2", case, a, dict({f: getattr(r, f) for f in EVIDENCE_FIELDS}, status=r.status, n_usable=r.n_usable))
    assert r.info["levels"] == 6 and r.status.tolist() == [1, -1, 1]
    print(f"T1301_seg2: the largest fraction of a bar {worst:.3g}, kernels {r.info['kernel_ms']:.3f} ms; reference: {time.time() - t0:.1f} s")


# ---------------------------------------------------------------- long tracks: trajectory refinement
def test_trajectory_refinement_on_long_tracks():
    from multicam_calibration_amd import refine_trajectories, refine_trajectories_system

    case = tso.long_refine_case()
    r = refine_trajectories_system(case["start"], case["uvs"], case["ext"], case["intr"], **refine_args(case))
    t0 = time.time()
    worst = tso.check_refine_system("long", case, {f: getattr(r, f) for f in REFINE_SYSTEM_FIELDS})
    t_ref = time.time() - t0
    assert r.info["levels"] == 4 and r.info["chunks"] == 1
    print(f"long refinement, one evaluation: the largest fraction of each bar {worst}, kernels {r.info['kernel_ms']:.3f} ms; reference: {t_ref:.1f} s")
    lp = refine_trajectories(case["start"], case["uvs"], case["ext"], case["intr"], max_iterations=2, **refine_args(case))
    t0 = time.time()
    frac = tso.check_refine_loop("long", case, {f: getattr(lp, f) for f in REFINE_LOOP_FIELDS})
    assert (lp.n_iterations == 2).all()
    print(f"long refinement, two iterations: cost at the returned points {frac:.3g} of its bar, kernels {lp.info['kernel_ms']:.3f} ms; reference: {time.time() - t0:.1f} s")


# ---------------------------------------------------------------- 76808 lanes: skeleton trajectories
def test_skeleton_trajectories_on_301_workgroups():
    from multicam_calibration_amd import refine_skeleton_trajectories, refine_skeleton_trajectories_system

    case = tso.long_skeleton_case()
    r = refine_skeleton_trajectories_system(case["start"], case["uvs"], case["ext"], case["intr"], **skeleton_args(case))
    t0 = time.time()
    worst, own = tso.check_skeleton_system("skeleton", case, skeleton_fields(r, case, SKELETON_SYSTEM_FIELDS), sto.CG_TOL)
    t_ref = time.time() - t0
    assert r.info["running_tracks"] == tso.K_SK
    print(f"skeleton, one evaluation: the largest fraction of each bar {worst}, CG iterations {r.cg_iterations} (the oracle's {own}), kernels {r.info['kernel_ms']:.3f} ms; reference: {t_ref:.1f} s")
    lp = refine_skeleton_trajectories(case["start"], case["uvs"], case["ext"], case["intr"], max_iterations=2, **skeleton_args(case))
    t0 = time.time()
    frac = tso.check_skeleton_loop("skeleton", case, skeleton_fields(lp, case, SKELETON_LOOP_FIELDS), lp.info["cg_iterations_total"])
    assert lp.n_iterations == 2 and lp.history[0, 3] == r.cg_iterations   # (the loop's first solve is the system call's)
    print(f"skeleton, two iterations: cost at the returned points {frac:.3g} of its bar, kernels {lp.info['kernel_ms']:.3f} ms; reference: {time.time() - t0:.1f} s")


# ---------------------------------------------------------------- W: 131 tracks in a chunk
def test_robust_loop_on_a_wide_chunk_and_one_track_per_chunk(monkeypatch):
    case = tso.wide_smooth_case()
    got = smooth(case)
    t0 = time.time()
    left_out, ran = tso.check_wide_smooth(case, got)
    t_ref = time.time() - t0
    running = np.flatnonzero(got["status"] == 1)
    counts = sorted(set(got["n_iterations"][running].tolist()))
    print(f"W: {left_out} of {ran} tracks left out as undecided, iteration counts {counts}, kernels {got['info']['kernel_ms']:.3f} ms; reference: {t_ref:.1f} s")
    assert ran == 129 and 10 * left_out <= ran and len(counts) >= 3 and got["info"]["chunks"] == 1 and got["info"]["tracks_per_chunk"] == tso.K_W
    budget = 1.5 * so.chunk_doubles(tso.T_W, 1, 3, "smooth") * 8 / 1048576.0
    monkeypatch.setenv("MCBA_SMOOTH_BUDGET_MB", repr(budget))
    parts = smooth(case)
    assert (parts["info"]["tracks_per_chunk"], parts["info"]["chunks"]) == so.expected_chunks(tso.T_W, tso.K_W, 3, budget, "smooth")[:2] == (1, tso.K_W)
    assert same_bits(got, parts, SMOOTH_FIELDS)


def test_trajectory_refinement_on_a_wide_chunk_and_seven_tracks_per_chunk(monkeypatch):
    from multicam_calibration_amd import refine_trajectories, refine_trajectories_system

    case = tso.wide_refine_case()
    r = refine_trajectories_system(case["start"], case["uvs"], case["ext"], case["intr"], **refine_args(case))
    t0 = time.time()
    worst = tso.check_refine_system("W", case, {f: getattr(r, f) for f in REFINE_SYSTEM_FIELDS}, dense=True)
    t_ref = time.time() - t0
    assert r.info["chunks"] == 1 and r.info["tracks_per_chunk"] == tso.K_W and r.status[64:67].tolist() == [-1, -1, 1]
    print(f"W refinement, one evaluation: the largest fraction of each bar {worst}, kernels {r.info['kernel_ms']:.3f} ms; reference: {t_ref:.1f} s")
    whole = refine_trajectories(case["start"], case["uvs"], case["ext"], case["intr"], **refine_args(case))
    budget = 7.5 * tro.chunk_doubles(tso.T_W, 1, 3, 3) * 8 / 1048576.0
    monkeypatch.setenv("MCBA_SMOOTH_BUDGET_MB", repr(budget))
    parts = refine_trajectories(case["start"], case["uvs"], case["ext"], case["intr"], **refine_args(case))
    assert whole.info["chunks"] == 1 and (parts.info["tracks_per_chunk"], parts.info["chunks"]) == tro.expected_chunks(tso.T_W, tso.K_W, 3, 3, budget)[:2] == (7, 19)
    assert same_bits({f: getattr(whole, f) for f in REFINE_LOOP_FIELDS}, {f: getattr(parts, f) for f in REFINE_LOOP_FIELDS}, REFINE_LOOP_FIELDS)
    assert len(set(whole.n_iterations[whole.status == 1].tolist())) >= 2
