"""refine_trajectories on the GPU (csrc/mcba_traj_refine.hip and the right-hand-side mode of csrc/mcba_smooth.hip, through
mcba_refine_trajectories and mcba_refine_trajectories_system) against tests/trajectory_refine_oracle.py, on its cases: T = 2 (no penalty row),
T = 3, T = 257 (one frame past a 256-frame evaluation workgroup; a single-camera stretch, an unseen gap, unseen ends), T = 333 with segment 2
(five levels, the phantom frame; K = 5 with a track of status -1 and one of status -3), C = 2 and C = 64.

One evaluation (refine_trajectories_system): information within 1e-12 max|H| of the oracle, every entry of the gradient within 1e-12 of the sum of
the absolute values of its terms, the step within 4 eps cond max|d| of the dense solve of the system built from the returned information and
gradient, the costs within 1e-9 max(1, cost) + 100 eps cond cost.  The loop: the history never rises, one further oracle step moves less than
10 xtol max|x|, n_iterations is the oracle's where that is decided (trajectory_refine_oracle.decided), statuses and counts exact, the
covariance within the section 8f-20 bar of the inverse of the dense matrix built from the returned information.  Identical bits: two calls,
any chunking, weights=None against ones, a zero or NaN weight against a NaN detection."""
import numpy as np
import pytest

import trajectory_refine_oracle as tro

pytestmark = pytest.mark.gpu

CASES = tro.cases()
LOOP_FIELDS = ("points", "information", "status", "n_usable", "n_single", "n_iterations", "cost", "history", "covariance", "std", "lag_covariance")


def args(case, **kw):
    a = dict(accel_std=case["accel_std"], pixel_std=case["pixel_std"], loss=case["loss"], f_scale=case["f_scale"], weights=case["weights"], segment=case["segment"])
    a.update(kw)
    return a


def loop(case, uvs=None, **kw):
    from multicam_calibration_amd import refine_trajectories

    r = refine_trajectories(case["start"], case["uvs"] if uvs is None else uvs, case["ext"], case["intr"], **args(case, **kw))
    return r, {f: getattr(r, f) for f in LOOP_FIELDS}


def same_bits(a, b, fields=LOOP_FIELDS):
    return all(np.array_equal(a[f], b[f], equal_nan=True) if a[f] is not None else b[f] is None for f in fields)


@pytest.mark.parametrize("name", sorted(CASES))
def test_one_evaluation_against_the_oracle(name):
    from multicam_calibration_amd import refine_trajectories_system

    case = CASES[name]
    r = refine_trajectories_system(case["start"], case["uvs"], case["ext"], case["intr"], **args(case))
    tro.check_system(name, {f: getattr(r, f) for f in ("information", "gradient", "step", "data_cost", "penalty_cost", "trial_costs", "status", "n_usable", "n_single")})
    if name == "T333_seg2":
        assert r.info["levels"] == 5 and r.info["segment"] == 2


def test_loop_and_covariance_against_the_oracle_and_identical_bits():
    left_out = total = 0
    for name in sorted(CASES):
        r, got = loop(CASES[name], uncertainty="lag")
        lo, ran = tro.check_loop(name, got)
        tro.check_covariance(name, got)
        ok = got["status"] == 1
        assert np.allclose(r.std[:, ok] ** 2, r.covariance[:, ok][..., (0, 1, 2), (0, 1, 2)], rtol=1e-15, atol=0) and np.isnan(r.std[:, ~ok]).all()
        left_out, total = left_out + lo, total + ran
        assert same_bits(got, loop(CASES[name], uncertainty="lag")[1]), name
        plain = loop(CASES[name])[1]
        assert plain["covariance"] is None and plain["std"] is None and plain["lag_covariance"] is None
        assert same_bits(got, plain, LOOP_FIELDS[:8]), name   # (the covariance is made after the loop: it changes nothing before it)
    print(f"undecided tracks {left_out} of {total}")
    assert 10 * left_out <= total, (left_out, total)


def test_chunks_over_tracks_return_the_same_bits(monkeypatch):
    """K = 5 in chunks of two tracks, the last one narrower; a chunk holds the track of status -1, another the one of status -3"""
    case = CASES["T333_seg2"]
    C, T, K = case["weff"].shape
    r, whole = loop(case, uncertainty="lag")
    assert r.info["chunks"] == 1 and r.info["tracks_per_chunk"] == K
    budget = 2.5 * tro.chunk_doubles(T, 1, C, 2, True, True) * 8 / 1048576.0
    monkeypatch.setenv("MCBA_SMOOTH_BUDGET_MB", repr(budget))
    r2, parts = loop(case, uncertainty="lag")
    want = tro.expected_chunks(T, K, C, 2, budget, True, True)
    assert want[:2] == (2, 3) and (r2.info["tracks_per_chunk"], r2.info["chunks"], r2.info["device_bytes"], r2.info["levels"]) == want
    assert same_bits(whole, parts)
    from multicam_calibration_amd import refine_trajectories_system

    fields = ("information", "gradient", "step", "data_cost", "penalty_cost", "trial_costs", "status", "n_usable", "n_single")
    b = refine_trajectories_system(case["start"], case["uvs"], case["ext"], case["intr"], **args(case))
    monkeypatch.delenv("MCBA_SMOOTH_BUDGET_MB")
    a = refine_trajectories_system(case["start"], case["uvs"], case["ext"], case["intr"], **args(case))
    assert b.info["chunks"] > 1 and a.info["chunks"] == 1
    assert all(np.array_equal(getattr(a, f), getattr(b, f), equal_nan=True) for f in fields)


def test_unit_weights_are_no_weights_and_an_unseen_weight_is_a_nan_detection():
    case = CASES["T333_seg2"]
    plain, ones = loop(case, weights=None, uncertainty=True)[1], loop(case, weights=np.ones(case["uvs"].shape[:3]), uncertainty=True)[1]
    assert same_bits(plain, ones)
    rng = np.random.default_rng(5)
    hit = rng.uniform(size=case["uvs"].shape[:3]) < 0.1
    w = np.array(case["weights"])
    w[hit] = np.where(rng.uniform(size=int(hit.sum())) < 0.5, 0.0, np.nan)
    uv = np.array(case["uvs"])
    uv[hit] = np.nan
    assert same_bits(loop(case, weights=w, uncertainty=True)[1], loop(case, uvs=uv, uncertainty=True)[1])


def test_a_list_of_cameras_and_scalar_parameters():
    """all_uvs as a list of C arrays, accel_std and pixel_std as scalars: the same bits as the stacked and broadcast forms"""
    case = CASES["C2"]
    a = loop(case)[1]
    b = loop(case, uvs=[case["uvs"][0], case["uvs"][1]], accel_std=np.full(1, case["accel_std"]), pixel_std=np.full(2, case["pixel_std"]))[1]
    assert same_bits(a, b) and (a["status"] == 1).all()
