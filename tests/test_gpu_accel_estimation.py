"""trajectory_evidence and estimate_accel_std on the GPU against tests/evidence_oracle.py, on the shapes at which the
log-determinant kernel can go wrong (segment 2 unless said; blocks n = ceil(T / 2)): T = 3 one level and a phantom frame, 4 no phantom frame,
7 a second segment of one block, 11 and 12 an empty last segment, 13, 257 with segment 3 several levels, 71 x 5 with a track of one usable
frame, a gap and zeros in the weights, K = 67 across a wavefront with two tracks in the middle that do not run (no usable frame, one) beside
one with exactly two, K = 1.  The bars are the oracle's (its docstring derives them)."""
import numpy as np
import pytest

import evidence_oracle as eo

pytestmark = pytest.mark.gpu

CASES = eo.cases()
FIELDS = ("neg2_log_evidence", "data", "penalty", "log_det")
EST_FIELDS = ("accel_std", "log_std", "edge", "status", "n_usable", "grid", "neg2_log_evidence_grid", "neg2_log_evidence")


def evidence(case, a, **kw):
    from multicam_calibration_amd import trajectory_evidence

    r = trajectory_evidence(case["points"], case["cov"], accel_std=a, weights=case["weights"], segment=case["segment"], **kw)
    return dict({f: getattr(r, f) for f in FIELDS}, status=r.status, n_usable=r.n_usable, info=r.info)


def estimate(case, accel_range=eo.RANGE, n_grid=9, rtol=1e-3, pool=None):
    from multicam_calibration_amd import estimate_accel_std

    r = estimate_accel_std(case["points"], case["cov"], accel_range=accel_range, n_grid=n_grid, rtol=rtol, weights=case["weights"], pool=pool, segment=case["segment"])
    return dict({f: getattr(r, f) for f in EST_FIELDS}, n_evaluations=r.n_evaluations, info=r.info)


@pytest.mark.parametrize("name", sorted(CASES))
def test_one_evaluation_meets_the_bars(name):
    case = CASES[name]
    worst = 0.0
    for a in eo.EVAL_AT:
        worst = max(worst, eo.check_evaluation(name, case, a, evidence(case, a)))
    print(f"{name}: the largest fraction of a bar {worst:.3g}")


@pytest.mark.parametrize("name,pool", [("T71_K5", None), ("T257_seg3", None), ("T71_K5", "all"), ("T71_K5", np.array([4, 9, 4, 9, 9]))], ids=["T71_K5", "T257", "pool_all", "pool_labels"])
def test_estimator_against_the_oracle(name, pool):
    case = CASES[name]
    got = estimate(case, pool=pool)
    undecided, units, wa, ws = eo.check_estimate(name, case, got, eo.RANGE, 9, 1e-3, pool)
    print(f"{name}: {undecided} of {units} units undecided; the largest fraction of the bar of log a {wa:.3g}, of the log_std interval {ws:.3g}; kernel ms {got['info']['kernel_ms']:.3g}, of which "
          f"log-determinant {got['info']['log_det_ms']:.3g}")
    assert 10 * undecided <= units and got["info"]["evaluations"] == got["n_evaluations"]
    again = estimate(case, pool=pool)
    assert all(np.array_equal(got[f], again[f], equal_nan=True) for f in EST_FIELDS)
    if pool is not None:
        run = got["status"] == 1
        assert np.isnan(got["accel_std"][~run]).all() and np.isnan(got["neg2_log_evidence_grid"][:, ~run]).all()


def test_k1_and_two_calls_return_the_same_bits():
    case = CASES["K67"]
    a, b = evidence(case, 0.1), evidence(case, 0.1)
    assert all(np.array_equal(a[f], b[f], equal_nan=True) for f in FIELDS)
    one = dict(case, points=case["points"][:, 5:6], cov=case["cov"][:, 5:6])
    c = evidence(one, 0.1)   # K = 1: the same track alone
    assert all(c[f][0] == a[f][5] for f in FIELDS)


def test_chunks_return_the_same_bits_and_a_pooled_call_is_refused(monkeypatch):
    from multicam_calibration_amd import ops

    case = CASES["T71_K5"]
    whole_e, whole = evidence(case, 0.1), estimate(case)
    assert whole["info"]["chunks"] == 1
    per_track = whole["info"]["device_bytes"] / 5
    monkeypatch.setenv("MCBA_SMOOTH_BUDGET_MB", repr(1.5 * per_track / 1048576.0))   # one track per chunk
    parts_e, parts = evidence(case, 0.1), estimate(case)
    assert parts["info"]["chunks"] == 5 and parts_e["info"]["chunks"] == 5
    monkeypatch.setenv("MCBA_SMOOTH_BUDGET_MB", repr(2.5 * per_track / 1048576.0))   # two tracks per chunk: three chunks, the last narrower
    three = estimate(case)
    assert three["info"]["chunks"] == 3 and three["info"]["tracks_per_chunk"] == 2
    assert all(np.array_equal(whole_e[f], parts_e[f], equal_nan=True) for f in FIELDS)
    for other in (parts, three):
        assert all(np.array_equal(whole[f], other[f], equal_nan=True) for f in EST_FIELDS) and other["n_evaluations"] == whole["n_evaluations"]
    with pytest.raises(ops.McbaError, match="MCBA_SMOOTH_BUDGET_MB"):
        estimate(case, pool="all")


def test_weights_none_is_a_plane_of_ones():
    case = dict(CASES["T13"])
    a, ea = evidence(case, 0.1), estimate(case)
    case["weights"] = np.ones(case["points"].shape[:2])
    b, eb = evidence(case, 0.1), estimate(case)
    assert all(np.array_equal(a[f], b[f]) for f in FIELDS) and all(np.array_equal(ea[f], eb[f], equal_nan=True) for f in EST_FIELDS)


def test_lower_edge():
    s = eo.linear_scene(40, seed=1)
    case = dict(points=s["points"], cov=s["cov"], segment=2, weights=None)
    got = estimate(case, accel_range=(0.01, 1.0))
    undecided, units, _, _ = eo.check_estimate("linear40", case, got, (0.01, 1.0), 9, 1e-3)
    assert undecided == 0 and got["edge"][0] == -1 and got["accel_std"][0] == 0.01 and np.isnan(got["log_std"][0]) and got["status"][0] == 1
    assert got["neg2_log_evidence"][0] == got["neg2_log_evidence_grid"][0, 0]


def test_refused_pivot_at_every_candidate_is_status_minus_two():
    """a range whose inverse squares are finite while six times them is not: every candidate's diagonal is infinite and its pivot refused"""
    case = CASES["T7"]
    got = estimate(case, accel_range=(1e-154, 1.1e-154), n_grid=3)
    assert got["status"][0] == -2 and np.isnan(got["accel_std"][0]) and np.isnan(got["log_std"][0]) and np.isnan(got["neg2_log_evidence_grid"]).all() and got["edge"][0] == 0
    e = evidence(case, 1e-154)
    assert e["status"][0] == -2 and all(np.isnan(e[f][0]) for f in FIELDS)
