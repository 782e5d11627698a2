"""tests/evidence_oracle.py on its own: its two routes to N(a) against each other, its search rule against scipy's
bounded minimiser, the estimate on data drawn from the model, pooling, and that the scenes of the estimator tests are decided by the oracle alone."""
import numpy as np
import pytest
import scipy.optimize

import evidence_oracle as eo

CASES = eo.cases()
MATCHED_SEED, MATCHED_A, MATCHED_RANGE = 0, 0.15, (0.01, 1.0)


@pytest.mark.parametrize("name", sorted(CASES))
def test_two_routes_agree_within_a_quarter_of_the_bar(name):
    case = CASES[name]
    worst = 0.0
    for k in range(case["points"].shape[1]):
        wk = None if case["weights"] is None else case["weights"][:, k]
        tr = eo.Track(case["points"][:, k], case["cov"][:, k], wk)
        if not tr.runs:
            continue
        for a in eo.EVAL_AT:
            r = eo.reference((name, k, float(a)), case["points"][:, k], case["cov"][:, k], a, wk)
            for f, bar in (("log_det", r["bars"]["log_det"]), ("data", r["bars"]["data"]), ("penalty", r["bars"]["penalty"]), ("N", r["bars"]["N"])):
                err = abs(r["dense"][f] - r[f])
                worst = max(worst, err / (bar / 4))
                assert err <= bar / 4, (name, k, a, f, err, bar)
            # the fast evaluation the search uses, against the same reference
            assert abs(tr.neg2(a) - r["N"]) <= r["bars"]["N"] / 4
    print(f"{name}: dense against long double, the largest fraction of a quarter bar {worst:.3g}")


@pytest.fixture(scope="module")
def matched():
    s = eo.matched_scene(300, 1, MATCHED_A, seed=MATCHED_SEED, gap=(100, 110))
    return s, eo.estimate(s["points"], s["cov"], MATCHED_RANGE)


def test_estimate_on_the_matched_model(matched):
    """T = 300, a = 0.15, anisotropic covariances, a 10-frame gap: the first seed (0 .. 9 tried in order) with |log(a_hat / a)| <= 3 log_std"""
    first = None
    for seed in range(10):
        s = eo.matched_scene(300, 1, MATCHED_A, seed=seed, gap=(100, 110))
        o = eo.estimate(s["points"], s["cov"], MATCHED_RANGE) if seed != MATCHED_SEED else matched[1]
        err, ls = abs(np.log(o["accel_std"][0] / MATCHED_A)), o["log_std"][0]
        print(f"seed {seed}: a_hat {o['accel_std'][0]:.6g}, |log(a_hat / a)| {err:.4g}, log_std {ls:.4g}, evaluations {o['n_evaluations']}")
        if err <= 3 * ls:
            first = seed
            break
    assert first == MATCHED_SEED
    o = matched[1]
    assert o["edge"][0] == 0 and o["status"][0] == 1 and o["n_evaluations"] == 17 + 16 + 2


def test_rule_against_scipy_bounded_minimiser(matched):
    o = matched[1]
    r = o["units"][0][1]
    tr = o["tracks"][0]
    ul, du = np.log(MATCHED_RANGE[0]), (np.log(MATCHED_RANGE[1]) - np.log(MATCHED_RANGE[0])) / 16
    m = scipy.optimize.minimize_scalar(lambda u: tr.neg2(np.exp(u)), bounds=(ul + (r["g_star"] - 1) * du, ul + (r["g_star"] + 1) * du), method="bounded", options=dict(xatol=1e-6))
    print(f"rule {r['u']:.6f}, scipy {m.x:.6f}")
    assert abs(m.x - r["u"]) <= 1e-3


def test_pooling_two_tracks_narrows_log_std():
    s = eo.matched_scene(120, 2, 0.05, seed=3)
    alone = eo.estimate(s["points"], s["cov"], (0.005, 0.5))
    pooled = eo.estimate(s["points"], s["cov"], (0.005, 0.5), pool="all")
    print(alone["accel_std"], alone["log_std"], pooled["accel_std"], pooled["log_std"])
    assert pooled["accel_std"][0] == pooled["accel_std"][1] and pooled["log_std"][0] < alone["log_std"].min()
    assert min(alone["accel_std"]) <= pooled["accel_std"][0] <= max(alone["accel_std"])


@pytest.mark.parametrize("name,pool", [("T71_K5", None), ("T257_seg3", None), ("T71_K5", "all"), ("T71_K5", np.array([4, 9, 4, 9, 9]))], ids=["T71_K5", "T257", "pool_all", "pool_labels"])
def test_estimator_scenes_are_decided(name, pool):
    """at most one unit in ten of the scenes the host-check and GPU tiers run may have a grid argmin within twice the bar of the runner-up"""
    case = CASES[name]
    o = eo.estimate(case["points"], case["cov"], eo.RANGE, 9, 1e-3, case["weights"], pool)
    und = [u for u, (mem, r) in o["units"].items() if not eo.decided(r, eo.unit_bar(name, case["points"], case["cov"], mem, r["a"], case["weights"]))]
    assert 10 * len(und) <= len(o["units"]) and all(r["edge"] == 0 for _, r in o["units"].values())


def test_lower_edge_scene():
    s = eo.linear_scene(40, seed=1)
    o = eo.estimate(s["points"], s["cov"], (0.01, 1.0), 9, 1e-3)
    (mem, r), = o["units"].values()
    assert r["edge"] == -1 and o["accel_std"][0] == 0.01 and np.isnan(o["log_std"][0]) and eo.decided(r, eo.unit_bar("linear40", s["points"], s["cov"], mem, 0.01))
