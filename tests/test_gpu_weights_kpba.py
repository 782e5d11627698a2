"""refine_extrinsics(weights=) and refine_extrinsics_system(weights=) on the GPU -- the weighted instantiations of k_kpba_status, k_kpba_reduce and
k_kpba_step through mcba_refine_extrinsics_weighted / _system_weighted -- against tests/weights_oracle.py.

One evaluation (kpba_oracle.check_block, check_step against block_system of the virtual rig, its blocks summed over the virtual cameras of each
physical camera): 2, 3, 11 (the group falls to 32) and 24 cameras (72 virtual ones); 70 and 257 points; 63, 64, 65 points at 6 cameras under each
forced MCBA_KPBA_G; dampings 0, 1e-4, 1 with soft_l1 and cauchy on the "outlier" scene; held bits as in the unweighted "held" case, the blind
camera blind by its weights; the same bits on a second call.
End to end (the three bars of kpba_oracle.check_result against tests/golden/kpba_weighted.npz: scipy on the virtual rig, the virtual cameras of a
physical camera tied): "six" (linear) and "outlier" (soft_l1) with the levels 0, 1/4, 1, 4 -- whichever of them the golden's two starts pin."""
import numpy as np
import pytest

import kpba_oracle as ko
import multicam_calibration_amd as m
import weights_oracle as wo
from multicam_calibration_amd import refine_extrinsics
from multicam_calibration_amd.geometry import refine_extrinsics_system

gpu = pytest.mark.gpu
# max_nfev: "outlier" (soft_l1, a quarter of the weights zero) takes 109 evaluations of the host build to these tolerances; the default 100 ends at
# status 0, 6e-10 above the optimum
TIGHT = dict(ftol=1e-15, xtol=1e-15, gtol=1e-10, max_nfev=200)
KEYS = ("point_status", "system", "trial_points", "step4")


def evaluate(i, **over):
    kw = dict(points=i["pts0"], held=i["held"], lam=i["lam"], loss=i["loss"], f_scale=i["f_scale"], step=i["step"], weights=i["weights"])
    kw.update(over)
    return refine_extrinsics_system(i["uvs"], i["ext0"], i["intr"], **kw)


def same_bits(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in KEYS) and (a["group"], a["workgroups"], a["NP"]) == (b["group"], b["workgroups"], b["NP"])


@gpu
@pytest.mark.parametrize("name", ["c2_p70", "c3_p257", "c11_p70", "c24_p70"])
def test_camera_counts(name):
    i, o = wo.system_case(name)
    assert o["used"].mean() >= 0.5
    got = evaluate(i)
    print(f"{name}: group {got['group']} workgroups {got['workgroups']} NP {got['NP']} kernel_ms {got['kernel_ms']:.3f}")
    assert name != "c11_p70" or got["group"] == 32
    wo.check_system(name, i, o, got)
    assert same_bits(got, evaluate(i))


@gpu
@pytest.mark.parametrize("n", [63, 64, 65])
def test_group_edges_at_every_group_size(monkeypatch, n):
    i, o = wo.system_case(f"g6_p{n}")
    got = {}
    for G in (16, 32, 64):
        monkeypatch.setenv("MCBA_KPBA_G", str(G))
        got[G] = evaluate(i)
        assert got[G]["group"] == G
        wo.check_system(f"g6_p{n} (G = {G})", i, o, got[G])
    for G in (16, 32):   # the point steps do not depend on the group size
        assert np.array_equal(got[G]["trial_points"], got[64]["trial_points"], equal_nan=True) and np.array_equal(got[G]["step4"], got[64]["step4"])


@gpu
@pytest.mark.parametrize("loss", ["soft_l1", "cauchy"])
@pytest.mark.parametrize("lam", [0.0, 1e-4, 1.0])
def test_losses_and_dampings_on_the_outlier_scene(loss, lam):
    name = f"outlier_{loss}_{lam}"
    i, o = wo.system_case(name)
    wo.check_system(name, i, o, evaluate(i))


@gpu
def test_held_bits():
    i, o = wo.system_case("held")
    got = evaluate(i)
    wo.check_system("held", i, o, got)
    bits = ko.held_bits(i["held"])
    assert bits[0] == 63 and bits[2] == 0b101010 and bits[3] == 63 and bin(bits[1]).count("1") == 1
    assert (got["acc"][3] == 0.0).all() and (got["acc"][0, :27] != 0.0).all() and (got["acc"][0, 27:] == 0.0).all()
    assert same_bits(got, evaluate(i, held=bits))
    alone = evaluate(i, step=None)
    assert np.array_equal(alone["system"], got["system"]) and "trial_points" not in alone


@gpu
def test_identities_of_one_evaluation():
    """all-ones weights are the unweighted call and a 0/1 plane the same mask written as NaN, bit for bit (a multiplication by 1.0 is exact); a
    constant plane 4 under the linear loss is held to the oracle's system for it, which is 4 times the unit one with the point steps unchanged"""
    i, o = wo.system_case("c3_p257")
    assert same_bits(evaluate(i, weights=np.ones_like(i["weights"])), evaluate(i, weights=None))
    mask = i["weights"] > 0
    a = evaluate(i, weights=mask.astype(np.float64))
    b = refine_extrinsics_system(wo.masked(i["uvs"], mask), i["ext0"], i["intr"], points=i["pts0"], held=i["held"], lam=i["lam"], loss=i["loss"], f_scale=i["f_scale"], step=i["step"])
    assert same_bits(a, b)
    # a constant plane under the linear loss: the oracle's system for it (U, Y Y^T, g_c, Y z and the costs times 4, the point steps unchanged)
    w4 = 4.0 * mask
    o4 = wo.block_system_virtual(i["uvs"], i["ext0"], i["intr"], i["pts0"], i["held"], w4, loss=i["loss"], f_scale=i["f_scale"], lam=i["lam"], step=i["step"])
    c = evaluate(i, weights=w4)
    wo.check_system("c3_p257, weights 4", dict(i, weights=w4), o4, c)
    o1 = wo.block_system_virtual(i["uvs"], i["ext0"], i["intr"], i["pts0"], i["held"], 1.0 * mask, loss=i["loss"], f_scale=i["f_scale"], lam=i["lam"], step=i["step"])
    assert abs(o4["cost"] / (4 * o1["cost"]) - 1) <= 1e-14 and np.abs(o4["trial"] - o1["trial"])[o1["used"]].max() <= 1e-12


def run(i, **over):
    kw = dict(points=i["pts0"], loss=i["loss"], weights=i["weights"], **TIGHT)
    kw.update(over)
    return refine_extrinsics(i["uvs"], i["ext0"], i["intr"], **kw)


@gpu
@pytest.mark.parametrize("name", list(wo.GOLDEN_CASES))
def test_pinned_cases_reach_the_weighted_golden_optimum(name):
    assert name in wo.pinned_cases(), f"{name} is not pinned in tests/golden/kpba_weighted.npz"
    i, o = wo.golden_case(name)
    r = run(i)
    print(f"{name}: status {r.status} nfev {r.nfev} njev {r.njev} optimality {r.optimality:.3g} scale {r.scale:.15g} group {r.info['group']} kernel_ms {r.info['kernel_ms']:.3f}")
    assert np.array_equal(r.held, o["held"]) and r.info["scale_camera"] == o["scale_camera"]
    ko.check_result(name, r.extrinsics, r.points, r.cost, o)
    assert r.cost <= r.cost0 and r.status in (1, 2, 3) and r.success
    assert np.array_equal(r.point_status == 1, np.isfinite(o["points"]).all(-1))
    assert (r.point_status == 1).mean() >= 0.5
    ref0, bound0 = wo.cost_virtual(i["ext0"], i["pts0"], i["uvs"], i["intr"], i["weights"], i["loss"])
    print(f"{name}: cost0 {r.cost0:.15g} oracle {ref0:.15g} error / bound {abs(r.cost0 - ref0) / bound0:.3g}")
    assert abs(r.cost0 - ref0) <= bound0
    X = np.where(np.isnan(r.points), i["pts0"], r.points)
    assert abs(wo.cost_virtual(r.extrinsics, X, i["uvs"], i["intr"], i["weights"], i["loss"])[0] / r.cost - 1) <= 1e-10
    again = run(i)
    assert np.array_equal(again.extrinsics, r.extrinsics) and np.array_equal(again.points, r.points, equal_nan=True) and again.cost == r.cost and np.array_equal(again.history, r.history)


@gpu
def test_identities_end_to_end():
    """inliers= composes with weights= (the product plane); points=None triangulates without the detections of weight 0; a constant plane under the
    linear loss returns the same extrinsics and points with the cost times w0; a 0/1 plane is the same mask written as NaN, bit for bit"""
    i, o = wo.golden_case("six") if "six" in wo.pinned_cases() else (None, None)
    assert i is not None
    loose = dict(ftol=1e-8, xtol=1e-8, gtol=1e-8, max_nfev=100)
    mask = np.random.default_rng(4).uniform(size=i["weights"].shape) > 0.1
    a, b = run(i, inliers=mask, **loose), run(i, weights=i["weights"] * mask, **loose)
    assert np.array_equal(a.extrinsics, b.extrinsics) and a.cost == b.cost and np.array_equal(a.point_status, b.point_status)
    auto = run(i, points=None, **loose)
    start = m.triangulate(wo.masked(i["uvs"], i["weights"]), i["ext0"], i["intr"])
    by_hand = run(i, points=start, **loose)
    assert np.array_equal(auto.extrinsics, by_hand.extrinsics) and auto.cost == by_hand.cost
    # a constant plane under the linear loss: the same extrinsics and points, the cost times w0, to the bars of kpba_oracle.check_result
    seen = (i["weights"] > 0).astype(np.float64)
    one, four = run(i, weights=seen), run(i, weights=4 * seen)
    ko.check_result("six, weights 4 against weights 1", four.extrinsics, four.points, four.cost / 4, dict(extrinsics=one.extrinsics, points=one.points, cost=one.cost, spread_pts=o["spread_pts"]))
    assert abs(four.cost / (4 * one.cost) - 1) <= 1e-10
    plain = refine_extrinsics(wo.masked(i["uvs"], i["weights"]), i["ext0"], i["intr"], points=i["pts0"], loss=i["loss"], **TIGHT)
    assert np.array_equal(one.extrinsics, plain.extrinsics) and one.cost == plain.cost and np.array_equal(one.points, plain.points, equal_nan=True)


@gpu
def test_a_camera_blind_by_its_weights_is_held_and_a_blind_scale_camera_refused():
    i, o = wo.golden_case("six") if "six" in wo.pinned_cases() else (None, None)
    assert i is not None
    w = i["weights"].copy()
    blind = next(c for c in range(1, 6) if c != o["scale_camera"])
    w[blind] = 0.0
    r = run(i, weights=w, scale_camera=o["scale_camera"], ftol=1e-8, xtol=1e-8, gtol=1e-8, max_nfev=100)
    assert r.held[blind].all() and np.array_equal(r.extrinsics[blind], i["ext0"][blind])
    w = i["weights"].copy()
    w[o["scale_camera"]] = np.nan
    with pytest.raises(m.ops.McbaError, match="scale_camera"):
        run(i, weights=w, scale_camera=o["scale_camera"])
