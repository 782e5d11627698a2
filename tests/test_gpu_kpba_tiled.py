"""The tiled Schur reduction of the extrinsics refinement (csrc/mcba_kpba_tiled.hip: k_kpba_factors, k_kpba_reduce_tiled, then k_kpba_finish; the
64-camera instantiations of k_kpba_status and k_kpba_step) through refine_extrinsics_system(reduction="tiled") and
refine_extrinsics(reduction="tiled"), 2 to 64 cameras.

One evaluation against kpba_oracle.block_system, piece by piece, within kpba_oracle's bounds (the ones tests/test_gpu_kpba_system.py holds the
resident reduction to; nothing here sets a tolerance) and its exact checks: statuses and the count, zero padding, zero rows and columns of held
scalars, tiles above the diagonal the transpose of their mirrors bit for bit, unused points untouched; two calls the same bits.  Inputs:
tests/kpba_wide.INPUTS, each run through the g++ build first by tests/test_hostcheck_kpba_wide.py.  With bands of B = 16 cameras and groups of
G = 16 points:
  cameras   2, 6, 15, 16 (one full band), 17 (a second band of one camera), 32 (two full bands), 33, 24, 25, 63, 64 (four bands, ten band pairs)
  points    15, 16, 17 at 25 cameras; 255, 256, 257 at 17; a chunk without a usable point; a chunk whose only usable point is its last;
            one chunk more than the cap of partial systems at 64 cameras (64 x 256 + 1 points) and at 3 (512 x 256 + 1): the grid stride
  losses    all five x f_scale 1, 3 x damping 0, 1e-4, 1 at 25 cameras with 15 % of the detections displaced
  held      33 cameras: the gauge camera at 63, one scale bit, 0b101010 in each of the three bands, a camera without detections in two bands
  weights   25 cameras, the levels 0, 1/4, 1, 4 and two values off them (0.37, 2.6), against weights_oracle's virtual rig with those six levels
Against the resident reduction on one input at 2, 6, 17 and 24 cameras: equal statuses, the cost within its bound, every entry of the two systems
within twice its bound (each is within one of the same reference; the sums differ in order).

The loop: every pinned case of tests/golden/kpba_wide.npz (25, 32, 32 with outliers and soft_l1, 64 cameras) and "six" and "outlier" of
tests/golden/kpba.npz meet kpba_oracle.check_result's bars at ftol = xtol = 1e-15, gtol = 1e-10 with reduction="tiled"; from the optimum of the
32-camera case the call ends within two evaluations; 25 cameras return a result where the default call refuses.
Every case prints each error as a fraction of its bound before it asserts."""
import numpy as np
import pytest

import kpba_oracle as ko
import kpba_wide as kw
import multicam_calibration_amd as m
import weights_oracle as wo
from multicam_calibration_amd import refine_extrinsics
from multicam_calibration_amd.geometry import refine_extrinsics_system

gpu = pytest.mark.gpu
TIGHT = dict(ftol=1e-15, xtol=1e-15, gtol=1e-10)
WORST = {}
FACTS = ("band", "band_pairs", "group", "workgroups", "NP")
WEIGHT_LEVELS = (0.0, 0.25, 1.0, 4.0, 0.37, 2.6)


def evaluate(i, **over):
    a = dict(points=i["pts0"], held=i["held"], lam=i["lam"], loss=i["loss"], f_scale=i["f_scale"], step=i["step"], reduction="tiled")
    a.update(over)
    return refine_extrinsics_system(i["uvs"], i["ext0"], i["intr"], **a)


def check_facts(name, i, got):
    C, P = len(i["ext0"]), len(i["pts0"])
    print(f"{name}: " + " ".join(f"{k} {got[k]}" for k in FACTS) + f" kernel_ms {got['kernel_ms']:.3f}")
    assert {k: got[k] for k in FACTS} == kw.launch_facts(C, P) and got["reduction"] == "tiled"


def check(name, i, o, got):
    check_facts(name, i, got)
    r = ko.check_block(name, got, o)
    r.update(ko.check_step(name, got["trial_points"], got["step4"], o, i["pts0"], i["uvs"], i["intr"], i["loss"], i["f_scale"]))
    ko.note_worst(WORST, r)
    print(ko.worst_line("tiled kernels so far", WORST))
    return r


def same_bits(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in ("point_status", "system", "trial_points", "step4")) and all(a[k] == b[k] for k in FACTS)


@gpu
@pytest.mark.parametrize("C", kw.CAMERA_COUNTS)
def test_camera_counts(C):
    i, o = kw.system_case(f"c{C}")
    got = evaluate(i)
    check(f"c{C}", i, o, got)
    assert same_bits(got, evaluate(i))


@gpu
@pytest.mark.parametrize("n", kw.GROUP_EDGES)
def test_points_around_a_group(n):
    i, o = kw.system_case(f"g25_p{n}")
    check(f"g25_p{n}", i, o, evaluate(i))


@gpu
@pytest.mark.parametrize("name", ["p255", "p256", "p257", "p600_gap", "p257_last"])
def test_point_counts_around_a_chunk(name):
    i, o = kw.system_case(name)
    check(name, i, o, evaluate(i))


@gpu
@pytest.mark.parametrize("name", kw.STRIDE)
def test_one_chunk_more_than_the_partial_cap(name):
    """the first shape at which a workgroup walks a second chunk, its tiles kept in registers across them; the one point of the last chunk is a
    used one (kpba_wide.system_case asserts it), or a pass that never reaches it would show nowhere"""
    i, o = kw.system_case(name)
    C, P = len(i["ext0"]), len(i["pts0"])
    assert (P + 255) // 256 == kw.partial_cap(C) + 1
    got = evaluate(i)
    check(name, i, o, got)
    if name == "stride64":
        assert same_bits(got, evaluate(i))


@gpu
@pytest.mark.parametrize("loss,f_scale,lam", kw.LOSS_GRID)
def test_losses_scales_and_dampings(loss, f_scale, lam):
    name = f"outlier_{loss}_{f_scale}_{lam}"
    i, o = kw.system_case(name)
    check(name, i, o, evaluate(i))


@gpu
def test_held_bits():
    i, o = kw.system_case("held")
    got = evaluate(i)
    check("held", i, o, got)
    bits = ko.held_bits(i["held"])
    assert bits[0] == 63 and bits[3] == 63 and bits[20] == 63 and bin(bits[1]).count("1") == 1 and (bits[[2, 17, 32]] == 0b101010).all()
    assert (got["acc"][[3, 20]] == 0.0).all() and (got["acc"][0, :27] != 0.0).all() and (got["acc"][0, 27:] == 0.0).all()
    assert same_bits(got, evaluate(i, held=bits))
    alone = evaluate(i, step=None)
    assert np.array_equal(alone["system"], got["system"]) and np.array_equal(alone["point_status"], got["point_status"]) and "trial_points" not in alone


@gpu
def test_weights_on_and_off_the_levels():
    """the weighted instantiations: weights drawn from 0, 1/4, 1, 4 and two values off those levels, against kpba_oracle.block_system of the virtual
    rig (one virtual camera per camera and positive value: tests/weights_oracle.py); all-ones weights are the unweighted call bit for bit"""
    C, P, seed = 25, 70, 610
    uvs, ext, intr, X = wo.scene(C=C, P=P, seed=seed, noise=0.3, p_unseen=0.3)
    uvs = [np.array(u) for u in uvs]
    w = wo.draw_levels(C, P, 9000 + seed, WEIGHT_LEVELS)
    assert wo.usable_fraction(uvs, w) >= 0.5 and all((w == l).any() for l in WEIGHT_LEVELS)
    ext0, pts0 = ko.perturbed_start(ext, X, 0, 5000 + seed)
    held, _ = ko.held_mask(ext0, wo.masked(uvs, w), pts0)
    rng = np.random.default_rng(7000 + seed)
    dtheta = np.concatenate([rng.normal(0, 1e-3, (C, 3)), rng.normal(0, 0.5, (C, 3))], axis=1) * ~held
    i = dict(uvs=uvs, weights=w, ext0=ext0, intr=intr, pts0=pts0, held=held, loss="linear", f_scale=1.0, lam=1e-4, step=(ext0 + dtheta, dtheta), levels=WEIGHT_LEVELS)
    o = wo.block_system_virtual(uvs, ext0, intr, pts0, held, w, loss="linear", f_scale=1.0, lam=1e-4, step=i["step"], levels=WEIGHT_LEVELS)
    assert o["used"].mean() >= 0.5
    got = evaluate(i, weights=w)
    check_facts("weights", i, got)
    r = wo.check_system("weights", i, o, got)
    ko.note_worst(WORST, r)
    assert same_bits(got, evaluate(i, weights=w))
    assert same_bits(evaluate(i, weights=np.ones_like(w)), evaluate(i))


@gpu
@pytest.mark.parametrize("C", kw.AGAINST_RESIDENT)
def test_against_the_resident_reduction(C):
    i, o = kw.system_case(f"c{C}")
    t, r = evaluate(i), evaluate(i, reduction="resident")
    assert r["reduction"] == "resident" and r["band"] == 0 and r["band_pairs"] == 0 and t["band"] == kw.BAND
    assert np.array_equal(t["point_status"], r["point_status"]) and t["count"] == r["count"]
    cond = float(o["cond"].max())
    Ud = np.sqrt(np.diagonal(o["U"]))
    bM = 2 * ko.BOUND_FACTOR * cond * ko.EPS * np.outer(Ud, Ud)
    bv = 2 * ko.BOUND_FACTOR * ko.EPS * Ud * (cond * o["fnorm"] + o["maxdet"] * np.sqrt(o["count"]))
    n6 = 6 * C
    (Ut, gt, zt), (Ur, gr, zr) = ko.unpack_acc(t["acc"]), ko.unpack_acc(r["acc"])
    ratios = dict(YY=ko._ratio(np.abs(t["YY"][:n6, :n6] - r["YY"][:n6, :n6]), bM), U=ko._ratio(np.abs(Ut - Ur), bM), gc=ko._ratio(np.abs(gt - gr), bv), Yz=ko._ratio(np.abs(zt - zr), bv),
                  cost=ko._ratio(abs(t["cost"] - r["cost"]), ko.cost_bound(o["cost"], o["fnorm"], o["maxdet"], o["count"])), gmax=ko._ratio(abs(t["gmax"] - r["gmax"]), 2 * o["gmax_bound"]))
    print(f"c{C}: tiled against resident: differences / twice the bound (cost: / the bound) " + " ".join(f"{k} {v:.3g}" for k, v in ratios.items()))
    assert max(ratios.values()) <= 1
    # the point steps do not depend on the reduction
    assert np.array_equal(t["trial_points"], r["trial_points"], equal_nan=True) and np.array_equal(t["step4"], r["step4"])


# ---------------------------------------------------------------- the loop
def run(i, **over):
    a = dict(points=i["pts0"], loss=i["loss"], reduction="tiled", **TIGHT)
    a.update(over)
    return refine_extrinsics(i["uvs"], i["ext0"], i["intr"], **a)


def check_loop(name, i, o, r):
    C = len(i["ext0"])
    print(f"{name}: status {r.status} nfev {r.nfev} njev {r.njev} optimality {r.optimality:.3g} scale {r.scale:.15g} group {r.info['group']} band pairs {r.info['band_pairs']} kernel_ms {r.info['kernel_ms']:.3f}")
    assert r.info["reduction"] == "tiled" and r.info["group"] == kw.GROUP and r.info["band"] == kw.BAND and r.info["band_pairs"] == kw.launch_facts(C, 1)["band_pairs"]
    assert np.array_equal(r.held, o["held"]) and r.info["scale_camera"] == o["scale_camera"]
    ko.check_result(name, r.extrinsics, r.points, r.cost, o)
    assert r.cost <= r.cost0 and r.status in (1, 2, 3) and r.success and r.message == m.solver.TERMINATION_MESSAGES[r.status]
    assert np.array_equal(r.point_status == 1, np.isfinite(o["points"]).all(-1))
    base0, base = ko.baseline_of(i["ext0"], 0, o["scale_camera"]), ko.baseline_of(r.extrinsics, 0, o["scale_camera"])
    assert abs(base / base0 - 1) <= 1e-12
    assert len(r.history) == r.nfev and r.history[0, 0] == r.cost0 and r.history[:, 2].sum() == r.njev
    ref0, bound0 = ko.cost_with_bound(i["ext0"], i["pts0"], i["uvs"], i["intr"], i["loss"])
    print(f"{name}: cost0 {r.cost0:.15g} oracle {ref0:.15g} error / bound {abs(r.cost0 - ref0) / bound0:.3g}")
    assert abs(r.cost0 - ref0) <= bound0
    X = np.where(np.isnan(r.points), i["pts0"], r.points)
    assert abs(ko.cost_of(r.extrinsics, X, i["uvs"], i["intr"], i["loss"]) / r.cost - 1) <= 1e-10


@gpu
@pytest.mark.parametrize("name", list(kw.CASES))
def test_wide_cases_reach_the_golden_optimum(name):
    assert name in kw.pinned_cases(), f"{name} is not pinned in tests/golden/kpba_wide.npz"
    i, o = kw.case(name)
    check_loop(name, i, o, run(i))


@gpu
@pytest.mark.parametrize("name", ["six", "outlier"])
def test_narrow_cases_reach_the_golden_optimum_through_the_tiled_reduction(name):
    i, o = ko.case(name)
    check_loop(name, i, o, run(i))


@gpu
def test_start_at_the_optimum_of_32_cameras():
    i, o = kw.case("w32")
    X = np.where(np.isnan(o["points"]), i["pts0"], o["points"])
    r = refine_extrinsics(i["uvs"], o["extrinsics"], i["intr"], points=X, loss="linear", scale_camera=o["scale_camera"], reduction="tiled")
    print(f"nfev {r.nfev} status {r.status} cost {r.cost:.15g} golden {o['cost']:.15g}")
    assert r.nfev <= 2 and r.success and abs(r.cost / o["cost"] - 1) <= 1e-12


@gpu
def test_25_cameras_where_the_default_refuses():
    i, o = kw.case("w25")
    with pytest.raises(NotImplementedError, match="2 to 24 cameras"):
        refine_extrinsics(i["uvs"], i["ext0"], i["intr"], points=i["pts0"], loss="linear")
    r = run(i, ftol=1e-8, xtol=1e-8, gtol=1e-8)
    assert r.success and r.cost < r.cost0 and r.extrinsics.shape == (25, 6) and np.isfinite(r.extrinsics).all() and r.info["band_pairs"] == 3
    again = run(i, ftol=1e-8, xtol=1e-8, gtol=1e-8)
    assert np.array_equal(again.extrinsics, r.extrinsics) and np.array_equal(again.points, r.points, equal_nan=True) and again.cost == r.cost and np.array_equal(again.history, r.history)
    auto = refine_extrinsics(i["uvs"], i["ext0"], i["intr"], loss="linear", reduction="tiled")   # points=None: triangulate takes 25 cameras
    assert auto.success and auto.cost < auto.cost0


@gpu
def test_refusals_say_why():
    i, o = kw.case("w25")
    wide = ([i["uvs"][0]] * 65, [i["ext0"][0]] * 65, [i["intr"][0]] * 65)
    with pytest.raises(NotImplementedError, match="2 to 64 cameras"):
        refine_extrinsics(*wide, points=i["pts0"], reduction="tiled")
    with pytest.raises(NotImplementedError, match="2 to 64 cameras"):
        refine_extrinsics_system(*wide, points=i["pts0"], held=np.zeros(65, np.int32), lam=0.0, reduction="tiled")
    for bad in ("banded", "", None, 1):
        with pytest.raises(ValueError, match="reduction"):
            refine_extrinsics(i["uvs"], i["ext0"], i["intr"], points=i["pts0"], reduction=bad)
        with pytest.raises(ValueError, match="reduction"):
            refine_extrinsics_system(i["uvs"], i["ext0"], i["intr"], points=i["pts0"], held=np.zeros(25, np.int32), lam=0.0, reduction=bad)
    with pytest.raises(NotImplementedError, match="2 to 24 cameras"):
        refine_extrinsics_system(i["uvs"], i["ext0"], i["intr"], points=i["pts0"], held=np.zeros(25, np.int32), lam=0.0)
