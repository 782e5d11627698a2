"""refine_extrinsics on the GPU (csrc/mcba_kpba.hip through mcba_refine_extrinsics) against tests/golden/kpba.npz (scipy, tests/kpba_oracle.py), at the
smallest shapes at which the kernels can go wrong: reduced systems of 12 rows (under one 16-row tile), 18 (one tile and a part), 36, 72 and 144 (nine
full tiles: the pinned cases "c2", "three", "six", "twelve", "c24"); "six" cut to one point short of, at and one past a group of 64, 32 and 16 points;
the smaller groups forced.

The bars are the host tier's (kpba_oracle.check_result): at ftol = xtol = 1e-15, gtol = 1e-10 the cost is within golden (1 + 1e-10), the extrinsics
within 1e-6 relative after the closing step, the used points within max(1e-6 relative, 10 x the golden's own two-start spread).  Every case prints
its figures before it asserts."""
import numpy as np
import pytest

import keypoint_scenes as ks
import kpba_oracle as ko
import multicam_calibration_amd as m
from multicam_calibration_amd import refine_extrinsics

gpu = pytest.mark.gpu
TIGHT = dict(ftol=1e-15, xtol=1e-15, gtol=1e-10)
FULL = [n for n in ko.pinned_cases() if n not in ko.TRUNCATED]


def run(i, **over):
    kw = dict(points=i["pts0"], loss=i["loss"], **TIGHT)
    kw.update(over)
    return refine_extrinsics(i["uvs"], i["ext0"], i["intr"], **kw)


def check(name, i, o, r):
    print(f"{name}: status {r.status} nfev {r.nfev} njev {r.njev} optimality {r.optimality:.3g} scale {r.scale:.15g} group {r.info['group']} kernel_ms {r.info['kernel_ms']:.3f}")
    assert np.array_equal(r.held, o["held"]) and r.info["scale_camera"] == o["scale_camera"]
    ko.check_result(name, r.extrinsics, r.points, r.cost, o)
    assert r.cost <= r.cost0 and r.status in (1, 2, 3) and r.success and r.message == m.solver.TERMINATION_MESSAGES[r.status]
    assert np.array_equal(r.point_status == 1, np.isfinite(o["points"]).all(-1)) and set(np.unique(r.point_status)) <= set(m.geometry.REFINE_POINT_STATUS)
    base0 = ko.baseline_of(i["ext0"], 0, o["scale_camera"])
    base = ko.baseline_of(r.extrinsics, 0, o["scale_camera"])
    print(f"{name}: baseline {base0:.15g} -> {base:.15g}")
    assert abs(base / base0 - 1) <= 1e-12
    assert len(r.history) == r.nfev and r.history[0, 0] == r.cost0 and r.history[:, 2].sum() == r.njev
    # the cost at the start against the oracle's at the same values, within the bound of one evaluation (kpba_oracle's docstring)
    ref0, bound0 = ko.cost_with_bound(i["ext0"], i["pts0"], i["uvs"], i["intr"], i["loss"])
    print(f"{name}: cost0 {r.cost0:.15g} oracle {ref0:.15g} error / bound {abs(r.cost0 - ref0) / bound0:.3g}")
    assert abs(r.cost0 - ref0) <= bound0
    # the stated cost is the last accepted evaluation's, and the objective at the returned values (the rescale changes no projection)
    assert r.history[r.history[:, 2] == 1, 0].min() == r.cost and r.history[r.history[:, 2] == 1, 0][-1] == r.cost
    X = np.where(np.isnan(r.points), i["pts0"], r.points)
    assert abs(ko.cost_of(r.extrinsics, X, i["uvs"], i["intr"], i["loss"]) / r.cost - 1) <= 1e-10
    assert r.info["kernel_ms"] > 0 and r.info["n_step"] == r.nfev - 1


def same_bits(a, b):
    return (np.array_equal(a.extrinsics, b.extrinsics) and np.array_equal(a.points, b.points, equal_nan=True) and a.cost == b.cost and a.cost0 == b.cost0 and a.optimality == b.optimality
            and a.nfev == b.nfev and a.status == b.status and np.array_equal(a.history, b.history) and a.scale == b.scale)


@gpu
@pytest.mark.parametrize("name", FULL)
def test_pinned_cases_reach_the_golden_optimum(name):
    """6 C = 12, 18, 36, 72, 144; linear, soft_l1 and (where scipy's two starts agree) huber"""
    i, o = ko.case(name)
    check(name, i, o, run(i))


@gpu
@pytest.mark.parametrize("name", ["six_p63", "six_p64", "six_p65"])
def test_point_counts_around_a_group(name):
    i, o = ko.case(name)
    r = run(i)
    assert r.info["group"] == 64
    check(name, i, o, r)


@gpu
@pytest.mark.parametrize("group", [16, 32])
def test_forced_smaller_groups(monkeypatch, group):
    """MCBA_KPBA_G, read per call: G - 1, G, G + 1 points of "six", and the full cases of 18, 36 and 144 rows"""
    monkeypatch.setenv("MCBA_KPBA_G", str(group))
    for name in [f"six_p{group - 1}", f"six_p{group}", f"six_p{group + 1}", "three", "six", "c24"]:
        i, o = ko.case(name)
        r = run(i)
        assert r.info["group"] == group
        check(f"{name} (G = {group})", i, o, r)


@gpu
@pytest.mark.parametrize("loss", ["cauchy", "arctan"])
def test_unpinned_losses_terminate_and_never_rise(loss):
    i, o = ko.case("outlier")
    r = run(i, loss=loss, ftol=1e-8, xtol=1e-8, gtol=1e-8, max_nfev=60)
    print(f"{loss}: cost {r.cost0:.6g} -> {r.cost:.6g}, status {r.status}, nfev {r.nfev}")
    assert r.cost <= r.cost0 and r.status in (0, 1, 2, 3) and r.nfev <= 60


@gpu
def test_points_that_take_no_part():
    """a point unseen by every camera, one with a single view, one with a NaN start -- appended, so that the others keep their lanes: NaN rows,
    status -1, and the others' result bit for bit that of the run without them"""
    i, o = ko.case("three")
    base = run(i, max_nfev=8)
    C = len(i["uvs"])
    extra_uv = [np.full((3, 2), np.nan) for _ in range(C)]
    extra_uv[1][1] = i["uvs"][1][0]                    # one view
    for c in range(C):
        extra_uv[c][2] = i["uvs"][c][0] if not np.isnan(i["uvs"][c][0]).any() else i["uvs"][c][1]   # seen, but its start is NaN
    uvs = [np.concatenate([i["uvs"][c], extra_uv[c]]) for c in range(C)]
    pts = np.concatenate([i["pts0"], [i["pts0"][0], i["pts0"][0], [np.nan, 0.0, 0.0]]])
    r = refine_extrinsics(uvs, i["ext0"], i["intr"], points=pts, loss="linear", max_nfev=8, **TIGHT)
    n = len(i["pts0"])
    assert (r.point_status[n:] == -1).all() and np.isnan(r.points[n:]).all()
    assert np.array_equal(r.point_status[:n], base.point_status)
    assert np.array_equal(r.extrinsics, base.extrinsics) and np.array_equal(r.points[:n], base.points, equal_nan=True) and r.cost == base.cost and np.array_equal(r.history, base.history)


@gpu
def test_camera_without_detections_is_held_whole():
    i, o = ko.case("six")
    uvs = [u.copy() for u in i["uvs"]]
    blind = next(c for c in range(1, len(uvs)) if c != o["scale_camera"])
    uvs[blind][:] = np.nan
    r = refine_extrinsics(uvs, i["ext0"], i["intr"], points=i["pts0"], loss="linear", scale_camera=o["scale_camera"])
    assert r.held[blind].all() and r.held[0].all() and r.held.sum() == 13
    assert np.array_equal(r.extrinsics[blind], i["ext0"][blind]) and np.array_equal(r.extrinsics[0], i["ext0"][0])
    assert r.cost < r.cost0 and r.success


@gpu
def test_inliers_mask_is_nan_by_hand_and_calls_repeat():
    i, o = ko.case("outlier")
    rng = np.random.default_rng(4)
    mask = rng.uniform(size=(len(i["uvs"]), len(i["pts0"]))) > 0.1
    by_hand = [np.where(mask[c][:, None], i["uvs"][c], np.nan) for c in range(len(i["uvs"]))]
    a = refine_extrinsics(i["uvs"], i["ext0"], i["intr"], points=i["pts0"], inliers=mask, max_nfev=6)
    b = refine_extrinsics(by_hand, i["ext0"], i["intr"], points=i["pts0"], max_nfev=6)
    c = refine_extrinsics(by_hand, i["ext0"], i["intr"], points=i["pts0"], max_nfev=6)
    assert same_bits(a, b) and same_bits(b, c) and np.array_equal(a.point_status, b.point_status)


@gpu
def test_start_at_the_optimum():
    i, o = ko.case("six")
    X = np.where(np.isnan(o["points"]), i["pts0"], o["points"])
    r = refine_extrinsics(i["uvs"], o["extrinsics"], i["intr"], points=X, loss="linear", scale_camera=o["scale_camera"])
    print(f"nfev {r.nfev} status {r.status} cost {r.cost:.15g} golden {o['cost']:.15g}")
    assert r.nfev <= 2 and r.success and abs(r.cost / o["cost"] - 1) <= 1e-12


@gpu
def test_default_start_is_triangulate():
    i, o = ko.case("three")
    r = refine_extrinsics(i["uvs"], i["ext0"], i["intr"], loss="linear", **TIGHT)
    print(f"cost {r.cost:.15g} golden {o['cost']:.15g}")
    assert r.cost <= o["cost"] * (1 + 1e-10) and r.cost <= r.cost0


@gpu
def test_refusals_say_why():
    i, o = ko.case("c2")
    a = (i["uvs"], i["ext0"], i["intr"])
    with pytest.raises(ValueError, match="max_nfev"):
        refine_extrinsics(*a, points=i["pts0"], max_nfev=1)
    with pytest.raises(ValueError, match="loss"):
        refine_extrinsics(*a, points=i["pts0"], loss="l2")
    with pytest.raises(ValueError, match="f_scale"):
        refine_extrinsics(*a, points=i["pts0"], f_scale=0.0)
    with pytest.raises(ValueError, match="gauge_camera == scale_camera"):
        refine_extrinsics(*a, points=i["pts0"], gauge_camera=1, scale_camera=1)
    with pytest.raises(NotImplementedError, match="2 to 24 cameras"):
        refine_extrinsics([i["uvs"][0]] * 25, [i["ext0"][0]] * 25, [i["intr"][0]] * 25, points=i["pts0"])


@gpu
def test_drifted_cameras_come_back():
    """from a start 0.3 degrees and 2 mm off on "six": the per-camera median reprojection error of every perturbed camera falls"""
    uvs, ext, intr, X = ks.make("six")
    rng = np.random.default_rng(9)
    ext0 = np.array(ext)
    for c in range(1, len(ext0)):
        ext0[c, :3] += np.deg2rad(0.3) * (lambda v: v / np.linalg.norm(v))(rng.normal(size=3))
        ext0[c, 3:] += 2.0 * (lambda v: v / np.linalg.norm(v))(rng.normal(size=3))
    X0 = m.triangulate(uvs, ext0, intr)
    _, before = m.keypoint_reprojection_errors(X0, uvs, ext0, intr)
    r = refine_extrinsics(uvs, ext0, intr, points=X0, loss="soft_l1")
    _, after = m.keypoint_reprojection_errors(np.where(np.isnan(r.points), X0, r.points), uvs, r.extrinsics, intr)
    print("median error per camera before", before, "after", after, r.message)
    assert (after[1:] < before[1:]).all() and r.success
