"""tests/fivepoint_oracle.py held to its own rules on the cases the other tiers use (no GPU): how many candidates the comparability rule leaves
out, the two routes to the candidates (the K5 its docstring quotes), exact recovery without noise, the winner on the thin scenes -- and, pinned
as a fact about the 8-point oracle, the failure the five-point generator is there for.  Also the host-side pieces of the feature that need no
device: draw_samples(size=5) and the ValueErrors of solver=."""
import numpy as np
import pytest

import fivepoint_oracle as fo
import keypoint_scenes as ks
import thin_scenes as ts
import twoview_oracle as tvo
from test_triangulate_cpu import scene

CASES = [("thin3", 0, 1), ("thin3", 1, 2), ("thin6", 0, 1), ("thin6", 1, 2), ("three", 0, 1)]
LEFT_OUT_CAP = 0.05
DE_MAX = 0.06    # the winners' worst on the six pairs below is 0.0512 ("thin3" (1, 2)); the next are 0.0297 and 0.0242: 0.06 is the issue's bar, met with 15 % to spare


@pytest.mark.parametrize("H", [64, 512])
@pytest.mark.parametrize("name,a,b", CASES)
def test_case_rules(name, a, b, H):
    ua, ub, ia, ib, _, _ = fo.pair_of(name, a, b)
    prep = tvo.prepare(ua, ub, ia, ib)
    smp = fo.draw_samples(len(ua), H, 0)
    per = fo.hypotheses(prep, smp)["per_sample"]
    n_real = sum(len(c["E"]) for c in per)
    n_out = sum(len(c["E"]) if c["undecided"] else int((~c["comparable"]).sum()) for c in per)
    live = np.array([len(c["E"]) for c in per])
    mult, n_cmp, _ = fo.route_multiple(prep, smp)
    print(f"{name} ({a}, {b}) H {H}: {n_real} real candidates ({live.mean():.2f} per sample, at most {live.max()}), {n_out} left out ({n_out / n_real:.4f}), "
          f"{sum(c['undecided'] for c in per)} undecided samples, {sum(c['void'] for c in per)} void; smallest sigma_5 / sigma_1 {min(c['sigma_ratio'] for c in per):.3g}, "
          f"smallest pivot ratio {min(c['pivot'] for c in per):.3g}; route multiple {mult:.4g} over {n_cmp} candidates")
    assert n_out <= LEFT_OUT_CAP * n_real
    assert not any(c["void"] for c in per) and live.max() <= fo.SLOTS
    assert 8 * mult <= fo.K5 and mult <= fo.K5_MEASURED * 1.001
    assert min(c["sigma_ratio"] for c in per) > 100 * fo.RANK_MIN and min(c["pivot"] for c in per) > 100 * fo.PIVOT_MIN


def test_noise_free_samples_hold_the_true_essential_matrix():
    uvs, ext, intr, X = scene(C=2, P=120, seed=5, noise=0.0)
    sc = (uvs, ext, intr, X)
    Et = fo.true_essential(sc, 0, 1)
    prep = tvo.prepare(uvs[0], uvs[1], intr[0], intr[1], iterations=25)
    worst = 0.0
    for route in ("action", "poly"):
        for s in fo.draw_samples(120, 32, 1):
            c = fo.candidates(prep["na"][s], prep["nb"][s], route)
            assert not c["void"] and len(c["E"]) >= 1
            worst = max(worst, min(fo.dE(e, Et) for e in c["E"]))
    print(f"noise-free: the true E is within {worst:.3g} of a candidate of every sample")
    assert worst < 1e-6


def test_compaction_is_the_index_order_of_the_live_slots():
    st = -np.ones((3, fo.SLOTS), np.int32)
    st[0, :4], st[2, :2] = 1, 1
    assert np.array_equal(fo.compaction(st), [0, 1, 2, 3, 20, 21])


@pytest.mark.parametrize("name,pairs", [("thin3", [(0, 1), (0, 2), (1, 2)]), ("thin6", [(0, 1), (0, 2), (1, 2)])])
def test_winner_on_the_thin_scenes(name, pairs):
    for a, b in pairs:
        ua, ub, ia, ib, _, sc = fo.pair_of(name, a, b)
        o = fo.two_view5(ua, ub, ia, ib, fo.draw_samples(len(ua), 64, 0), tvo.THRESHOLD)
        d = fo.dE(o["hyp"]["E"][o["winner"]], fo.true_essential(sc, a, b))
        second = np.sort(o["score"]["cost"])[1] / o["cost"]
        print(f"{name} ({a}, {b}): winner sample {o['sample']} slot {o['slot']}: {o['n_inliers']} of {len(ua)} inliers, dE {d:.4f}, second-best cost {second:.3f} x")
        assert o["n_inliers"] == len(ua) and d <= DE_MAX and o["comparable"]


def test_the_eight_point_oracle_fails_on_the_slab():
    """the failure being fixed, as a fact about tests/twoview_oracle.py: 512 8-point hypotheses on "thin3" (1, 2) keep a third of the points,
    report status 1 and an essential matrix far from the true one"""
    ua, ub, ia, ib, _, sc = fo.pair_of("thin3", 1, 2)
    o = tvo.two_view(ua, ub, ia, ib, tvo.draw_samples(len(ua), 512, 0), tvo.THRESHOLD)
    d = fo.dE(o["hyp"]["E"][o["winner"]], fo.true_essential(sc, 1, 2))
    print(f"8-point on thin3 (1, 2): {o['n_inliers']} of {len(ua)} inliers, dE {d:.3f}")
    assert d > 0.3 and tvo.min_inliers(len(ua)) <= o["n_inliers"] < len(ua) // 2


# ---------------------------------------------------------------- host-side pieces of the product
def test_draw_samples_of_five():
    from multicam_calibration_amd import geometry

    np.random.seed(123)
    before = np.random.get_state()[1].copy()
    a, b = geometry.draw_samples(111, 70, [0, 2, 1], size=5), geometry.draw_samples(111, 70, [0, 2, 1], size=5)
    assert np.array_equal(np.random.get_state()[1], before)
    assert a.dtype == np.int32 and a.shape == (70, 5) and np.array_equal(a, b) and np.array_equal(a, fo.draw_samples(111, 70, [0, 2, 1]))
    assert a.min() >= 0 and a.max() < 111 and all(len(set(r)) == 5 for r in a.tolist())
    assert np.array_equal(geometry.draw_samples(111, 70, [0, 2, 1], size=8), tvo.draw_samples(111, 70, [0, 2, 1]))
    assert np.array_equal(geometry.draw_samples(111, 70, [0, 2, 1]), tvo.draw_samples(111, 70, [0, 2, 1]))
    for bad in (dict(size=6), dict(size=7)):
        with pytest.raises(ValueError):
            geometry.draw_samples(111, 70, 0, **bad)
    with pytest.raises(ValueError):
        geometry.draw_samples(7, 1, 0, size=5)     # status -1 keeps its meaning: fewer than 8 common points, for either solver


def test_solver_keyword_and_launch_constants():
    import inspect
    import os

    from conftest import ROOT
    from multicam_calibration_amd import geometry, ops

    uvs, _, intr, _ = ts.make("thin3")
    for fn, args in ((geometry.estimate_relative_pose, (uvs[0], uvs[1], intr[0], intr[1])), (geometry.extrinsics_from_keypoints, (uvs, intr))):
        assert inspect.signature(fn).parameters["solver"].default == "8point"
        with pytest.raises(ValueError, match="solver"):
            fn(*args, threshold=2.5, solver="7point", device=10 ** 6)
        with pytest.raises(ValueError, match="1024"):
            fn(*args, threshold=2.5, solver="5point", n_hypotheses=1025, device=10 ** 6)
    # seven common points: status -1 for the five-point solver too, before any device is touched
    u1 = np.array(uvs[1])
    u1[7:] = np.nan
    tr, inl, info = geometry.estimate_relative_pose(uvs[0], u1, intr[0], intr[1], threshold=2.5, solver="5point", n_hypotheses=64, device=10 ** 6, return_info=True)
    assert info["status"] == -1 and info["n_common"] == 7 and np.isnan(tr).all() and not inl.any() and info["sample"] == -1 and info["slot"] == -1
    src = open(os.path.join(ROOT, "include", "mcba.h")).read()
    for macro, value in (("MCBA_TWOVIEW5_SAMPLE", ops.TWOVIEW5_SAMPLE), ("MCBA_TWOVIEW5_SLOTS", ops.TWOVIEW5_SLOTS), ("MCBA_TWOVIEW5_MAX_SAMPLES", ops.TWOVIEW5_MAX_SAMPLES)):
        assert f"#define {macro} {value}" in src, macro
    assert (ops.TWOVIEW5_SAMPLE, ops.TWOVIEW5_SLOTS, ops.TWOVIEW5_MAX_SAMPLES) == (5, 10, 1024)
    lib = ops.load_library()
    assert hasattr(lib, "mcba_two_view_ransac5") and "mcba_two_view_ransac5" in {s[0] for s in ops.SYMBOLS} and lib.mcba_abi_version() == 7
