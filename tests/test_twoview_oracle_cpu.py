"""tests/twoview_oracle.py held to its own rules on the scenes the other tiers use (no GPU): the conditioning and ambiguity figures its docstring
quotes, the two routes to E, exact recovery without noise, and the chain + scipy against the stored optima of tests/golden/kpba.npz.  Also the
host-side pieces of the feature that need no device: draw_samples and calibration._co_detection_counts."""
import os

import numpy as np
import pytest

import kpba_oracle as ko
import keypoint_scenes as ks
import twoview_oracle as tvo
from oracle import triangulate_oracle as tri
from test_triangulate_cpu import scene

_cache = {}


def stages(name, H):
    if (name, H) not in _cache:
        ua, ub, ia, ib, idx, sc = tvo.pair_of(name)
        smp = tvo.draw_samples(len(ua), H, 0)
        _cache[(name, H)] = (tvo.two_view(ua, ub, ia, ib, smp, tvo.THRESHOLD), smp)
    return _cache[(name, H)]


@pytest.mark.parametrize("H", [64, 512])
@pytest.mark.parametrize("name", tvo.SCENES)
def test_scene_rules(name, H):
    o, smp = stages(name, H)
    hyp, sc = o["hyp"], o["score"]
    ok = ~hyp["ill"]
    mult = tvo.route_multiple(o["prep"], smp)
    und = sc["undecided"][ok]
    front = np.sort(o["vote"]["in_front"])[::-1]
    ill_cost = sc["cost"][hyp["ill"] & np.isfinite(sc["cost"])]
    print(f"{name} H {H}: M {len(o['inliers'])} ill {hyp['ill'].mean():.4f} route multiple {mult:.3g} undecided {und.mean():.3g} winner {o['winner']} cost {o['cost']:.6g} inliers {o['n_inliers']} "
          f"in front {o['vote']['in_front']} cheapest ill / winner {ill_cost.min() / o['cost'] if len(ill_cost) else np.inf:.3g}")
    assert hyp["ill"].mean() <= 0.02
    assert 8 * mult <= tvo.K_E and mult <= tvo.K_E_MEASURED * 1.001
    assert und.mean() <= 0.01 and not und.any()          # the chosen scenes have none
    assert not sc["undecided"][o["winner"]].any() and not hyp["ill"][o["winner"]]
    assert o["comparable"]
    assert front[0] - front[1] > 0.1 * o["n_inliers"]
    b = sc["cost_bound"][ok]
    assert (b < 1e-6 * sc["cost"][ok]).all()             # the bound is rounding, not slack


def test_noise_free_scene_gives_the_true_pose():
    uvs, ext, intr, X = scene(C=2, P=120, seed=5, noise=0.0)
    o = tvo.two_view(uvs[0], uvs[1], intr[0], intr[1], tvo.draw_samples(120, 32, 1), 0.5, iterations=25)
    R0, R1 = ks.rodrigues(ext[0][:3]), ks.rodrigues(ext[1][:3])
    R = R1 @ R0.T
    t = ext[1][3:] - R @ ext[0][3:]
    assert o["n_inliers"] == 120 and o["n_in_front"] == 120
    assert np.abs(o["rt12"][:9].reshape(3, 3) - R).max() < 1e-9 and np.abs(o["rt12"][9:] - t / np.linalg.norm(t)).max() < 1e-9
    Xa = X @ R0.T + ext[0][3:]
    assert np.abs(o["points"] * np.linalg.norm(t) - Xa).max() < 1e-6


def test_candidates_are_the_four_decompositions():
    o, _ = stages("three", 64)
    E = o["hyp"]["E"][o["winner"]].reshape(3, 3)
    Rt = tvo.candidates(E)
    for c in range(4):
        R, t = Rt[c][:9].reshape(3, 3), Rt[c][9:]
        assert abs(np.linalg.det(R) - 1) < 1e-12 and abs(np.linalg.norm(t) - 1) < 1e-12
        assert np.abs(tvo.skew(t) @ R - (E if c in (0, 3) else -E)).max() < 1e-12


@pytest.mark.parametrize("name", ["three", "six"])
def test_chain_and_scipy_reproduce_the_stored_optimum(name):
    if name == "six" and os.environ.get("MCBA_SLOW_TESTS") != "1":
        pytest.skip("about a minute of scipy: MCBA_SLOW_TESTS=1")
    i, o = ko.case(name)
    ch = tvo.chain(i["uvs"], i["intr"], tvo.THRESHOLD)
    pts0 = tri.triangulate(i["uvs"], ch["extrinsics"], i["intr"])
    r = ko.solve(i["uvs"], ch["extrinsics"], i["intr"], pts0, loss=i["loss"], scale_camera=o["scale_camera"], baseline=ko.baseline_of(o["extrinsics"], 0, o["scale_camera"]))
    spread = ko.relative_spread(r["extrinsics"], o["extrinsics"])
    print(f"{name}: tree {ch['tree']} scales {ch['scales']} extrinsics vs golden {spread:.3g} cost {r['cost']:.12g} golden {o['cost']:.12g}")
    assert spread <= 1e-7 and abs(r["cost"] / o["cost"] - 1) <= 1e-9


# ---------------------------------------------------------------- host-side pieces of the product
def test_draw_samples_is_seeded_and_leaves_the_global_generator_alone():
    from multicam_calibration_amd import geometry

    np.random.seed(123)
    before = np.random.get_state()[1].copy()
    a = geometry.draw_samples(111, 70, [0, 2, 1])
    b = geometry.draw_samples(111, 70, [0, 2, 1])
    assert np.array_equal(np.random.get_state()[1], before)
    assert a.dtype == np.int32 and a.shape == (70, 8) and np.array_equal(a, b) and np.array_equal(a, tvo.draw_samples(111, 70, [0, 2, 1]))
    assert a.min() >= 0 and a.max() < 111 and all(len(set(r)) == 8 for r in a.tolist())
    assert not np.array_equal(a, geometry.draw_samples(111, 70, [0, 1, 2]))
    with pytest.raises(ValueError):
        geometry.draw_samples(7, 1, 0)


@pytest.mark.parametrize("C,P", [(2, 1), (5, 63), (6, 64), (7, 1000), (64, 5000)])
def test_co_detection_counts_both_routes(monkeypatch, C, P):
    from multicam_calibration_amd import calibration as cal

    seen = np.random.default_rng(C * 1000 + P).uniform(size=(C, P)) < 0.6
    ref = seen.astype(np.int64) @ seen.astype(np.int64).T
    got = cal._co_detection_counts(seen)
    assert got.dtype == np.int64 and np.array_equal(got, ref)
    monkeypatch.delattr(np, "bitwise_count", raising=False)
    assert not hasattr(np, "bitwise_count")
    old = cal._co_detection_counts(seen)
    assert old.dtype == np.int64 and np.array_equal(old, ref)
