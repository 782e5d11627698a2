"""mcba_two_view_ransac5 (csrc/mcba_fivepoint.hip) and solver="5point" of the two public functions above it on the GPU,
held to tests/fivepoint_oracle.py by the rules of that module's docstring: the candidate table at its launch edges (one sample; 7, 64 and 103
samples -- a lane short of, at and past a wavefront of samples, the packed table short of, across and over several chunks of the scoring grid;
8 points; 1024 + 1 points, a second workgroup of the scorer), the scores of the packed table through twoview_oracle.check_scores and the winner
and pose through check_pose (the oracle scoring the very table that came back), bitwise repeatability, solver="8point" bit-identical to no
keyword, the chain on a thin scene against the optimum reached from the true extrinsics, every tree edge of "thin6", and the error paths.
Output buffers start as sentinels."""
import numpy as np
import pytest

import fivepoint_oracle as fo
import keypoint_scenes as ks
import kpba_oracle as ko
import thin_scenes as ts
import twoview_oracle as tvo
from multicam_calibration_amd import geometry, ops, refine_extrinsics
from multicam_calibration_amd.calibration import _spanning_tree
from multicam_calibration_amd.triangulation import _cam_blocks

pytestmark = pytest.mark.gpu
THR = tvo.THRESHOLD
SLOTS, CAP = ops.TWOVIEW5_SLOTS, ops.TWOVIEW5_MAX_SAMPLES
TIGHT = dict(ftol=1e-15, xtol=1e-15, gtol=1e-10, max_nfev=200)   # tests/test_gpu_twoview.py's
CHAIN_BAR = 1e-6                                                  # ... and its bar on the chain's result (kpba_oracle.check_result; the truth-start test)
SENTINEL = 7.0


def call5(ua, ub, ia, ib, samples, threshold, H=None):
    """mcba_two_view_ransac5 through ops.call; every output starts as a sentinel.  Returns the outputs (an error raises, with `last` holding them)."""
    cam, dist = _cam_blocks([np.zeros(6)] * 2, [ia, ib])
    ua, ub = np.ascontiguousarray(ua), np.ascontiguousarray(ub)
    M = len(ua)
    H = len(samples) if H is None else H
    S = SLOTS * max(H, 1)
    g = dict(rt12=np.full(12, SENTINEL), best=np.full(4, SENTINEL), mask=np.full(M, 7, np.uint8), points=np.full((M, 3), SENTINEL), E=np.full((S, 9), SENTINEL), cost=np.full(S, SENTINEL),
             count=np.full(S, 7, np.uint32), status=np.full(S, 7, np.int32), kernel_ms=np.full(6, SENTINEL))
    call5.last = g
    smp = np.ascontiguousarray(samples, dtype=np.int32)
    ops.call("mcba_two_view_ransac5", M, ua.ctypes.data, ub.ctypes.data, cam.ctypes.data, dist.ctypes.data, H, smp.ctypes.data, float(threshold), 5, 0, g["rt12"].ctypes.data, g["best"].ctypes.data,
             g["mask"].ctypes.data, g["points"].ctypes.data, g["E"].ctypes.data, g["cost"].ctypes.data, g["count"].ctypes.data, g["status"].ctypes.data, g["kernel_ms"].ctypes.data)
    g["inliers"] = g["mask"].astype(bool)
    return g


def untouched(g):
    return all((g[k] == 7).all() for k in ("rt12", "best", "mask", "points", "E", "cost", "count", "status", "kernel_ms"))


_cache = {}


def case(name, H, M=None):
    """(uv_a, uv_b, intr_a, intr_b, samples, prep, per-sample candidates of the oracle) of pair (0, 1) of a scene, the first M points: computed once,
    read-only"""
    if (name, H, M) not in _cache:
        ua, ub, ia, ib, _, _ = fo.pair_of(name)
        ua, ub = np.ascontiguousarray(ua[:M]), np.ascontiguousarray(ub[:M])
        smp = fo.draw_samples(len(ua), H, 0)
        prep = tvo.prepare(ua, ub, ia, ib)
        _cache[(name, H, M)] = (ua, ub, ia, ib, smp, prep, fo.hypotheses(prep, smp)["per_sample"])
    return _cache[(name, H, M)]


def check_call(label, g, ua, ub, ia, ib, per, pose=True):
    """the candidate table against the oracle's; then the oracle scores the packed table that came back: costs, counts, winner, mask, pose, points"""
    H = len(per)
    fo.check_candidates(label, g["E"].reshape(H, SLOTS, 9), g["status"].reshape(H, SLOTS), dict(hyp=dict(per_sample=per)))
    live = fo.compaction(g["status"].reshape(H, SLOTS))
    assert len(live) > 0 and np.isinf(g["cost"][g["status"] != 1]).all() and (g["count"][g["status"] != 1] == 0).all()
    assert g["best"][0] in live and (g["kernel_ms"] >= 0).all()
    o = tvo.two_view(ua, ub, ia, ib, None, THR, essential_in=g["E"][live])
    packed = dict(g, cost=g["cost"][live], count=g["count"][live], status=g["status"][live], best=np.r_[float(np.searchsorted(live, g["best"][0])), g["best"][1:]])
    tvo.check_scores(label, packed, o)
    if pose and o["comparable"]:
        tvo.check_pose(label, packed, o)
    return o


# ---------------------------------------------------------------- the launch edges
@pytest.mark.parametrize("H", [1, 7, 64, 103])
def test_samples_at_the_launch_edges(H):
    ua, ub, ia, ib, smp, _, per = case("thin3", 103)
    g = call5(ua, ub, ia, ib, smp[:H], THR)
    o = check_call(f"thin3 H {H}", g, ua, ub, ia, ib, per[:H])
    assert o["comparable"] or H == 1
    if H >= 64:                      # the point of the feature: a handful of minimal samples takes every point of the slab
        assert g["best"][2] == len(ua)


def test_eight_points():
    ua, ub, ia, ib, smp, _, per = case("thin3", 7, 8)
    g = call5(ua, ub, ia, ib, smp, THR)
    check_call("thin3 M 8", g, ua, ub, ia, ib, per, pose=False)   # (eight points: candidates of a sample tie on its five; check_scores compares the winner where the rule allows)


def test_one_point_past_a_workgroup_of_the_scoring_kernel():
    ua, ub, ia, ib, smp, _, per = case("thin3_1025", 7)
    assert len(ua) == ops.TWOVIEW_POINTS_PER_BLOCK + 1
    g = call5(ua, ub, ia, ib, smp, THR)
    o = check_call("thin3 M 1025", g, ua, ub, ia, ib, per)
    assert o["comparable"]


def test_sixty_millimetre_cloud():
    ua, ub, ia, ib, smp, _, per = case("three", 64)
    g = call5(ua, ub, ia, ib, smp, THR)
    assert check_call("three H 64", g, ua, ub, ia, ib, per)["comparable"]


# ---------------------------------------------------------------- repeatability, the default
def test_two_calls_return_the_same_bits():
    ua, ub, ia, ib, smp, _, _ = case("thin3", 103)
    a, b = call5(ua, ub, ia, ib, smp, THR), call5(ua, ub, ia, ib, smp, THR)
    for k in ("rt12", "best", "mask", "points", "E", "cost", "count", "status"):
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    uvs, _, intr, _ = ts.make("thin3")
    p, q = (geometry.estimate_relative_pose(uvs[0], uvs[1], intr[0], intr[1], threshold=THR, n_hypotheses=64, solver="5point", return_info=True) for _ in range(2))
    assert np.array_equal(p[0], q[0]) and np.array_equal(p[1], q[1]) and np.array_equal(p[2]["points"], q[2]["points"], equal_nan=True) and np.array_equal(p[2]["samples"], q[2]["samples"])


def test_the_default_solver_is_the_eight_point_one_bit_for_bit():
    uvs, _, intr, _ = ks.make("three")
    a = geometry.estimate_relative_pose(uvs[0], uvs[1], intr[0], intr[1], threshold=THR, return_info=True)
    b = geometry.estimate_relative_pose(uvs[0], uvs[1], intr[0], intr[1], threshold=THR, return_info=True, solver="8point")
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2]["samples"], b[2]["samples"]) and a[2]["samples"].shape[1] == 8
    for k in ("n_common", "n_inliers", "cost", "hypothesis", "n_in_front", "status"):
        assert a[2][k] == b[2][k], k
    assert np.array_equal(a[2]["points"], b[2]["points"], equal_nan=True) and b[2]["sample"] == b[2]["hypothesis"] and b[2]["slot"] == 0
    r, s = geometry.extrinsics_from_keypoints(uvs, intr, threshold=THR, refine=False), geometry.extrinsics_from_keypoints(uvs, intr, threshold=THR, refine=False, solver="8point")
    assert np.array_equal(r.extrinsics, s.extrinsics) and np.array_equal(r.points, s.points, equal_nan=True)


# ---------------------------------------------------------------- the public functions on thin scenes
def test_estimate_relative_pose_five_point_matches_the_oracle():
    uvs, _, intr, _ = ts.make("thin3")
    o = fo.two_view5(uvs[0], uvs[1], intr[0], intr[1], fo.draw_samples(len(uvs[0]), 64, 0), THR)
    tr, inl, info = geometry.estimate_relative_pose(uvs[0], uvs[1], intr[0], intr[1], threshold=THR, n_hypotheses=64, solver="5point", return_info=True)
    want = np.r_[tvo.rodrigues_inv(o["rt12"][:9].reshape(3, 3)), o["rt12"][9:]]
    print(f"thin3 (0, 1): transform error {np.abs(tr - want).max():.3g}; inliers {info['n_inliers']} of {info['n_common']}; sample {info['sample']} slot {info['slot']} hypothesis {info['hypothesis']}")
    assert o["comparable"] and info["status"] == 1 and (info["sample"], info["slot"], info["hypothesis"]) == (o["sample"], o["slot"], o["winner"])
    assert np.abs(tr - want).max() <= 1e-9 and np.array_equal(inl, o["inliers"]) and info["samples"].shape == (64, 5) and info["n_inliers"] == len(uvs[0])


def test_chain_on_a_thin_scene_reaches_the_optimum_of_the_true_start():
    """extrinsics_from_keypoints(solver="5point", refine=True) on "thin3" against refine_extrinsics from the scene's true extrinsics, moved into
    camera 0's frame and rescaled to that optimum's own baseline: every camera centre within tests/test_gpu_twoview.py's bar on the chain."""
    uvs, ext, intr, _ = ts.make("thin3")
    ref = refine_extrinsics(uvs, ext, intr, loss="linear", gauge_camera=0, scale_camera=1, **TIGHT)
    R0, t0 = ks.rodrigues(ref.extrinsics[0][:3]), ref.extrinsics[0][3:]
    want = np.zeros((len(ext), 6))
    for c in range(1, len(ext)):
        R = ks.rodrigues(ref.extrinsics[c][:3]) @ R0.T
        want[c] = np.r_[tvo.rodrigues_inv(R), ref.extrinsics[c][3:] - R @ t0]
    r = geometry.extrinsics_from_keypoints(uvs, intr, threshold=THR, n_hypotheses=64, solver="5point", refine=True, loss="linear", scale_camera=1, baseline=ko.baseline_of(ref.extrinsics, 0, 1), **TIGHT)
    got, ctr = ko.centres(r.extrinsics), ko.centres(want)
    err = np.abs(got - ctr) / np.maximum(1.0, np.abs(ctr))
    print(f"thin3 chain: tree {r.tree} edges {[(e['n_inliers'], e['n_common']) for e in r.edges]} cost {r.refinement.cost:.12g} (truth start {ref.cost:.12g}); centres {err.max():.3g} (bar {CHAIN_BAR})")
    assert all(e["status"] == 1 and e["n_inliers"] >= 0.95 * e["n_common"] for e in r.edges)
    assert err.max() <= CHAIN_BAR


def test_every_tree_edge_of_thin6():
    uvs, _, intr, _ = ts.make("thin6")
    seen = np.stack([np.isfinite(u).all(-1) for u in uvs])
    for i, j in _spanning_tree(seen, 0):
        _, inl, info = geometry.estimate_relative_pose(uvs[i], uvs[j], intr[i], intr[j], threshold=THR, n_hypotheses=64, seed=[0, int(i), int(j)], solver="5point", return_info=True)
        print(f"thin6 ({i}, {j}): {info['n_inliers']} of {info['n_common']} inliers, status {info['status']}")
        assert info["status"] == 1 and info["n_inliers"] >= 0.95 * info["n_common"]


# ---------------------------------------------------------------- error paths
def test_error_paths_leave_the_outputs_unwritten():
    ua, ub, ia, ib, smp, _, _ = case("thin3", 103)
    twice = smp.copy()
    twice[17, 4] = twice[17, 2]
    beyond = smp.copy()
    beyond[3, 0] = len(ua)
    for what, args in (("M = 7", (ua[:7], ub[:7], ia, ib, np.zeros((1, 5), np.int32) + np.arange(5, dtype=np.int32), THR)),
                       ("H = cap + 1", (ua, ub, ia, ib, fo.draw_samples(len(ua), CAP + 1, 0), THR)),
                       ("H = 0", (ua, ub, ia, ib, smp, THR, 0)),
                       ("a repeated index", (ua, ub, ia, ib, twice, THR)),
                       ("an index out of range", (ua, ub, ia, ib, beyond, THR)),
                       ("threshold = 0", (ua, ub, ia, ib, smp, 0.0))):
        with pytest.raises(ops.McbaError) as e:
            call5(*args)
        print(what, "->", e.value)
        assert e.value.code == ops.ERR_ARG and untouched(call5.last), what
    uvs, _, intr, _ = ts.make("thin3")
    with pytest.raises(ValueError, match="1024"):
        geometry.estimate_relative_pose(uvs[0], uvs[1], intr[0], intr[1], threshold=THR, n_hypotheses=CAP + 1, solver="5point")
