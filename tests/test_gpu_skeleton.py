"""refine_skeleton and estimate_bone_lengths on the GPU (csrc/mcba_skeleton.hip through mcba_refine_skeleton, mcba_refine_skeleton_system and
mcba_bone_lengths) against tests/skeleton_oracle.py, on its cases: K = 1 (no bones), 2, 3 as a chain and as a star, 5 (G = 51 frames per
workgroup, one idle lane), 33 (G = 7, 25 idle lanes), 64 as a chain (63 levels of barriers) and as a star, a forest of two pieces; T = 1, G - 1,
G, G + 1 and 3 G + 1 for K = 5 and K = 64; C = 1 (nothing usable), 2 and 6; frames whose unseen keypoints split a tree, a piece of single-view
keypoints only, a single-view leaf and a single-view inner node with usable children.

One evaluation (refine_skeleton_system): information within 1e-12 max|.| of the oracle, the gradient within 1e-12 of its scale, the step within
4 eps cond max|d| of the dense solve of the system built from the returned information, directions and gradient, the costs within
1e-9 max(1, cost) + 100 eps cond cost.  The loop: cost <= cost_start exactly, one further oracle step moves less than 10 xtol max|x|,
n_iterations is the oracle's where that is decided (skeleton_oracle.decided; at most one frame in ten is not), statuses exact, the covariance
within the section 8f-20 bar of the inverse of the dense matrix built from the returned information and directions.  Identical bits: two calls,
a frame alone against the same frame among 3 G + 1, weights=None against ones, a zero or NaN weight against a NaN detection.
estimate_bone_lengths equals numpy's nanmedian of the float64 distances exactly."""
import numpy as np
import pytest

import skeleton_oracle as sko

pytestmark = pytest.mark.gpu

CASES = sko.cases()
LOOP_FIELDS = ("points", "keypoint_status", "frame_status", "n_iterations", "cost", "cost_start", "bone_residual", "covariance", "std", "information", "direction")


def args(case, **kw):
    a = dict(bones=case["bones"], bone_length=case["bone_length"], bone_std=case["bone_std"], pixel_std=case["pixel_std"], loss=case["loss"], f_scale=case["f_scale"], weights=case["weights"])
    a.update(kw)
    return a


def loop(case, frames=slice(None), uvs=None, covariance=True, **kw):
    """(result, its fields with the per-bone planes laid out by the bone's child end) on the frames of the slice"""
    from multicam_calibration_amd import refine_skeleton

    kw = args(case, **kw)
    if kw["weights"] is not None:
        kw["weights"] = np.asarray(kw["weights"])[:, frames]
    r = refine_skeleton(case["start"][frames], (case["uvs"] if uvs is None else uvs)[:, frames], case["ext"], case["intr"], covariance=covariance, **kw)
    assert np.array_equal(r.parent, case["parent"])
    got = {f: getattr(r, f) for f in LOOP_FIELDS}
    sub = dict(case, start=case["start"][frames])
    got["bone_residual"] = sko.by_child(r.bone_residual, sub)
    if covariance:
        got["direction"] = sko.by_child(r.direction, sub)
    return r, got


def same_bits(a, b, fields=LOOP_FIELDS):
    return all(np.array_equal(a[f], b[f], equal_nan=True) if a[f] is not None else b[f] is None for f in fields)


@pytest.mark.parametrize("name", sko.SYSTEM_CASES)
def test_one_evaluation_against_the_oracle(name):
    from multicam_calibration_amd import refine_skeleton_system

    case = CASES[name]
    r = refine_skeleton_system(case["start"], case["uvs"], case["ext"], case["intr"], lam=sko.SYSTEM_LAM, **args(case))
    got = {f: getattr(r, f) for f in ("information", "gradient", "step", "data_cost", "bone_cost", "trial_cost", "keypoint_status", "frame_status")}
    got["direction"] = sko.by_child(r.direction, case)
    sko.check_system(name, got)
    K = case["start"].shape[1]
    assert r.info["frames_per_workgroup"] == 256 // K and r.info["levels"] == sko.plan(case["parent"])["levels"]


def test_loop_and_covariance_against_the_oracle_and_identical_bits():
    left_out = total = 0
    for name in sko.LOOP_CASES:
        r, got = loop(CASES[name])
        lo, ran = sko.check_loop(name, got)
        sko.check_covariance(name, got)
        ok = got["keypoint_status"] > 0
        assert np.allclose(r.std[ok] ** 2, r.covariance[ok][..., (0, 1, 2), (0, 1, 2)], rtol=1e-15, atol=0) and np.isnan(r.std[~ok]).all()
        left_out, total = left_out + lo, total + ran
        assert same_bits(got, loop(CASES[name])[1]), name                       # two calls
        plain = loop(CASES[name], covariance=False)[0]
        assert plain.covariance is None and plain.information is None and np.array_equal(plain.points, r.points, equal_nan=True) and np.array_equal(plain.n_iterations, r.n_iterations)
    print(f"undecided frames {left_out} of {total}")
    assert 10 * left_out <= total, (left_out, total)


def test_one_camera_fits_nothing():
    r, got = loop(CASES["C1"])
    assert (r.frame_status == -1).all() and (r.keypoint_status == -2).all() and (r.n_iterations == 0).all()
    assert all(np.isnan(got[f]).all() for f in ("points", "cost", "cost_start", "bone_residual", "covariance", "std", "information", "direction"))


def test_special_frames():
    r, _ = loop(CASES["special"])
    st = r.keypoint_status
    assert list(st[0]) == [2, -1, 2, 2, 2, 2, 2]          # the tree split by the unseen keypoint 1: every piece holds a usable keypoint
    assert list(st[1]) == [2, 2, -1, -2, 2, 2, -2]        # {3, 6}: a piece of single-view keypoints only
    assert list(st[2]) == [2, 2, 2, 2, 1, 2, 1] and list(st[3]) == [2, 1, 2, 2, 2, 2, 2] and list(st[4]) == [2, 2, 1, 1, 2, 2, 1]
    assert list(st[5]) == [2, 2, 2, 2, 2, -1, 2]          # a NaN in the start
    assert np.isfinite(r.points[st > 0]).all() and np.isnan(r.points[st < 0]).all()
    truth = CASES["special"]["truth"]
    single = st == 1
    assert np.linalg.norm(r.points[single][:3] - truth[single][:3], axis=1).max() < 2.0   # the three of frames 2 and 3: located, to within a few bone_std


@pytest.mark.parametrize("name", ["K5", "K64_chain"])
def test_frame_counts_at_the_workgroup_edges_give_the_bits_of_the_whole(name):
    case = CASES[name]
    G = 256 // case["start"].shape[1]
    assert case["start"].shape[0] == 3 * G + 1
    full = loop(case)[1]
    for T in (1, G - 1, G, G + 1):
        part = loop(case, frames=slice(0, T))[1]
        assert all(np.array_equal(part[f], full[f][:T], equal_nan=True) for f in LOOP_FIELDS), (name, T)
    last = loop(case, frames=slice(3 * G, 3 * G + 1))[1]                         # a frame alone against the same frame among 3 G + 1
    assert all(np.array_equal(last[f][0], full[f][3 * G], equal_nan=True) for f in LOOP_FIELDS), name


def test_unit_weights_are_no_weights_and_unseen_is_unseen():
    case = CASES["C6"]
    plain, ones = loop(case, weights=None)[1], loop(case, weights=np.ones(case["uvs"].shape[:3]))[1]
    assert same_bits(plain, ones)
    rng = np.random.default_rng(5)
    hit = rng.uniform(size=case["uvs"].shape[:3]) < 0.1
    w = np.array(case["weights"])
    w[hit] = np.where(rng.uniform(size=int(hit.sum())) < 0.5, 0.0, np.nan)
    uv = np.array(case["uvs"])
    uv[hit] = np.nan
    assert same_bits(loop(case, weights=w)[1], loop(case, uvs=uv)[1])


@pytest.mark.parametrize("T", [1, 2, 256, 257, 600])
def test_bone_lengths_are_numpys_nanmedians(T):
    from multicam_calibration_amd import estimate_bone_lengths

    rng = np.random.default_rng(100 + T)
    K = 6
    pts = rng.normal(0, 40, (T, K, 3))
    pts[rng.uniform(size=(T, K)) < 0.2] = np.nan
    pts[:, 5] = np.nan                                                          # bone (4, 5): no frame has it
    bones = np.array([[0, 1], [1, 2], [3, 0], [2, 3], [4, 5], [4, 0]])
    r = estimate_bone_lengths(pts, bones)
    length, std, count = sko.bone_lengths(pts, bones)
    assert np.array_equal(r.count, count) and r.count[4] == 0
    assert np.array_equal(r.length, length, equal_nan=True) and np.array_equal(r.std, std, equal_nan=True)   # exact: no fused multiply-add in the distance
    assert np.isnan(r.length[4]) and np.isnan(r.std[4])
