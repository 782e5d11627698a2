"""Consensus triangulation on the GPU (csrc/mcba_consensus.hip) through the public function, against the numpy statement of its definition in
tests/consensus_oracle.py: mask, pair and status equal, the winning cost to rtol 1e-9, the points to the refinement gate 5e-6 mm -- the gates of
the host tier (tests/test_hostcheck_consensus.py), with the same ambiguity rule (consensus_oracle.decided).  Every comparison prints its
figures (-s); DESIGN.md section 8f-9 records them."""
import numpy as np
import pytest

import multicam_calibration_amd as m

import consensus_oracle as co
import keypoint_scenes as ks

pytestmark = pytest.mark.gpu
GATE_MM = 5e-6
FORMS = ("lane", "wave", "lane2")   # MCBA_CONSENSUS_FORM (development only): the fused lane form, the wavefront form, the lane form in two launches


def consensus(uvs, ext, intr, threshold, **kw):
    pts, inl, info = m.triangulate_consensus(uvs, ext, intr, threshold=threshold, return_info=True, **kw)
    assert pts.shape == (len(uvs[0]), 3) and inl.shape == (len(uvs), len(uvs[0])) and inl.dtype == bool
    return dict(info, points=pts, inliers=inl)


@pytest.mark.parametrize("threshold", [1.0, 2.5])
@pytest.mark.parametrize("name", ["six", "three", "twelve", "outlier"])
def test_scenes_match_the_oracle(name, threshold):
    uvs, ext, intr, _, o = co.scene_oracle(name, threshold)
    got = consensus(uvs, ext, intr, threshold)
    ok = co.compare(got, o, GATE_MM, f"{name} @ {threshold}")
    assert ok.all()   # the numpy prototype leaves out no point of these scenes: the ambiguity rule is a guard
    fit = o["status"] == 1
    assert np.all(got["cost"][fit] <= got["cost0"][fit]) and np.all(got["n_iterations"][~fit] == 0)


@pytest.mark.parametrize("C,P", co.BOUNDARY_CASES)
def test_launch_boundaries(C, P):
    uvs, ext, intr, o = co.boundary_oracle(C, P)
    got = consensus(uvs, ext, intr, 2.5)
    co.compare(got, o, GATE_MM, f"C {C} P {P}")


def test_one_point_no_point_and_a_blind_camera():
    uvs, ext, intr, o = co.boundary_oracle(8, 257)
    one = [u[3:4] for u in uvs]
    co.compare(consensus(one, ext, intr, 2.5), co.consensus(one, ext, intr, 2.5), GATE_MM, "P = 1")
    none = [u[:0] for u in uvs]
    pts, inl, info, err = m.triangulate_consensus(none, ext, intr, threshold=2.5, return_info=True, return_errors=True, device=10 ** 6)   # (no device is touched)
    assert pts.shape == (0, 3) and inl.shape == (8, 0) and err.shape == (8, 0) and info["pair"].shape == (0, 2) and info["status"].shape == (0,)
    blind = [u.copy() for u in uvs]
    blind[5][:] = np.nan
    ob = co.consensus(blind, ext, intr, 2.5)
    got = consensus(blind, ext, intr, 2.5)
    co.compare(got, ob, GATE_MM, "camera 5 sees nothing")
    assert not got["inliers"][5].any() and not np.any(got["pair"] == 5)


def test_exact_ties_go_to_the_lower_pair():
    uvs, ext, intr, _ = co.duplicated_camera_scene()
    o = co.consensus(uvs, ext, intr, 2.5)
    got = consensus(uvs, ext, intr, 2.5)
    assert np.array_equal(got["inliers"], o["inliers"]) and np.array_equal(got["status"], o["status"])
    assert np.abs(got["points"] - o["points"]).max() <= GATE_MM
    np.testing.assert_allclose(got["hypothesis_cost"], o["hypothesis_cost"], rtol=1e-9)
    # the oracle's pair or its exact-tie twin: unrolled device code need not round the twins identically
    twins = sum(tuple(g) != tuple(w) for g, w in zip(got["pair"], o["pair"]))
    print(f"{twins} of {len(o['pair'])} points end on the twin of the oracle's pair")
    assert all(tuple(g) in (tuple(w), co.twin_pair(w)) for g, w in zip(got["pair"], o["pair"]))


def test_both_kernel_forms_pick_the_same_winner(monkeypatch):
    uvs, ext, intr, _, o = co.scene_oracle("six", 2.5)
    res = {}
    for form in FORMS:
        monkeypatch.setenv("MCBA_CONSENSUS_FORM", form)
        res[form] = consensus(uvs, ext, intr, 2.5)
        co.compare(res[form], o, GATE_MM, f"six, form {form}")
    monkeypatch.setenv("MCBA_CONSENSUS_FORM", "neither")
    with pytest.raises(m.ops.McbaError):
        consensus(uvs, ext, intr, 2.5)
    monkeypatch.delenv("MCBA_CONSENSUS_FORM")
    for form in FORMS[1:]:
        for key in ("inliers", "pair", "points", "hypothesis_cost", "status", "n_iterations"):
            assert np.array_equal(res["lane"][key], res[form][key], equal_nan=True), (form, key)
    # ... and on a rig the wavefront form is the default for
    uvs, ext, intr, o = co.boundary_oracle(9, 130)
    monkeypatch.setenv("MCBA_CONSENSUS_FORM", "lane")
    lane = consensus(uvs, ext, intr, 2.5)
    monkeypatch.delenv("MCBA_CONSENSUS_FORM")
    wave = consensus(uvs, ext, intr, 2.5)
    for key in ("inliers", "pair", "points", "hypothesis_cost", "status"):
        assert np.array_equal(lane[key], wave[key], equal_nan=True), key


def test_outlier_scene_flags_exactly_the_displaced_detections(golden):
    uvs, ext, intr, X, _ = co.scene_oracle("outlier", 2.5)
    pts, inl, info = m.triangulate_consensus(uvs, ext, intr, threshold=2.5, return_info=True)
    seen = ~np.isnan(np.stack(uvs)).any(-1)
    displaced = seen & (ks.errors(X, uvs, ext, intr) > 5.0)           # farther than 5 px from the truth's projection
    has = info["status"] != -1
    assert displaced.sum() >= 40 and np.array_equal(~inl & seen & has[None], displaced & has[None])
    gold = golden("geometry.npz")
    ok = ~np.isnan(gold["outlier_start"]).any(1)

    def rms(A):
        return np.sqrt(np.mean(np.sum((A[ok] - X[ok]) ** 2, axis=1)))

    print(f"flagged {int((~inl & seen & has[None]).sum())} of {int(seen[:, has].sum())} detections; rms to truth: consensus {rms(pts):.4f}, soft_l1 {rms(gold['outlier_soft_l1']):.4f}, "
          f"median of pairs {rms(gold['outlier_start']):.4f} mm")
    assert rms(pts) < rms(gold["outlier_soft_l1"])


def test_errors_are_the_reprojection_errors_at_the_returned_points():
    for C, P in ((8, 257), (9, 130)):
        uvs, ext, intr, _ = co.boundary_oracle(C, P)
        pts, inl, err = m.triangulate_consensus(uvs, ext, intr, threshold=2.5, return_errors=True)
        want, _ = m.keypoint_reprojection_errors(pts, uvs, ext, intr)
        assert err.shape == (C, P) and np.array_equal(err, want, equal_nan=True)
        pts2, inl2 = m.triangulate_consensus(uvs, ext, intr, threshold=2.5)
        assert np.array_equal(pts2, pts, equal_nan=True) and np.array_equal(inl2, inl)


def test_zero_iterations_and_other_losses():
    uvs, ext, intr, _, o = co.scene_oracle("outlier", 2.5)
    hyp = consensus(uvs, ext, intr, 2.5, max_iterations=0)
    fit = o["status"] == 1
    np.testing.assert_allclose(hyp["points"][fit], o["hypothesis"][fit], rtol=0, atol=1e-9)
    assert np.all(hyp["n_iterations"] == 0) and np.array_equal(hyp["cost"], hyp["cost0"], equal_nan=True)
    for loss in ("soft_l1", "cauchy"):
        got = consensus(uvs, ext, intr, 2.5, loss=loss, f_scale=1.5)
        assert np.array_equal(got["inliers"], hyp["inliers"]) and np.array_equal(got["pair"], hyp["pair"])       # the search does not depend on the refit
        want = m.refine_triangulation(hyp["points"], [np.where(hyp["inliers"][c][:, None], uvs[c], np.nan) for c in range(len(uvs))], ext, intr, loss=loss, f_scale=1.5)
        assert np.array_equal(np.isnan(got["points"]), np.isnan(want)) and np.abs(got["points"] - want)[fit].max() <= GATE_MM, loss   # (another kernel: not bit for bit)


def test_arguments_are_refused_before_the_device_is_touched():
    uvs, ext, intr, _, _ = co.scene_oracle("three", 2.5)
    far = dict(device=10 ** 6)                                          # a device that does not exist: reaching it would be another error
    with pytest.raises(TypeError):
        m.triangulate_consensus(uvs, ext, intr, **far)                  # no default threshold
    for kw in (dict(threshold=0.0), dict(threshold=-1.0), dict(threshold=np.nan), dict(threshold=2.5, min_views=1), dict(threshold=2.5, loss="l2"), dict(threshold=2.5, f_scale=0.0),
               dict(threshold=2.5, max_iterations=-1), dict(threshold=2.5, undistort_iterations=-1)):
        with pytest.raises(ValueError):
            m.triangulate_consensus(uvs, ext, intr, **kw, **far)
    with pytest.raises(NotImplementedError):
        m.triangulate_consensus(uvs[:1], ext[:1], intr[:1], threshold=2.5, **far)
