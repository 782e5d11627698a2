"""calibration_uncertainty on the GPU at the edges of its launches (csrc/mcba_cov.hip), beside the end-to-end cases of tests/test_gpu_covariance.py:

  frames without data first and last in a group of k_cov_frames, alone in the last group, and a whole group of them;
  the camera chain alone (k_cov_cam_factor / _linv / _gram) against the long-double inverse of the Schur complement the device itself reduced, at the
  natural four-frame shapes: 64 cond_2 eps of THAT matrix, the project's bound applied to what the kernels started from;
  two calls, the same bits; k_cov_wss past its grid cap of 1024 blocks; as many scalars as free parameters;
  the failing pivot on the device (the atomicMin of k_cov_cam_factor, the message), the handle after it, the 26-camera limit of fix_intrinsics.

Metric and bound are those of tests/test_gpu_covariance.py; every test prints its figures before it asserts."""
import numpy as np
import pytest

import covariance_oracle as cvo
from multicam_calibration_amd import calibration_uncertainty, ops, synth
from test_gpu_covariance import check_against, check_exact, check_frame_stage, check_launch_shape, run

gpu = pytest.mark.gpu


# ---------------------------------------------------------------- frames without data at the group edges
@gpu
@pytest.mark.parametrize("blank", [(8,), (7,), (16,), tuple(range(8))], ids=["first_of_a_group", "last_of_a_group", "alone_in_the_last_group", "a_whole_group"])
def test_frames_without_data_at_group_edges(blank):
    """C = 2, F = 17 (groups 0..7, 8..15, 16): the blanked frames' blocks are NaN, they are counted and leave p; every other block and the camera
    block are the oracle's of the remaining frames (the oracle deletes the columns of a frame without data)"""
    pr, _ = cvo.case("c2_f17")
    uvs = pr["uvs"].copy()
    uvs[:, list(blank)] = np.nan
    o = cvo.covariance(pr["x"], uvs, pr["obj"], **pr["kwargs"])
    assert o["nodata"].sum() == len(blank) and o["n_free"] == 18 + 6 * (17 - len(blank))
    u = calibration_uncertainty(uvs, pr["extrinsics"], pr["intrinsics"], pr["obj"], pr["poses"], **pr["kwargs"])
    check_launch_shape(u, 24, f"c2_f17 without {blank}")
    assert np.isnan(u.pose_covariance[list(blank)]).all() and np.isnan(u.pose_std[list(blank)]).all()
    assert u.info["n_degenerate_frames"] == len(blank)
    check_against(u, o, f"c2_f17 without {blank}", skip_frames=blank)
    check_exact(u, o, 2)
    check_frame_stage(u, o, f"c2_f17 without {blank}")


# ---------------------------------------------------------------- the camera chain against the device's own Schur complement
@gpu
@pytest.mark.parametrize("name", ["c27_f5_missing", "c40_f9_missing_huber_fs07"])
def test_camera_chain_against_the_devices_own_schur_complement(name):
    """linearise with the IRLS weight and reduce with lambda = 0 on a handle, keep S0, then covariance() on the same handle: the camera block against
    sigma2 S_g^-1 of that S0 (its upper triangle, what k_cov_cam_factor reads) in long double, within 64 cond_2 eps of its scaled form"""
    pr, o = cvo.case(name)
    kw = pr["kwargs"]
    C = pr["uvs"].shape[0]
    prob = ops.Problem(pr["uvs"], pr["obj"], loss=kw["loss"], f_scale=kw["f_scale"])
    try:
        prob.set_params(0, pr["x"])
        prob.set_curvature_floor(1.0)
        prob.linearize(0)
        S0 = prob.reduce_fetch(0.0)["S0"].copy()
        cam, _, info = prob.covariance(0, kw["gauge_camera"], 0.04)
    finally:
        prob.close()
    assert info[6] == 4 and info[7] == cvo.expected_ld(12 * C)
    held = cvo.held_camera_params(C, kw["gauge_camera"], False)
    ref, cond = cvo.camera_reference(S0, held, 0.04)
    e = cvo.rel_err(cam, ref)
    e_oracle = cvo.rel_err(ref, o["camera_covariance"] * (0.04 / o["sigma2"]))
    print(f"{name}: n {12 * C} cond(S_g scaled) {cond:.3g} (of H: {o['cond']:.3g}) cameras against the device's S0 {e:.3g} = {e / (cond * cvo.EPS):.2f} cond eps (bound 64); "
          f"that reference against the oracle {e_oracle:.3g} (bound {o['bound']:.3g})")
    assert e <= cvo.BOUND_FACTOR * cond * cvo.EPS
    assert e_oracle <= o["bound"]   # the device's S0 is the oracle's Schur complement
    assert (cam[held] == 0.0).all() and (cam[:, held] == 0.0).all()


@gpu
def test_two_calls_return_the_same_bits():
    """27 cameras: the only atomics of the chain are on integers, so a second call is the first, bit for bit"""
    pr, _ = cvo.case("c27_f5_missing")
    a, b = run(pr), run(pr)
    assert a.info["group"] == b.info["group"] == 4
    for k in ("camera_covariance", "pose_covariance", "intrinsics_std", "extrinsics_std", "pose_std"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert (a.sigma2, a.n_residuals, a.n_free) == (b.sigma2, b.n_residuals, b.n_free)


# ---------------------------------------------------------------- the noise scale
@gpu
def test_noise_scale_past_the_grid_cap():
    """C = 2, F = 9720: 2 099 520 scalars, more than the 1024 x 2048 that k_cov_wss covers without striding.  sigma2 to 1e-12 relative against the
    residual-only oracle, the counts exactly"""
    p = synth.make_problem(2, 9720)
    assert p["uvs"].size == 2099520 > 1024 * 2048
    x = np.concatenate([p["true_cam"].ravel(), p["true_poses"].ravel()])
    sigma2, m, n_free = cvo.noise_scale(x, p["uvs"], p["obj"])
    pr = dict(uvs=p["uvs"], obj=p["obj"], extrinsics=p["true_cam"][:, 6:].copy(), intrinsics=cvo.make_case(2, 1)["intrinsics"], poses=p["true_poses"], kwargs={})
    u = run(pr, frame_covariance=False)
    print(f"F = 9720: sigma2 {u.sigma2:.17g} (oracle {sigma2:.17g}, {abs(u.sigma2 - sigma2) / sigma2:.3g} relative) m {u.n_residuals} p {u.n_free}")
    assert (u.n_residuals, u.n_free) == (m, n_free) == (2099520, 18 + 6 * 9720)
    assert abs(u.sigma2 - sigma2) <= 1e-12 * sigma2
    assert u.info["group"] == 0 and u.pose_covariance is None


def exactly_determined():
    """2 cameras, 1 frame, a 2 x 2 board of 100 mm pitch, one corner missing in each camera, intrinsics held: 12 present scalars, 12 free parameters
    (6 extrinsics + 6 of the pose).  cond_2 of the scaled H is 8e3 at this seed (the test below holds the oracle to that without a GPU)."""
    p = synth.make_problem(2, 1, rows=2, cols=2, pitch=100.0, seed=0)
    uvs = p["uvs"].copy()
    uvs[0, 0, 3] = np.nan
    uvs[1, 0, 0] = np.nan
    cam = p["true_cam"]
    intr = []
    for c in range(2):
        K = np.eye(3)
        K[0, 0], K[1, 1], K[0, 2], K[1, 2] = cam[c, :4]
        intr.append((K, np.array([cam[c, 4], cam[c, 5], 0.0, 0.0, 0.0])))
    return dict(uvs=uvs, obj=p["obj"], extrinsics=cam[:, 6:].copy(), intrinsics=intr, poses=p["true_poses"], x=np.concatenate([cam.ravel(), p["true_poses"].ravel()]),
                kwargs=dict(gauge_camera=0, loss="soft_l1", f_scale=1.0, fix_intrinsics=True, sigma=None))


def test_the_exactly_determined_problem_is_well_conditioned():
    """(no GPU) the oracle's H of `exactly_determined` is positive definite with m == p == 12 and cond_2 below 1e4"""
    pr = exactly_determined()
    o = cvo.covariance(pr["x"], pr["uvs"], pr["obj"], **dict(pr["kwargs"], sigma=0.2))
    print(f"m {o['n_residuals']} p {o['n_free']} cond {o['cond']:.3g}")
    assert o["n_residuals"] == o["n_free"] == 12 and o["cond"] < 1e4
    assert np.isnan(cvo.covariance(pr["x"], pr["uvs"], pr["obj"], **pr["kwargs"])["sigma2"])


@gpu
def test_as_many_scalars_as_free_parameters():
    """m == p: without sigma a RuntimeWarning, sigma2 NaN, the free entries NaN and the held ones 0; with sigma given the oracle's numbers"""
    pr = exactly_determined()
    with pytest.warns(RuntimeWarning, match="cannot be estimated"):
        u = run(pr)
    held = cvo.held_camera_params(2, 0, True)
    assert np.isnan(u.sigma2) and (u.n_residuals, u.n_free) == (12, 12)
    cam = u.camera_covariance
    assert np.isnan(cam[np.ix_(~held, ~held)]).all() and (cam[held] == 0.0).all() and (cam[:, held] == 0.0).all()
    assert np.isnan(u.pose_covariance).all() and u.info["n_degenerate_frames"] == 0
    o = cvo.covariance(pr["x"], pr["uvs"], pr["obj"], **dict(pr["kwargs"], sigma=0.2))
    g = run(pr, sigma=0.2)
    check_launch_shape(g, 12, "m == p")
    check_against(g, o, "m == p (2 cameras, 1 frame, 3 corners each)")
    check_exact(g, o, 2)


# ---------------------------------------------------------------- error paths on the device
@gpu
@pytest.mark.parametrize("fixed, gauge, blind", [(False, 0, 1), (False, 1, 1), (True, 0, 1)], ids=["12_wide", "12_wide_gauge", "6_wide"])
def test_a_camera_without_detections_names_its_first_pivot(fixed, gauge, blind):
    """C = 3, F = 8, every detection of camera `blind` NaN: U_c = 0 and W_cf = 0 exactly, so every free row of the camera fails the scaling and
    atomicMin leaves the lowest: 12 c (parameter 0), or 6 c (parameter 6: the first extrinsic) with the 6-wide block.  Not run: the 6-wide block with
    the blind camera as the gauge camera.  Every variable of that camera is held, so no row of it can fail, and holding a camera without data fixes
    no gauge: the system of the others is singular and its first failing pivot, if any, is decided by rounding."""
    pr = cvo.make_case(3, 8, gauge_camera=gauge, fix_intrinsics=fixed)
    uvs = pr["uvs"].copy()
    uvs[blind] = np.nan
    pivot, par = (6 * blind, 6) if fixed else (12 * blind, 0)
    with pytest.raises(ValueError, match=rf"not positive definite: pivot {pivot} \(camera {blind}, parameter {par}\)"):
        calibration_uncertainty(uvs, pr["extrinsics"], pr["intrinsics"], pr["obj"], pr["poses"], **pr["kwargs"])


@gpu
def test_the_handle_after_a_failed_pivot():
    """parameters that zero a camera's focal lengths make its k1 row of S0 exactly zero (d u / d k1 = fx x r^2): pivot 12 c + 4.  Good parameters on the
    same handle afterwards: linearize + reduce_fetch give the bits of a fresh handle, and a second covariance() the oracle's numbers (the device
    words of the verdict are reset per call)"""
    pr, o = cvo.case("c3_f30_missing_cauchy_gauge2")
    bad = pr["x"].copy()
    bad[12:14] = 0.0
    lam = 1e-3

    def reduced(prob):
        prob.linearize(0)
        return {k: v.copy() for k, v in prob.reduce_fetch(lam).items()}

    fresh = ops.Problem(pr["uvs"], pr["obj"], loss="cauchy")
    fresh.set_params(0, pr["x"])
    want = reduced(fresh)
    fresh.close()
    prob = ops.Problem(pr["uvs"], pr["obj"], loss="cauchy")
    try:
        prob.set_params(0, bad)
        with pytest.raises(ValueError, match=r"pivot 16 \(camera 1, parameter 4\)"):
            prob.covariance(0, 2)
        prob.set_params(0, pr["x"])
        got = reduced(prob)
        for k in want:
            assert np.array_equal(want[k], got[k]), k
        cam, fr, info = prob.covariance(0, 2)
    finally:
        prob.close()
    assert info[4] == -1 and info[6] == 8
    e_cam, e_fr = cvo.rel_err(cam, o["camera_covariance"]), cvo.rel_err(fr, o["pose_covariance"])
    print(f"after a failed pivot: bound {o['bound']:.3g} cameras {e_cam:.3g} frames {e_fr:.3g}")
    assert e_cam <= o["bound"] and e_fr <= o["bound"] and abs(info[0] - o["sigma2"]) <= 1e-12 * o["sigma2"]


@gpu
def test_fix_intrinsics_stops_at_26_cameras():
    """27 cameras: refused by name; 26 run (covariance_oracle's "c26_f8_fixed_gauge3", held to the oracle in tests/test_gpu_covariance.py)"""
    pr, _ = cvo.case("c27_f5_missing")
    with pytest.raises(ValueError, match="at most 26 cameras"):
        run(pr, fix_intrinsics=True)
    assert cvo.CASES["c26_f8_fixed_gauge3"]["C"] == 26 and cvo.CASES["c26_f8_fixed_gauge3"]["fix_intrinsics"]
