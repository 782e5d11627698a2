"""calibration_uncertainty on the GPU (csrc/mcba_cov.hip through mcba_covariance) against tests/covariance_oracle.py.

Metric, for the camera block and every frame block: max |Sigma_gpu - Sigma_ref| / sqrt(Sigma_ref,ii Sigma_ref,jj), and the same on the
standard deviations.  Bound: 64 cond_2(H_scaled) 2.2e-16 with cond_2 from the oracle -- the forward-error form for inverting a matrix whose
entries carry a few eps of summation error; two float64 host algorithms on the oracle's own H differ by 0.1 .. 2.4 cond eps at these shapes,
64 leaves the GPU's different summation order a factor of about 25.  Every case prints its figures before it asserts.

Every case also asserts the launch shape the call reports (info["group"], info["ld"]) against covariance_oracle.expected_group / expected_ld, and holds
the frame stage on its own -- the returned blocks against the long-double evaluation of sigma2 V_f^-1 + Y_f Sigma_cc Y_f^T at the camera covariance
the GPU itself returned -- to covariance_oracle.FRAME_BOUND_FACTOR cond_2(V_f) eps, orders below the end-to-end bound.  The edges of the launches
(frames without data at group edges, the two halves against the device's own input, the error paths) are in tests/test_gpu_covariance_edges.py."""
import os

import numpy as np
import pytest

import covariance_oracle as cvo
from multicam_calibration_amd import calibration_uncertainty, ops

gpu = pytest.mark.gpu


def run(pr, **over):
    kw = dict(pr["kwargs"])
    kw.update(over)
    return calibration_uncertainty(pr["uvs"], pr["extrinsics"], pr["intrinsics"], pr["obj"], pr["poses"], **kw)


def check_against(u, o, label, skip_frames=()):
    keep = np.array([f for f in range(o["pose_covariance"].shape[0]) if f not in skip_frames])
    e_cam = cvo.rel_err(u.camera_covariance, o["camera_covariance"])
    e_fr = cvo.rel_err(u.pose_covariance[keep], o["pose_covariance"][keep])
    e_std = max(cvo.rel_err_std(u.intrinsics_std, o["intrinsics_std"]), cvo.rel_err_std(u.extrinsics_std, o["extrinsics_std"]), cvo.rel_err_std(u.pose_std[keep], o["pose_std"][keep]))
    unit = o["cond"] * cvo.EPS
    print(f"{label}: cond {o['cond']:.3g} bound {o['bound']:.3g} cameras {e_cam:.3g} frames {e_fr:.3g} std {e_std:.3g}  (cond eps: {e_cam / unit:.2f} / {e_fr / unit:.2f} / {e_std / unit:.2f})")
    assert e_cam <= o["bound"] and e_fr <= o["bound"] and e_std <= o["bound"]


def check_launch_shape(u, n, label, force=0, frames=True):
    """the group and row stride the call says it launched against the LDS formula of the kernel's comment"""
    print(f"{label}: n {n} group {u.info['group']} (expected {cvo.expected_group(n, force) if frames else 0}) ld {u.info['ld']} (expected {cvo.expected_ld(n)})")
    assert u.info["group"] == (cvo.expected_group(n, force) if frames else 0) and u.info["ld"] == cvo.expected_ld(n)


def check_frame_stage(u, o, label):
    """the frame blocks against the long-double frame stage fed the camera covariance the GPU returned, in units of cond_2(V_f) eps"""
    ref, cond_v = cvo.frame_reference(o, u.camera_covariance, u.sigma2)
    e = cvo.frame_stage_error(u.pose_covariance, ref, cond_v)
    print(f"{label}: frame stage {e:.3g} cond(V_f) eps (bound {cvo.FRAME_BOUND_FACTOR:g}; cond(V_f) {np.nanmin(cond_v):.3g} .. {np.nanmax(cond_v):.3g}): {e * np.nanmax(cond_v) / (cvo.BOUND_FACTOR * o['cond']):.2g} of the end-to-end bound")
    assert e <= cvo.FRAME_BOUND_FACTOR


def system_size(pr):
    return (6 if pr["kwargs"]["fix_intrinsics"] else 12) * pr["uvs"].shape[0]


def check_exact(u, o, C):
    cam = u.camera_covariance
    d = np.sqrt(np.diagonal(cam))
    assert (np.abs(cam - cam.T) <= 1e-14 * np.outer(d, d)).all()
    assert (cam[o["held"]] == 0.0).all() and (cam[:, o["held"]] == 0.0).all()
    assert (u.intrinsics_std.ravel()[o["held"].reshape(C, 12)[:, :6].ravel()] == 0.0).all() and (u.extrinsics_std.ravel()[o["held"].reshape(C, 12)[:, 6:].ravel()] == 0.0).all()
    good = ~o["nodata"]
    pc = u.pose_covariance[good]
    assert np.array_equal(pc, pc.transpose(0, 2, 1))
    assert (np.linalg.eigvalsh(pc) > 0).all()
    corr = np.diagonal(u.camera_correlation)
    assert (corr[~o["held"]] == 1.0).all() and np.isnan(corr[o["held"]]).all()
    assert np.isnan(u.camera_correlation[o["held"]]).all()
    assert u.n_residuals == o["n_residuals"] and u.n_free == o["n_free"]
    assert abs(u.sigma2 - o["sigma2"]) <= 1e-12 * o["sigma2"]
    assert u.info["n_degenerate_frames"] == int(o["nodata"].sum()) and u.info["kernel_ms"] > 0


@gpu
@pytest.mark.parametrize("name", sorted(cvo.CASES))
def test_cases_match_the_oracle(name):
    pr, o = cvo.case(name)
    if name == "c3_f30_missing_cauchy_gauge2":
        assert pr["uvs"].shape[1] == 25   # the frames the filter keeps
    assert pr["uvs"].shape[1] == cvo.KEPT_FRAMES.get(name, pr["uvs"].shape[1])
    u = run(pr)
    check_launch_shape(u, system_size(pr), name)
    check_against(u, o, name)
    check_exact(u, o, pr["uvs"].shape[0])
    check_frame_stage(u, o, name)


@gpu
def test_four_frame_workgroups_match_the_oracle(monkeypatch):
    """k_cov_frames with 4 frames per workgroup -- the shape of rigs of 27 cameras and more, which "c27_f5_missing" and "c40_f9_missing_huber_fs07"
    reach unforced -- forced at C = 2, F = 130 and at n = 120 (MCBA_COV_FRAMES_G, read per call): the small-n end of that shape, one and two
    panels, and F = 3, 4, 5: one short of, at and one past a group of 4."""
    monkeypatch.setenv("MCBA_COV_FRAMES_G", "4")
    for name in ("c2_f130", "c10_f8", "c2_f3", "c2_f4", "c2_f5"):
        pr, o = cvo.case(name)
        u = run(pr)
        check_launch_shape(u, system_size(pr), name + " (G = 4)", force=4)
        assert u.info["group"] == 4
        check_against(u, o, name + " (G = 4)")
        check_exact(u, o, pr["uvs"].shape[0])
        check_frame_stage(u, o, name + " (G = 4)")


@gpu
def test_frame_covariance_can_be_left_out():
    pr, o = cvo.case("c2_f4")
    u = run(pr, frame_covariance=False)
    assert u.pose_covariance is None and u.pose_std is None
    check_launch_shape(u, 24, "c2_f4 without frame blocks", frames=False)
    assert cvo.rel_err(u.camera_covariance, o["camera_covariance"]) <= o["bound"]


@gpu
def test_degenerate_frame():
    """every detection of one frame NaN: its block is NaN, it is counted, everything else is the oracle of the other three frames"""
    pr, _ = cvo.case("c2_f4")
    uvs = pr["uvs"].copy()
    uvs[:, 2] = np.nan
    u = calibration_uncertainty(uvs, pr["extrinsics"], pr["intrinsics"], pr["obj"], pr["poses"], **pr["kwargs"])
    keep = [0, 1, 3]
    x3 = np.concatenate([pr["x"][:24], pr["poses"][keep].ravel()])
    o = cvo.covariance(x3, pr["uvs"][:, keep], pr["obj"], **pr["kwargs"])
    assert np.isnan(u.pose_covariance[2]).all() and np.isnan(u.pose_std[2]).all()
    assert u.info["n_degenerate_frames"] == 1
    assert u.n_residuals == o["n_residuals"] and u.n_free == o["n_free"] and abs(u.sigma2 - o["sigma2"]) <= 1e-12 * o["sigma2"]
    e_cam, e_fr = cvo.rel_err(u.camera_covariance, o["camera_covariance"]), cvo.rel_err(u.pose_covariance[keep], o["pose_covariance"])
    print(f"degenerate frame: bound {o['bound']:.3g} cameras {e_cam:.3g} frames {e_fr:.3g}")
    assert e_cam <= o["bound"] and e_fr <= o["bound"]
    assert cvo.rel_err_std(u.pose_std[keep], o["pose_std"]) <= o["bound"]


@gpu
def test_meaning_end_to_end():
    """after a converged linear-loss bundle adjustment of 0.2 px noise the estimated sigma2 is 0.04 within 10 % (seven standard errors of the
    estimate, 0.04 sqrt(2 / 10 476) = 1.4 %), and the standard deviations are the oracle's at the returned point"""
    import multicam_calibration_amd as mc
    from multicam_calibration_amd import synth

    p = synth.make_problem(2, 50)
    ext, intr, poses, use, res = mc.bundle_adjust(p["uvs"], p["extrinsics"], p["intrinsics"], p["obj"], p["poses"], loss="linear", ftol=1e-12, xtol=1e-12, gtol=1e-12, verbose=0)
    uvs = p["uvs"][:, use]
    u = calibration_uncertainty(uvs, ext, intr, p["obj"], poses, loss="linear")
    print(f"sigma2 {u.sigma2:.5f} (m {u.n_residuals}, p {u.n_free})")
    assert abs(u.sigma2 - 0.04) <= 0.1 * 0.04
    o = cvo.covariance(mc.serialize_params(ext, intr, poses), uvs, p["obj"], loss="linear")
    e = cvo.rel_err_std(u.intrinsics_std[1], o["intrinsics_std"][1])
    print(f"intrinsics_std of camera 1: {u.intrinsics_std[1]}  rel. error {e:.3g}  bound {o['bound']:.3g}")
    assert e <= o["bound"]


def test_refusals_before_any_device():
    pr, _ = cvo.case("c2_f4")
    args = (pr["uvs"], pr["extrinsics"], pr["intrinsics"], pr["obj"], pr["poses"])
    with pytest.raises(ValueError, match="named losses only"):
        calibration_uncertainty(*args, loss=lambda z: np.stack([z, np.ones_like(z), np.zeros_like(z)]))
    with pytest.raises(ValueError, match="sparse-Schur handle"):
        calibration_uncertainty(np.zeros((41, 3, 4, 2)), np.zeros((41, 6)), [(np.eye(3), np.zeros(5))] * 41, np.zeros((4, 3)), np.zeros((3, 6)))
    with pytest.raises(ValueError, match="gauge_camera"):
        calibration_uncertainty(*args, gauge_camera=2)


@gpu
def test_sparse_handle_is_refused():
    pr, _ = cvo.case("c2_f4")
    prob = ops.Problem(pr["uvs"], pr["obj"], schur="sparse")
    prob.set_params(0, pr["x"])
    with pytest.raises(ops.McbaError) as ei:
        prob.covariance(0, 0)
    assert ei.value.code == ops.ERR_ARG and "sparse-Schur" in str(ei.value)
    prob.close()


@gpu
def test_handle_is_untouched():
    """reduce_fetch at the same x and lambda before and after a covariance() call (re-linearised in between, with the Triggs floor the caller had
    set) gives the same bits, and the curvature floor is the caller's"""
    pr, _ = cvo.case("c3_f30_missing_cauchy_gauge2")
    prob = ops.Problem(pr["uvs"], pr["obj"], loss="cauchy")
    prob.set_params(0, pr["x"] * (1 + 1e-4))
    prob.set_curvature_floor(0.1)
    lam = 1e-3
    prob.linearize(0)
    before = {k: v.copy() for k, v in prob.reduce_fetch(lam).items()}
    prob.covariance(0, 2)
    assert prob.lib.mcba_get_curvature_floor(prob.handle) == 0.1
    with pytest.raises(ops.McbaError):
        prob.reduce_fetch(lam)   # the linearisation is gone: the handle says so instead of reducing the covariance's
    prob.linearize(0)
    after = prob.reduce_fetch(lam)
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    prob.close()
