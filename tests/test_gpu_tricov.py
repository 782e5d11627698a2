"""triangulation_uncertainty on the GPU (csrc/mcba_tricov.hip through mcba_triangulation_covariance) against tests/tricov_oracle.py, at the smallest
shapes at which the kernels can go wrong: one point; n = 36 (no multiple of 16 or 32), n = 72 (a full 64-column panel and a partial one), n = 144,
n = 288; one lane and one point past a wavefront and past a 16-point group; the smaller groups forced -- and reached unforced at 30, 48, 49 and 64
cameras (tricov_oracle.WIDE_CASES: n = 768 = ld, twelve panels of diag_blocks), every case asserting the group the call reports.

Metric and bound are the oracle's (its docstring derives both factors): detection term max |got - ref|_ij / sqrt(ref_ii ref_jj) <= k cond_2(H_s) eps,
calibration term |got - ref|_ij <= k cond_2(H_s) eps sqrt(T_ii T_jj), k = 64, or 2000 for the two cases of the "outlier" scene.  Every case prints its
figures before it asserts."""
import numpy as np
import pytest

import keypoint_scenes as ks
import tricov_oracle as tco
import multicam_calibration_amd as m
from multicam_calibration_amd import triangulation_uncertainty

gpu = pytest.mark.gpu


def as_dict(u):
    return dict(detection=u.detection_covariance, calibration=u.calibration_covariance, views=u.n_views, status=u.status, sigma2=u.sigma2, n_residuals=u.n_residuals, n_free=u.n_free,
                n_unusable=u.info["n_unusable"], n_degenerate=u.info["n_degenerate"])


def run(i, with_cov=True, sigma=tco.SIGMA, **over):
    kw = dict(camera_covariance=i["camera_covariance"] if with_cov else None, sigma=sigma, loss=i["loss"], f_scale=i["f_scale"])
    kw.update(over)
    return triangulation_uncertainty(i["points"], i["uvs"], i["ext"], i["intr"], **kw)


def check_exact(u, o):
    ok = o["status"] == 1
    for blocks in (u.covariance, u.detection_covariance, u.calibration_covariance):
        if blocks is not None:
            assert np.array_equal(blocks, blocks.transpose(0, 2, 1), equal_nan=True)
            assert np.isnan(blocks[~ok]).all() and np.isfinite(blocks[ok]).all()
    assert (np.linalg.eigvalsh(u.detection_covariance[ok]) > 0).all()
    assert np.array_equal(u.std[ok], np.sqrt(np.diagonal(u.covariance[ok], axis1=1, axis2=2))) and np.isnan(u.std[~ok]).all()
    if u.calibration_covariance is not None:
        assert np.array_equal(u.covariance[ok], u.detection_covariance[ok] + u.calibration_covariance[ok])
    assert u.info["kernel_ms"] > 0 and set(np.unique(u.status)) <= set(m.uncertainty.POINT_STATUS)


@gpu
@pytest.mark.parametrize("name", sorted(tco.CASES))
def test_cases_match_the_oracle(name):
    """every case with its dense random positive semi-definite camera covariance and without one"""
    i, o = tco.case(name)
    C = len(i["ext"])
    u = run(i)
    print(f"{name}: {C} cameras, group {u.info['group']} (expected {tco.expected_group(C)}), ld {u.info['ld']}")
    assert u.info["group"] == tco.expected_group(C) and u.info["ld"] == (12 * C + 63) // 64 * 64
    tco.check_against_oracle(name, as_dict(u), o)
    check_exact(u, o)
    alone = run(i, with_cov=False)
    assert alone.info["group"] == 0 and alone.info["ld"] == u.info["ld"]
    tco.check_against_oracle(name + " (no camera covariance)", as_dict(alone), o, with_cov=False)
    check_exact(alone, o)
    assert alone.calibration_covariance is None and np.array_equal(alone.covariance, alone.detection_covariance, equal_nan=True)
    assert np.array_equal(alone.detection_covariance, u.detection_covariance, equal_nan=True)   # k_tricov_scale and k_tricov_cal write the same bits


@gpu
@pytest.mark.parametrize("name", tco.POOLED_CASES)
def test_pooled_sigma_matches_the_oracle(name):
    """sigma=None: sigma2, n_residuals and n_free of the oracle, sigma2 to 1e-12 relative; the blocks are the given-sigma ones rescaled"""
    i, o = tco.case(name)
    tco.check_pooled(name, as_dict(run(i, sigma=None)), as_dict(run(i)), o)
    tco.check_pooled(name + " (no camera covariance)", as_dict(run(i, with_cov=False, sigma=None)), as_dict(run(i, with_cov=False)), o)


@gpu
@pytest.mark.parametrize("group", ["5", "10"])
def test_smaller_groups_match_the_oracle(monkeypatch, group):
    """k_tricov_cal with 10 and 5 points per workgroup -- the shapes of rigs beyond 29 and beyond 48 cameras -- forced at C = 3 and C = 12
    (MCBA_TRICOV_G, read per call).  The bound is the same."""
    monkeypatch.setenv("MCBA_TRICOV_G", group)
    for name in ("three", "twelve", "c3_p17"):
        i, o = tco.case(name)
        u = run(i)
        assert u.info["group"] == int(group) == tco.expected_group(len(i["ext"]), force=int(group))
        tco.check_against_oracle(f"{name} (G = {group})", as_dict(u), o)
        check_exact(u, o)


@gpu
def test_zero_camera_covariance_gives_exact_zeros():
    i, o = tco.case("six")
    ok = o["status"] == 1
    u = run(i, camera_covariance=np.zeros((72, 72)))
    assert (u.calibration_covariance[ok] == 0.0).all() and np.isnan(u.calibration_covariance[~ok]).all()
    assert np.array_equal(u.covariance[ok], u.detection_covariance[ok])


@gpu
def test_one_camera_block_leaves_unseeing_points_at_exact_zero():
    """a camera covariance that is non-zero in the block of camera 1 alone: exact zeros for the points camera 1 does not see, the oracle's
    numbers for the others"""
    i, o = tco.case("three")
    S = np.zeros((36, 36))
    S[12:24, 12:24] = i["camera_covariance"][12:24, 12:24]
    u = run(i, camera_covariance=S)
    ref = tco.uncertainty(i["points"], i["uvs"], i["ext"], i["intr"], camera_covariance=S, sigma=tco.SIGMA)
    tco.check_against_oracle("three, camera 1's block alone", as_dict(u), ref)
    ok = ref["status"] == 1
    unseen = np.isnan(i["uvs"][1]).any(-1) & ok
    assert unseen.sum() > 10 and (u.calibration_covariance[unseen] == 0.0).all()
    assert (np.abs(u.calibration_covariance[ok & ~unseen]).max(axis=(1, 2)) > 0).all()


@gpu
def test_inliers_mask_is_the_same_as_nans_by_hand():
    i, o = tco.case("six")
    rng = np.random.default_rng(3)
    mask = rng.uniform(size=(6, 300)) > 0.2
    by_hand = [np.where(mask[c][:, None], i["uvs"][c], np.nan) for c in range(6)]
    a = run(i, inliers=mask, sigma=None)
    b = triangulation_uncertainty(i["points"], by_hand, i["ext"], i["intr"], camera_covariance=i["camera_covariance"], loss=i["loss"], f_scale=i["f_scale"])
    for name in ("covariance", "detection_covariance", "calibration_covariance", "std", "n_views", "status"):
        assert np.array_equal(getattr(a, name), getattr(b, name), equal_nan=True), name
    assert (a.sigma2, a.n_residuals, a.n_free) == (b.sigma2, b.n_residuals, b.n_free)
    assert np.array_equal(a.n_views, (mask & ~np.isnan(np.stack(i["uvs"])).any(-1)).sum(0))
    ref = tco.uncertainty(i["points"], by_hand, i["ext"], i["intr"], camera_covariance=i["camera_covariance"], sigma=tco.SIGMA)
    tco.check_against_oracle("six, masked", as_dict(run(i, inliers=mask)), ref)


@gpu
def test_no_usable_point_gives_a_nan_sigma_and_a_warning():
    """m <= 3 P_u happens only at P_u = 0 (a usable point brings four scalars or more for its three coordinates): every point seen by one camera"""
    i, _ = tco.case("c3_p17")
    uvs = [i["uvs"][0], np.full_like(i["uvs"][1], np.nan), np.full_like(i["uvs"][2], np.nan)]
    with pytest.warns(RuntimeWarning, match="cannot be estimated"):
        u = triangulation_uncertainty(i["points"], uvs, i["ext"], i["intr"], camera_covariance=i["camera_covariance"])
    assert np.isnan(u.sigma2) and (u.n_residuals, u.n_free) == (0, 0) and (u.status == -1).all() and u.info["n_unusable"] == 17
    assert np.isnan(u.covariance).all() and np.isnan(u.calibration_covariance).all()


@gpu
def test_calibration_uncertainty_object_is_accepted():
    i, o = tco.case("c2_p1")
    unc = m.CalibrationUncertainty(camera_covariance=i["camera_covariance"], intrinsics_std=None, extrinsics_std=None, camera_correlation=None, pose_covariance=None, pose_std=None, sigma2=1.0,
                                   n_residuals=0, n_free=0, info={})
    a, b = run(i, camera_covariance=unc), run(i)
    assert np.array_equal(a.covariance, b.covariance)


@gpu
def test_degenerate_points():
    """camera 1 a copy of camera 0, points seen by those two alone: status -2, NaN blocks, counted; the other points unchanged, bit for bit"""
    i, _ = tco.case("three")
    uvs = [u.copy() for u in i["uvs"]]
    ext, intr = i["ext"].copy(), list(i["intr"])
    ext[1], intr[1] = ext[0], intr[0]
    uvs[1] = uvs[0] + 0.1
    S = i["camera_covariance"]
    ref = tco.uncertainty(i["points"], uvs, ext, intr, camera_covariance=S, sigma=tco.SIGMA)
    two_alone = ~np.isnan(uvs[0]).any(-1) & np.isnan(uvs[2]).any(-1)
    assert two_alone.sum() > 10 and (ref["status"][two_alone] == -2).all()
    u = triangulation_uncertainty(i["points"], uvs, ext, intr, camera_covariance=S, sigma=tco.SIGMA)
    tco.check_against_oracle("three, camera 1 = camera 0", as_dict(u), ref)
    assert (u.status[two_alone] == -2).all() and np.isnan(u.covariance[two_alone]).all() and u.info["n_degenerate"] == ref["n_degenerate"] == int((u.status == -2).sum())
    assert u.info["n_unusable"] == int((u.status == -1).sum())
    pooled = triangulation_uncertainty(i["points"], uvs, ext, intr, camera_covariance=S)
    pref = tco.uncertainty(i["points"], uvs, ext, intr)
    print(f"pooled sigma2 {pooled.sigma2:.17g} (oracle {pref['sigma2']:.17g}), m {pooled.n_residuals}, free {pooled.n_free}")
    assert (pooled.n_residuals, pooled.n_free) == (pref["n_residuals"], pref["n_free"]) and abs(pooled.sigma2 - pref["sigma2"]) <= 1e-12 * pref["sigma2"]
    keep = u.status != -2
    sub = triangulation_uncertainty(i["points"][keep], [x[keep] for x in uvs], ext, intr, camera_covariance=S, sigma=tco.SIGMA)
    assert np.array_equal(sub.covariance, u.covariance[keep], equal_nan=True) and np.array_equal(sub.detection_covariance, u.detection_covariance[keep], equal_nan=True)


@gpu
def test_predicted_covariance_is_the_scatter_of_refined_points():
    """One true point 4096 times, 6 cameras, independent N(0, 0.3^2) px detection noise: the sample covariance of the refined points matches the
    mean predicted detection_covariance within 10 % on the diagonal (the standard error of a variance from 4096 samples is sqrt(2 / 4096) = 2.2 %:
    10 % is 4.5 of them), and the pooled estimate gives 0.09 within 10 %."""
    uvs, ext, intr, X = ks.make("six")
    P = 4096
    rng = np.random.default_rng(77)
    exact = [ks.project5(X[:1], ext[c], *intr[c]) for c in range(6)]
    det = [np.repeat(e, P, axis=0) + rng.normal(0, 0.3, (P, 2)) for e in exact]
    start = np.repeat(X[:1], P, axis=0)
    refined = m.refine_triangulation(start, det, ext, intr, loss="linear")
    u = triangulation_uncertainty(refined, det, ext, intr, sigma=0.3)
    assert (u.status == 1).all()
    sample = np.cov(refined.T)
    predicted = u.detection_covariance.mean(axis=0)
    ratio = np.diagonal(sample) / np.diagonal(predicted)
    pooled = triangulation_uncertainty(refined, det, ext, intr)
    print(f"sample variances {np.diagonal(sample)}, predicted {np.diagonal(predicted)}, ratio {ratio}; pooled sigma2 {pooled.sigma2:.5f} (m {pooled.n_residuals}, free {pooled.n_free})")
    assert (np.abs(ratio - 1) <= 0.10).all()
    assert abs(pooled.sigma2 - 0.09) <= 0.10 * 0.09
    assert (pooled.n_residuals, pooled.n_free) == (12 * P, 3 * P)


@gpu
def test_bundle_adjust_to_point_uncertainty():
    """bundle_adjust -> calibration_uncertainty -> triangulation_uncertainty(camera_covariance=unc) on the board corners of three frames: the
    oracle fed the same Sigma_cc within the bound, and a calibration term that is not zero"""
    p = m.synth.make_problem(2, 50)
    ext, intr, poses, use, res = m.bundle_adjust(p["uvs"], p["extrinsics"], p["intrinsics"], p["obj"], p["poses"], loss="linear", ftol=1e-12, xtol=1e-12, gtol=1e-12, verbose=0)
    uvs = p["uvs"][:, use]
    unc = m.calibration_uncertainty(uvs, ext, intr, p["obj"], poses, loss="linear")
    frames = [0, 7, 19]
    pts = np.concatenate([p["obj"] @ ks.rodrigues(poses[f][:3]).T + poses[f][3:] for f in frames])
    det = [np.concatenate([uvs[c, f] for f in frames]) for c in range(2)]
    sigma = float(np.sqrt(unc.sigma2))
    u = triangulation_uncertainty(pts, det, ext, intr, camera_covariance=unc, sigma=sigma)
    ref = tco.uncertainty(pts, det, ext, intr, camera_covariance=unc.camera_covariance, sigma=sigma)
    tco.check_against_oracle("bundle_adjust(2, 50), three boards", as_dict(u), ref)
    ok = ref["status"] == 1
    print(f"std (detection) {np.sqrt(np.diagonal(u.detection_covariance[ok], axis1=1, axis2=2)).mean(0)}, std (calibration) {np.sqrt(np.diagonal(u.calibration_covariance[ok], axis1=1, axis2=2)).mean(0)}")
    assert ok.sum() > 100 and (np.diagonal(u.calibration_covariance[ok], axis1=1, axis2=2) > 0).all()


@gpu
def test_calibration_to_point_uncertainty_at_27_cameras():
    """calibration_uncertainty (k_cov_frames in its four-frame shape) -> triangulation_uncertainty(camera_covariance=unc) at 27 cameras on the board
    corners of two frames: the oracle fed the same Sigma_cc within the bound, both calls reporting their natural groups, a calibration term that is
    not zero.  The camera covariance of a real calibration: strongly correlated, the gauge camera's rows zero."""
    import covariance_oracle as cvo

    pr, _ = cvo.case("c27_f5_missing")
    unc = m.calibration_uncertainty(pr["uvs"], pr["extrinsics"], pr["intrinsics"], pr["obj"], pr["poses"], **pr["kwargs"])
    assert unc.info["group"] == 4 == cvo.expected_group(324)
    frames = [1, 4]
    pts = np.concatenate([pr["obj"] @ ks.rodrigues(pr["poses"][f][:3]).T + pr["poses"][f][3:] for f in frames])
    det = [np.concatenate([pr["uvs"][c, f] for f in frames]) for c in range(27)]
    sigma = float(np.sqrt(unc.sigma2))
    u = triangulation_uncertainty(pts, det, pr["extrinsics"], pr["intrinsics"], camera_covariance=unc, sigma=sigma)
    ref = tco.uncertainty(pts, det, pr["extrinsics"], pr["intrinsics"], camera_covariance=unc.camera_covariance, sigma=sigma)
    assert u.info["group"] == 16 == tco.expected_group(27) and u.info["ld"] == 384
    tco.check_against_oracle("calibration_uncertainty(27, 5), two boards", as_dict(u), ref)
    check_exact(u, ref)
    ok = ref["status"] == 1
    assert ok.sum() == 108 and (np.diagonal(u.calibration_covariance[ok], axis1=1, axis2=2) > 0).all()
