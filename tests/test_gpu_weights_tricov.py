"""triangulation_uncertainty(weights=) on the GPU -- the weighted instantiations of k_tricov_point and k_tricov_cal through
mcba_triangulation_covariance_weighted -- against tests/weights_oracle.py (the virtual rig, T Sigma T^T for the camera covariance; the direct
statement for weights off the levels), within tricov_oracle.check_against_oracle and check_pooled as the unweighted tests use them.  2, 3, 6 and 16
cameras (48 virtual ones), 17 and 33 points: one side of k_tricov_cal's 16-point groups each; with and without a camera covariance; the smaller
groups forced; inliers= times weights= is the product plane."""
import numpy as np
import pytest

import multicam_calibration_amd as m
import tricov_oracle as tco
import weights_oracle as wo
from multicam_calibration_amd import triangulation_uncertainty

gpu = pytest.mark.gpu


def as_dict(u):
    return dict(detection=u.detection_covariance, calibration=u.calibration_covariance, views=u.n_views, status=u.status, sigma2=u.sigma2, n_residuals=u.n_residuals, n_free=u.n_free,
                n_unusable=u.info["n_unusable"], n_degenerate=u.info["n_degenerate"])


def run(i, with_cov=True, sigma=tco.SIGMA, **over):
    kw = dict(camera_covariance=i["camera_covariance"] if with_cov else None, sigma=sigma, loss=i["loss"], f_scale=i["f_scale"], weights=i["weights"])
    kw.update(over)
    return triangulation_uncertainty(i["points"], i["uvs"], i["ext"], i["intr"], **kw)


@gpu
@pytest.mark.parametrize("name", list(wo.TRICOV_CASES))
def test_cases_match_the_oracle(name):
    i, o = wo.tricov_case(name)
    assert (o["status"] == 1).mean() >= 0.5
    u = run(i)
    tco.check_against_oracle(name, as_dict(u), o)
    alone = run(i, with_cov=False)
    tco.check_against_oracle(name + " (no camera covariance)", as_dict(alone), o, with_cov=False)
    assert alone.calibration_covariance is None and np.array_equal(alone.detection_covariance, u.detection_covariance, equal_nan=True)
    again = run(i)
    assert np.array_equal(again.covariance, u.covariance, equal_nan=True) and again.sigma2 == u.sigma2   # the same bits


@gpu
def test_wide_rig_takes_the_one_tile_weighted_kernel_unforced():
    """49 cameras (tricov_oracle's "c49_p11", arctan): the weighted instantiation of k_tricov_cal at one row tile, five points per workgroup because
    nothing larger fits -- not forced; against the oracle of the 147 virtual cameras, T Sigma T^T for the camera covariance"""
    i, _ = tco.case("c49_p11")
    w = wo.draw_levels(49, 11, 9049)
    assert wo.usable_fraction(i["uvs"], w) == 1.0
    o = wo.uncertainty_virtual(i["points"], i["uvs"], i["ext"], i["intr"], w, camera_covariance=i["camera_covariance"], sigma=tco.SIGMA, loss=i["loss"], f_scale=i["f_scale"])
    u = run(dict(i, weights=w))
    print(f"c49_p11, weighted: group {u.info['group']}, ld {u.info['ld']}")
    assert u.info["group"] == 5 == tco.expected_group(49) and u.info["ld"] == 640
    tco.check_against_oracle("c49_p11, weighted", as_dict(u), o)


@gpu
@pytest.mark.parametrize("name", wo.POOLED_CASES)
def test_pooled_sigma_matches_the_oracle(name):
    i, o = wo.tricov_case(name)
    tco.check_pooled(name, as_dict(run(i, sigma=None)), as_dict(run(i)), o)
    tco.check_pooled(name + " (no camera covariance)", as_dict(run(i, with_cov=False, sigma=None)), as_dict(run(i, with_cov=False)), o)


@gpu
@pytest.mark.parametrize("group", ["5", "10"])
def test_smaller_groups_match_the_oracle(monkeypatch, group):
    monkeypatch.setenv("MCBA_TRICOV_G", group)
    for name in ("c6_p33", "c3_p33", "c2_p17"):
        i, o = wo.tricov_case(name)
        tco.check_against_oracle(f"{name} (G = {group})", as_dict(run(i)), o)


@gpu
def test_inliers_times_weights_is_the_product_plane():
    i, o = wo.tricov_case("c6_p33")
    mask = np.random.default_rng(3).uniform(size=i["weights"].shape) > 0.2
    a = run(i, inliers=mask, sigma=None)
    b = run(i, weights=i["weights"] * mask, sigma=None)
    for k, v in as_dict(a).items():
        assert np.array_equal(v, as_dict(b)[k], equal_nan=True), k
    ref = wo.uncertainty_virtual(i["points"], i["uvs"], i["ext"], i["intr"], i["weights"] * mask, camera_covariance=i["camera_covariance"], sigma=tco.SIGMA, loss=i["loss"], f_scale=i["f_scale"])
    tco.check_against_oracle("c6_p33, masked", as_dict(run(i, inliers=mask)), ref)


@gpu
def test_identities():
    """all-ones weights are the unweighted call and a 0/1 plane the same mask written as NaN, bit for bit (a multiplication by 1.0 is exact); a
    constant plane w0 under the linear loss with sigma given is held to the oracle for it: H times w0, so the detection term over w0 and the
    calibration term unchanged"""
    i, o = wo.tricov_case("c16_p33")
    plain = run(i, weights=None, sigma=None)
    ones = run(i, weights=np.ones_like(i["weights"]), sigma=None)
    for k, v in as_dict(plain).items():
        assert np.array_equal(v, as_dict(ones)[k], equal_nan=True), k
    mask = i["weights"] > 0
    a, b = run(i, weights=mask.astype(np.float64), sigma=None), triangulation_uncertainty(i["points"], wo.masked(i["uvs"], mask), i["ext"], i["intr"], camera_covariance=i["camera_covariance"], loss=i["loss"])
    for k, v in as_dict(a).items():
        assert np.array_equal(v, as_dict(b)[k], equal_nan=True), k
    o4 = wo.uncertainty_virtual(i["points"], i["uvs"], i["ext"], i["intr"], 4.0 * mask, camera_covariance=i["camera_covariance"], sigma=tco.SIGMA, loss=i["loss"], f_scale=i["f_scale"])
    o1 = wo.uncertainty_virtual(i["points"], i["uvs"], i["ext"], i["intr"], 1.0 * mask, camera_covariance=i["camera_covariance"], sigma=tco.SIGMA, loss=i["loss"], f_scale=i["f_scale"])
    ok = o1["status"] == 1
    assert np.abs(4 * o4["detection"][ok] / o1["detection"][ok] - 1).max() <= 1e-12 and np.abs(o4["calibration"][ok] - o1["calibration"][ok]).max() <= 1e-12 * np.abs(o1["calibration"][ok]).max()
    tco.check_against_oracle("c16_p33, weights 4", as_dict(run(i, weights=4.0 * mask)), o4)


@gpu
def test_true_inverse_variances_give_sigma2_of_about_one():
    """detections with noise sigma_cp and weights 1 / sigma_cp^2: the pooled sigma2 is 1 within its sampling error (4 standard deviations of a
    chi-square over m - 3 P_u degrees of freedom)"""
    from test_triangulate_cpu import scene
    uvs, ext, intr, X = scene(C=6, P=400, seed=5, noise=0.0, p_unseen=0.1)
    rng = np.random.default_rng(6)
    sig = rng.choice([0.2, 0.5, 1.5], size=(6, 400))
    uvs = [u + rng.normal(size=u.shape) * sig[c][:, None] for c, u in enumerate(uvs)]
    w = 1 / sig ** 2
    pts = m.refine_triangulation(X, uvs, ext, intr, loss="linear", weights=w)
    u = triangulation_uncertainty(pts, uvs, ext, intr, weights=w)
    dof = u.n_residuals - u.n_free
    print(f"sigma2 {u.sigma2:.4f} over {dof} degrees of freedom")
    assert abs(u.sigma2 - 1) <= 4 * np.sqrt(2 / dof)
