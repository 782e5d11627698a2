"""triangulation_uncertainty without a GPU: the oracle's own credentials (tests/tricov_oracle.py) and the argument refusals of the public function,
which come before any device is touched."""
import numpy as np
import pytest
from scipy.optimize import least_squares

import multicam_calibration_amd as m
import keypoint_scenes as ks
import tricov_oracle as tco


def retriangulate(X0, det, theta, d5):
    """scipy's minimiser of one point's plain least-squares reprojection cost in the cameras that see it"""
    cams = [c for c in range(len(theta)) if not np.isnan(det[c]).any()]

    def res(X):
        out = []
        for c in cams:
            th = theta[c]
            K = np.array([[th[0], 0, th[2]], [0, th[1], th[3]], [0, 0, 1.0]])
            out.append(det[c] - ks.project5(X, th[6:], K, np.r_[th[4], th[5], d5[c][2:]]))
        return np.concatenate(out)

    return least_squares(res, X0, method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15).x


def test_oracle_G_is_the_derivative_of_the_retriangulated_point():
    """-G = dX/dtheta: central differences of scipy's re-triangulated point with respect to all 36 camera parameters of scene "three" at
    residual-free detections (linear loss)"""
    i, o = tco.case("three_exact")
    theta, d5 = tco.camera_blocks(i["ext"], i["intr"])
    det = np.stack(i["uvs"])
    usable = np.flatnonzero(o["status"] == 1)
    worst = 0.0
    for p in usable[:: max(1, len(usable) // 8)][:8]:
        fd = np.empty((3, 36))
        for j in range(36):
            h = 1e-5 * max(1.0, abs(theta.ravel()[j]))
            tp, tm = theta.copy().ravel(), theta.copy().ravel()
            tp[j] += h
            tm[j] -= h
            fd[:, j] = (retriangulate(i["points"][p], det[:, p], tp.reshape(-1, 12), d5) - retriangulate(i["points"][p], det[:, p], tm.reshape(-1, 12), d5)) / (2 * h)
        err = np.abs(-o["G"][p] - fd).max() / np.abs(o["G"][p]).max()
        worst = max(worst, err)
    print(f"-G against central differences of scipy's re-triangulation: {worst:.3g} relative")
    assert worst <= 1e-5


def test_oracle_camera_rows_against_central_differences():
    rng = np.random.default_rng(8)
    d5 = np.array([-0.1, 0.02, 1e-3, -7e-4, 0.02])
    for rvec in (np.zeros(3), np.array([0.2, 0.4, -0.3])):
        theta = np.r_[880.0, 870.0, 600.0, 520.0, d5[0], d5[1], rvec, -40.0, 15.0, 60.0]
        X = rng.normal(0, 60, (4, 3)) + np.r_[0, 0, 800.0]

        def proj(th):
            K = np.array([[th[0], 0, th[2]], [0, th[1], th[3]], [0, 0, 1.0]])
            return ks.project5(X, th[6:], K, np.r_[th[4], th[5], d5[2:]])

        uv, A, B = tco.camera_rows(X, theta, d5)
        assert np.abs(uv - proj(theta)).max() < 1e-9
        for k in range(12):
            step = 1e-6 * max(1.0, abs(theta[k]))
            h = step * np.eye(12)[k]
            fd = (proj(theta + h) - proj(theta - h)) / (2 * step)
            assert np.abs(B[:, :, k] - fd).max() <= 1e-6 * max(np.abs(fd).max(), 1e-300), k


@pytest.mark.parametrize("name", sorted(tco.CASES))
def test_two_host_formulations_agree_within_the_bound(name):
    """the spread between the oracle's two float64 formulations, in units of 64 cond eps (recorded in the oracle's docstring, where the robust
    cases' bound factor is derived from it): inside the linear bound on the linear cases, near what was recorded on the robust ones"""
    i, o = tco.case(name)
    det, cal = tco.formulation_spread(name)
    ok = o["status"] == 1
    print(f"{name} ({i['loss']}): usable {ok.sum()} / {len(ok)}, cond {np.nanmin(o['cond']):.3g} .. {np.nanmax(o['cond']):.3g}, spread detection {det:.3g} calibration {cal:.3g} x 64 cond eps")
    robust = name in tco.ROBUST_CASES
    assert robust == name.startswith("outlier") or name in tco.WIDE_CASES
    limit = 2 * tco.HOST_SPREAD if robust else 1.0
    assert np.array_equal(o["bound"][ok], (tco.ROBUST_BOUND_FACTOR if robust else tco.BOUND_FACTOR) * o["cond"][ok] * tco.EPS)
    assert det <= limit and cal <= limit
    assert tco.ROBUST_BOUND_FACTOR == 25 * tco.HOST_SPREAD * tco.BOUND_FACTOR == 2000
    assert np.array_equal(o["detection"], o["detection"].transpose(0, 2, 1), equal_nan=True)


def test_expected_group_switches_where_the_lds_formula_says():
    """k_tricov_cal takes 16 points per workgroup up to 29 cameras, 10 up to 48 and 5 up to the cap of 64; a forced group wins where it fits"""
    assert tco.LDS_LIMIT == 163840 and tco.cal_lds(768, 5) <= tco.LDS_LIMIT < tco.cal_lds(768, 10)
    for C in range(2, 65):
        assert tco.expected_group(C) == (16 if C <= 29 else 10 if C <= 48 else 5), C
    assert tco.expected_group(3, force=5) == 5 and tco.expected_group(12, force=10) == 10 and tco.expected_group(64, force=16) == 5 and tco.expected_group(3, force=8) == 16


def test_argument_refusals_come_before_the_device():
    i, _ = tco.case("three")
    pts, uvs, ext, intr = i["points"], i["uvs"], i["ext"], i["intr"]
    S = i["camera_covariance"]
    with pytest.raises(ValueError, match="named losses"):
        m.triangulation_uncertainty(pts, uvs, ext, intr, loss=lambda z: z)
    with pytest.raises(ValueError, match="loss must be one of"):
        m.triangulation_uncertainty(pts, uvs, ext, intr, loss="tukey")
    with pytest.raises(NotImplementedError, match="2 to 64"):
        m.triangulation_uncertainty(pts, uvs[:1], ext[:1], intr[:1])
    with pytest.raises(NotImplementedError, match="2 to 64"):
        m.triangulation_uncertainty(pts, [uvs[0]] * 65, np.repeat(ext[:1], 65, axis=0), [intr[0]] * 65)
    bad = S.copy()
    bad[3, 17] += 1e-6
    with pytest.raises(ValueError, match="symmetric"):
        m.triangulation_uncertainty(pts, uvs, ext, intr, camera_covariance=bad)
    with pytest.raises(ValueError, match=r"\(36, 36\)"):
        m.triangulation_uncertainty(pts, uvs, ext, intr, camera_covariance=S[:24, :24])
    nonfinite = S.copy()
    nonfinite[0, 0] = np.inf
    with pytest.raises(ValueError, match="finite"):
        m.triangulation_uncertainty(pts, uvs, ext, intr, camera_covariance=nonfinite)
    with pytest.raises(ValueError, match="inliers"):
        m.triangulation_uncertainty(pts, uvs, ext, intr, inliers=np.ones((len(pts), 3), bool))
    with pytest.raises(ValueError, match="points must be"):
        m.triangulation_uncertainty(pts[:-1], uvs, ext, intr)
    assert m.uncertainty.POINT_STATUS == {1: "ok", -1: "too few views", -2: "degenerate"}


def test_without_a_gpu_the_call_raises():
    """no host path: ops.McbaError where no device is visible (where one is, nothing is launched from this tier)"""
    import ctypes

    n = ctypes.c_int()
    if m.ops.load_library().mcba_device_count(ctypes.byref(n)) == 0 and n.value > 0:
        return
    i, _ = tco.case("c2_p1")
    with pytest.raises(m.ops.McbaError):
        m.triangulation_uncertainty(i["points"], i["uvs"], i["ext"], i["intr"], camera_covariance=i["camera_covariance"])
