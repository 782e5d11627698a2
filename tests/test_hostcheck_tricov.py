"""csrc/mcba_tricov_math.h -- the per-lane text of the triangulation-uncertainty kernels (csrc/mcba_tricov.hip) -- compiled with g++
(tests/hostcheck/tricov_hostcheck.cpp, plain -O2) and held, without a GPU, to the bound of the GPU tier (tests/test_gpu_tricov.py) against
tests/tricov_oracle.py on every case: detection term max |got - ref|_ij / sqrt(ref_ii ref_jj) <= k cond_2(H_scaled) 2.2e-16, calibration term
|got - ref|_ij <= k cond_2(H_scaled) 2.2e-16 sqrt(T_ii T_jj), T = |G| |Sigma_cc| |G|^T; k = 64, or 2000 for the two cases of the "outlier" scene (the
oracle's docstring derives both; the wide robust cases of tricov_oracle.ROBUST_CASES are held to 2000 as well)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import keypoint_scenes as ks
import tricov_oracle as tco

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck", "tricov_hostcheck.cpp")


def P(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


@pytest.fixture(scope="module")
def hc(tmp_path_factory):
    lib = str(tmp_path_factory.mktemp("tricov_hostcheck") / "libtricov_hostcheck.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-o", lib, SRC])
    h = ctypes.CDLL(lib)
    h.hc_tricov.argtypes = [ctypes.c_int, ctypes.c_size_t] + [ctypes.c_void_p] * 5 + [ctypes.c_int, ctypes.c_double, ctypes.c_double] + [ctypes.c_void_p] * 6
    h.hc_tricov_rows.argtypes = [ctypes.c_void_p] * 6
    h.hc_tricov_rows.restype = None
    return h


def host_uncertainty(hc, points, uvs, ext, intr, camera_covariance=None, sigma=None, loss="linear", f_scale=1.0):
    """the host build on the arguments of tricov_oracle.uncertainty: dict with the oracle's keys (3 x 3 blocks unpacked as the package does)"""
    theta, d5 = tco.camera_blocks(ext, intr)
    uv = np.ascontiguousarray(np.stack([np.asarray(u, dtype=np.float64) for u in uvs]))
    pts = np.ascontiguousarray(points, dtype=np.float64)
    C, n_pts = uv.shape[:2]
    S = None if camera_covariance is None else np.ascontiguousarray(camera_covariance, dtype=np.float64)
    det, cal, G = np.empty((n_pts, 6)), None if S is None else np.empty((n_pts, 6)), np.empty((n_pts, 3, 12 * C))
    views, status, info = np.empty(n_pts, np.int32), np.empty(n_pts, np.int32), np.empty(8)
    assert hc.hc_tricov(C, n_pts, P(pts), P(uv), P(theta), P(d5), P(S), tco.LOSS_NAMES.index(loss), f_scale, float("nan") if sigma is None else sigma ** 2, P(det), P(cal), P(G), P(views),
                        P(status), P(info)) == 0
    idx = [0, 1, 2, 1, 3, 4, 2, 4, 5]
    return dict(detection=det[:, idx].reshape(-1, 3, 3), calibration=None if cal is None else cal[:, idx].reshape(-1, 3, 3), G=G, views=views, status=status, sigma2=info[0],
                n_residuals=int(info[1]), n_free=int(info[2]), n_unusable=int(info[3]), n_degenerate=int(info[4]))


@pytest.mark.parametrize("name", sorted(tco.CASES))
def test_host_build_matches_the_oracle(hc, name):
    i, o = tco.case(name)
    got = host_uncertainty(hc, i["points"], i["uvs"], i["ext"], i["intr"], i["camera_covariance"], tco.SIGMA, i["loss"], i["f_scale"])
    tco.check_against_oracle(name, got, o)
    if name in tco.POOLED_CASES:
        tco.check_pooled(name, host_uncertainty(hc, i["points"], i["uvs"], i["ext"], i["intr"], i["camera_covariance"], None, i["loss"], i["f_scale"]), got, o)
    ok = o["status"] == 1
    assert (np.linalg.eigvalsh(got["detection"][ok]) > 0).all()
    gerr = np.abs(got["G"][ok] - o["G"][ok]).max() / np.abs(o["G"][ok]).max()
    print(f"{name}: G relative to its largest entry {gerr:.3g}")
    assert gerr <= np.nanmax(o["bound"])
    # without a camera covariance: the detection term alone, the same bits
    alone = host_uncertainty(hc, i["points"], i["uvs"], i["ext"], i["intr"], None, tco.SIGMA, i["loss"], i["f_scale"])
    assert alone["calibration"] is None and np.array_equal(alone["detection"], got["detection"], equal_nan=True)


def test_camera_rows_against_central_differences(hc):
    """A_c and B_c of the header against central differences of keypoint_scenes.project5, at a camera with zero rotation vector (the series branch
    of rot_coeffs), one with a tiny one (still the series) and an ordinary one; p1, p2, k3 non-zero"""
    rng = np.random.default_rng(5)
    d5 = np.array([-0.12, 0.03, 1e-3, -5e-4, 0.01])
    for rvec in (np.zeros(3), np.array([1e-3, -2e-3, 5e-4]), np.array([0.3, -0.2, 0.5])):
        theta = np.r_[900.0, 910.0, 640.0, 500.0, d5[0], d5[1], rvec, 30.0, -20.0, 50.0]
        X = rng.normal(0, 80, 3) + np.r_[0, 0, 900.0]

        def proj(th, Xw):
            K = np.array([[th[0], 0, th[2]], [0, th[1], th[3]], [0, 0, 1.0]])
            return ks.project5(Xw, th[6:], K, np.r_[th[4], th[5], d5[2:]])

        uv, A, B = np.empty(2), np.empty((2, 3)), np.empty((2, 12))
        hc.hc_tricov_rows(P(theta), P(d5), P(X), P(uv), P(A), P(B))
        assert np.abs(uv - proj(theta, X)).max() < 1e-9
        fdA, fdB = np.empty((2, 3)), np.empty((2, 12))
        for k in range(3):
            h = 1e-4 * np.eye(3)[k]
            fdA[:, k] = (proj(theta, X + h) - proj(theta, X - h)) / 2e-4
        for k in range(12):
            step = (1.0, 1.0, 1.0, 1.0, 1e-2, 1e-2, 1e-6, 1e-6, 1e-6, 1e-3, 1e-3, 1e-3)[k]   # (the model is linear in the first six: no truncation error)
            h = step * np.eye(12)[k]
            fdB[:, k] = (proj(theta + h, X) - proj(theta - h, X)) / (2 * step)
        eA = np.abs(A - fdA).max() / np.abs(fdA).max()
        eB = (np.abs(B - fdB) / np.maximum(np.abs(fdB).max(axis=0), 1e-300)).max()   # per column: the columns differ by orders of magnitude
        print(f"rvec {rvec}: A {eA:.3g}  B (per column) {eB:.3g}")
        assert eA < 1e-7 and eB < 1e-6
        # ... and against the oracle's independent analytic form
        _, Ao, Bo = tco.camera_rows(X[None], theta, d5)
        assert np.abs(A - Ao[0]).max() <= 1e-12 * np.abs(Ao).max()
        assert (np.abs(B - Bo[0]) / np.abs(Bo[0]).max(axis=0).clip(1e-300)).max() <= 1e-11


def test_status_verdicts(hc):
    """-1: fewer than two views, or a NaN in the point; -2: camera 1 a copy of camera 0 and a point those two alone see, or a point on the baseline.
    Such points are NaN, leave the pooled sums and are counted; the others are what they are without them."""
    i, o = tco.case("three")
    uvs = [u.copy() for u in i["uvs"]]
    ext = i["ext"].copy()
    intr = list(i["intr"])
    ext[1], intr[1] = ext[0], intr[0]
    uvs[1] = uvs[0] + 0.1
    pts = i["points"].copy()
    seen0 = ~np.isnan(uvs[0]).any(-1)
    deg = np.flatnonzero(seen0)[:3]
    for p in deg:
        uvs[2][p] = np.nan
    one_view = np.flatnonzero(seen0 & ~np.isnan(uvs[2]).any(-1))[0]
    uvs[0][one_view] = np.nan
    uvs[1][one_view] = np.nan
    nan_point = np.flatnonzero(seen0 & ~np.isnan(uvs[2]).any(-1))[5]
    pts[nan_point, 1] = np.nan
    S = i["camera_covariance"]
    got = host_uncertainty(hc, pts, uvs, ext, intr, S, sigma=tco.SIGMA)
    ref = tco.uncertainty(pts, uvs, ext, intr, camera_covariance=S, sigma=tco.SIGMA)
    assert (got["status"][deg] == -2).all() and got["status"][one_view] == -1 and got["status"][nan_point] == -1
    tco.check_against_oracle("three, degenerate", got, ref)
    assert got["n_degenerate"] == ref["n_degenerate"] >= 3
    assert np.isnan(got["calibration"][got["status"] != 1]).all()
    # the usable points do not notice the others
    keep = got["status"] == 1
    sub = host_uncertainty(hc, pts[keep], [u[keep] for u in uvs], ext, intr, S, sigma=0.3)
    full = host_uncertainty(hc, pts, uvs, ext, intr, S, sigma=0.3)
    assert np.array_equal(sub["detection"], full["detection"][keep]) and np.array_equal(sub["calibration"], full["calibration"][keep])
    # a point on the baseline of two cameras: both rays are the same line
    uv2, ext2, intr2, X2 = i["uvs"][:2], i["ext"][:2], i["intr"][:2], None
    c0 = -ks.rodrigues(ext2[0][:3]).T @ ext2[0][3:]
    c1 = -ks.rodrigues(ext2[1][:3]).T @ ext2[1][3:]
    X2 = (c0 + 3.0 * (c1 - c0))[None]
    det2 = [ks.project5(X2, ext2[c], *intr2[c]) for c in range(2)]
    on_line = host_uncertainty(hc, X2, det2, ext2, intr2)
    assert on_line["status"][0] == -2 and tco.uncertainty(X2, det2, ext2, intr2)["status"][0] == -2


def test_sanitized_stand_alone_program(tmp_path):
    """the header under AddressSanitizer + UBSan in a program of its own (its own main, two cases: 2 cameras x 1 point; 3 cameras x 5 points with a
    camera covariance, a degenerate point and one with a single view), run as a child process with the sanitizer runtime linked in"""
    exe = str(tmp_path / "tricov_sanitized")
    subprocess.check_call(["g++", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-DTRICOV_MAIN", "-o", exe, SRC])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "tricov hostcheck ok" in r.stdout
