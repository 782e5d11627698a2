"""triangulate() oracle (oracle/triangulate_oracle.py, parity unpinned: see its header) against synthetic truth, and the
reference's NaN / pairing semantics (geometry.py:392-433) restated from its source."""
import numpy as np

import multicam_calibration_amd as m
from oracle import triangulate_oracle as tri


def scene(C=5, P=300, seed=0, noise=0.0, p_unseen=0.0):
    p = m.synth.make_problem(C, 2, seed=seed, noise=0.0)
    cam = p["true_cam"].copy()
    rng = np.random.default_rng(seed + 7)
    T = m.synth._T(p["true_poses"][0])
    X = rng.normal(0, 60, (P, 3)) @ T[:3, :3].T + T[:3, 3]   # a cloud where the board would be (world = camera 0)
    uvs = np.stack([m.synth.project(cam[c:c + 1], np.zeros((1, 6)), X)[0, 0] for c in range(C)])
    uvs += rng.normal(0, noise, uvs.shape) if noise else 0.0
    if p_unseen:
        uvs[rng.uniform(size=(C, P)) < p_unseen] = np.nan
    intr = [(np.array([[c[0], 0, c[2]], [0, c[1], c[3]], [0, 0, 1.0]]), np.r_[c[4:6], 0, 0, 0]) for c in cam]
    return list(uvs), cam[:, 6:], intr, X


def test_oracle_recovers_noise_free_points():
    uvs, ext, intr, X = scene()
    assert np.abs(tri.triangulate(uvs, ext, intr, iterations=20) - X).max() < 1e-9
    assert np.abs(tri.triangulate(uvs, ext, intr) - X).max() < 1e-6   # cv2's 5 undistortion iterations


def test_oracle_undistort_inverts_the_projection_model():
    uvs, ext, intr, X = scene(C=2, P=50)
    K, d = intr[1]
    cam_nodist = np.r_[K[0, 0], K[1, 1], K[0, 2], K[1, 2], 0, 0, ext[1]]
    ideal = m.synth.project(cam_nodist[None], np.zeros((1, 6)), X)[0, 0]
    np.testing.assert_allclose(tri.undistort_points(uvs[1], K, d, iterations=25), ideal, atol=1e-9)


def test_oracle_nan_semantics():
    uvs, ext, intr, X = scene(C=4, P=40, p_unseen=0.45, seed=3)
    out = tri.triangulate(uvs, ext, intr, iterations=20)
    seen = (~np.isnan(np.stack(uvs)).any(-1)).sum(0)
    assert np.array_equal(np.isnan(out).any(1), seen < 2)          # fewer than two views -> NaN row (geometry.py:427-428)
    assert np.abs(out[seen >= 2] - X[seen >= 2]).max() < 1e-8
    uvs[2][5, 0] = np.nan                                            # one coordinate missing = camera does not see the point
    assert not np.isnan(tri.triangulate(uvs, ext, intr)[5]).any() or seen[5] < 3


def _undistort_unguarded(uvs, K, k, iterations):
    """The iteration without OpenCV's icdist < 0 guard, as the oracle had it before the guard."""
    k1, k2, p1, p2, k3 = k
    x0 = (uvs[..., 0] - K[0, 2]) / K[0, 0]
    y0 = (uvs[..., 1] - K[1, 2]) / K[1, 1]
    x, y = x0.copy(), y0.copy()
    for _ in range(iterations):
        r2 = x * x + y * y
        icdist = 1.0 / (1 + ((k3 * r2 + k2) * r2 + k1) * r2)
        dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        x, y = (x0 - dx) * icdist, (y0 - dy) * icdist
    return np.stack([x * K[0, 0] + K[0, 2], y * K[1, 1] + K[1, 2]], axis=-1)


def test_oracle_undistort_icdist_guard():
    """OpenCV's cvUndistortPointsInternal stops at icdist < 0 and returns the unrefined point (its test undistortPoints.regression_14583)."""
    K = np.array([[1000.0, 0, 640.0], [0, 1000.0, 512.0], [0, 0, 1]])
    k = np.array([-0.5, 0.0, 0.0, 0.0, 0.0])
    far = np.array([[640.0 + 1000.0 * 1.6, 512.0 + 1000.0 * 1.2], [640.0 - 1000.0 * 2.0, 512.0]])   # r = 2: 1 + k1 r^2 = -1 at the first round
    for it in (1, 5, 20):
        np.testing.assert_array_equal(tri.undistort_points(far, K, k, it), far)
        assert not np.array_equal(_undistort_unguarded(far, K, k, it), far)                       # (what the guard replaces)
    # inside the valid radius nothing changes, bit for bit, at realistic and at strong distortion
    rng = np.random.default_rng(4)
    image = rng.uniform([0, 0], [1280, 1024], (500, 2))
    image[7] = np.nan
    image[9, 1] = np.nan
    centre = rng.uniform([240, 112], [1040, 912], (500, 2))                                        # r < 0.57: k1 = -0.5 converges there
    for kk, uv in ((k, centre), (np.array([-0.12, 0.03, 1e-3, -5e-4, 0.01]), image), (np.array([0.0, 0.0, 2e-3, -1e-3, 0.0]), image), (np.array([0.0, 0.0, 0.0, 0.0, 0.05]), image)):
        for it in (0, 1, 5, 20):
            want = _undistort_unguarded(uv, K, kk, it)
            want[np.isnan(uv).any(-1)] = np.nan
            np.testing.assert_array_equal(tri.undistort_points(uv, K, kk, it), want)
    # a point whose iterate leaves the radius later: the unrefined point too
    mid = np.array([[640.0 + 1000.0 * 1.35, 512.0]])
    assert 1 + k[0] * 1.35 ** 2 > 0
    got = tri.undistort_points(mid, K, k, 20)
    x = 1.35
    for _ in range(20):
        d = 1 + k[0] * x * x
        if 1.0 / d < 0:
            x = 1.35
            break
        x = 1.35 / d
    assert got[0, 0] == 640.0 + 1000.0 * x and got[0, 1] == 512.0
