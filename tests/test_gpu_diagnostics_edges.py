"""The kernels users call directly (csrc/mcba_diag.hip: k_reproj_diag, k_undistort, k_sel_hist / k_sel_pick) against the
oracles at their launch boundaries and hard inputs: camera groups of 40, frame blocks of 64, boards of 4 to 200 points,
incomplete detections, undistortion rounds, grazing and edge-on boards, OpenCV's icdist < 0 guard and exact medians."""
import numpy as np
import pytest

from oracle import diagnostics_oracle as dgo
from oracle import triangulate_oracle as tri

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mc():
    import multicam_calibration_amd as m

    m.ops.load_library()
    return m


# ---------------------------------------------------------------- reprojection diagnostics
def _dists(C, seed=0):
    """Five distortion coefficients of its own for every camera; cameras 39, 40 and 41 (the edge of the first launch group of
    40) get strongly different ones, so a camera that reads a neighbour's distortion moves the arrays and the medians."""
    rng = np.random.default_rng(seed)
    d = np.stack([rng.uniform(-0.12, -0.04, C), rng.uniform(0.0, 0.04, C), rng.uniform(-1e-3, 1e-3, C), rng.uniform(-1e-3, 1e-3, C),
                  rng.uniform(-0.01, 0.01, C)], 1)
    strong = {39: [-0.25, 0.08, 2e-3, -1e-3, 0.02], 40: [0.12, -0.05, -2e-3, 1.5e-3, -0.01], 41: [-0.02, 0.0, 5e-4, 5e-4, 0.0]}
    for c, v in strong.items():
        if c < C:
            d[c] = v
    return d


def _intr(p, dists):
    return [(K, dists[c]) for c, (K, _) in enumerate(p["intrinsics"])]


def _check(mc, uvs, ext, intr, obj, poses, iterations=5):
    """GPU against the oracle at the tolerances of test_gpu_diagnostics.py; the medians alone (arrays=False) are the same bits."""
    med, rep, tra = mc.reprojection_errors(uvs, ext, intr, obj, poses, undistort_iterations=iterations)
    med0, rep0, tra0 = dgo.reprojection_errors(uvs, ext, intr, obj, poses, iterations)
    assert rep.shape == rep0.shape and tra.shape == tra0.shape
    np.testing.assert_allclose(rep, rep0, rtol=0, atol=1e-9)
    assert np.array_equal(np.isnan(tra), np.isnan(tra0))
    np.testing.assert_allclose(tra, tra0, rtol=0, atol=1e-6, equal_nan=True)
    assert np.array_equal(np.isnan(med), np.isnan(med0))
    np.testing.assert_allclose(med, med0, rtol=1e-7, equal_nan=True)
    med2, rep2, tra2 = mc.reprojection_errors(uvs, ext, intr, obj, poses, undistort_iterations=iterations, arrays=False)
    assert rep2 is None and tra2 is None
    np.testing.assert_array_equal(med2, med)
    return med, rep, tra


@pytest.mark.parametrize("C", [1, 39, 40, 41, 80, 81])
def test_camera_groups_vs_oracle(mc, C):
    """k_reproj_diag runs in launch groups of 40 cameras (DiagCams, c0, blockIdx.y): every camera against the oracle, arrays included."""
    p = mc.synth.make_problem(C, 3, seed=60 + C, missing=0.15 if C > 1 else 0.0)
    _check(mc, p["uvs"], p["extrinsics"], _intr(p, _dists(C, C)), p["obj"], p["poses"])


@pytest.mark.parametrize("F", [1, 63, 64, 65, 257])
def test_frame_blocks_vs_oracle(mc, F):
    """A ragged last wavefront, and workgroups whose four wavefronts lie partly past the last frame block: the whole (C, F, N, 2)
    arrays are compared, so a write for a frame f >= F into camera 0's rows shows up as a mismatch in camera 1's."""
    p = mc.synth.make_problem(2, F, seed=70 + F, missing=0.5 if F > 1 else 0.0, scalar_nans=3 if F > 1 else 0)   # (the oracle fits complete frames only)
    _check(mc, p["uvs"], p["extrinsics"], _intr(p, _dists(2, F)), p["obj"], p["poses"])


@pytest.mark.parametrize("shape", [(2, 2), (2, 3, 5), (9, 11), (10, 20)])
def test_board_sizes_vs_oracle(mc, shape):
    """N = 4 (an exactly determined homography), 5, 99 and 200 points (more points than lanes in a wavefront)."""
    rows, cols = shape[:2]
    p = mc.synth.make_problem(3, 12, rows=rows, cols=cols, seed=80 + rows * cols, missing=0.1)
    n = shape[2] if len(shape) > 2 else rows * cols
    _check(mc, p["uvs"][:, :, :n], p["extrinsics"], _intr(p, _dists(3, n)), p["obj"][:n], p["poses"])


def test_planar_board_off_the_z0_plane_vs_oracle(mc):
    """A board at constant z != 0: the reprojection uses all of X_o, the homography only its XY."""
    p = mc.synth.make_problem(3, 20, seed=85, noise=0.0)
    obj = p["obj"].copy()
    obj[:, 2] = 7.5
    uvs = mc.synth.project(p["true_cam"], p["true_poses"], obj) + np.random.default_rng(3).normal(0, 0.3, p["uvs"].shape)
    med, rep, tra = _check(mc, uvs, p["extrinsics"], _intr(p, _dists(3, 85)), obj, p["poses"])
    flat = _check(mc, uvs, p["extrinsics"], _intr(p, _dists(3, 85)), p["obj"], p["poses"])[1]
    assert np.abs(rep - flat).max() > 1.0   # (the offset is seen: the test is not blind to X_o[2])


def test_incomplete_detections_vs_oracle(mc):
    p = mc.synth.make_problem(43, 3, seed=90)
    uvs = p["uvs"].copy()
    uvs[0, 1, 3, 1] = np.nan           # one missing scalar: u present, v NaN
    uvs[1, 2, -1] = np.nan             # only the last board point missing
    uvs[2, 0] = np.nan                 # a whole frame missing in one camera
    uvs[42, :, 7, 0] = np.nan          # a camera of the second launch group without a complete frame
    intr = _intr(p, _dists(43, 90))
    med, rep, tra = _check(mc, uvs, p["extrinsics"], intr, p["obj"], p["poses"])
    assert np.isnan(med[42]) and np.isfinite(np.delete(med, 42)).all()
    for c, f in ((0, 1), (1, 2), (2, 0)):
        assert np.isnan(tra[c, f]).all() and np.isfinite(rep[c, f]).all()
    uvs[:, :, 5, 1] = np.nan           # every frame incomplete in every camera
    med, rep, tra = _check(mc, uvs, p["extrinsics"], intr, p["obj"], p["poses"])
    assert np.isnan(med).all() and np.isnan(tra).all() and np.isfinite(rep).all()


@pytest.mark.parametrize("iterations", [0, 1, 5, 20])
def test_undistortion_rounds_vs_oracle(mc, iterations):
    p = mc.synth.make_problem(2, 9, seed=95, missing=0.1)
    _check(mc, p["uvs"], p["extrinsics"], _intr(p, _dists(2, 95)), p["obj"], p["poses"], iterations)


def _one_camera(angles_deg, noise, seed=0, through_centre=None, rows=6, cols=9):
    """Camera 0 at the origin looking down +z, boards tilted about their x axis by `angles_deg` (90 = edge-on) 450 mm away;
    `through_centre`: that frame's board plane contains the optical centre (edge-on: collinear detections)."""
    from multicam_calibration_amd import synth

    rng = np.random.default_rng(seed)
    obj = synth.board_points(rows, cols)
    c = obj.mean(0)
    poses = []
    for i, a in enumerate(angles_deg):
        r = np.array([np.deg2rad(a), 0.0, 0.0])
        if i != through_centre:
            r += rng.normal(0, 0.02, 3)
        t = np.array([30.0, 0.0 if i == through_centre else rng.normal(0, 20), 450.0])
        poses.append(np.r_[r, t - synth._rot(r) @ c])
    poses = np.array(poses)
    cam = np.array([[1150.0, 1148.0, 640.0, 512.0, -0.08, 0.02, 0, 0, 0, 0, 0, 0]])
    uvs = synth.project(cam, poses, obj) + rng.normal(0, noise, (1, len(poses), obj.shape[0], 2))
    K = np.array([[1150.0, 0, 640.0], [0, 1148.0, 512.0], [0, 0, 1]])
    poses0 = poses + np.r_[1e-3 * np.ones(3), 0.5 * np.ones(3)] * rng.normal(size=poses.shape)   # the solver's view of the poses
    return uvs, np.zeros((1, 6)), [(K, np.array([-0.08, 0.02, 0.0, 0.0, 0.0]))], obj, poses0


@pytest.mark.parametrize("noise", [0.0, 0.5, 3.0])
def test_homography_grazing_board_vs_oracle(mc, noise):
    """Boards 70 to 85 degrees from the optical axis: strong perspective, the kernel's 24 LM rounds against the oracle's 60."""
    _check(mc, *_one_camera([70, 72, 75, 78, 80, 85], noise, seed=int(noise * 10)))


@pytest.mark.parametrize("noise", [0.0, 0.5, 3.0])
def test_homography_minimal_board_vs_oracle(mc, noise):
    """Four board points: the homography interpolates them exactly whatever the noise."""
    _check(mc, *_one_camera([10, 40, 60, 75], noise, seed=7, rows=2, cols=2))


@pytest.mark.parametrize("angle,noise", [(89.0, 0.0), (89.0, 0.5), (89.9, 0.0), (89.99, 0.0)])
def test_homography_edge_on_board_vs_oracle(mc, angle, noise):
    """One frame's board nearly edge-on, its plane through the optical centre: nearly collinear detections, the worst-conditioned
    normal equations the start can meet.  (0.5 px of noise at 89.9 degrees leaves the transfer error so flat that the oracle's own
    60 rounds have not converged: no reference exists there.)"""
    _check(mc, *_one_camera([20, 35, angle], noise, seed=11, through_centre=2))


# ---------------------------------------------------------------- undistortion
K_TEST = np.array([[1150.0, 0, 655.0], [0, 1140.0, 500.0], [0, 0, 1]])
DISTS = {"all": np.array([-0.12, 0.03, 1e-3, -5e-4, 0.01]), "tangential": np.array([0.0, 0.0, 2e-3, -1.5e-3, 0.0]),
         "k3": np.array([0.0, 0.0, 0.0, 0.0, 0.08])}


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 2 ** 20 + 3])
def test_undistort_point_counts(mc, n):
    uv = np.random.default_rng(n).uniform(0, 1280, (n, 2))
    if n > 3:
        uv[n // 2] = np.nan
        uv[-1, 0] = np.nan             # the last point of the last (partial) block
    got = mc.undistort_points(uv, K_TEST, DISTS["all"])
    assert got.shape == (n, 2)
    np.testing.assert_allclose(got, tri.undistort_points(uv, K_TEST, DISTS["all"]), rtol=0, atol=1e-10)


@pytest.mark.parametrize("kind", sorted(DISTS))
@pytest.mark.parametrize("iterations", [0, 1, 5, 20])
def test_undistort_models_and_rounds(mc, kind, iterations):
    uv = np.random.default_rng(iterations).uniform(0, 1280, (3, 5, 7, 2))
    uv[0, 1, 2] = np.nan
    uv[1, 2, 3, 0] = np.nan
    uv[2, 4, 6, 1] = np.nan
    got = mc.undistort_points(uv, K_TEST, DISTS[kind], iterations=iterations)
    want = tri.undistort_points(uv, K_TEST, DISTS[kind], iterations)
    assert got.shape == uv.shape
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-10)
    assert np.array_equal(np.isnan(got), np.isnan(uv).any(-1, keepdims=True).repeat(2, -1))   # a row with one NaN is NaN in both
    if iterations == 0:
        ok = ~np.isnan(got)
        np.testing.assert_allclose(got[ok], uv[ok], rtol=0, atol=1e-12)                           # (u - cx) / fx * fx + cx: a few ulp of 1280 px


def test_undistort_input_forms(mc):
    uv = np.random.default_rng(2).uniform(0, 1280, (40, 2))
    want = tri.undistort_points(uv, K_TEST, DISTS["all"])
    got1 = mc.undistort_points(uv[7], K_TEST, DISTS["all"])
    assert got1.shape == (2,)
    np.testing.assert_allclose(got1, want[7], rtol=0, atol=1e-10)
    np.testing.assert_allclose(mc.undistort_points(uv.tolist(), K_TEST, list(DISTS["all"])), want, rtol=0, atol=1e-10)
    u32 = uv.astype(np.float32)
    np.testing.assert_allclose(mc.undistort_points(u32, K_TEST, DISTS["all"]), tri.undistort_points(u32.astype(np.float64), K_TEST, DISTS["all"]), rtol=0, atol=1e-10)
    assert np.isnan(mc.undistort_points(np.full((5, 3, 2), np.nan), K_TEST, DISTS["all"])).all()


# ---------------------------------------------------------------- OpenCV's icdist < 0 guard
K_GUARD = np.array([[1000.0, 0, 640.0], [0, 1000.0, 512.0], [0, 0, 1]])
D_GUARD = np.array([-0.5, 0.0, 0.0, 0.0, 0.0])


def test_undistort_guard_vs_oracle(mc):
    """Past the model's valid radius (1 + k1 r^2 < 0 at r = 2, or reached by a later iterate at r = 1.35) the unrefined point comes back."""
    far = np.array([[640.0 + 1600.0, 512.0 + 1200.0], [640.0 - 2000.0, 512.0], [640.0 + 1350.0, 512.0], [700.0, 540.0]])
    for it in (1, 5, 20):
        got = mc.undistort_points(far, K_GUARD, D_GUARD, iterations=it)
        np.testing.assert_allclose(got, tri.undistort_points(far, K_GUARD, D_GUARD, it), rtol=0, atol=1e-10)
        np.testing.assert_allclose(got[:3 if it > 1 else 2], far[:3 if it > 1 else 2], rtol=0, atol=1e-10)   # (r = 1.35 leaves the radius in round 2)


@pytest.mark.parametrize("C", [3, 9])   # one lane per point / one wavefront per point
def test_triangulate_guard_vs_oracle(mc, C):
    from test_triangulate_cpu import scene

    uvs, ext, intr, X = scene(C=C, P=300, seed=30 + C, noise=0.2)
    intr[1] = (intr[1][0], np.array([-0.5, 0.05, 0.0, 0.0, 0.0]))   # strong barrel distortion in camera 1
    uvs[1] = uvs[1].copy()
    K = intr[1][0]
    uvs[1][::7] = K[:2, 2] + np.array([1.9, -0.8]) * K[0, 0]       # detections far outside the valid radius
    want = tri.triangulate(uvs, ext, intr)
    got = mc.triangulate(uvs, ext, intr)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want).any(1)
    assert np.abs(got[ok] - want[ok]).max() <= 1e-8 * np.abs(want[ok]).max()


# ---------------------------------------------------------------- exact medians
def _exact_problem(mc, offsets, C=1):
    """Errors the kernel computes exactly: unit camera at the origin, boards at z = 1 without rotation, integer board
    coordinates -> the prediction is the board point itself, bit for bit; detections = prediction + (offset, 0), so each
    per-point error is |u - X|, the same subtraction in numpy as in the kernel (and sqrt(fl(r^2)) = |r|)."""
    F, N = offsets.shape[1:3]
    obj = np.zeros((N, 3))
    obj[:, 0] = np.arange(N) % 4
    obj[:, 1] = np.arange(N) // 4
    uvs = np.empty((C, F, N, 2))
    uvs[..., 0] = obj[:, 0] + offsets
    uvs[..., 1] = obj[:, 1]
    err = np.abs(uvs[..., 0] - obj[:, 0])
    cam = np.r_[1.0, 1.0, 0.0, 0.0, 0.0, 0.0, np.zeros(6)]
    x = np.concatenate([np.tile(cam, C), np.tile(np.r_[0.0, 0.0, 0.0, 0.0, 0.0, 1.0], F)])
    prob = mc.ops.Problem(uvs, obj)
    prob.set_params(0, x)
    mean_cf = prob.frame_errors(0)[0]
    return prob, err, mean_cf


def _assert_median(prob, err, mask=None):
    med, cnt = prob.error_median(mask)
    sel = err if mask is None else err[:, mask.astype(bool)]
    assert cnt == int((~np.isnan(sel)).sum())
    want = np.nanmedian(sel) if cnt else np.nan
    # np.nanmedian's two middle values: (a + b) / 2, which is what the host computes as 0.5 * (a + b) -- bit for bit either way
    assert (med == want) or (np.isnan(med) and np.isnan(want)), (med, want, cnt)


def test_exact_median_noise_free_zeros(mc):
    rng = np.random.default_rng(1)
    off = np.zeros((1, 30, 12))
    off[0, :7] = rng.uniform(0.1, 2.0, (7, 12))     # most errors are exactly 0.0
    prob, err, mean_cf = _exact_problem(mc, off)
    assert (mean_cf[0, 7:] == 0.0).all()            # (the premise: a noise-free frame has exactly zero error)
    _assert_median(prob, err)
    for k in range(5):
        _assert_median(prob, err, (np.arange(30) % 5 == k).astype(np.uint8))
    prob.close()


def test_exact_median_identical_values(mc):
    off = np.full((2, 40, 8), 0.375)
    off[:, ::9] = 0.75
    off[0, 3, :3] = 0.25
    prob, err, _ = _exact_problem(mc, off, C=2)
    _assert_median(prob, err)
    for k in (0, 1, 2):
        m = np.zeros(40, np.uint8)
        m[k::4] = 1
        _assert_median(prob, err, m)
    prob.close()


def test_exact_median_many_binades(mc):
    """Errors spanning more than 2^40: a few frames posed far off, most at sub-micropixel error."""
    rng = np.random.default_rng(7)
    off = rng.uniform(1e-9, 1e-7, (1, 64, 12)) * rng.choice([-1.0, 1.0], (1, 64, 12))
    off[0, ::8] = rng.uniform(1e3, 1e5, (8, 12))
    off[0, 5, :6] = 2.0 ** rng.integers(-40, 16, 6)
    prob, err, _ = _exact_problem(mc, off)
    assert np.nanmax(err) / np.nanmin(err[err > 0]) > 2.0 ** 40
    _assert_median(prob, err)
    for k in range(3):
        _assert_median(prob, err, (np.arange(64) % 3 == k).astype(np.uint8))
    prob.close()


def test_exact_median_of_one_two_three_values(mc):
    off = np.full((1, 6, 3), np.nan)
    off[0, 0, 0] = 5e-7
    off[0, 1, :2] = [3.0, 1e-9]
    off[0, 2, :] = [2.0, 1e-6, 7.5]
    prob, err, _ = _exact_problem(mc, off)
    for f in range(3):
        m = np.zeros(6, np.uint8)
        m[f] = 1
        _assert_median(prob, err, m)
        assert prob.error_median(m)[1] == f + 1
    m = np.zeros(6, np.uint8)
    m[3] = 1
    _assert_median(prob, err, m)                    # nothing selected: NaN
    prob.close()

