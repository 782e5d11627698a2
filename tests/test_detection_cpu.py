"""Chessboard detection without a GPU: the host helpers, the renderer the GPU tier relies on, the kernels' arithmetic (csrc/mcba_detect_math.h
compiled with g++) against the numpy transcriptions, input checks and the no-GPU error."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import chessboard_scenes as scenes
import cv_transcriptions as cvt
from multicam_calibration_amd import detection, ops, synth

HERE = os.path.dirname(os.path.abspath(__file__))


def P(a):
    return ctypes.c_void_p(a.ctypes.data)


@pytest.fixture(scope="module")
def hc(tmp_path_factory):
    src = os.path.join(HERE, "hostcheck", "detect_hostcheck.cpp")
    lib = str(tmp_path_factory.mktemp("detect_hostcheck") / "libdetect_hostcheck.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", lib, src])
    h = ctypes.CDLL(lib)
    h.hc_rect_subpix.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_float, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    h.hc_pearson.restype = ctypes.c_double
    return h


def test_objpoints_match_the_reference_formula():
    for shape, s in [((7, 10), 12.5), ((5, 7), 1.0), ((3, 3), 2.0)]:
        o = detection.generate_chessboard_objpoints(shape, s)
        assert o.dtype == np.float32 and o.shape == (shape[0] * shape[1], 3)
        k = np.arange(len(o))
        np.testing.assert_array_equal(o[:, 0], (k % shape[0]) * np.float32(s))
        np.testing.assert_array_equal(o[:, 1], (k // shape[0]) * np.float32(s))
        assert np.all(o[:, 2] == 0)


def test_summarize_detections_counts_and_labels():
    pd = pytest.importorskip("pandas")
    uvs = np.zeros((3, 5, 4, 2))
    uvs[0, [1, 2]] = np.nan
    uvs[1, 2, 0, 1] = np.nan
    uvs[2, :] = np.nan
    t = detection.summarize_detections(uvs)
    assert isinstance(t, pd.DataFrame)
    assert list(t.index) == ["Camera 0", "Camera 1", "Camera 2"] and list(t.columns) == list(t.index)
    np.testing.assert_array_equal(t.values, [[3, 3, 0], [3, 4, 0], [0, 0, 0]])


def test_extend_grid_reproduces_an_exact_homography():
    H = np.array([[31.0, 4.0, 200.0], [-3.0, 28.0, 150.0], [0.002, -0.001, 1.0]])
    rows, cols = 10, 7
    full = np.mgrid[0:cols + 2, 0:rows + 6].T.astype(np.float64)
    p = np.c_[full.reshape(-1, 2), np.ones(full[..., 0].size)] @ H.T
    uv_full = (p[:, :2] / p[:, 2:]).reshape(full.shape)
    ext = detection.extend_grid(uv_full[3:-3, 1:-1], 3, 1)
    assert ext.shape == (rows + 6, cols + 2, 2)
    assert np.abs(ext - uv_full).max() < 1e-9


def test_anchor_template_is_the_disc():
    t = detection._anchor_template()
    assert t.shape == (40, 40) and t.dtype == np.uint8
    assert int((t == 0).sum()) == 317
    np.testing.assert_array_equal(t, cvt.template())


def test_renderer_corners_are_synth_projection():
    pose = scenes.look_at_pose((7, 10), 40.0, np.radians(35), 0.3, 0.4)
    cam = (900.0, 905.0, 320.0, 240.0, -0.08, 0.02)
    cam12 = np.r_[cam, np.zeros(6)][None]
    pose_s = pose.copy()
    pose_s[3:] = pose[3:] * 12.5
    uv = scenes.corners((7, 10), pose_s, cam, square=12.5)
    np.testing.assert_allclose(uv, scenes.corners((7, 10), pose, cam), rtol=0, atol=1e-9)
    ref = synth.project(cam12, pose_s[None], detection.generate_chessboard_objpoints((7, 10), 12.5).astype(np.float64))[0, 0]
    np.testing.assert_allclose(uv, ref, rtol=0, atol=1e-9)


def test_renderer_pixel_centre_convention():
    """A fronto-parallel board with its edges on whole pixel coordinates: the pixel whose centre lies on an edge is half black, half white."""
    cam = (100.0, 100.0, 31.0, 40.0, 0.0, 0.0)
    pose = np.r_[0.0, 0.0, 0.0, -0.0, 0.0, 10.0]  # 10 px per square, corner (0, 0) at pixel (31, 40)
    img = scenes.render((3, 3), pose, cam, (80, 90), supersample=4).astype(float)
    # pixel column 31 covers [30.5, 31.5]: the edge x = 31 halves it; columns 30 and 32 lie wholly on either side (row 35: square row -1)
    assert img[35, 30] == scenes.BLACK and img[35, 32] == scenes.WHITE
    assert img[35, 31] == 0.5 * (scenes.BLACK + scenes.WHITE)
    # and row 40 is halved by the edge y = 40 (column 35: square column 0)
    assert img[39, 35] == scenes.WHITE and img[41, 35] == scenes.BLACK and img[40, 35] == 0.5 * (scenes.BLACK + scenes.WHITE)


def test_grey_formula_exact(hc):
    rng = np.random.default_rng(0)
    bgr = np.concatenate([rng.integers(0, 256, (1 << 20, 3)), np.array([[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 255, 0], [0, 0, 255]])]).astype(np.uint8)
    # and every grey triple
    g = np.arange(256, dtype=np.uint8)
    bgr = np.ascontiguousarray(np.concatenate([bgr, np.repeat(g[:, None], 3, 1)]))
    out = np.empty(len(bgr), dtype=np.uint8)
    hc.hc_grey(ctypes.c_long(len(bgr)), P(bgr), P(out))
    np.testing.assert_array_equal(out, cvt.grey(bgr))
    np.testing.assert_array_equal(out[-256:], g)


def _test_image(seed=1, size=(96, 80)):
    pose = scenes.look_at_pose((3, 3), 12.0, np.radians(20), 0.7, 0.3)
    return scenes.render((3, 3), pose, (140.0, 140.0, 48.0, 40.0, 0.0, 0.0), size, supersample=2, blur=0.8, noise=2.0, seed=seed)


def test_rect_subpix_patches_with_replicated_borders(hc):
    img = _test_image()
    H, W = img.shape
    for cx, cy in [(40.3, 30.7), (1.2, 2.9), (W - 1.5, H - 0.2), (-0.4, 5.5), (20.0, 20.0), (W + 3.25, -2.5)]:
        for pw, ph in [(13, 13), (9, 15)]:
            out = np.empty(pw * ph, dtype=np.float32)
            hc.hc_rect_subpix(P(img), W, H, cx, cy, pw, ph, P(out))
            np.testing.assert_allclose(out.reshape(ph, pw), cvt.rect_subpix(img, cx, cy, pw, ph), rtol=0, atol=1e-6)


def test_subpix_iteration_and_refinement(hc):
    img = _test_image()
    H, W = img.shape
    mask = np.empty(11 * 11, dtype=np.float32)
    hc.hc_subpix_mask(5, 5, P(mask))
    np.testing.assert_array_equal(mask.reshape(11, 11), cvt.subpix_mask(5, 5))
    starts = np.array([[40.6, 31.2], [47.5, 42.1], [3.0, 4.0], [60.2, 35.9], [W - 2.0, H - 3.0]], dtype=np.float32)
    for x, y in starts:
        xy = np.array([x, y], dtype=np.float32)
        ok = hc.hc_subpix_iteration(P(img), W, H, 5, 5, P(xy))
        r = cvt.subpix_iteration(img, x, y, 5, 5)
        assert bool(ok) == (r is not None)
        if r is not None:
            np.testing.assert_allclose(xy, r[:2], rtol=0, atol=1e-6)
    out = np.empty_like(starts)
    hc.hc_corner_subpix(P(img), W, H, len(starts), P(starts), 5, 5, P(out))
    np.testing.assert_allclose(out, cvt.corner_subpix(img, starts, 5, 5), rtol=0, atol=1e-4)


def test_four_point_transform_warp_and_correlation(hc):
    img = _test_image()
    H, W = img.shape
    rng = np.random.default_rng(3)
    tgt = np.array([[0, 40], [0, 0], [40, 0], [40, 40]], dtype=np.float64)
    tpl = cvt.template()
    for _ in range(20):
        quad = np.array([[10, 60], [12, 8], [70, 12], [66, 70]], dtype=np.float64) + rng.uniform(-8, 8, (4, 2))
        quad = quad.astype(np.float32).astype(np.float64)
        M = np.empty(9)
        assert hc.hc_persp4(P(np.ascontiguousarray(tgt)), P(np.ascontiguousarray(quad)), P(M)) == 1
        Mr = cvt.perspective_transform(tgt, quad)
        np.testing.assert_allclose(M.reshape(3, 3), Mr, rtol=1e-12, atol=1e-12 * np.abs(Mr).max())
        np.testing.assert_array_equal(M.reshape(3, 3), cvt.perspective_transform_ge(tgt, quad))   # the kernels' elimination, bit for bit
        reg = np.empty(1600, dtype=np.uint8)
        hc.hc_warp(P(img), W, H, P(M), P(reg))
        np.testing.assert_array_equal(reg.reshape(40, 40), cvt.warp_region(img, M.reshape(3, 3)))
        c = hc.hc_pearson(1600, P(reg), P(np.ascontiguousarray(tpl.ravel())))
        assert abs(c - cvt.correlation(reg.reshape(40, 40), tpl)) < 1e-12
    flat = np.full(1600, 77, dtype=np.uint8)
    assert hc.hc_pearson(1600, P(flat), P(np.ascontiguousarray(tpl.ravel()))) == 0.0
    t = np.empty(1600, dtype=np.uint8)
    hc.hc_template(P(t))
    np.testing.assert_array_equal(t.reshape(40, 40), tpl)


def test_device_homography_matches_numpy_dlt(hc):
    rng = np.random.default_rng(5)
    H = np.array([[25.0, 3.0, 100.0], [-2.0, 22.0, 80.0], [0.001, 0.002, 1.0]])
    xy = np.mgrid[1:8, 3:13].T.reshape(-1, 2).astype(np.float64)
    p = np.c_[xy, np.ones(len(xy))] @ H.T
    uv = p[:, :2] / p[:, 2:] + rng.normal(0, 0.3, (len(xy), 2))
    out = np.empty(9)
    hc.hc_homography(P(np.ascontiguousarray(xy)), P(np.ascontiguousarray(uv)), len(xy), P(out))
    np.testing.assert_allclose(out.reshape(3, 3), detection.homography_dlt(xy, uv), rtol=1e-9, atol=1e-12)


def test_input_checks():
    g = np.zeros((64, 64), dtype=np.uint8)
    with pytest.raises(ValueError):
        detection.detect_chessboard(g.astype(np.float32))
    with pytest.raises(ValueError):
        detection.detect_chessboard(np.zeros((64, 64, 4), dtype=np.uint8))
    with pytest.raises(ValueError):
        detection.detect_chessboard(np.zeros(64, dtype=np.uint8))
    with pytest.raises(ValueError):
        detection.detect_chessboard(g, board_shape=(1, 5))
    with pytest.raises(ValueError):
        detection.detect_chessboards(np.zeros((2, 64, 64, 2), dtype=np.uint8))
    with pytest.raises(ValueError):
        detection.detect_chessboards([g, np.zeros((32, 64), dtype=np.uint8)])
    with pytest.raises(ValueError):
        detection.detect_chessboard(np.zeros((7, 64), dtype=np.uint8))
    with pytest.raises(ValueError):
        detection.detect_chessboards(np.zeros((2, 64, 5), dtype=np.uint8))
    with pytest.raises(ValueError):
        detection.reorder_chessboard_corners(np.zeros((4, 4), dtype=np.uint8), np.zeros((4, 2)), (2, 2))
    with pytest.raises(NotImplementedError):
        detection.detect_chessboard(g, board_shape=(31, 5))
    with pytest.raises(NotImplementedError):
        detection.detect_chessboard(g, board_shape=(30, 30))
    with pytest.raises(NotImplementedError):
        detection.detect_chessboard(g, subpix_winSize=(16, 5))
    with pytest.raises(NotImplementedError):
        detection.detect_chessboard(np.zeros((8, 4097), dtype=np.uint8))
    with pytest.raises(NotImplementedError):
        detection.detect_chessboard(g, scale_factor=2)


def test_no_gpu_is_a_loud_error():
    n = ctypes.c_int()
    rc = ops.load_library().mcba_device_count(ctypes.byref(n))
    if rc == 0 and n.value > 0:
        pytest.skip("a GPU is visible here")
    g = np.zeros((64, 64), dtype=np.uint8)
    uv = np.zeros((70, 2), dtype=np.float32)
    for call in (lambda: detection.detect_chessboard(g), lambda: detection.detect_chessboards(g[None]), lambda: detection.corner_subpix(g, uv[:3]),
                 lambda: detection.reorder_chessboard_corners(g, uv, (7, 10))):
        with pytest.raises(ops.McbaError):
            call()
