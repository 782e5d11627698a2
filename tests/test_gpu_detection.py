"""Chessboard detection on the MI355X: the refinement and anchor seams against the numpy transcriptions, detection on rendered views,
negatives, consistency, and detect -> calibrate() -> bundle_adjust() end to end."""
import contextlib
import io
import math

import numpy as np
import pytest

import chessboard_scenes as scenes
import cv_transcriptions as cvt
import multicam_calibration_amd as m
from multicam_calibration_amd import detection

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _view(board_shape, size, seed, tilt=35.0, scale_factor=1.0):
    rng = np.random.default_rng(seed)
    for _ in range(200):
        pose, cam = scenes.random_view(rng, board_shape, size, max_tilt_deg=tilt)
        if scenes.eligible(board_shape, pose, cam, size, scale_factor):
            return pose, cam
    raise AssertionError("no eligible view")


def _render(board_shape, pose, cam, size, seed=0, **kw):
    kw.setdefault("blur", 0.8)
    kw.setdefault("noise", 2.0)
    return scenes.render(board_shape, pose, cam, size, seed=seed, device=DEV, **kw)


def _truth_error(uvs, truth):
    return np.linalg.norm(np.asarray(uvs, dtype=np.float64) - truth, axis=-1)


# ---------------------------------------------------------------- 1. refinement seam
def test_subpix_equals_the_transcription():
    rng = np.random.default_rng(1)
    size = (640, 480)
    pose, cam = _view((7, 10), size, 11)
    img = _render((7, 10), pose, cam, size)
    truth = scenes.corners((7, 10), pose, cam)
    start = (truth + rng.uniform(1, 3, truth.shape) * rng.choice([-1, 1], truth.shape)).astype(np.float32)
    # corners near the border, and one that wanders off (start on a flat area: moved too far -> the start point)
    extra = np.array([[2.0, 3.0], [size[0] - 2.5, size[1] - 1.5], [1.0, size[1] / 2], [5.0, 5.0]], dtype=np.float32)
    start = np.concatenate([start, extra])
    got = detection.corner_subpix(img, start, (5, 5))
    ref = cvt.corner_subpix(img, start, 5, 5)
    assert np.abs(got - ref).max() <= 1e-3, np.abs(got - ref).max()
    assert _truth_error(got[:70], truth).max() < 0.3
    for w in ((3, 3), (7, 4)):
        np.testing.assert_allclose(detection.corner_subpix(img, start[:10], w), cvt.corner_subpix(img, start[:10], *w), rtol=0, atol=1e-3)


# ---------------------------------------------------------------- 2. anchor seam
@pytest.mark.parametrize("board_shape", [(7, 10), (5, 7)])
def test_anchor_equals_the_transcription_and_orders_every_rotation(board_shape):
    size = (800, 800)
    cols, rows = board_shape
    cam = (900.0, 900.0, 400.0, 400.0, 0.0, 0.0)
    for k, spin in enumerate([0.0, math.pi / 2, math.pi * 0.999, -math.pi / 2]):
        pose = scenes.look_at_pose(board_shape, 40.0, math.radians(20), 0.5, spin)
        img = _render(board_shape, pose, cam, size, seed=k)
        truth = scenes.corners(board_shape, pose, cam)
        grid = truth.reshape(rows, cols, 2)
        # what a detector hands over: the grid in some flip of the true order (each of the four)
        for fr in (False, True):
            for fc in (False, True):
                g = grid[::-1] if fr else grid
                g = g[:, ::-1] if fc else g
                uvs = np.ascontiguousarray(g.reshape(-1, 2))
                out, sorted_scores, (quads, regions, tpl, scores) = detection.reorder_chessboard_corners(img, uvs, board_shape)
                np.testing.assert_array_equal(out, truth)
                # (the transcription solves the 4-point transform by the kernels' own elimination, so the regions agree bit for bit)
                reg_ref, sc_ref = cvt.anchor_scores(img, np.concatenate(quads))
                np.testing.assert_array_equal(np.asarray(regions), reg_ref)
                np.testing.assert_allclose(scores, sc_ref, rtol=0, atol=1e-6)
                assert sorted_scores[0] - sorted_scores[1] > 0.2
                # the quads are the reference's extended grid (exact grid: the DLT reproduces it)
                ext = detection.extend_grid(g, 3, 1)
                np.testing.assert_allclose(quads[0][0], np.float32([ext[2, 0], ext[0, 0], ext[0, 2], ext[2, 2]]), rtol=0, atol=1e-3)


# ---------------------------------------------------------------- 3. detection on rendered views
def _view_set():
    views = []
    rng = np.random.default_rng(2024)
    for board_shape in [(5, 7), (7, 10)]:
        for size in [(640, 480), (1280, 1024)]:
            for sf in (1.0, 0.5):
                n = 0
                while n < 28:
                    pose, cam = scenes.random_view(rng, board_shape, size, max_tilt_deg=60.0)
                    if not scenes.eligible(board_shape, pose, cam, size, sf):
                        continue
                    views.append((board_shape, size, sf, pose, cam, int(rng.integers(1 << 30))))
                    n += 1
    return views


def test_detection_on_rendered_views():
    views = _view_set()
    assert len(views) >= 200
    accepted, errors, wrong = 0, [], 0
    for board_shape, size, sf, pose, cam, seed in views:
        img = _render(board_shape, pose, cam, size, seed=seed)
        r = detection.detect_chessboard(img, board_shape=board_shape, scale_factor=sf)
        if r is None:
            continue
        uvs, scores = r
        assert uvs.dtype == np.float32 and uvs.shape == (board_shape[0] * board_shape[1], 2)
        assert scores.dtype == np.float64 and scores.shape == (4,) and np.all(np.diff(scores) <= 0)
        e = _truth_error(uvs, scenes.corners(board_shape, pose, cam))
        side = scenes.min_square_px(board_shape, pose, cam)
        if e.max() >= 0.5 * side:
            wrong += 1
            continue
        accepted += 1
        errors.append(e)
    e = np.concatenate(errors)
    print("accepted %d / %d, median %.4f px, max %.4f px" % (accepted, len(views), np.median(e), e.max()))
    assert wrong == 0
    assert accepted >= 0.95 * len(views)
    assert np.median(e) <= 0.05
    assert e.max() <= 0.3


# ---------------------------------------------------------------- 3b. square boards, and a pole over the margin
def _right_handed(uvs, board_shape):
    """cross(d_col, d_row) > 0 (u right, v down) at every cell of the returned order."""
    g = np.asarray(uvs, dtype=np.float64).reshape(board_shape[1], board_shape[0], 2)
    dc = g[:-1, 1:] - g[:-1, :-1]
    dr = g[1:, :-1] - g[:-1, :-1]
    return bool(np.all(dc[..., 0] * dr[..., 1] - dc[..., 1] * dr[..., 0] > 0))


def test_square_board_every_rotation():
    """Square boards (contract rule 3): the lattice is laid out right-handed and the anchor is scored on that layout and its transpose, so
    a square board comes back in the true order whatever its in-plane rotation -- the transposed layout is the one that wins at 90 and 270
    degrees."""
    bs = (6, 6)
    size = (800, 800)
    cam = (900.0, 900.0, 400.0, 400.0, -0.03, 0.01)
    frames, truths, sides = [], [], []
    for spin in (0.0, math.pi / 2, math.pi * 0.999, -math.pi / 2):
        for tilt, axis in ((0.0, 0.0), (25.0, 0.7), (45.0, 2.2)):
            pose = scenes.look_at_pose(bs, 22.0, math.radians(tilt), axis, spin)
            assert scenes.eligible(bs, pose, cam, size)
            frames.append(_render(bs, pose, cam, size, seed=len(frames)))
            truths.append(scenes.corners(bs, pose, cam))
            sides.append(scenes.min_square_px(bs, pose, cam))
    uvs, scores, status = detection.detect_chessboards(np.stack(frames), board_shape=bs)
    assert (status == 1).sum() >= len(frames) - 1, status
    for i in np.flatnonzero(status == 1):
        e = _truth_error(uvs[i], truths[i])
        assert e.max() <= 0.3, (i, e.max(), sides[i])
        assert _right_handed(uvs[i], bs)
    # without the anchor: every assembled lattice is laid out right-handed
    nr_uvs, _, nr_status = detection.detect_chessboards(np.stack(frames), board_shape=bs, reorder=False)
    assert (nr_status == 1).sum() >= len(frames) - 1
    for i in np.flatnonzero(nr_status == 1):
        assert _right_handed(nr_uvs[i], bs)
    # the anchor only permutes the refined lattice
    for i in np.flatnonzero(status == 1):
        np.testing.assert_array_equal(np.sort(nr_uvs[i].reshape(-1)), np.sort(uvs[i].reshape(-1)))


def test_pole_over_the_margin():
    """A dark pole across the image, over the white margin beside the board (not over a corner or an anchor region): still detected."""
    bs = (7, 10)
    size = (1280, 1024)
    cam = (1100.0, 1100.0, 640.0, 512.0, -0.05, 0.02)
    pose = scenes.look_at_pose(bs, 24.0, math.radians(10), 0.0, 0.0)
    assert scenes.eligible(bs, pose, cam, size)
    mid = (bs[1] - 1) / 2.0
    u = scenes.project(np.array([[bs[0] + 0.35, mid, 0.0], [bs[0] + 0.65, mid, 0.0]]), pose, cam)[:, 0]
    img = _render(bs, pose, cam, size, pole=(u.min(), u.max(), 60))
    assert (img[:, int(u.mean())] < 80).mean() > 0.9   # the pole is there
    r = detection.detect_chessboard(img, board_shape=bs)
    assert r is not None
    assert _truth_error(r[0], scenes.corners(bs, pose, cam)).max() <= 0.3


# ---------------------------------------------------------------- 4. negatives
def test_negatives_are_never_accepted():
    size = (640, 480)
    bs = (7, 10)
    pose, cam = _view(bs, size, 5, tilt=20.0)
    frames = []
    rng = np.random.default_rng(9)
    frames.append(np.full((480, 640), 128, np.uint8))
    frames.append(np.clip(rng.normal(128, 40, (480, 640)), 0, 255).astype(np.uint8))
    far = np.r_[0.0, 0.0, 0.0, 0.0, 0.0, -1000.0]  # (behind the camera: background only)
    frames.append(scenes.render(bs, far, cam, size, background=20, dots=(24, 5, 240), device=DEV))
    frames.append(scenes.render(bs, far, cam, size, background=10, dots=(40, 9, 250), blur=1.0, device=DEV))
    frames.append(_render((7, 11), *_view((7, 11), size, 6, tilt=20.0), size))
    frames.append(_render((7, 9), *_view((7, 9), size, 7, tilt=20.0), size))
    frames.append(_render((8, 10), *_view((8, 10), size, 8, tilt=20.0), size))
    # the board cut by the image edge: shifted right by 0.6 of the image width
    p2 = pose.copy()
    p2[3] += 0.6 * p2[5] * size[0] / cam[0]
    frames.append(_render(bs, p2, cam, size))
    frames.append(_render(bs, pose, cam, size, anchor=False))
    expect_ambiguous = [False] * (len(frames) - 1) + [True]
    uvs, scores, status = detection.detect_chessboards(np.stack(frames), board_shape=bs)
    assert not np.any(status == 1), status
    assert status[-1] == 2 and np.isfinite(scores[-1]).all()
    assert np.isnan(uvs[status != 1]).all()
    assert [bool(s == 2) for s in status] == expect_ambiguous


# ---------------------------------------------------------------- 5. consistency
def _some_frames(n=12, size=(640, 480), bs=(7, 10), seed=3):
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        pose, cam = scenes.random_view(rng, bs, size, max_tilt_deg=50.0)
        if scenes.eligible(bs, pose, cam, size):
            out.append(_render(bs, pose, cam, size, seed=len(out)))
    out[3] = np.full_like(out[3], 90)
    return np.stack(out)


def test_consistency_bgr_batch_runs_chunks():
    frames = _some_frames()
    a = detection.detect_chessboards(frames)
    assert (a[2] == 1).sum() >= 10
    b = detection.detect_chessboards(np.repeat(frames[..., None], 3, axis=3))
    c = detection.detect_chessboards(frames)
    per_frame = frames[0].size + 4 * frames[0].size + (1 << 16)
    d = detection.detect_chessboards(frames, memory_budget=3 * per_frame)   # several chunks
    for other in (b, c, d):
        for x, y in zip(a, other):
            np.testing.assert_array_equal(x, y)
    for i in range(len(frames)):
        r = detection.detect_chessboard(frames[i])
        if a[2][i] == 1:
            np.testing.assert_array_equal(r[0], a[0][i].astype(np.float32))
            np.testing.assert_array_equal(r[1], a[1][i])
        else:
            assert r is None
    half = detection.detect_chessboards(frames, scale_factor=0.5)
    half2 = detection.detect_chessboards(list(frames), scale_factor=0.5)
    for x, y in zip(half, half2):
        np.testing.assert_array_equal(x, y)
    nr = detection.detect_chessboards(frames, reorder=False)
    assert np.isnan(nr[1]).all() and ((nr[2] == 1) >= (a[2] == 1)).all()


# ---------------------------------------------------------------- 6. end to end
def test_detect_calibrate_bundle_adjust():
    C, F = 4, 40
    size = (1280, 1024)
    bs = (7, 10)
    square = 12.5
    rng = np.random.default_rng(77)
    obj = detection.generate_chessboard_objpoints(bs, square).astype(np.float64)
    # a ring of cameras looking at the origin; the board moves about the origin, always facing the camera ring from above
    radius = 600.0
    cams = []
    for c in range(C):
        phi = 2 * math.pi * c / C
        pos = np.array([radius * math.cos(phi), radius * math.sin(phi), 350.0])
        z = -pos / np.linalg.norm(pos)
        x = np.cross(z, [0.0, 0.0, 1.0])
        x /= np.linalg.norm(x)
        R = np.stack([x, np.cross(z, x), z])
        f = 1150.0 + 20 * c
        cams.append(dict(R=R, t=-R @ pos, K=(f, f * 1.002, 640.0 + 5 * c, 512.0 - 4 * c, -0.06, 0.015)))
    uvs = np.full((C, F, len(obj), 2), np.nan)
    for fi in range(F):
        # a board facing the cameras fi % C and fi % C + 1 (about 40 degrees from each), centre near the origin
        ca, cb = cams[fi % C], cams[(fi + 1) % C]
        n = -(ca["R"].T @ ca["t"]) - (cb["R"].T @ cb["t"])
        n /= np.linalg.norm(n)
        zb = -n                                 # the board's +z points away from its viewers
        xb = np.cross([0.0, 0.0, 1.0], zb)
        xb /= np.linalg.norm(xb)
        Rb = np.stack([xb, np.cross(zb, xb), zb], 1) @ scenes.rotation([rng.uniform(-0.25, 0.25), rng.uniform(-0.25, 0.25), rng.uniform(-2.5, 2.5)])
        centre = rng.normal(0, 30, 3)
        tb = centre - Rb @ np.array([(bs[0] - 1) / 2 * square, (bs[1] - 1) / 2 * square, 0.0])
        frames, keep = [], []
        for c, cm in enumerate(cams):
            Rc = cm["R"] @ Rb
            tc = cm["R"] @ tb + cm["t"]
            if Rc[2, 2] < 0.5:   # seen from behind, or tilted by more than 60 degrees
                continue
            pose = np.r_[synth_rotvec(Rc), tc / square]
            if not scenes.eligible(bs, pose, cm["K"], size):
                continue
            frames.append(scenes.render(bs, pose, cm["K"], size, blur=0.8, noise=2.0, seed=fi * 10 + c, device=DEV))
            keep.append(c)
        if frames:
            u, _, st = detection.detect_chessboards(np.stack(frames), board_shape=bs)
            for j, c in enumerate(keep):
                if st[j] == 1:
                    uvs[c, fi] = u[j]
    seen = ~np.isnan(uvs).any(axis=(2, 3))
    assert seen.sum(1).min() >= 8, seen.sum(1)
    with contextlib.redirect_stdout(io.StringIO()):
        np.random.seed(0)
        ext, intr, poses, _ = m.calibrate(uvs, [size] * C, obj, verbose=False)
        ext, intr, poses, use, res = m.bundle_adjust(uvs, ext, intr, obj, poses, n_frames=None, verbose=0)
    for c in range(C):
        K = intr[c][0]
        assert abs(K[0, 0] / cams[c]["K"][0] - 1) < 0.005 and abs(K[1, 1] / cams[c]["K"][1] - 1) < 0.005, (c, K)
    # camera centres in camera 0's frame
    T0 = np.eye(4)
    T0[:3, :3], T0[:3, 3] = cams[0]["R"], cams[0]["t"]
    for c in range(C):
        Rc = scenes.rotation(ext[c][:3])
        centre0 = -Rc.T @ ext[c][3:]
        Tc = np.eye(4)
        Tc[:3, :3], Tc[:3, 3] = cams[c]["R"], cams[c]["t"]
        true0 = (T0 @ np.linalg.inv(Tc))[:3, 3]
        assert np.linalg.norm(centre0 - true0) < 0.01 * radius, (c, centre0, true0)
    cam12 = np.array([np.r_[K[0, 0], K[1, 1], K[0, 2], K[1, 2], d[0], d[1], e] for (K, d), e in zip(intr, ext)])
    proj = m.synth.project(cam12, poses, obj)
    u = uvs[:, use]
    ok = ~np.isnan(u).any(-1)
    err = np.linalg.norm(proj - u, axis=-1)[ok]
    print("end to end: %d detections, median reprojection error %.4f px" % (seen.sum(), np.median(err)))
    assert np.median(err) <= 0.1


def synth_rotvec(R):
    th = math.acos(max(-1.0, min(1.0, (np.trace(R) - 1) / 2)))
    w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    if th < 1e-12:
        return np.zeros(3)
    if math.pi - th < 1e-6:
        raise ValueError("rotation by pi")
    return w * th / (2 * math.sin(th))
