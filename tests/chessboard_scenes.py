"""A small chessboard renderer for the detection tests (torch: on the GPU in the GPU tier, on the host for small CPU images).

A board of board_shape = (cols, rows) inner corners and square size 1 lies in its plane z = 0: inner corner (c, r) at (c, r, 0), the squares
from -1 to cols (x) and -1 to rows (y), square (a, b) black when a + b is even.  White paper around it reaches 1 square beyond the squares
in x and 2.5 in y, so that the four anchor regions of reorder_chessboard_corners lie on paper; the anchor is a dark disc of radius 1/2
centred on (-1/2, -5/2).  The camera is synth's model: pinhole fx, fy, cx, cy and radial k1, k2, the board pose (rotation vector, t) taking
board points into the camera frame.  Pixel (i, j) covers [j - 1/2, j + 1/2] x [i - 1/2, i + 1/2]: its centre is (u, v) = (j, i).
"""
import math

import numpy as np
import torch

WHITE, BLACK, BACKGROUND = 215.0, 35.0, 110.0
PAPER_X = (-2.0, 1.0)      # paper from -2 to cols + 1
PAPER_Y = (-3.5, 2.5)      # and from -3.5 to rows + 2.5
ANCHOR = (-0.5, -2.5, 0.5)


def rotation(rv):
    rv = np.asarray(rv, dtype=np.float64)
    th = np.linalg.norm(rv)
    if th == 0:
        return np.eye(3)
    k = rv / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * K @ K


def project(points, pose, cam):
    """board points (n, 3) -> pixels (n, 2) through pose (6,) and cam (fx, fy, cx, cy, k1, k2)."""
    fx, fy, cx, cy, k1, k2 = cam
    Xc = np.asarray(points, dtype=np.float64) @ rotation(pose[:3]).T + np.asarray(pose[3:])
    a, b = Xc[:, 0] / Xc[:, 2], Xc[:, 1] / Xc[:, 2]
    s = a * a + b * b
    d = 1 + k1 * s + k2 * s * s
    return np.stack([fx * a * d + cx, fy * b * d + cy], -1)


def corners(board_shape, pose, cam, square=1.0):
    cols, rows = board_shape
    g = np.mgrid[0:rows, 0:cols].reshape(2, -1)
    pts = np.stack([g[1], g[0], np.zeros(rows * cols)], -1) * square
    return project(pts, pose, cam)


def paper_outline(board_shape, pose, cam, n=40):
    """Points along the paper's border (and so around the anchor): for the 'fully inside the image' test."""
    cols, rows = board_shape
    x0, x1 = PAPER_X[0], cols + PAPER_X[1]
    y0, y1 = PAPER_Y[0], rows + PAPER_Y[1]
    t = np.linspace(0, 1, n)
    e = [np.stack([x0 + (x1 - x0) * t, np.full(n, y0)], -1), np.stack([x0 + (x1 - x0) * t, np.full(n, y1)], -1),
         np.stack([np.full(n, x0), y0 + (y1 - y0) * t], -1), np.stack([np.full(n, x1), y0 + (y1 - y0) * t], -1)]
    p = np.concatenate(e)
    return project(np.c_[p, np.zeros(len(p))], pose, cam)


def min_square_px(board_shape, pose, cam):
    """The shortest projected edge between neighbouring corners of the squares (the outer ring included)."""
    cols, rows = board_shape
    g = np.mgrid[-1:rows + 1, -1:cols + 1].astype(np.float64)
    pts = np.stack([g[1].ravel(), g[0].ravel(), np.zeros(g[0].size)], -1)
    uv = project(pts, pose, cam).reshape(rows + 2, cols + 2, 2)
    dx = np.linalg.norm(np.diff(uv, axis=1), axis=-1).min()
    dy = np.linalg.norm(np.diff(uv, axis=0), axis=-1).min()
    return float(min(dx, dy))


def render(board_shape, pose, cam, size, *, supersample=4, blur=0.0, noise=0.0, seed=0, device="cpu", anchor=True, background=BACKGROUND,
           dots=None, pole=None, bgr=False):
    """uint8 image (H, W) (or (H, W, 3) BGR with equal channels) of the board.

    dots: (pitch_px, radius_px, value) bright dots on a grid over the background (LED arrays); pole: (u0, u1, value) a vertical bar across
    the whole image between columns u0 and u1, drawn over everything."""
    W, H = size
    fx, fy, cx, cy, k1, k2 = (float(v) for v in cam)
    cols, rows = board_shape
    dt = torch.float64
    S = int(supersample)
    off = (torch.arange(S, dtype=dt, device=device) + 0.5) / S - 0.5
    v = torch.arange(H, dtype=dt, device=device)[:, None] + off[None, :]
    u = torch.arange(W, dtype=dt, device=device)[:, None] + off[None, :]
    V = v.reshape(-1)[:, None].expand(H * S, W * S)
    U = u.reshape(-1)[None, :].expand(H * S, W * S)
    xd, yd = (U - cx) / fx, (V - cy) / fy
    x, y = xd.clone(), yd.clone()
    for _ in range(20):  # undistort: x d(x, y) = xd
        s = x * x + y * y
        d = 1 + k1 * s + k2 * s * s
        x, y = xd / d, yd / d
    R = rotation(pose[:3])
    A = np.c_[R[:, 0], R[:, 1], np.asarray(pose[3:], dtype=np.float64)]   # (x, y, 1) ~ A (X, Y, 1)
    Ai = torch.tensor(np.linalg.inv(A), dtype=dt, device=device)
    X = Ai[0, 0] * x + Ai[0, 1] * y + Ai[0, 2]
    Y = Ai[1, 0] * x + Ai[1, 1] * y + Ai[1, 2]
    Z = Ai[2, 0] * x + Ai[2, 1] * y + Ai[2, 2]
    front = Z > 0
    X, Y = X / Z, Y / Z
    img = torch.full_like(X, float(background))
    if dots is not None:
        pitch, radius, value = dots
        du = torch.remainder(U + 0.5 * pitch, pitch) - 0.5 * pitch
        dv = torch.remainder(V + 0.5 * pitch, pitch) - 0.5 * pitch
        img = torch.where(du * du + dv * dv <= radius * radius, torch.full_like(img, float(value)), img)
    paper = front & (X >= PAPER_X[0]) & (X <= cols + PAPER_X[1]) & (Y >= PAPER_Y[0]) & (Y <= rows + PAPER_Y[1])
    img = torch.where(paper, torch.full_like(img, WHITE), img)
    fa, fb = torch.floor(X), torch.floor(Y)
    sq = paper & (fa >= -1) & (fa <= cols - 1) & (fb >= -1) & (fb <= rows - 1)
    black = sq & (torch.remainder(fa + fb, 2) == 0)
    img = torch.where(black, torch.full_like(img, BLACK), img)
    if anchor:
        ax, ay, ar = ANCHOR
        disc = paper & ((X - ax) ** 2 + (Y - ay) ** 2 <= ar * ar)
        img = torch.where(disc, torch.full_like(img, BLACK), img)
    if pole is not None:
        u0, u1, value = pole
        img = torch.where((U >= u0) & (U <= u1), torch.full_like(img, float(value)), img)
    img = img.reshape(H, S, W, S).mean(dim=(1, 3))
    if blur > 0:
        r = int(math.ceil(3 * blur))
        k = torch.exp(-0.5 * (torch.arange(-r, r + 1, dtype=dt, device=device) / blur) ** 2)
        k = k / k.sum()
        p = torch.nn.functional.pad(img[None, None], (r, r, r, r), mode="replicate")
        p = torch.nn.functional.conv2d(p, k.view(1, 1, 1, -1))
        img = torch.nn.functional.conv2d(p, k.view(1, 1, -1, 1))[0, 0]
    if noise > 0:
        g = torch.Generator(device=device)
        g.manual_seed(int(seed))
        img = img + noise * torch.randn(img.shape, generator=g, dtype=dt, device=device)
    out = torch.clamp(torch.round(img), 0, 255).to(torch.uint8).cpu().numpy()
    return np.repeat(out[..., None], 3, axis=2) if bgr else out


def look_at_pose(board_shape, distance, tilt, tilt_axis, spin, shift=(0.0, 0.0)):
    """A board pose: the board's centre at `distance` on the optical axis (plus a lateral shift), rotated in its plane by `spin` and tilted
    by `tilt` about the in-plane axis at angle `tilt_axis` (radians)."""
    cols, rows = board_shape
    centre = np.array([(cols - 1) / 2.0, (rows - 1) / 2.0 - 0.5, 0.0])
    Rz = rotation([0, 0, spin])
    axis = np.array([math.cos(tilt_axis), math.sin(tilt_axis), 0.0])
    Rt = rotation(axis * tilt)
    R = Rt @ Rz
    t = np.array([shift[0], shift[1], distance]) - R @ centre
    w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    th = math.acos(max(-1.0, min(1.0, (np.trace(R) - 1) / 2)))
    rv = w * th / (2 * math.sin(th)) if th > 1e-12 else np.zeros(3)
    if abs(math.pi - th) < 1e-6:
        raise ValueError("rotation by pi: pick another spin")
    return np.r_[rv, t]


def random_view(rng, board_shape, size, max_tilt_deg=60.0):
    """A random camera and board pose for an image of `size` = (W, H): the board fills 30..75 % of the shorter side."""
    W, H = size
    f = rng.uniform(0.9, 1.4) * W
    cam = (f, f * rng.uniform(0.99, 1.01), W / 2 + rng.uniform(-10, 10), H / 2 + rng.uniform(-10, 10), rng.uniform(-0.1, 0.0), rng.uniform(0.0, 0.03))
    cols, rows = board_shape
    extent = max(cols + 3, rows + 6)
    frac = rng.uniform(0.3, 0.75)
    distance = f * extent / (frac * min(W, H))
    spin = rng.uniform(-math.pi, math.pi) * 0.999
    tilt = math.radians(rng.uniform(0, max_tilt_deg))
    shift = (rng.uniform(-0.15, 0.15) * W * distance / f, rng.uniform(-0.15, 0.15) * H * distance / f)
    return look_at_pose(board_shape, distance, tilt, rng.uniform(0, 2 * math.pi), spin, shift), cam


def eligible(board_shape, pose, cam, size, scale_factor=1.0, margin=2.0, min_square=10.0):
    W, H = size
    o = paper_outline(board_shape, pose, cam)
    inside = (o[:, 0] >= margin).all() and (o[:, 0] <= W - 1 - margin).all() and (o[:, 1] >= margin).all() and (o[:, 1] <= H - 1 - margin).all()
    return bool(inside and min_square_px(board_shape, pose, cam) * scale_factor >= min_square)
