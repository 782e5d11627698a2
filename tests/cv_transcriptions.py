"""numpy transcriptions of the OpenCV routines the chessboard detection contract names (test helper; the product never imports it).

cornerSubPix / getRectSubPix follow OpenCV's published iteration: the float32 patch is formed operation by operation in float32, the sums
in float64.  The warp is bilinear with border value 0 and rounded to uint8; the score is np.corrcoef."""
import numpy as np

f32 = np.float32


def grey(bgr):
    b, g, r = (bgr[..., k].astype(np.uint32) for k in range(3))
    return ((1868 * b + 9617 * g + 4899 * r + 8192) >> 14).astype(np.uint8)


def rect_subpix(img, cx, cy, pw, ph):
    """getRectSubPix(img, (pw, ph), (cx, cy)) into float32, replicated borders."""
    H, W = img.shape
    x0 = f32(cx) - f32(f32(pw - 1) * f32(0.5))
    y0 = f32(cy) - f32(f32(ph - 1) * f32(0.5))
    fx, fy = np.floor(x0), np.floor(y0)
    a, b = f32(x0 - fx), f32(y0 - fy)
    one = f32(1)
    a11, a12, a21, a22 = f32((one - a) * (one - b)), f32(a * (one - b)), f32((one - a) * b), f32(a * b)
    ix = int(fx) + np.arange(pw)
    iy = int(fy) + np.arange(ph)
    xa, xb = np.clip(ix, 0, W - 1), np.clip(ix + 1, 0, W - 1)
    ya, yb = np.clip(iy, 0, H - 1), np.clip(iy + 1, 0, H - 1)
    im = img.astype(np.float32)
    p00, p01 = im[np.ix_(ya, xa)], im[np.ix_(ya, xb)]
    p10, p11 = im[np.ix_(yb, xa)], im[np.ix_(yb, xb)]
    return ((p00 * a11 + p01 * a12) + p10 * a21) + p11 * a22


def subpix_mask(w, h):
    """OpenCV 4's mask: float32 y = (i - h) / h and x = (j - w) / w, float32 exp(-y y) and exp(-x x), their float32 product (the exponentials
    rounded once from float64: the correctly rounded float exp)."""
    y = (np.arange(2 * h + 1) - h).astype(np.float32) / f32(h)
    x = (np.arange(2 * w + 1) - w).astype(np.float32) / f32(w)
    vy = np.exp((-y * y).astype(np.float64)).astype(np.float32)
    vx = np.exp((-x * x).astype(np.float64)).astype(np.float32)
    return vy[:, None] * vx[None, :]


def subpix_iteration(img, x, y, w, h):
    """One cornerSubPix update from the float32 corner (x, y): (x', y', err) or None when det <= DBL_EPSILON^2."""
    patch = rect_subpix(img, x, y, 2 * w + 3, 2 * h + 3)
    m = subpix_mask(w, h).astype(np.float64)
    tgx = (patch[1:-1, 2:] - patch[1:-1, :-2]).astype(np.float64)
    tgy = (patch[2:, 1:-1] - patch[:-2, 1:-1]).astype(np.float64)
    gxx, gxy, gyy = tgx * tgx * m, tgx * tgy * m, tgy * tgy * m
    py, px = np.mgrid[-h:h + 1, -w:w + 1].astype(np.float64)
    a, b, c = gxx.sum(), gxy.sum(), gyy.sum()
    bb1 = (gxx * px + gxy * py).sum()
    bb2 = (gxy * px + gyy * py).sum()
    det = a * c - b * b
    if abs(det) <= np.finfo(np.float64).eps ** 2:
        return None
    scale = 1.0 / det
    nx = f32(float(x) + c * scale * bb1 - b * scale * bb2)
    ny = f32(float(y) - b * scale * bb1 + a * scale * bb2)
    err = float(f32(f32(nx - f32(x)) ** 2 + f32(ny - f32(y)) ** 2))
    return nx, ny, err


def corner_subpix(img, corners, w, h, max_iter=30, eps=0.001):
    """cv2.cornerSubPix(img, corners, (w, h), (-1, -1), (EPS + MAX_ITER, max_iter, eps)) -> float32 (n, 2)."""
    H, W = img.shape
    out = np.asarray(corners, dtype=np.float32).reshape(-1, 2).copy()
    for k in range(out.shape[0]):
        x0, y0 = out[k]
        x, y = x0, y0
        for _ in range(max_iter):
            r = subpix_iteration(img, x, y, w, h)
            if r is None:
                break
            x, y, err = r
            if x < 0 or x >= W or y < 0 or y >= H:
                break
            if not err > eps * eps:
                break
        if abs(x - x0) > w or abs(y - y0) > h:
            x, y = x0, y0
        out[k] = (x, y)
    return out


def perspective_transform(src, dst):
    """cv2.getPerspectiveTransform(src, dst): 3 x 3 M with M (src, 1) ~ (dst, 1), M[2, 2] = 1."""
    src = np.asarray(src, dtype=np.float64).reshape(4, 2)
    dst = np.asarray(dst, dtype=np.float64).reshape(4, 2)
    A = np.zeros((8, 8))
    rhs = np.zeros(8)
    for k, ((x, y), (u, v)) in enumerate(zip(src, dst)):
        A[k] = [x, y, 1, 0, 0, 0, -x * u, -y * u]
        A[k + 4] = [0, 0, 0, x, y, 1, -x * v, -y * v]
        rhs[k], rhs[k + 4] = u, v
    return np.append(np.linalg.solve(A, rhs), 1.0).reshape(3, 3)


def perspective_transform_ge(src, dst):
    """The same transform as the detection kernels solve it: the 8 x 8 system of perspective_transform by Gaussian elimination with partial
    pivoting (first maximum), operation by operation in float64 -- bitwise what csrc/mcba_detect_math.h's persp4 computes."""
    src = [float(v) for v in np.asarray(src, dtype=np.float64).ravel()]
    dst = [float(v) for v in np.asarray(dst, dtype=np.float64).ravel()]
    A = [[0.0] * 9 for _ in range(8)]
    for k in range(4):
        x, y, u, v = src[2 * k], src[2 * k + 1], dst[2 * k], dst[2 * k + 1]
        A[k] = [x, y, 1.0, 0.0, 0.0, 0.0, -x * u, -y * u, u]
        A[k + 4] = [0.0, 0.0, 0.0, x, y, 1.0, -x * v, -y * v, v]
    for c in range(8):
        p = c
        for r in range(c + 1, 8):
            if abs(A[r][c]) > abs(A[p][c]):
                p = r
        A[c], A[p] = A[p], A[c]
        for r in range(c + 1, 8):
            f = A[r][c] / A[c][c]
            for k in range(c, 9):
                A[r][k] -= f * A[c][k]
    M = [0.0] * 9
    for c in range(7, -1, -1):
        v = A[c][8]
        for k in range(c + 1, 8):
            v -= A[c][k] * M[k]
        M[c] = v / A[c][c]
    M[8] = 1.0
    return np.array(M).reshape(3, 3)


def warp_region(img, M, size=40):
    """size x size uint8 region: pixel (x, y) = bilinear value of img at M (x, y, 1) (border 0), rounded half to even."""
    H, W = img.shape
    y, x = np.mgrid[0:size, 0:size].astype(np.float64)
    X = M[0, 0] * x + M[0, 1] * y + M[0, 2]
    Y = M[1, 0] * x + M[1, 1] * y + M[1, 2]
    Z = M[2, 0] * x + M[2, 1] * y + M[2, 2]
    sx, sy = X / Z, Y / Z
    fx, fy = np.floor(sx), np.floor(sy)
    ax, ay = sx - fx, sy - fy
    x0, y0 = fx.astype(np.int64), fy.astype(np.int64)

    def tap(xx, yy):
        ok = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
        return np.where(ok, img[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)].astype(np.float64), 0.0)

    v = (1.0 - ay) * ((1.0 - ax) * tap(x0, y0) + ax * tap(x0 + 1, y0)) + ay * ((1.0 - ax) * tap(x0, y0 + 1) + ax * tap(x0 + 1, y0 + 1))
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def template(size=40):
    y, x = np.mgrid[0:size, 0:size]
    return np.where((x - 10) ** 2 + (y - 10) ** 2 <= 100, 0, 255).astype(np.uint8)


def correlation(region, tpl):
    if np.std(region) > 0:
        return float(np.corrcoef(region.ravel(), tpl.ravel())[0, 1])
    return 0.0


def anchor_scores(img, quads):
    """The four regions and scores of reorder_chessboard_corners for the given source quads (4, 4, 2)."""
    tgt = np.float32([[0, 40], [0, 0], [40, 0], [40, 40]])
    tpl = template()
    regions, scores = [], []
    for q in np.asarray(quads, dtype=np.float32).reshape(4, 4, 2):
        M = perspective_transform_ge(tgt, q)
        r = warp_region(img, M)
        regions.append(r)
        scores.append(correlation(r, tpl))
    return np.array(regions), np.array(scores)
