"""Chessboard detection on the GPU: SURVEY.md section 8f-7; reference multicam_calibration/detection.py.

Same names, signatures and return values as the reference's detect_chessboard, reorder_chessboard_corners, extend_grid,
generate_chessboard_objpoints and summarize_detections; extra arguments are keyword-only and come last.  detect_chessboards is the batched
form (one C-ABI crossing per batch; csrc/mcba_detect.hip, include/mcba.h "chessboard detection").  cv2 is not imported.

What the output means:

1. Coordinates: OpenCV's pixel-centre convention.  Pixel (row i, column j) covers [j - 1/2, j + 1/2] x [i - 1/2, i + 1/2].
2. Order: uvs[k] is the image of generate_chessboard_objpoints(board_shape, s)[k] = (k % board_shape[0], k // board_shape[0], 0) s.  The
   anchor that fixes it is a dark disc of radius s / 2 centred on board point (-s / 2, -5 s / 2, 0) (where reorder_chessboard_corners'
   extend_grid(.., 3, 1) and region 0 put the template's disc).  The flips are the reference's: the best region (np.argmax: first maximum)
   2 or 3 flips the rows, 1 or 2 the columns; a frame is rejected when best - second < match_score_min_diff.
3. Square boards: the lattice is laid out right-handed in the image (cross(d_col, d_row) > 0, u right, v down), and the anchor is scored on
   that layout and on its transpose; the one whose best region scores higher is kept (the reference only flips what OpenCV returned).
4. Anchor template: 40 x 40 uint8, 255 except 0 where (x - 10)^2 + (y - 10)^2 <= 100 (317 pixels).  Each region is the image warped through
   the 4-point transform of its quad, bilinear with border value 0, rounded to uint8; its score is the Pearson correlation with the
   template, 0 for a constant region.
5. Refinement: OpenCV's cornerSubPix iteration on the full-resolution grey image whatever scale_factor is (Gaussian mask exp(-x^2) exp(-y^2),
   the (2w + 3) x (2h + 3) bilinear patch with replicated borders, central differences, float32 corner, float64 sums, at most 30 iterations,
   stop once the squared step is <= 0.001^2, exit when det <= DBL_EPSILON^2 or the corner leaves the image, back to the start point if it
   moved more than the half-window).
6. Grey: OpenCV's fixed-point BGR -> Y, (1868 B + 9617 G + 4899 R + 8192) >> 14.
7. scale_factor < 1: the search runs on a bilinear downscale; corners map back as (x + 1/2) / s - 1/2.
8. Determinism: bitwise the same from run to run and between a batch and its frames one at a time.
9. No CPU fallback: without a GPU every function that touches the device raises ops.McbaError.

adaptive_threshold and normalize_image are findChessboardCorners flags: accepted so that the signature matches, without effect here.
"""
import warnings

import numpy as np

from . import ops

MAX_CANDIDATES = 1024    # MCBA_DETECT_MAX_CANDIDATES
MAX_CORNERS = 512        # MCBA_DETECT_MAX_CORNERS
MAX_BOARD_SIDE = 30      # MCBA_DETECT_MAX_BOARD_SIDE
MAX_WINDOW = 15          # MCBA_DETECT_MAX_WINDOW
MAX_IMAGE_SIDE = 4096    # MCBA_DETECT_MAX_IMAGE_SIDE
MIN_IMAGE_SIDE = 8       # the library's smallest image side
TEMPLATE_SIZE = 40
STATUS_NONE, STATUS_ACCEPTED, STATUS_AMBIGUOUS = 0, 1, 2
_STATUS_OVERFLOW = 3


def _board(board_shape):
    cols, rows = (int(v) for v in board_shape)
    if cols < 2 or rows < 2:
        raise ValueError("board_shape: each dimension must be at least 2")
    if cols > MAX_BOARD_SIDE or rows > MAX_BOARD_SIDE or cols * rows > MAX_CORNERS:
        raise NotImplementedError("chessboard detection supports at most %d corners per side and %d corners" % (MAX_BOARD_SIDE, MAX_CORNERS))
    return cols, rows


def _window(subpix_winSize):
    w, h = (int(v) for v in subpix_winSize)
    if w < 1 or h < 1:
        raise ValueError("subpix_winSize must be positive")
    if w > MAX_WINDOW or h > MAX_WINDOW:
        raise NotImplementedError("subpix_winSize: at most %d" % MAX_WINDOW)
    return w, h


def _frames(images):
    """uint8 (B, H, W) or (B, H, W, 3), or a list of equally sized frames -> a C-contiguous array and its channel count."""
    if isinstance(images, (list, tuple)):
        if len(images) == 0:
            raise ValueError("no frames")
        shapes = {np.shape(im) for im in images}
        if len(shapes) != 1:
            raise ValueError("frames must all have the same size")
        for im in images:
            if np.asarray(im).dtype != np.uint8:
                raise ValueError("frames must be uint8")
        images = np.stack([np.asarray(im) for im in images])
    a = np.asarray(images)
    if a.dtype != np.uint8:
        raise ValueError("frames must be uint8, not %s" % a.dtype)
    if a.ndim == 3:
        ch = 1
    elif a.ndim == 4 and a.shape[3] == 3:
        ch = 3
    elif a.ndim == 4:
        raise ValueError("colour frames must have 3 channels (BGR), not %d" % a.shape[3])
    else:
        raise ValueError("frames must have shape (B, H, W) or (B, H, W, 3)")
    if a.shape[1] < MIN_IMAGE_SIDE or a.shape[2] < MIN_IMAGE_SIDE:
        raise ValueError("frames must be at least %d x %d pixels" % (MIN_IMAGE_SIDE, MIN_IMAGE_SIDE))
    if a.shape[1] > MAX_IMAGE_SIDE or a.shape[2] > MAX_IMAGE_SIDE:
        raise NotImplementedError("image sides of at most %d pixels" % MAX_IMAGE_SIDE)
    return np.ascontiguousarray(a), ch


def _image(image):
    a = np.asarray(image)
    if a.dtype != np.uint8:
        raise ValueError("image must be uint8, not %s" % a.dtype)
    if a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] != 3):
        raise ValueError("image must have shape (H, W) or (H, W, 3)")
    if a.shape[0] < MIN_IMAGE_SIDE or a.shape[1] < MIN_IMAGE_SIDE:
        raise ValueError("image must be at least %d x %d pixels" % (MIN_IMAGE_SIDE, MIN_IMAGE_SIDE))
    if a.shape[0] > MAX_IMAGE_SIDE or a.shape[1] > MAX_IMAGE_SIDE:
        raise NotImplementedError("image sides of at most %d pixels" % MAX_IMAGE_SIDE)
    return np.ascontiguousarray(a), (1 if a.ndim == 2 else 3)


# ------------------------------------------------------------------ batched detection
def detect_chessboards(images, *, board_shape=(7, 10), subpix_winSize=(5, 5), scale_factor=1, adaptive_threshold=True, normalize_image=True, reorder=True,
                       match_score_min_diff=0.2, device=0, memory_budget=0, return_kernel_ms=False):
    """Detect a chessboard in each of a batch of frames (one C-ABI call; the library splits the batch into chunks whose device memory stays
    within memory_budget bytes, 0 = its default of 256 MiB).

    Returns (uvs, match_scores, status): uvs float64 (B, N, 2), NaN where nothing was accepted (the layout all_calib_uvs[c] needs);
    match_scores (B, 4) sorted descending, NaN where no grid was assembled (kept for frames rejected as ambiguous: the reference's qc_data);
    status int8 (B): 0 no board, 1 accepted, 2 rejected because the anchor was ambiguous.  With reorder=False no anchor is scored: every
    assembled grid is accepted in the lattice's own order and match_scores is NaN.  return_kernel_ms: also the kernels' time."""
    cols, rows = _board(board_shape)
    w, h = _window(subpix_winSize)
    frames, ch = _frames(images)
    B, H, W = frames.shape[:3]
    s = float(scale_factor)
    if not (0.0 < s <= 1.0):
        raise NotImplementedError("scale_factor must lie in (0, 1]")
    N = cols * rows
    uvs = np.empty((B, N, 2), dtype=np.float32)
    scores = np.empty((B, 4))
    status = np.empty(B, dtype=np.int8)
    ms = np.zeros(1)
    ops.call("mcba_detect_chessboards", B, H, W, ch, frames.ctypes.data, cols, rows, w, h, s, int(bool(reorder)), float(match_score_min_diff), int(memory_budget),
             int(device), uvs.ctypes.data, scores.ctypes.data, status.ctypes.data, ms.ctypes.data)
    over = np.flatnonzero(status == _STATUS_OVERFLOW)
    if len(over):
        warnings.warn("chessboard detection: %d frame(s) had more than %d corner candidates and were not searched: %s"
                      % (len(over), MAX_CANDIDATES, over[:20].tolist()))
        status[over] = STATUS_NONE
    out = (uvs.astype(np.float64), scores, status)
    return out + (float(ms[0]),) if return_kernel_ms else out


# ------------------------------------------------------------------ detect_chessboard (detection.py:300-405)
def detect_chessboard(image, *, board_shape=(7, 10), subpix_winSize=(5, 5), scale_factor=1, adaptive_threshold=True, normalize_image=True, reorder=True,
                      match_score_min_diff=0.2, device=0):
    """Detect the corners of a chessboard and order them using the anchor disc beside it (see the module docstring).

    image: uint8 (H, W) or BGR (H, W, 3).  Returns None when no board is found or the anchor is ambiguous; else uvs float32 (N, 2), and with
    reorder=True (uvs, match_scores) where match_scores float64 (4,) is sorted descending.  adaptive_threshold and normalize_image are
    OpenCV flags, accepted for the signature and without effect."""
    img, _ = _image(image)
    uvs, scores, status = detect_chessboards(img[None], board_shape=board_shape, subpix_winSize=subpix_winSize, scale_factor=scale_factor, reorder=reorder,
                                             match_score_min_diff=match_score_min_diff, device=device)
    if status[0] != STATUS_ACCEPTED:
        return None
    if reorder:
        return uvs[0].astype(np.float32), scores[0].copy()
    return uvs[0].astype(np.float32)


# ------------------------------------------------------------------ the pieces of the pipeline, one image at a time
def corner_subpix(image, corners, subpix_winSize=(5, 5), *, device=0):
    """cv2.cornerSubPix(grey, corners, subpix_winSize, (-1, -1), (EPS + MAX_ITER, 30, 0.001)) on the device.  corners (n, 2) -> float32 (n, 2)."""
    img, ch = _image(image)
    w, h = _window(subpix_winSize)
    start = np.ascontiguousarray(np.asarray(corners, dtype=np.float32).reshape(-1, 2))
    out = np.empty_like(start)
    ops.call("mcba_detect_subpix", img.shape[0], img.shape[1], ch, img.ctypes.data, start.shape[0], start.ctypes.data, w, h, int(device), out.ctypes.data, None)
    return out


def _anchor_template(size=TEMPLATE_SIZE):
    """White square with the black disc (x - 10)^2 + (y - 10)^2 <= 100: what cv2.circle(.., (10, 10), 10, 0, -1) fills (317 pixels)."""
    y, x = np.mgrid[0:size, 0:size]
    return np.where((x - size // 4) ** 2 + (y - size // 4) ** 2 <= (size // 4) ** 2, 0, 255).astype(np.uint8)


# ------------------------------------------------------------------ reorder_chessboard_corners (detection.py:436-489)
def reorder_chessboard_corners(image, uvs, board_shape, template_size=40, *, device=0):
    """Reorder chessboard corners using the anchor disc.  Returns (uvs_reordered, sorted_match_scores, vis_info) with vis_info =
    (all_source_pts, regions, template, match_scores): the four source quads (each float32 (1, 4, 2)), the four warped 40 x 40 uint8
    regions, the template and the unsorted scores.  As in the reference the template is 40 x 40 whatever template_size says."""
    img, ch = _image(image)
    cols, rows = _board(board_shape)
    u = np.ascontiguousarray(np.asarray(uvs, dtype=np.float32).reshape(rows * cols, 2))
    scores = np.empty(4)
    regions = np.empty((4, TEMPLATE_SIZE, TEMPLATE_SIZE), dtype=np.uint8)
    quads = np.empty((4, 4, 2), dtype=np.float32)
    ops.call("mcba_detect_anchor", img.shape[0], img.shape[1], ch, img.ctypes.data, cols, rows, u.ctypes.data, int(device), scores.ctypes.data, regions.ctypes.data,
             quads.ctypes.data, None)
    uv_grid = np.asarray(uvs).reshape(rows, cols, 2)
    best = int(np.argmax(scores))
    if best in (2, 3):
        uv_grid = uv_grid[::-1, :]
    if best in (1, 2):
        uv_grid = uv_grid[:, ::-1]
    match_scores = [float(v) for v in scores]
    vis_info = ([quads[k][None] for k in range(4)], [regions[k] for k in range(4)], _anchor_template(), match_scores)
    return uv_grid.reshape(-1, 2), np.sort(scores)[::-1], vis_info


# ------------------------------------------------------------------ host-only helpers
def generate_chessboard_objpoints(chess_board_shape, chess_board_square_size):
    """(N, 3) float32 board points in the reference's order: point k = (k % shape[0], k // shape[0], 0) * square_size (detection.py:492-518)."""
    rows, cols = chess_board_shape
    objpoints = np.zeros((rows * cols, 3), np.float32)
    objpoints[:, :2] = np.mgrid[0:rows, 0:cols].T.reshape(-1, 2) * chess_board_square_size
    return objpoints


def homography_dlt(src, dst):
    """Least-squares homography src -> dst (n >= 4 points, (n, 2) each): Hartley-normalised DLT, the right singular vector of the smallest
    singular value; scaled so that H[2, 2] = 1."""
    src = np.asarray(src, dtype=np.float64).reshape(-1, 2)
    dst = np.asarray(dst, dtype=np.float64).reshape(-1, 2)

    def norm(p):
        m = p.mean(axis=0)
        d = np.sqrt(((p - m) ** 2).sum(1)).mean()
        s = np.sqrt(2.0) / d if d > 0 else 1.0
        return np.array([[s, 0, -s * m[0]], [0, s, -s * m[1]], [0, 0, 1.0]])

    Ta, Tb = norm(src), norm(dst)
    a = src @ Ta[:2, :2].T + Ta[:2, 2]
    b = dst @ Tb[:2, :2].T + Tb[:2, 2]
    n = len(a)
    A = np.zeros((2 * n, 9))
    A[0::2, 0:2], A[0::2, 2] = a, 1
    A[1::2, 3:5], A[1::2, 5] = a, 1
    A[0::2, 6:9] = -b[:, :1] * np.c_[a, np.ones(n)]
    A[1::2, 6:9] = -b[:, 1:] * np.c_[a, np.ones(n)]
    Hn = np.linalg.svd(A)[2][-1].reshape(3, 3)
    H = np.linalg.inv(Tb) @ Hn @ Ta
    return H / H[2, 2]


def extend_grid(uv_grid, extend_rows, extend_cols):
    """The (rows + 2 extend_rows, cols + 2 extend_cols, 2) grid that the least-squares homography of uv_grid (rows, cols, 2) predicts
    (detection.py:264-297, with a numpy DLT in place of cv2.findHomography)."""
    uv_grid = np.asarray(uv_grid)
    rows = uv_grid.shape[0] + 2 * extend_rows
    cols = uv_grid.shape[1] + 2 * extend_cols
    xy_grid_full = np.mgrid[0:cols, 0:rows].T
    xy_grid = xy_grid_full[extend_rows:rows - extend_rows, extend_cols:cols - extend_cols]
    H = homography_dlt(xy_grid.reshape(-1, 2), uv_grid.reshape(-1, 2))
    pts = np.c_[xy_grid_full.reshape(-1, 2), np.ones(rows * cols)] @ H.T
    return (pts[:, :2] / pts[:, 2:]).reshape(xy_grid_full.shape)


def summarize_detections(all_calib_uvs):
    """pandas DataFrame of the number of frames each pair of cameras both detected the board in (index and columns 'Camera i')."""
    try:
        import pandas as pd
    except ImportError as e:
        raise ImportError("summarize_detections needs pandas") from e
    has_detection = ~np.isnan(all_calib_uvs).any(axis=(2, 3))
    n_shared = (has_detection[:, None, :] & has_detection[None, :, :]).sum(2)
    names = [f"Camera {i}" for i in range(len(all_calib_uvs))]
    return pd.DataFrame(n_shared, index=names, columns=names)
