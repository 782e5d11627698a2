"""`triangulate()` on the GPU (reference geometry.py:328-433).

Same signature and return value as the reference.  The reference undistorts with cv2.undistortPoints, triangulates every
camera pair with cv2.triangulatePoints and takes the nan-median over the pairs; here one HIP kernel does all three per
point (`csrc/mcba_triangulate.hip`: OpenCV's fixed-point undistortion for the 5-coefficient model, the 4x4 DLT null vector
by one-sided Jacobi, a sorting network for the median; beyond 8 cameras one wavefront per point with the camera pairs
across its lanes and the median by rank counting).  OpenCV is absent from this image, so parity with cv2's numbers is
unpinned; the kernel is checked against a numpy restatement of the two published algorithms (oracle/triangulate_oracle.py)
and against exact recovery of synthetic points.
"""
import ctypes

import numpy as np

from . import ops


def _cam_blocks(all_extrinsics, all_intrinsics):
    C = len(all_extrinsics)
    cam = np.zeros((C, 12))
    dist = np.zeros((C, 5))
    for c, (ext, (K, d)) in enumerate(zip(all_extrinsics, all_intrinsics)):
        K = np.asarray(K, dtype=np.float64)
        if K[0, 1] != 0:
            raise NotImplementedError("camera matrices with skew are not supported")
        d = np.ravel(np.asarray(d, dtype=np.float64))
        if d.size > 5 and np.any(d[5:] != 0):
            raise NotImplementedError("only the 5-coefficient distortion model (k1, k2, p1, p2, k3) is supported")
        cam[c, :4] = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
        cam[c, 6:] = np.asarray(ext, dtype=np.float64)
        dist[c, : min(5, d.size)] = d[:5]
    cam[:, 4:6] = dist[:, :2]
    return cam, dist


def _stack_uvs(all_uvs, all_extrinsics, all_intrinsics):
    uvs = np.ascontiguousarray(np.stack([np.asarray(u, dtype=np.float64) for u in all_uvs]))
    if uvs.ndim != 3 or uvs.shape[2] != 2 or uvs.shape[0] != len(all_extrinsics) or len(all_extrinsics) != len(all_intrinsics):
        raise ValueError("all_uvs must be one (n_points, 2) array per camera, matching all_extrinsics / all_intrinsics")
    return uvs


def _weight_plane(weights, C, P):
    """weights=None, or the (C, P) float64 plane of per-detection weights w >= 0 (relative inverse variances; 0 or NaN = the detection is
    unseen), checked.  ValueError: another shape, a negative or an infinite weight."""
    if weights is None:
        return None
    w = np.ascontiguousarray(weights, dtype=np.float64)
    if w.shape != (C, P):
        raise ValueError(f"weights must be ({C}, {P}): one per camera and point, got {w.shape}")
    if (w < 0).any() or np.isinf(w).any():
        raise ValueError("weights must be finite and not negative (0 or NaN: the detection is unseen)")
    return w


DEFAULT_MAX_ITERATIONS = 100   # linearisations per point of the refinement (geometry.refine_triangulation)


def triangulate(all_uvs, all_extrinsics, all_intrinsics, device=0, undistort_iterations=5, return_kernel_ms=False, *, refine=False, loss="soft_l1", f_scale=1.0, weights=None):
    """all_uvs: per camera (n_points, 2), NaN = not seen.  Returns (n_points, 3); NaN rows where fewer than two cameras see
    the point (geometry.py:361-433).

    refine=True: the reference's estimate (the median over the camera pairs) is only the start; every point is then moved to the minimiser
    of its robust reprojection cost (`geometry.refine_triangulation` with `loss`, `f_scale` and its default iteration limit).  The
    detections go to the device once; the two kernels run back to back there.

    weights (with refine=True only; ValueError otherwise, so that weights are never silently ignored): (C, P) per-detection weights as
    `geometry.refine_triangulation` takes them.  The refinement is weighted; the median over the pairs is not, but skips the detections of
    weight 0 or NaN."""
    uvs = _stack_uvs(all_uvs, all_extrinsics, all_intrinsics)
    C, P = uvs.shape[:2]
    if not 2 <= C <= 64:
        raise NotImplementedError("triangulate() supports 2 to 64 cameras")
    if refine and loss not in ops.LOSSES:
        raise ValueError(f"loss must be one of {sorted(ops.LOSSES)}")
    if refine and not f_scale > 0:
        raise ValueError("`f_scale` must be positive.")
    if weights is not None and not refine:
        raise ValueError("weights= needs refine=True: the median over the camera pairs is unweighted")
    w = _weight_plane(weights, C, P)
    cam, dist = _cam_blocks(all_extrinsics, all_intrinsics)
    out = np.empty((P, 3))
    ms = ctypes.c_double(0.0)
    if w is not None:
        ops.call("mcba_triangulate_refine_weighted", C, P, uvs.ctypes.data, w.ctypes.data, cam.ctypes.data, dist.ctypes.data, None, int(undistort_iterations), ops.LOSSES[loss], float(f_scale),
                 DEFAULT_MAX_ITERATIONS, int(device), out.ctypes.data, None, ctypes.addressof(ms))
    elif refine:
        ops.call("mcba_triangulate_refine", C, P, uvs.ctypes.data, cam.ctypes.data, dist.ctypes.data, None, int(undistort_iterations), ops.LOSSES[loss], float(f_scale), DEFAULT_MAX_ITERATIONS,
                 int(device), out.ctypes.data, None, ctypes.addressof(ms))
    else:
        ops.call("mcba_triangulate", C, P, uvs.ctypes.data, cam.ctypes.data, dist.ctypes.data, int(undistort_iterations), int(device), out.ctypes.data, ctypes.addressof(ms))
    return (out, ms.value) if return_kernel_ms else out
