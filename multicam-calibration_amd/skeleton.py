"""refine_skeleton -- the K keypoints of a frame refined together on their raw detections, joined by bones of known length (SURVEY.md section
8f-22); estimate_bone_lengths -- those lengths and their spread from located keypoints.  Every other step of the keypoint chain treats the
keypoints of a frame as unrelated points; here a keypoint only one camera saw is located by its ray and one bone to a located neighbour, and
keypoints two cameras or more saw get tighter, most along the depth direction.

The reference has no counterpart (it saves keypoints in a format an outside skeletal model reads).  Everything runs on the GPU: per frame a
Levenberg-Marquardt loop whose linear system is block structured on the skeleton's forest and eliminated leaf to root without fill."""
import ctypes
from dataclasses import dataclass

import numpy as np

from . import ops
from .trajectory import _accel_argument, _check_loss, _check_segment, _detection_arguments, _loop_arguments

KEYPOINT_STATUS = {2: "fitted, two views or more", 1: "fitted, one view", -1: "no view or a non-finite start", -2: "in a piece without a keypoint of two views"}
FRAME_STATUS = {1: "converged", 0: "iteration limit", -1: "nothing to fit"}
MAX_KEYPOINTS = 64
_SYM = np.array([[0, 1, 2], [1, 3, 4], [2, 4, 5]])


@dataclass
class BoneLengths:
    length: np.ndarray   # (E,): the exact nan-median of the per-frame distances, NaN for a bone no frame has
    std: np.ndarray      # (E,): 1.4826 x the exact nan-median of |distance - length|
    count: np.ndarray    # (E,): frames that have both ends
    info: dict           # kernel_ms


@dataclass
class SkeletonRefinement:
    points: np.ndarray           # (T, K, 3): NaN for a keypoint that was not fitted
    keypoint_status: np.ndarray  # (T, K): a key of KEYPOINT_STATUS
    frame_status: np.ndarray     # (T,): a key of FRAME_STATUS
    n_iterations: np.ndarray     # (T,): trial steps made
    cost: np.ndarray             # (T,): the objective at the result, NaN where nothing was fitted
    cost_start: np.ndarray       # (T,): ... at the start
    bone_residual: np.ndarray    # (T, E): (|x_a - x_b| - L) / s at the result, NaN for a bone dropped in the frame
    info: dict                   # kernel_ms, frames_per_workgroup, levels, frames_per_chunk, chunks, device_bytes, most_iterations
    covariance: np.ndarray = None   # covariance=True: (T, K, 3, 3), the keypoint's block of the inverse of the Gauss-Newton matrix at the result
    std: np.ndarray = None          # ... the square roots of its diagonal
    information: np.ndarray = None  # ... (T, K, 3, 3), the diagonal blocks of that matrix, bones included
    direction: np.ndarray = None    # ... (T, E, 3), the unit vector of every bone from its parent end to its child end (`parent`), NaN where dropped
    parent: np.ndarray = None       # (K,): the parent of every keypoint in the walk from the lowest-numbered keypoint of each piece, -1 = root


@dataclass
class SkeletonSystem:
    information: np.ndarray      # (T, K, 3, 3): diagonal blocks of the Gauss-Newton matrix at the points, bones included, undamped
    gradient: np.ndarray         # (T, K, 3): of the whole objective
    direction: np.ndarray        # (T, E, 3): u, from the bone's parent end to its child end
    step: np.ndarray             # (T, K, 3): the solution of the system damped by lam diag
    data_cost: np.ndarray        # (T,)
    bone_cost: np.ndarray        # (T,)
    trial_cost: np.ndarray       # (T,): the objective at points + step
    keypoint_status: np.ndarray  # (T, K)
    frame_status: np.ndarray     # (T,): 1 or -1
    parent: np.ndarray           # (K,)
    info: dict


def forest_parents(bones, K):
    """(parent (K,), child (E,)): bones (E, 2) as a parent array by a walk from the lowest-numbered keypoint of each piece (-1 = root), and per bone
    the end that is the child.  ValueError for an index outside 0 .. K - 1, a self-bone, a repeated bone or a cycle."""
    b = np.asarray(bones)
    if b.size == 0:
        b = np.zeros((0, 2), np.int64)
    if b.ndim != 2 or b.shape[1] != 2:
        raise ValueError("bones must be (E, 2)")
    if not np.issubdtype(b.dtype, np.integer):
        if not (np.isfinite(b).all() and (b == np.floor(b)).all()):
            raise ValueError("bones must hold keypoint indices")
        b = b.astype(np.int64)
    if ((b < 0) | (b >= K)).any():
        raise ValueError(f"a bone's keypoint lies outside 0 .. {K - 1}")
    if (b[:, 0] == b[:, 1]).any():
        raise ValueError("a bone joins a keypoint with itself")
    pairs = {tuple(sorted(map(int, e))) for e in b}
    if len(pairs) != len(b):
        raise ValueError("a bone is repeated")
    nbr = [[] for _ in range(K)]
    for e, (i, j) in enumerate(b):
        nbr[int(i)].append((int(j), e))
        nbr[int(j)].append((int(i), e))
    parent, child, seen = np.full(K, -1, np.int32), np.full(len(b), -1, np.int32), np.zeros(K, bool)
    used = np.zeros(len(b), bool)
    for root in range(K):
        if seen[root]:
            continue
        seen[root] = True
        queue = [root]
        while queue:
            i = queue.pop(0)
            for j, e in sorted(nbr[i]):
                if used[e]:
                    continue
                used[e] = True
                if seen[j]:
                    raise ValueError("the bones hold a cycle: the skeleton must be a forest")
                seen[j], parent[j], child[e] = True, i, j
                queue.append(j)
    return parent, child


def _per_bone(value, name, E):
    v = np.asarray(value, dtype=np.float64)
    if v.shape not in ((), (E,)):
        raise ValueError(f"{name} must be a scalar or ({E},)")
    v = np.ascontiguousarray(np.broadcast_to(v, (E,)))
    with np.errstate(over="ignore", divide="ignore"):
        if not (np.isfinite(v).all() and (v > 0).all() and np.isfinite(1.0 / (v * v)).all()):
            raise ValueError(f"{name} must be positive and finite")
    return v


def _arguments(start, all_uvs, all_extrinsics, all_intrinsics, bones, bone_length, bone_std, pixel_std, loss, f_scale, weights):
    """the checked arrays both calls take: pts (T, K, 3), uvs (C, T, K, 2), cam (C, 12), dist (C, 5), parent (K), child (E), L (K), s (K), pstd (C), w (C, T, K) or None"""
    if callable(loss) or loss not in ops.LOSSES:
        raise ValueError(f"loss must be one of {sorted(ops.LOSSES)}")
    pts, uvs, cam, dist, pstd, w = _detection_arguments("refine_skeleton", "keypoint", start, all_uvs, all_extrinsics, all_intrinsics, pixel_std, f_scale, weights, MAX_KEYPOINTS)
    K = pts.shape[1]
    parent, child = forest_parents(bones, K)
    E = len(child)
    if np.asarray(bone_length).shape != (E,):
        raise ValueError(f"bone_length must be ({E},): one per bone")
    Lb, sb = _per_bone(bone_length, "bone_length", E), _per_bone(bone_std, "bone_std", E)
    L, s = np.ones(K), np.ones(K)
    L[child], s[child] = Lb, sb
    return pts, uvs, cam, dist, parent, child, L, s, pstd, w


def _info(info8):
    return {"kernel_ms": float(info8[4]), "frames_per_workgroup": int(info8[1]), "levels": int(info8[0]), "frames_per_chunk": int(info8[2]), "chunks": int(info8[3]),
            "device_bytes": int(info8[6]), "most_iterations": int(info8[5])}


def _per_bone_out(plane, child):
    """(T, K, ...) indexed by the bone's child end -> (T, E, ...)"""
    return np.ascontiguousarray(plane[:, child])


def estimate_bone_lengths(points, bones, *, device=0):
    """The length of every bone and its spread from located keypoints, for example `refine_triangulation(...)` of a recording.  points (T, K, 3),
    NaN = missing; bones (E, 2) pairs of keypoints (any pairs: no forest is asked for here).  Per bone, over the frames that have both ends:
    length = the exact median of the distances (np.nanmedian, the mean of the two middle values for an even count), std = 1.4826 x the exact
    median of |distance - length| (the robust estimate of a normal spread), count = those frames.  A bone no frame has is NaN, NaN, 0.
    ValueError (before a device is touched): wrong shapes, T == 0, no bone, a keypoint index outside 0 .. K - 1.  Without a GPU: ops.McbaError."""
    pts = np.ascontiguousarray(points, dtype=np.float64)
    if pts.ndim != 3 or pts.shape[2] != 3 or pts.shape[0] == 0 or pts.shape[1] == 0:
        raise ValueError("points must be (T, K, 3) with at least one frame and one keypoint")
    T, K = pts.shape[:2]
    b = np.asarray(bones)
    if b.ndim != 2 or b.shape[1] != 2 or len(b) == 0 or not np.issubdtype(b.dtype, np.integer):
        raise ValueError("bones must be (E, 2) keypoint indices, at least one bone")
    if len(b) > 65535:
        raise ValueError("at most 65535 bones")
    if ((b < 0) | (b >= K)).any():
        raise ValueError(f"a bone's keypoint lies outside 0 .. {K - 1}")
    b = np.ascontiguousarray(b, dtype=np.int32)
    E = len(b)
    length, std, count = np.empty(E), np.empty(E), np.empty(E, np.int32)
    ms = ctypes.c_double(0.0)
    ops.call("mcba_bone_lengths", T, K, pts.ctypes.data, E, b.ctypes.data, int(device), length.ctypes.data, std.ctypes.data, count.ctypes.data, ctypes.addressof(ms))
    return BoneLengths(length=length, std=std, count=count, info={"kernel_ms": ms.value})


def refine_skeleton(start, all_uvs, all_extrinsics, all_intrinsics, *, bones, bone_length, bone_std, pixel_std=1.0, loss="linear", f_scale=3.0, weights=None, max_iterations=50, xtol=1e-8,
                    covariance=False, device=0):
    """Refine the K keypoints of every frame together.  Frames are independent.  Per frame, over the positions x_k of
    its active keypoints, minimise

        0.5 sum_k sum_{c sees k} f^2 [rho(ru^2 / f^2) + rho(rv^2 / f^2)] + 0.5 sum_{active bones (a, b)} ((|x_a - x_b| - L) / s)^2,
        (ru, rv) = sqrt(w_ctk) (detection - projection_c(x_k)) / pixel_std_c

    start (T, K, 3): where the iteration begins, NaN = no start -- `refine_triangulation(...)` reshaped, or a smoother's fill
    (`smooth_trajectories(...).points`) so that keypoints one camera saw have a start as well.  all_uvs (C, T, K, 2) or a list of C arrays
    (T, K, 2): raw detections, NaN = unseen.  all_extrinsics, all_intrinsics: the cameras as `refine_triangulation` takes them, at most 64.
    bones (E, 2): the skeleton, a forest over at most 64 keypoints; bone_length (E,) and bone_std (a scalar or (E,)) in the points' unit, for
    example from `estimate_bone_lengths`.  pixel_std: the detection noise in pixels, a scalar or (C,).  loss: one of scipy's five rho per scalar
    residual as `refine_triangulation` takes them, f = f_scale in units of pixel_std; the bone term is always quadratic.  weights: None or
    (C, T, K) per-detection weights (0 or NaN: the detection is unseen).

    A keypoint is usable in a frame with two views or more and a finite start, single with exactly one view and a finite start; otherwise it is
    out of the frame (status -1) and its bones are dropped there, which may split a tree.  A connected piece of what is left is fitted when it
    holds a usable keypoint (a piece of n single keypoints has 2 n + n - 1 < 3 n equations: status -2).  Everything not fitted is NaN.  A single
    keypoint has two solutions -- its ray meets the sphere about its neighbour twice -- and the fit converges to the one near the start; that is
    not resolved here.

    Levenberg-Marquardt per frame, `refine_triangulation`'s iteration with the frame's whole objective: damping lam diag(H) from 1e-4, / 10 on
    acceptance (floor 1e-12), x 10 on rejection; a trial is accepted when the objective is not larger, so the result is never worse than the
    start.  A frame stops (frame_status 1) when a step has max |d| < xtol max |x| over its active keypoints or lam reaches 1e12, and at
    max_iterations trials (frame_status 0).  Two calls return the same bits, and a frame's result does not depend on the frames around it.

    covariance=True: covariance (T, K, 3, 3) and std -- every fitted keypoint's block of the inverse of the Gauss-Newton matrix at the result,
    bones included, in units where pixel_std is the detection noise: the plane `smooth_trajectories` takes -- with information and direction,
    from which that matrix can be rebuilt.  Covariances between keypoints are not returned.

    ValueError (before a device is touched): wrong shapes, T == 0 or K == 0, more than 64 keypoints or cameras, a bone index outside 0 .. K - 1,
    a self-bone, a repeated bone, a cycle, bone_length, bone_std, pixel_std or f_scale not positive and finite, an unknown loss, a negative or
    infinite weight, max_iterations < 1, xtol < 0.  Without a GPU: ops.McbaError -- there is no host path."""
    pts, uvs, cam, dist, parent, child, L, s, pstd, w = _arguments(start, all_uvs, all_extrinsics, all_intrinsics, bones, bone_length, bone_std, pixel_std, loss, f_scale, weights)
    C, T, K = uvs.shape[:3]
    max_iterations = _loop_arguments(max_iterations, xtol)
    if not any(covariance is v for v in (False, True)):
        raise ValueError("covariance must be False or True")
    out, kst, fst, nit = np.empty((T, K, 3)), np.empty((T, K), np.int32), np.empty(T, np.int32), np.empty(T, np.int32)
    cost, cost0, bres, info = np.empty(T), np.empty(T), np.empty((T, K)), np.zeros(8)
    c6, h6, u3 = (np.empty((T, K, 6)), np.empty((T, K, 6)), np.empty((T, K, 3))) if covariance else (None, None, None)
    ms = ctypes.c_double(0.0)
    p = lambda a: None if a is None else a.ctypes.data
    ops.call("mcba_refine_skeleton", T, K, C, p(uvs), p(cam), p(dist), p(w), p(pstd), p(pts), p(parent), p(L), p(s), ops.LOSSES[loss], float(f_scale), max_iterations, float(xtol), int(device),
             p(out), p(kst), p(fst), p(nit), p(cost), p(cost0), p(bres), p(c6), p(h6), p(u3), p(info), ctypes.addressof(ms))
    res = SkeletonRefinement(points=out, keypoint_status=kst, frame_status=fst, n_iterations=nit, cost=cost, cost_start=cost0, bone_residual=_per_bone_out(bres, child), info=_info(info),
                             parent=parent)
    if covariance:
        res.covariance = np.ascontiguousarray(c6[..., _SYM])
        with np.errstate(invalid="ignore"):
            res.std = np.sqrt(res.covariance[..., (0, 1, 2), (0, 1, 2)])
        res.information = np.ascontiguousarray(h6[..., _SYM])
        res.direction = _per_bone_out(u3, child)
    return res


def refine_skeleton_system(points, all_uvs, all_extrinsics, all_intrinsics, *, bones, bone_length, bone_std, pixel_std=1.0, loss="linear", f_scale=3.0, weights=None, lam=1e-4, device=0):
    """One evaluation of refine_skeleton laid open, at `points` (T, K, 3) with the damping `lam` and before anything is accepted: the diagonal
    blocks of the Gauss-Newton matrix (bones included, undamped), the gradient of the whole objective, the bones' directions, the step of the
    damped system, the data and the bone term of the objective at the points and the objective at points + step -- what a test holds against a
    dense oracle.  Arguments, statuses and errors as refine_skeleton; whatever is not fitted is NaN."""
    pts, uvs, cam, dist, parent, child, L, s, pstd, w = _arguments(points, all_uvs, all_extrinsics, all_intrinsics, bones, bone_length, bone_std, pixel_std, loss, f_scale, weights)
    C, T, K = uvs.shape[:3]
    if not (np.isfinite(lam) and lam >= 0):
        raise ValueError("lam must be finite and not negative")
    h6, g, u3, d = np.empty((T, K, 6)), np.empty((T, K, 3)), np.empty((T, K, 3)), np.empty((T, K, 3))
    kst, fst = np.empty((T, K), np.int32), np.empty(T, np.int32)
    dc, bc, tc, info = np.empty(T), np.empty(T), np.empty(T), np.zeros(8)
    ms = ctypes.c_double(0.0)
    p = lambda a: None if a is None else a.ctypes.data
    ops.call("mcba_refine_skeleton_system", T, K, C, p(uvs), p(cam), p(dist), p(w), p(pstd), p(pts), p(parent), p(L), p(s), ops.LOSSES[loss], float(f_scale), float(lam), int(device),
             p(h6), p(g), p(u3), p(d), p(kst), p(fst), p(dc), p(bc), p(tc), p(info), ctypes.addressof(ms))
    return SkeletonSystem(information=np.ascontiguousarray(h6[..., _SYM]), gradient=g, direction=_per_bone_out(u3, child), step=d, data_cost=dc, bone_cost=bc, trial_cost=tc,
                          keypoint_status=kst, frame_status=fst, parent=parent, info=_info(info))


@dataclass
class SkeletonTrajectoryRefinement:
    points: np.ndarray         # (T, K, 3): NaN for a track whose status is not 1
    status: np.ndarray         # (K,): a key of trajectory.TRAJECTORY_REFINE_STATUS
    n_usable: np.ndarray       # (K,): frames two cameras or more see
    n_single: np.ndarray       # (K,): frames exactly one camera sees
    converged: bool            # the call stopped on a small step or on nothing accepted, not on the iteration limit alone
    n_iterations: int          # outer (Gauss-Newton) iterations made
    cost: float                # the call's objective at the result
    cost_start: float          # ... at the start
    history: np.ndarray        # (n_iterations, 4): objective, accepted step, alpha, CG iterations of that solve
    bone_residual: np.ndarray  # (T, E): (|x_a - x_b| - L) / s at the result, NaN for a bone that was dropped
    information: np.ndarray    # (T, K, 3, 3): H of the data term at the result (the prior and the bones are rebuilt from accel_std and direction)
    direction: np.ndarray      # (T, E, 3): the unit vector of every bone from its parent end to its child end (`parent`), NaN where dropped
    parent: np.ndarray         # (K,): as SkeletonRefinement.parent
    info: dict                 # kernel_ms, levels, segment, cg_iterations_total, running_tracks, device_bytes


@dataclass
class SkeletonTrajectorySystem:
    information: np.ndarray    # (T, K, 3, 3): H of the data term at the points
    gradient: np.ndarray       # (T, K, 3): of the whole objective
    direction: np.ndarray      # (T, E, 3)
    step: np.ndarray           # (T, K, 3): the iterate of the preconditioned recurrence for (M + B) d = -G when it ended
    cg_iterations: int
    cg_residual: float         # sqrt(r^T z / r0^T z0) of the recurrence when it ended
    data_cost: float
    penalty_cost: float
    bone_cost: float
    trial_costs: np.ndarray    # (4,): the objective at x + alpha d, alpha = 1, 1/2, 1/4, 1/8
    status: np.ndarray         # (K,)
    n_usable: np.ndarray       # (K,)
    n_single: np.ndarray       # (K,)
    parent: np.ndarray         # (K,)
    info: dict
    resolve_check: np.ndarray = None   # resolve_check=True: (2, T, K, 3), M z = -G by the elimination and again by the re-solve from its factors


def _trajectory_arguments(start, all_uvs, all_extrinsics, all_intrinsics, accel_std, bones, bone_length, bone_std, pixel_std, loss, f_scale, weights, cg_tol, cg_max, segment):
    """_arguments plus what the time prior and the inner solve take: acc (K,), cg_max"""
    _check_loss(loss, "refine_skeleton_trajectories", known=ops.LOSSES)
    args = _arguments(start, all_uvs, all_extrinsics, all_intrinsics, bones, bone_length, bone_std, pixel_std, loss, f_scale, weights)
    acc = _accel_argument(accel_std, args[0].shape[1])
    if not 0.0 < cg_tol < 1.0:
        raise ValueError("cg_tol must lie inside (0, 1)")
    cg_max = int(cg_max)
    if cg_max < 1:
        raise ValueError("cg_max must be at least 1")
    _check_segment(segment)
    return args + (acc, cg_max)


def _trajectory_info(info8):
    return {"kernel_ms": float(info8[4]), "levels": int(info8[0]), "segment": int(info8[1]), "cg_iterations_total": int(info8[3]), "running_tracks": int(info8[2]),
            "device_bytes": int(info8[6])}


def refine_skeleton_trajectories(start, all_uvs, all_extrinsics, all_intrinsics, *, accel_std, bones, bone_length, bone_std, pixel_std=1.0, loss="linear", f_scale=3.0, weights=None,
                                 max_iterations=30, xtol=1e-8, cg_tol=1e-6, cg_max=200, segment=None, device=0):
    """Refine the K keypoint tracks of a recording together: `refine_trajectories`' fit of every track to its raw detections under the
    second-difference prior, and `refine_skeleton`'s bones between the keypoints of a frame, in one problem.  Over
    x_{t,k} of the running tracks, minimise

        0.5 sum_t sum_k sum_{c sees (t,k)} f^2 [rho(ru^2 / f^2) + rho(rv^2 / f^2)] + 0.5 sum_k a_k^-2 sum_t |x_{t-1,k} - 2 x_{t,k} + x_{t+1,k}|^2
          + 0.5 sum_t sum_{active bones (k, p)} ((|x_{t,k} - x_{t,p}| - L) / s)^2

    Arguments as `refine_trajectories` (start, all_uvs, cameras, accel_std, pixel_std, loss -- linear, soft_l1 or huber --, f_scale, weights,
    segment) and `refine_skeleton` (bones (E, 2), a forest over at most 64 keypoints, bone_length (E,), bone_std).  accel_std can be had from
    triangulated tracks with `estimate_accel_std`, as bone_length and bone_std from `estimate_bone_lengths`.  A track runs under
    `refine_trajectories`' rule (two usable frames, a finite start; status as TRAJECTORY_REFINE_STATUS); a bone is active, in every frame, when
    both its tracks run, and is dropped for the whole call otherwise (bone_residual NaN).  The bone term is always quadratic.

    Gauss-Newton in step form on the call's objective.  The system of an iteration, (M + B) d = -G with M the tracks' block-pentadiagonal
    matrices and B the bones' terms, is solved by conjugate gradients preconditioned with M: one elimination of the smoother per outer iteration,
    one re-solve from its factors per CG iteration, until the residual (in the M^-1 norm) has fallen by cg_tol or after cg_max iterations.
    Every iterate of that recurrence is a descent direction, so the objective never rises however early it ends.  The number of CG iterations
    grows with the stiffness of the bones against what else holds a keypoint: a few where every keypoint is seen by two cameras, tens through
    one-camera stretches and unseen gaps at bone_std of the order of the 3-D noise, hundreds for nearly rigid bones.
    The largest alpha of 1, 1/2, 1/4, 1/8 whose objective is not above the current one is taken (none: the call stops where it is); the call
    stops when alpha max |d| < xtol max |x| or at max_iterations.  An unseen stretch whose bone direction only the prior holds is a flat valley:
    such a call can crawl at alpha = 1/8 to the iteration limit and returns converged = False, never worse than its start.  Two calls return the
    same bits.

    A start at which the objective is not finite (a bone of zero length) gives every running track status -3; a refused pivot of the
    elimination ends the loop with status -2 on that track.

    ValueError (before a device is touched): the errors of `refine_trajectories` and `refine_skeleton`, cg_tol outside (0, 1), cg_max < 1.  A call
    that does not fit the device-memory budget MCBA_SMOOTH_BUDGET_MB whole is refused (ops.McbaError): bones couple the tracks, so it cannot run
    in chunks.  Without a GPU: ops.McbaError -- there is no host path."""
    pts, uvs, cam, dist, parent, child, L, s, pstd, w, acc, cg_max = _trajectory_arguments(start, all_uvs, all_extrinsics, all_intrinsics, accel_std, bones, bone_length, bone_std, pixel_std,
                                                                                         loss, f_scale, weights, cg_tol, cg_max, segment)
    C, T, K = uvs.shape[:3]
    max_iterations = _loop_arguments(max_iterations, xtol)
    out, h6, bres, u3 = np.empty((T, K, 3)), np.empty((T, K, 6)), np.empty((T, K)), np.empty((T, K, 3))
    status, nus, nsg = (np.empty(K, np.int32) for _ in range(3))
    conv, nit = np.zeros(1, np.int32), np.zeros(1, np.int32)
    cost, cost0, hist, info = np.empty(1), np.empty(1), np.empty((max_iterations, 4)), np.zeros(8)
    ms = ctypes.c_double(0.0)
    p = lambda a: None if a is None else a.ctypes.data
    ops.call("mcba_refine_skeleton_trajectories", T, K, C, p(uvs), p(cam), p(dist), p(w), p(pstd), p(pts), p(acc), p(parent), p(L), p(s), ops.LOSSES[loss], float(f_scale), max_iterations,
             float(xtol), float(cg_tol), cg_max, 0 if segment is None else int(segment), int(device), p(out), p(h6), p(status), p(nus), p(nsg), p(conv), p(nit), p(cost), p(cost0), p(hist),
             p(bres), p(u3), p(info), ctypes.addressof(ms))
    return SkeletonTrajectoryRefinement(points=out, status=status, n_usable=nus, n_single=nsg, converged=bool(conv[0]), n_iterations=int(nit[0]), cost=float(cost[0]),
                                        cost_start=float(cost0[0]), history=np.ascontiguousarray(hist[:int(nit[0])]), bone_residual=_per_bone_out(bres, child),
                                        information=np.ascontiguousarray(h6[..., _SYM]), direction=_per_bone_out(u3, child), parent=parent, info=_trajectory_info(info))


def refine_skeleton_trajectories_system(points, all_uvs, all_extrinsics, all_intrinsics, *, accel_std, bones, bone_length, bone_std, pixel_std=1.0, loss="linear", f_scale=3.0, weights=None,
                                        cg_tol=1e-6, cg_max=200, segment=None, device=0, resolve_check=False):
    """One evaluation of refine_skeleton_trajectories laid open, at `points` (T, K, 3) and before anything is accepted: the information blocks of
    the data term, the gradient of the whole objective, the bones' directions, the step the preconditioned recurrence ended at with its
    iteration count and final relative residual, the three terms of the objective at the points and the objective at x + alpha d for alpha = 1,
    1/2, 1/4, 1/8 -- what a test holds against a dense oracle.  Arguments, statuses and errors as refine_skeleton_trajectories.
    resolve_check=True (for tests): also (2, T, K, 3), the solution of M z = -G by the elimination and, after the right-hand-side halves of every
    stored record were overwritten with NaN, by the re-solve from the stored factors; tracks that do not run are NaN."""
    pts, uvs, cam, dist, parent, child, L, s, pstd, w, acc, cg_max = _trajectory_arguments(points, all_uvs, all_extrinsics, all_intrinsics, accel_std, bones, bone_length, bone_std, pixel_std,
                                                                                         loss, f_scale, weights, cg_tol, cg_max, segment)
    C, T, K = uvs.shape[:3]
    h6, g, u3, d = np.empty((T, K, 6)), np.empty((T, K, 3)), np.empty((T, K, 3)), np.empty((T, K, 3))
    status, nus, nsg = (np.empty(K, np.int32) for _ in range(3))
    cgi, cgr, dc, pc, bc, tc, info = np.zeros(1, np.int32), np.empty(1), np.empty(1), np.empty(1), np.empty(1), np.empty(4), np.zeros(8)
    if not any(resolve_check is v for v in (False, True)):
        raise ValueError("resolve_check must be False or True")
    rs = np.full((2, T, K, 3), np.nan) if resolve_check else None
    ms = ctypes.c_double(0.0)
    p = lambda a: None if a is None else a.ctypes.data
    ops.call("mcba_refine_skeleton_trajectories_system", T, K, C, p(uvs), p(cam), p(dist), p(w), p(pstd), p(pts), p(acc), p(parent), p(L), p(s), ops.LOSSES[loss], float(f_scale),
             float(cg_tol), cg_max, 0 if segment is None else int(segment), int(device), p(h6), p(g), p(u3), p(d), p(status), p(nus), p(nsg), p(cgi), p(cgr), p(dc), p(pc), p(bc), p(tc),
             p(rs), p(info), ctypes.addressof(ms))
    if rs is not None:
        rs[:, :, status != 1] = np.nan
    return SkeletonTrajectorySystem(information=np.ascontiguousarray(h6[..., _SYM]), gradient=g, direction=_per_bone_out(u3, child), step=d, cg_iterations=int(cgi[0]),
                                    cg_residual=float(cgr[0]), data_cost=float(dc[0]), penalty_cost=float(pc[0]), bone_cost=float(bc[0]), trial_costs=tc, status=status, n_usable=nus,
                                    n_single=nsg, parent=parent, info=_trajectory_info(info), resolve_check=rs)
