"""Skeleton-constrained refinement on the MI355X: kernel_ms (HIP events around k_skel_refine) and the wall time of the whole call -- the planes
of sqrt(w) / pixel_std, the uploads, the kernel, the copies out -- of refine_skeleton at 10^5 and 10^6 frames x 20 keypoints x 6 cameras, each
for a chain of 20 (19 levels of barriers per sweep) and a star of 20 (1 level).  Beside them, from the same process and on the same T K
detections, refine_triangulation (the linear loss, every keypoint alone): how these keypoints were refined before.  What the comparison shows
is what a frame's tree sweeps cost on top of its projections; no ratio is gated.  One process, one warm-up round, then the median of REPS.

  python scripts/skeleton_refinement_timing.py [--out DIR] [--frames 100000,1000000] [--reps R]"""
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, C, BASE = 20, 6, 100000


def make_scene(T, bones, seed=3):
    """(start (T, K, 3), uvs (C, T, K, 2), extrinsics, intrinsics, bone_length (E,)): a synthetic rig; per frame the skeleton laid out afresh where the
    rig's board would be, bones of 8 .. 30 mm with 0.5 mm of jitter in random directions, 0.5 px noise, 35 % of the detections dropped; the start
    is the truth with 0.3 mm of noise"""
    import numpy as np

    import multicam_calibration_amd as m
    from multicam_calibration_amd.skeleton import forest_parents

    p = m.synth.make_problem(C, 2, seed=seed, noise=0.0)
    cam = p["true_cam"]
    pose = m.synth._T(p["true_poses"][0])
    rng = np.random.default_rng(seed)
    parent, child = forest_parents(bones, K)
    L = np.zeros(K)
    L[child] = rng.uniform(8.0, 30.0, len(child))
    x = np.zeros((T, K, 3))
    level = np.zeros(K, int)
    for k in range(K):
        j = k
        while parent[j] >= 0:
            j, level[k] = parent[j], level[k] + 1
    for k in sorted(range(K), key=lambda k: level[k]):
        if parent[k] < 0:
            x[:, k] = pose[:3, 3] + rng.normal(0, 25.0, (T, 3))
        else:
            v = rng.normal(size=(T, 3))
            x[:, k] = x[:, parent[k]] + v / np.linalg.norm(v, axis=1, keepdims=True) * (L[k] + rng.normal(0, 0.5, T))[:, None]
    uv = np.stack([m.synth.project(cam[c:c + 1], np.zeros((1, 6)), x.reshape(-1, 3))[0, 0].reshape(T, K, 2) for c in range(C)])
    uv += rng.normal(0, 0.5, uv.shape)
    uv[rng.uniform(size=(C, T, K)) < 0.35] = np.nan
    intr = [(np.array([[c[0], 0, c[2]], [0, c[1], c[3]], [0, 0, 1.0]]), np.r_[c[4:6], 0, 0, 0]) for c in cam]
    return x + rng.normal(0, 0.3, x.shape), uv, cam[:, 6:], intr, L[child]


def per_keypoint(start, uv, ext, intr, reps):
    """(kernel_ms, call_ms) of mcba_triangulate_refine on the T K keypoints, each alone: medians of reps after a warm-up"""
    import numpy as np

    from multicam_calibration_amd import ops
    from multicam_calibration_amd.geometry import _keypoint_inputs

    P = start.shape[0] * start.shape[1]
    kern, wall = [], []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        pts, uvs, cam, dist = _keypoint_inputs(start.reshape(P, 3), uv.reshape(C, P, 2), ext, intr)
        out, info, ms = np.empty((P, 3)), np.empty((P, 4)), ctypes.c_double(0.0)
        ops.call("mcba_triangulate_refine", C, P, uvs.ctypes.data, cam.ctypes.data, dist.ctypes.data, pts.ctypes.data, 0, ops.LOSSES["linear"], 3.0, 100, 0, out.ctypes.data, info.ctypes.data,
                 ctypes.addressof(ms))
        wall.append((time.perf_counter() - t0) * 1e3)
        kern.append(ms.value)
    return float(np.median(kern[1:])), float(np.median(wall[1:])), int(np.isfinite(out).all(1).sum())


def measure(T, shape, reps):
    import numpy as np

    from multicam_calibration_amd import refine_skeleton

    bones = np.array([[k, k + 1] for k in range(K - 1)] if shape == "chain" else [[0, k] for k in range(1, K)])
    start, uv, ext, intr, L = make_scene(BASE, bones)
    n = T // BASE
    start, uv = np.tile(start, (n, 1, 1)), np.tile(uv, (1, n, 1, 1))     # frames are independent: 10^6 frames are the 10^5 ten times
    kern, wall = [], []
    for _ in range(reps + 1):   # the first round warms up
        t0 = time.perf_counter()
        r = refine_skeleton(start, uv, ext, intr, bones=bones, bone_length=L, bone_std=0.5, pixel_std=0.5)
        wall.append((time.perf_counter() - t0) * 1e3)
        kern.append(r.info["kernel_ms"])
    out = {"frames": T, "keypoints": K, "cameras": C, "skeleton": shape, "kernel_ms": float(np.median(kern[1:])), "call_ms": float(np.median(wall[1:])), "all_kernel_ms": kern[1:],
           "levels": r.info["levels"], "frames_per_workgroup": r.info["frames_per_workgroup"], "chunks": r.info["chunks"], "most_iterations": r.info["most_iterations"],
           "mean_iterations": float(r.n_iterations.mean()), "frames_at_the_limit": int((r.frame_status == 0).sum()), "fitted_usable": int((r.keypoint_status == 2).sum()),
           "fitted_single": int((r.keypoint_status == 1).sum())}
    k_ms, c_ms, located = per_keypoint(start, uv, ext, intr, reps)
    out["refine_triangulation"] = {"kernel_ms": k_ms, "call_ms": c_ms, "located": located}
    return out


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def main():
    sys.path.insert(0, ROOT)
    out_dir = arg("--out", os.path.join(ROOT, "profiles"))
    frames = [int(v) for v in arg("--frames", "100000,1000000").split(",")]
    reps = int(arg("--reps", "3"))
    os.makedirs(out_dir, exist_ok=True)
    results = []
    for T in frames:
        for shape in ("chain", "star"):
            results.append(measure(T, shape, reps))
            print(json.dumps(results[-1]), flush=True)
            with open(os.path.join(out_dir, "skeleton_refinement_timing.json"), "w") as fh:
                json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
