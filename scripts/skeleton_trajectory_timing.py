"""Skeleton trajectories on the MI355X: the wall time of the whole call, kernel_ms (HIP events around every bracket of launches), the outer and the
conjugate-gradient iterations and the kernel time per CG iteration of refine_skeleton_trajectories at 10^4 and 10^5 frames x 20 keypoints (a chain) x
6 cameras; beside them, from the same process and on the same detections, one solve of refine_trajectories (max_iterations=1: one linearisation,
one elimination, one trial) -- what an outer iteration cost before the bones.  The kernel time per CG iteration is measured as the difference of
two one-iteration calls with cg_max = 33 and cg_max = 1 at a cg_tol no solve reaches, over the 32 iterations between them: an operator, a re-solve
from the stored factors and the vector updates -- to be held against the elimination it replaces, which refine_trajectories' solve contains.  No
ratio is gated.  One process, one warm-up round, then the median of REPS.

  python scripts/skeleton_trajectory_timing.py [--out DIR] [--frames 10000,100000] [--reps R]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, C = 20, 6


def make_scene(T, seed=3):
    """(start (T, K, 3), uvs (C, T, K, 2), extrinsics, intrinsics, bones, bone_length): a synthetic rig; the root a smooth track where the rig's board
    would be, every other keypoint of the chain at its bone's length (8 .. 30 mm) from its parent in a direction that turns smoothly; 0.5 px noise,
    20 % of the detections dropped, a one-camera stretch of 40 frames on keypoint 5 and an unseen gap of 20 on keypoint 12 in every 1000 frames; the
    start is the truth with 0.3 mm of noise"""
    import numpy as np

    import multicam_calibration_amd as m

    p = m.synth.make_problem(C, 2, seed=seed, noise=0.0)
    cam = p["true_cam"]
    pose = m.synth._T(p["true_poses"][0])
    rng = np.random.default_rng(seed)
    bones = np.array([[k, k + 1] for k in range(K - 1)])
    L = rng.uniform(8.0, 30.0, K - 1)
    tt = np.arange(T)[:, None]
    x = np.zeros((T, K, 3))
    x[:, 0] = pose[:3, 3] + 40.0 * np.stack([np.sin(2 * np.pi * tt[:, 0] / 900 + i) + 0.3 * np.sin(2 * np.pi * tt[:, 0] / 130 + 2 * i) for i in range(3)], axis=1)
    for k in range(1, K):
        n = rng.normal(size=(3, 3))
        v = n[0] + 0.6 * (n[1] * np.sin(2 * np.pi * tt / rng.uniform(80, 200) + rng.uniform(0, 6)) + n[2] * np.cos(2 * np.pi * tt / rng.uniform(80, 200)))
        x[:, k] = x[:, k - 1] + L[k - 1] * v / np.linalg.norm(v, axis=1, keepdims=True)
    uv = np.stack([m.synth.project(cam[c:c + 1], np.zeros((1, 6)), x.reshape(-1, 3))[0, 0].reshape(T, K, 2) for c in range(C)])
    uv += rng.normal(0, 0.5, uv.shape)
    uv[rng.uniform(size=(C, T, K)) < 0.2] = np.nan
    for a in range(100, T - 400, 1000):
        uv[1:, a:a + 40, 5] = np.nan
        uv[:, a + 300:a + 320, 12] = np.nan
    intr = [(np.array([[c[0], 0, c[2]], [0, c[1], c[3]], [0, 0, 1.0]]), np.r_[c[4:6], 0, 0, 0]) for c in cam]
    return x + rng.normal(0, 0.3, x.shape), uv, cam[:, 6:], intr, bones, L


def median_of(fn, reps):
    import numpy as np

    kern, wall = [], []
    for _ in range(reps + 1):   # the first round warms up
        t0 = time.perf_counter()
        r = fn()
        wall.append((time.perf_counter() - t0) * 1e3)
        kern.append(r.info["kernel_ms"])
    return r, float(np.median(kern[1:])), float(np.median(wall[1:]))


def measure(T, reps):
    from multicam_calibration_amd import refine_skeleton_trajectories, refine_trajectories

    start, uv, ext, intr, bones, L = make_scene(T)
    joint = dict(accel_std=0.15, bones=bones, bone_length=L, bone_std=0.5, pixel_std=0.5)
    r, k_ms, c_ms = median_of(lambda: refine_skeleton_trajectories(start, uv, ext, intr, **joint), reps)
    out = {"frames": T, "keypoints": K, "cameras": C, "skeleton": "chain", "bone_std": 0.5, "accel_std": 0.15, "kernel_ms": k_ms, "call_ms": c_ms, "outer_iterations": r.n_iterations,
           "converged": r.converged, "cg_iterations": [int(v) for v in r.history[:, 3]], "cg_iterations_total": r.info["cg_iterations_total"], "alphas": [float(v) for v in r.history[:, 2]],
           "cost_start": r.cost_start, "cost": r.cost, "levels": r.info["levels"], "device_bytes": r.info["device_bytes"]}
    one = dict(joint, max_iterations=1, cg_tol=1e-300)
    _, k33, _ = median_of(lambda: refine_skeleton_trajectories(start, uv, ext, intr, cg_max=33, **one), reps)
    _, k1, _ = median_of(lambda: refine_skeleton_trajectories(start, uv, ext, intr, cg_max=1, **one), reps)
    out["kernel_ms_per_cg_iteration"] = (k33 - k1) / 32.0
    out["kernel_ms_of_an_outer_iteration_with_one_cg_iteration"] = k1
    t, tk, tc = median_of(lambda: refine_trajectories(start, uv, ext, intr, accel_std=0.15, pixel_std=0.5, max_iterations=1), reps)
    out["refine_trajectories_one_solve"] = {"kernel_ms": tk, "call_ms": tc}
    return out


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def main():
    sys.path.insert(0, ROOT)
    out_dir = arg("--out", os.path.join(ROOT, "profiles"))
    frames = [int(v) for v in arg("--frames", "10000,100000").split(",")]
    reps = int(arg("--reps", "3"))
    os.makedirs(out_dir, exist_ok=True)
    results = []
    for T in frames:
        results.append(measure(T, reps))
        print(json.dumps(results[-1]), flush=True)
        with open(os.path.join(out_dir, "skeleton_trajectory_timing.json"), "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
