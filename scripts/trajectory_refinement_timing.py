"""Trajectory refinement on the MI355X: wall time of refine_trajectories (gathering the chunks, the uploads, the kernels, the copies out) and
kernel_ms of its kernels (HIP events) per Gauss-Newton iteration, at 10^5 frames x 20 tracks x 6 cameras and at one wide case (2000 frames x
20 tracks x 64 cameras), with the linear loss and with huber.  Warm, median of REPS.  Beside them, from the same run: kernel_ms of one solve of
smooth_trajectories (linear loss) at the same T and K, the levels, the tracks per chunk, and the kernel time of the covariance part of
uncertainty="lag".  Nothing here is gated.

  python scripts/trajectory_refinement_timing.py [--out DIR] [--shapes 100000x20x6,2000x20x64] [--reps R] [--iter ITER]
  python scripts/trajectory_refinement_timing.py --child TxKxC --reps R --iter ITER        one measurement (JSON on stdout)"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_scene(T, K, C, seed=3):
    """(start (T, K, 3), uvs (C, T, K, 2), extrinsics, intrinsics): a synthetic rig, smooth tracks where its board would be, 0.5 px noise, 20 % of
    the detections dropped, 5 % displaced by N(0, 40^2) px"""
    import numpy as np

    sys.path.insert(0, ROOT)
    import multicam_calibration_amd as m

    p = m.synth.make_problem(C, 2, seed=seed, noise=0.0)
    cam = p["true_cam"]
    pose = m.synth._T(p["true_poses"][0])
    rng = np.random.default_rng(seed)
    t = np.arange(T)[:, None, None]
    x = pose[:3, 3] + 40.0 * np.sin(t * rng.uniform(0.01, 0.05, (1, K, 3)) + rng.uniform(0, 6.28, (1, K, 3)))
    uv = np.stack([m.synth.project(cam[c:c + 1], np.zeros((1, 6)), x.reshape(-1, 3))[0, 0].reshape(T, K, 2) for c in range(C)])
    uv += rng.normal(0, 0.5, uv.shape)
    hit = rng.uniform(size=(C, T, K)) < 0.05
    uv[hit] += rng.normal(0, 40.0, (int(hit.sum()), 2))
    uv[rng.uniform(size=(C, T, K)) < 0.2] = np.nan
    intr = [(np.array([[c[0], 0, c[2]], [0, c[1], c[3]], [0, 0, 1.0]]), np.r_[c[4:6], 0, 0, 0]) for c in cam]
    return x + rng.normal(0, 0.3, x.shape), uv, cam[:, 6:], intr


def child(shape, reps, iters):
    import numpy as np

    sys.path.insert(0, ROOT)
    from multicam_calibration_amd import refine_trajectories, smooth_trajectories

    T, K, C = (int(v) for v in shape.split("x"))
    start, uv, ext, intr = make_scene(T, K, C)
    out = {"shape": shape, "frames": T, "tracks": K, "cameras": C}
    for loss in ("linear", "huber"):
        wall, kern, its = [], [], []
        for _ in range(reps + 1):   # the first round warms up
            t0 = time.perf_counter()
            r = refine_trajectories(start, uv, ext, intr, accel_std=0.15, pixel_std=0.5, loss=loss, max_iterations=iters)
            wall.append((time.perf_counter() - t0) * 1e3)
            kern.append(r.info["kernel_ms"])
            its.append(int(r.n_iterations.max()))
        n = its[-1]
        out[loss] = {"call_ms": float(np.median(wall[1:])), "kernel_ms": float(np.median(kern[1:])), "iterations": n, "kernel_ms_per_iteration": float(np.median(kern[1:])) / n,
                     "all_kernel_ms": kern[1:], "ok_tracks": int((r.status == 1).sum()), "single_frames": int(r.n_single.sum()), "usable_frames": int(r.n_usable.sum())}
        out.update(levels=r.info["levels"], segment=r.info["segment"], tracks_per_chunk=r.info["tracks_per_chunk"], chunks=r.info["chunks"], device_bytes=r.info["device_bytes"])
    r = refine_trajectories(start, uv, ext, intr, accel_std=0.15, pixel_std=0.5, loss="linear", max_iterations=1, uncertainty="lag")
    out["one_iteration_with_lag_covariance_kernel_ms"] = r.info["kernel_ms"]
    kern = []
    for _ in range(reps + 1):
        s = smooth_trajectories(start, 0.3, accel_std=0.15, loss="linear")
        kern.append(s.info["kernel_ms"])
    out["smooth_trajectories_one_solve_kernel_ms"] = float(np.median(kern[1:]))
    print(json.dumps(out))


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def main():
    out_dir = arg("--out", os.path.join(ROOT, "profiles"))
    shapes = arg("--shapes", "100000x20x6,2000x20x64").split(",")
    reps, iters = arg("--reps", "3"), arg("--iter", "5")
    os.makedirs(out_dir, exist_ok=True)
    results = []
    for shape in shapes:
        r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, __file__, "--child", shape, "--reps", reps, "--iter", iters], cwd=ROOT, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-3000:] + r.stderr[-3000:])
            raise SystemExit("step failed (exit %d): %s" % (r.returncode, shape))
        results.append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(json.dumps(results[-1]), flush=True)
        with open(os.path.join(out_dir, "trajectory_refinement_timing.json"), "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    if "--child" in sys.argv:
        child(arg("--child", "2000x20x6"), int(arg("--reps", "3")), int(arg("--iter", "5")))
    else:
        main()
