"""Trajectory smoothing on the MI355X: wall time of smooth_trajectories (gathering the chunks, the uploads, the kernels, the copies out) and
kernel_ms of its kernels (HIP events) per IRLS iteration, at 10^4, 10^5 and 10^6 frames x 20 tracks, with the linear loss (one solve) and with
soft_l1 (at most ITER solves, so that the largest shape stays a short run).  Warm, median of REPS.  Beside them: the levels, the tracks per chunk,
the HBM rate that the floor of 96 B per frame and track (24 B p + 48 B Sigma in, 24 B out) would mean if one iteration's kernels moved nothing
else -- every kernel of an iteration is inside that time, so this is a lower bound on what the level-0 kernels reach -- as a share of 8 TB/s,
and scipy.linalg.solveh_banded on the same box for one track, times 20, for context.  Nothing here is gated.

  python scripts/trajectory_smoothing_timing.py [--out DIR] [--shapes 10000x20,100000x20,1000000x20] [--reps R] [--iter ITER]
  python scripts/trajectory_smoothing_timing.py --child TxK --reps R --iter ITER        one measurement (JSON on stdout)"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_BYTES_PER_S = 8.0e12
FLOOR_BYTES = 96.0


def make_scene(T, K, seed=3):
    import numpy as np

    rng = np.random.default_rng(seed)
    t = np.arange(T)[:, None, None]
    x = 8.0 * np.sin(t * rng.uniform(0.01, 0.05, (1, K, 3)) + rng.uniform(0, 6.28, (1, K, 3)))
    std = rng.uniform(0.05, 0.25, (T, K))
    pts = x + std[:, :, None] * rng.standard_normal((T, K, 3))
    pts[rng.uniform(size=(T, K)) < 0.03] = np.nan                       # missing detections
    bad = rng.uniform(size=(T, K)) < 0.02                              # gross errors
    pts[bad] += 5.0 * rng.standard_normal((int(bad.sum()), 3))
    return pts, std


def banded_solve_ms(pts, std, accel_std):
    """one track through scipy.linalg.solveh_banded (the upper banded form of the same system, unit weights)"""
    import numpy as np
    import scipy.linalg

    T = len(pts)
    us = np.isfinite(pts[:, 0])
    w = np.where(us, 1.0 / std ** 2, 0.0)
    v = np.zeros(T + 3)
    v[2:T] = 1.0
    t = np.arange(T)
    ia2 = 1.0 / accel_std ** 2
    ab = np.zeros((9, 3 * T))
    ab[8] = np.repeat(w + ia2 * (v[t + 2] + 4.0 * v[t + 1] + v[t]), 3)
    ab[5, 3:] = np.repeat(ia2 * -2.0 * (v[t + 1] + v[t + 2])[:T - 1], 3)
    ab[2, 6:] = np.repeat(ia2 * v[t + 2][:T - 2], 3)
    b = (w[:, None] * np.nan_to_num(pts)).ravel()
    t0 = time.perf_counter()
    x = scipy.linalg.solveh_banded(ab, b, lower=False)
    return (time.perf_counter() - t0) * 1e3, x.reshape(T, 3)


def child(shape, reps, iters):
    import numpy as np

    sys.path.insert(0, ROOT)
    from multicam_calibration_amd import smooth_trajectories

    T, K = (int(v) for v in shape.split("x"))
    pts, std = make_scene(T, K)
    out = {"shape": shape, "frames": T, "tracks": K}
    for loss, it in (("linear", 1), ("soft_l1", iters)):
        wall, kern, solves = [], [], []
        for _ in range(reps + 1):   # the first round warms up
            t0 = time.perf_counter()
            r = smooth_trajectories(pts, std, accel_std=0.05, loss=loss, max_iterations=it)
            wall.append((time.perf_counter() - t0) * 1e3)
            kern.append(r.info["kernel_ms"])
            solves.append(int(r.n_iterations.max()))
        n = solves[-1]
        k_it = float(np.median(kern[1:])) / n
        out[loss] = {"call_ms": float(np.median(wall[1:])), "kernel_ms": float(np.median(kern[1:])), "solves": n, "kernel_ms_per_solve": k_it, "all_kernel_ms": kern[1:],
                     "floor_share_of_hbm": FLOOR_BYTES * T * K / (k_it * 1e-3) / HBM_BYTES_PER_S, "ok_tracks": int((r.status == 1).sum())}
        out.update(levels=r.info["levels"], segment=r.info["segment"], tracks_per_chunk=r.info["tracks_per_chunk"], chunks=r.info["chunks"], device_bytes=r.info["device_bytes"])
        if loss == "linear":
            ms, x = banded_solve_ms(pts[:, 0], std[:, 0], 0.05)
            out["solveh_banded_ms_one_track"] = ms
            out["solveh_banded_ms_all_tracks"] = ms * K
            out["largest_difference_to_solveh_banded"] = float(np.abs(r.points[:, 0] - x).max())
    print(json.dumps(out))


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def main():
    out_dir = arg("--out", os.path.join(ROOT, "profiles"))
    shapes = arg("--shapes", "10000x20,100000x20,1000000x20").split(",")
    reps, iters = arg("--reps", "3"), arg("--iter", "5")
    os.makedirs(out_dir, exist_ok=True)
    results = []
    for shape in shapes:
        r = subprocess.run(["timeout", "-k", "10", "400", sys.executable, __file__, "--child", shape, "--reps", reps, "--iter", iters], cwd=ROOT, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-3000:] + r.stderr[-3000:])
            raise SystemExit("step failed (exit %d): %s" % (r.returncode, shape))
        results.append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(json.dumps(results[-1]), flush=True)
        with open(os.path.join(out_dir, "trajectory_smoothing_timing.json"), "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    if "--child" in sys.argv:
        child(arg("--child", "10000x20"), int(arg("--reps", "3")), int(arg("--iter", "5")))
    else:
        main()
