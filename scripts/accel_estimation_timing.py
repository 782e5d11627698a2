"""estimate_accel_std on the MI355X: wall time of the call and kernel_ms of its kernels (HIP events), at 10^6 frames x 20
tracks and 10^4 x 200, with the default grid (17 + 16 + 2 linear solves) -- and, in the same run, one linear solve of smooth_trajectories at the same
shape.  Warm, median of REPS.  Written out: the ratio kernel time / (evaluations x one solve's kernel time), which is 1 when a candidate costs
what a solve costs, and the share of the log-determinant kernels (k_evidence_logdet of every level, which reads 6 of the 63
factor planes, and k_evidence_final) in the estimator's kernel time.  Nothing here is gated.

  python scripts/accel_estimation_timing.py [--out DIR] [--shapes 1000000x20,10000x200] [--reps R]
  python scripts/accel_estimation_timing.py --child TxK --reps R        one measurement (JSON on stdout)"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A_TRUE, RANGE = 0.05, (0.005, 0.5)


def make_scene(T, K, seed=3):
    """tracks whose second differences are N(0, A_TRUE^2) per coordinate (bounded: the velocity is pulled back), isotropic noise, 3 % missing"""
    import numpy as np

    rng = np.random.default_rng(seed)
    acc = A_TRUE * rng.standard_normal((T, K, 3))
    x = np.cumsum(np.cumsum(acc, axis=0), axis=0)
    x -= np.linspace(0.0, 1.0, T)[:, None, None] * x[-1]   # (a motion linear in time: the prior does not see it)
    std = rng.uniform(0.05, 0.25, (T, K))
    pts = x + std[:, :, None] * rng.standard_normal((T, K, 3))
    pts[rng.uniform(size=(T, K)) < 0.03] = np.nan
    return pts, std


def child(shape, reps):
    import numpy as np

    sys.path.insert(0, ROOT)
    from multicam_calibration_amd import estimate_accel_std, smooth_trajectories

    T, K = (int(v) for v in shape.split("x"))
    pts, std = make_scene(T, K)
    wall, kern, ld, swall, skern = [], [], [], [], []
    for _ in range(reps + 1):   # the first round warms up
        t0 = time.perf_counter()
        s = smooth_trajectories(pts, std, accel_std=A_TRUE)
        swall.append((time.perf_counter() - t0) * 1e3)
        skern.append(s.info["kernel_ms"])
        t0 = time.perf_counter()
        r = estimate_accel_std(pts, std, accel_range=RANGE)
        wall.append((time.perf_counter() - t0) * 1e3)
        kern.append(r.info["kernel_ms"])
        ld.append(r.info["log_det_ms"])
    k, l, sk = float(np.median(kern[1:])), float(np.median(ld[1:])), float(np.median(skern[1:]))
    ok = r.status == 1
    print(json.dumps({"shape": shape, "frames": T, "tracks": K, "evaluations": r.n_evaluations, "call_ms": float(np.median(wall[1:])), "kernel_ms": k, "log_det_kernel_ms": l,
                      "smooth_call_ms": float(np.median(swall[1:])), "smooth_kernel_ms_one_solve": sk, "kernel_ms_over_evaluations_times_one_solve": k / (r.n_evaluations * sk),
                      "log_det_share_of_kernel_ms": l / k, "all_kernel_ms": kern[1:], "all_smooth_kernel_ms": skern[1:], "levels": r.info["levels"], "segment": r.info["segment"],
                      "tracks_per_chunk": r.info["tracks_per_chunk"], "chunks": r.info["chunks"], "smooth_chunks": s.info["chunks"], "device_bytes": r.info["device_bytes"],
                      "ok_tracks": int(ok.sum()), "on_an_edge": int((r.edge[ok] != 0).sum()), "accel_std_true": A_TRUE, "accel_std_median": float(np.median(r.accel_std[ok])),
                      "accel_std_min": float(r.accel_std[ok].min()), "accel_std_max": float(r.accel_std[ok].max()), "log_std_median": float(np.nanmedian(r.log_std[ok]))}))


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def main():
    out_dir = arg("--out", os.path.join(ROOT, "profiles"))
    shapes = arg("--shapes", "1000000x20,10000x200").split(",")
    reps = arg("--reps", "3")
    os.makedirs(out_dir, exist_ok=True)
    results = []
    for shape in shapes:
        r = subprocess.run(["timeout", "-k", "10", "500", sys.executable, __file__, "--child", shape, "--reps", reps], cwd=ROOT, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-3000:] + r.stderr[-3000:])
            raise SystemExit("step failed (exit %d): %s" % (r.returncode, shape))
        results.append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(json.dumps(results[-1]), flush=True)
        with open(os.path.join(out_dir, "accel_estimation_timing.json"), "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    if "--child" in sys.argv:
        child(arg("--child", "10000x200"), int(arg("--reps", "3")))
    else:
        main()
