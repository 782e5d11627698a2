"""Floor-plane alignment timing on the MI355X: the four public calls end to end from host arrays, the kernel time of each call (HIP
events) and the share of the call that is not kernel time (PCIe copies, allocation, host work), plus rocprofv3 --kernel-trace --stats
per kernel in a run of its own.  At 1e5 and 1e6 frames (12 keypoints per frame, 30 % outliers above the floor).

  python scripts/flatibration_timing.py [--out DIR]     driver: every step a child process under its own `timeout -k`
                                                       (results and rocprofv3 output under DIR, default build/flatibration_timing)
  python scripts/flatibration_timing.py --child N       one measurement (JSON on stdout)

The CPU column is the reference code path (sklearn 1.7.2 RANSAC, numpy argmin / percentile) as measured once on the build machine's CPU,
quoted as the denominator; it is not re-measured here.  Inputs come from tests/flat_problem.py."""
import ctypes
import glob
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU_MS = {100000: None, 300000: dict(ransac=78, get_floor_points=41, percentile=10), 1000000: dict(ransac=245, get_floor_points=125, percentile=42)}
K = 12
HBM_PEAK = 8.0e12  # bytes/s, datasheet (measured float4 copy: 6.29e12)


def child(N, reps):
    import numpy as np

    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import flat_problem as fp

    import multicam_calibration_amd as m
    from multicam_calibration_amd import flatibration as fl
    from multicam_calibration_amd import ops

    lib = ops.load_library()
    kp = fp.keypoints(N, K, seed=1, nan_frames=0.0, nan_entries=0.0, ties=False)
    P = fp.floor_points(N, 0.3, 2)
    ms = ctypes.c_double()

    def timed(fn):
        best = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            best.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(best))

    np.random.seed(0)
    t = m.flatibrate(P)
    out = {"frames": N, "keypoints": K}
    out["e2e_ms"] = {
        "get_floor_points": timed(lambda: m.get_floor_points(kp)),
        "flatibrate": timed(lambda: m.flatibrate(P)),
        "center_arena_midrange": timed(lambda: m.center_arena(t, P)),
        "center_arena_median": timed(lambda: m.center_arena(t, P, center_method="median")),
        "center_arena_mean": timed(lambda: m.center_arena(t, P, center_method="mean")),
        "flip_z_axis": timed(lambda: m.flip_z_axis(t)),
    }
    # kernel time of one call of each entry point (HIP events around the call's kernels)
    kd = np.ascontiguousarray(kp)
    o3, ix = np.empty((N, 3)), np.empty(N, dtype=np.int32)
    lib.mcba_flat_floor_points(N, K, kd.ctypes.data, 0, 0, o3.ctypes.data, ix.ctypes.data, ctypes.addressof(ms))
    k_floor = ms.value
    idx, _ = fl.draw_subsets(N)
    planes = np.ascontiguousarray(fl.hypotheses(P, idx))
    cnt, mom, sh = np.empty(100, dtype=np.uint64), np.empty((100, 9)), np.ascontiguousarray(P[0, :2])
    lib.mcba_flat_ransac(N, P.ctypes.data, 100, planes.ctypes.data, 10.0, sh.ctypes.data, 0, cnt.ctypes.data, mom.ctypes.data, None, ctypes.addressof(ms))
    k_ransac = ms.value
    rt = np.ascontiguousarray(np.r_[np.eye(3).ravel(), np.zeros(3)])
    ranks = np.array([N // 100, N // 100 + 1, N - N // 100 - 2, N - N // 100 - 1], dtype=np.int64)
    vals, sums, nans = np.empty(8), np.empty(2), np.empty(2, dtype=np.uint64)
    lib.mcba_flat_order_stats(N, P.ctypes.data, rt.ctypes.data, 4, ranks.ctypes.data, 0, vals.ctypes.data, sums.ctypes.data, nans.ctypes.data, ctypes.addressof(ms))
    k_stats = ms.value
    out["kernel_ms"] = {"floor_points": k_floor, "ransac_100_hypotheses": k_ransac, "order_stats_4_ranks": k_stats}
    in_bytes = {"floor_points": N * K * 24, "ransac_100_hypotheses": N * 24, "order_stats_4_ranks": N * 24}
    out["h2d_bytes"] = in_bytes
    out["floor_points_kernel_hbm_fraction_of_peak"] = (N * K * 24 + N * 28) / (k_floor * 1e-3) / HBM_PEAK
    e2e = out["e2e_ms"]
    out["non_kernel_share"] = {"get_floor_points": 1 - k_floor / e2e["get_floor_points"], "flatibrate": 1 - k_ransac / e2e["flatibrate"],
                               "center_arena_midrange": 1 - k_stats / e2e["center_arena_midrange"]}
    out["cpu_reference_ms_build_machine"] = CPU_MS.get(N)
    print(json.dumps(out))


def run(cmd, seconds, **kw):
    r = subprocess.run(["timeout", "-k", "10", str(seconds)] + cmd, cwd=ROOT, capture_output=True, text=True, **kw)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-3000:] + r.stderr[-3000:])
        raise SystemExit("step failed (exit %d): %s" % (r.returncode, " ".join(cmd)))
    return r.stdout


def main():
    out_dir = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "build", "flatibration_timing")
    os.makedirs(out_dir, exist_ok=True)
    results = []
    for N in (100000, 1000000):
        res = json.loads(run([sys.executable, __file__, "--child", str(N)], 600).strip().splitlines()[-1])
        results.append(res)
        print(json.dumps(res, indent=1))
    for N in (100000, 1000000):  # kernel statistics, profiler in a run of its own
        d = os.path.join(out_dir, "rocprof_%d" % N)
        run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "flat", "--", sys.executable, __file__, "--child", str(N), "--reps", "2"], 600)
        for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            print("== %d frames: %s" % (N, os.path.relpath(f, out_dir)))
            for line in open(f):
                if line.startswith('"Name"') or any(k in line for k in ("k_floor", "k_ransac", "k_sel_", "k_flat")):
                    print(line.rstrip())
    with open(os.path.join(out_dir, "flatibration_timing.json"), "w") as fh:
        json.dump(results, fh, indent=1)


if __name__ == "__main__":
    if "--child" in sys.argv:
        child(int(sys.argv[sys.argv.index("--child") + 1]), int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 7)
    else:
        main()
