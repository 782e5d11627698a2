"""Trajectory uncertainty on the MI355X: kernel_ms (HIP events) of mcba_smooth_covariance at 10^4, 10^5 and 10^6 frames x 20 tracks, without
and with the lag-one blocks, the share of it spent in k_smooth_selinv (the rest: prepare, count and the elimination), its ratio to one linear
solve of smooth_trajectories at the same shape in the same process, the wall time of the call, and the device bytes per frame and track.
Warm, median of REPS; a fresh process per shape, each under its own time limit.  The scene is that of scripts/trajectory_smoothing_timing.py.
Nothing here is gated.

  python scripts/trajectory_uncertainty_timing.py [--out DIR] [--shapes 10000x20,100000x20,1000000x20] [--reps R]
  python scripts/trajectory_uncertainty_timing.py --child TxK --reps R        one measurement (JSON on stdout)"""
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def covariance_call(pts, cov6, acc, lag):
    """the C call itself: info8[7] (the selected inversion alone) is not part of the Python result"""
    import numpy as np

    from multicam_calibration_amd import ops

    T, K = pts.shape[:2]
    c6, l9 = np.empty((T, K, 6)), np.empty((T - 1, K, 9)) if lag else None
    st, nu, info = np.empty(K, np.int32), np.empty(K, np.int32), np.zeros(8)
    t0 = time.perf_counter()
    ops.call("mcba_smooth_covariance", T, K, pts.ctypes.data, cov6.ctypes.data, acc.ctypes.data, None, 0, 0, c6.ctypes.data, None if l9 is None else l9.ctypes.data, st.ctypes.data, nu.ctypes.data,
             info.ctypes.data, None)
    return (time.perf_counter() - t0) * 1e3, info, st


def child(shape, reps):
    import numpy as np

    sys.path.insert(0, ROOT)
    from multicam_calibration_amd import smooth_trajectories
    from trajectory_smoothing_timing import make_scene

    T, K = (int(v) for v in shape.split("x"))
    pts, std = make_scene(T, K)
    pts = np.ascontiguousarray(pts)
    cov6 = np.zeros((T, K, 6))
    cov6[..., 0] = cov6[..., 3] = cov6[..., 5] = std * std
    acc = np.full(K, 0.05)
    out = {"shape": shape, "frames": T, "tracks": K}
    solve = [smooth_trajectories(pts, std, accel_std=0.05).info["kernel_ms"] for _ in range(reps + 1)][1:]   # the first round warms up
    out["solve_kernel_ms"] = float(np.median(solve))
    for lag in (False, True):
        wall, kern, sel = [], [], []
        for _ in range(reps + 1):
            ms, info, st = covariance_call(pts, cov6, acc, lag)
            wall.append(ms), kern.append(float(info[4])), sel.append(float(info[7]))
        k = float(np.median(kern[1:]))
        out["lag" if lag else "diagonal"] = {"call_ms": float(np.median(wall[1:])), "kernel_ms": k, "selinv_ms": float(np.median(sel[1:])), "selinv_share": float(np.median(sel[1:])) / k,
                                             "ratio_to_one_solve": k / out["solve_kernel_ms"], "all_kernel_ms": kern[1:], "levels": int(info[0]), "segment": int(info[1]),
                                             "tracks_per_chunk": int(info[2]), "chunks": int(info[3]), "device_bytes": int(info[6]),
                                             "device_bytes_per_frame_track": float(info[6]) / (T * int(info[2])), "ok_tracks": int((st == 1).sum())}
    print(json.dumps(out))


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def main():
    out_dir = arg("--out", os.path.join(ROOT, "profiles"))
    shapes = arg("--shapes", "10000x20,100000x20,1000000x20").split(",")
    reps = arg("--reps", "3")
    os.makedirs(out_dir, exist_ok=True)
    results = []
    for shape in shapes:
        r = subprocess.run(["timeout", "-k", "10", "400", sys.executable, __file__, "--child", shape, "--reps", reps], cwd=ROOT, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-3000:] + r.stderr[-3000:])
            raise SystemExit("step failed (exit %d): %s" % (r.returncode, shape))
        results.append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(json.dumps(results[-1]), flush=True)
        with open(os.path.join(out_dir, "trajectory_uncertainty_timing.json"), "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    if "--child" in sys.argv:
        child(arg("--child", "10000x20"), int(arg("--reps", "3")))
    else:
        main()
