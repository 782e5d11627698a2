"""Chessboard detection timing on the MI355X: frames/s of detect_chessboards for a batch of 256 frames at 640x480, 1280x1024 and 2048x1536,
grey and BGR, scale_factor 1 and 0.5; the kernels' share of each call (HIP events) against the host-to-device copy of the frames (the same bytes
copied alone by torch from pageable host memory, as the call copies them: the lower bound of the call), plus rocprofv3 --kernel-trace --stats
per kernel in a run of its own.

  python scripts/detection_timing.py [--out DIR]        driver: every step a child process under its own `timeout -k`
                                                       (results and rocprofv3 output under DIR, default build/detection_timing)
  python scripts/detection_timing.py --child W H C S    one measurement (JSON on stdout)

There is no CPU column: the reference detector is cv2.findChessboardCorners + cornerSubPix, and cv2 is not installed on the machines this
project is measured on -- unmeasured.  Frames come from tests/chessboard_scenes.py (a 7 x 10 board in half of the frames)."""
import glob
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(640, 480), (1280, 1024), (2048, 1536)]
BATCH = 256


def frames(W, H, C, n=BATCH):
    import numpy as np

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import chessboard_scenes as scenes

    rng = np.random.default_rng(0)
    distinct = []
    while len(distinct) < 8:
        pose, cam = scenes.random_view(rng, (7, 10), (W, H), max_tilt_deg=45.0)
        if scenes.eligible((7, 10), pose, cam, (W, H), 0.5):
            distinct.append(scenes.render((7, 10), pose, cam, (W, H), blur=0.8, noise=2.0, seed=len(distinct), device="cuda", supersample=2))
    distinct += [np.full((H, W), 100, np.uint8)] * 8   # no board in half of the frames
    out = np.stack([distinct[i % len(distinct)] for i in range(n)])
    return np.ascontiguousarray(np.repeat(out[..., None], 3, axis=3)) if C == 3 else out


def child(W, H, C, S, reps=5):
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    from multicam_calibration_amd import detection

    f = frames(W, H, C)
    detection.detect_chessboards(f[:8], scale_factor=S)   # warm-up (module load, first allocation)
    e2e, kern = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        uvs, scores, status, ms = detection.detect_chessboards(f, scale_factor=S, return_kernel_ms=True)
        e2e.append((time.perf_counter() - t0) * 1e3)
        kern.append(ms)
    dev = torch.empty(f.nbytes, dtype=torch.uint8, device="cuda")
    host = torch.from_numpy(f.reshape(-1))
    copy = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dev.copy_(host)
        torch.cuda.synchronize()
        copy.append((time.perf_counter() - t0) * 1e3)
    e, k, c = float(np.median(e2e)), float(np.median(kern)), float(np.median(copy))
    return {"size": [W, H], "channels": C, "scale_factor": S, "batch": BATCH, "accepted": int((status == 1).sum()), "e2e_ms": e,
            "frames_per_s": BATCH / (e * 1e-3), "kernel_ms": k, "kernel_ms_per_frame": k / BATCH, "h2d_copy_ms": c, "h2d_share_of_call": c / e,
            "call_over_copy_bound": e / c, "cpu_reference": "unmeasured (cv2 absent)"}


def run(cmd, seconds, log):
    with open(log, "w") as fh:
        p = subprocess.run(["timeout", "-k", "10", str(seconds)] + cmd, stdout=subprocess.PIPE, stderr=fh, cwd=ROOT, text=True)
    return p.returncode, p.stdout


def driver(out):
    os.makedirs(out, exist_ok=True)
    results = []
    for W, H in SIZES:
        for C in (1, 3):
            for S in (1.0, 0.5):
                tag = "%dx%d_c%d_s%g" % (W, H, C, S)
                rc, so = run([sys.executable, os.path.abspath(__file__), "--child", str(W), str(H), str(C), str(S)], 600, os.path.join(out, tag + ".err"))
                if rc != 0:
                    print("%s: rc=%d, stopping (see %s.err)" % (tag, rc, tag))
                    return 1
                r = json.loads(so.strip().splitlines()[-1])
                results.append(r)
                print("%-22s %8.1f frames/s  call %8.2f ms  kernels %8.2f ms  copy %7.2f ms  (call / copy %.2f)"
                      % (tag, r["frames_per_s"], r["e2e_ms"], r["kernel_ms"], r["h2d_copy_ms"], r["call_over_copy_bound"]))
    with open(os.path.join(out, "detection_timing.json"), "w") as fh:
        json.dump(results, fh, indent=1)
    # per kernel: one rocprofv3 run of its own (1280x1024 grey, scale 1 and 0.5)
    for S in (1.0, 0.5):
        d = os.path.join(out, "rocprof_s%g" % S)
        rc, _ = run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "det", "--", sys.executable, os.path.abspath(__file__),
                     "--child", "1280", "1024", "1", str(S)], 900, os.path.join(out, "rocprof_s%g.err" % S))
        if rc != 0:
            print("rocprofv3 (scale %g): rc=%d, stopping" % (S, rc))
            return 1
        for st in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            print("rocprofv3 kernel stats, 1280x1024 grey, scale %g (%d frames x 6 calls + warm-up): %s" % (S, BATCH, st))
            with open(st) as fh:
                for line in fh.read().splitlines()[:12]:
                    print("  " + line)
    return 0


if __name__ == "__main__":
    if "--child" in sys.argv:
        i = sys.argv.index("--child")
        W, H, C, S = int(sys.argv[i + 1]), int(sys.argv[i + 2]), int(sys.argv[i + 3]), float(sys.argv[i + 4])
        print(json.dumps(child(W, H, C, S)))
    else:
        out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "build", "detection_timing")
        sys.exit(driver(out))
