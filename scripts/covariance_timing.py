"""Calibration uncertainty on the MI355X: wall time of Problem.covariance (one linearisation, the Schur reduction with lambda = 0, the
covariance kernels, the copies out) and kernel_ms of the covariance kernels (HIP events: k_cov_cam's three launches + k_cov_frames), with and
without the frame blocks -- k_cov_frames is the difference --, at 6 x 10 000 x 54 and at the 24 x 6 250 x 200 shard.  Warm, median of five.
Against the roof that binds: at the first shape the W rows of the records are read once (HBM, 8.0 TB/s), at the second the product
Z = Y Sigma_cc costs 6 F n^2 FP64 FMA on the matrix cores (78.6 TFLOP/s).  Yardstick: one LM tick at the same shape (103 us / 653 us on record,
DESIGN.md section 5).

  python scripts/covariance_timing.py [--out DIR] [--shapes 6x10000x54,24x6250x200] [--reps R]
  python scripts/covariance_timing.py --child CxFxN --reps R            one measurement (JSON on stdout)
  python scripts/covariance_timing.py --design JSON                     rewrite the marked block of DESIGN.md section 8 from a result file"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_BYTES_PER_S = 8.0e12
FP64_MFMA_FLOPS = 78.6e12
LM_TICK_US = {"6x10000x54": 103.0, "24x6250x200": 653.0}
BOARDS = {54: (6, 9), 200: (10, 20)}
BEGIN, END = "<!-- covariance_timing:begin -->", "<!-- covariance_timing:end -->"


def child(shape, reps):
    import numpy as np

    sys.path.insert(0, ROOT)
    from multicam_calibration_amd import ops, synth

    C, F, N = (int(v) for v in shape.split("x"))
    rows, cols = BOARDS[N]
    p = synth.make_problem(C, F, rows=rows, cols=cols)
    x = np.concatenate([p["true_cam"].ravel(), p["true_poses"].ravel()])
    prob = ops.Problem(p["uvs"], p["obj"], loss="soft_l1")
    prob.set_params(0, x)
    wall, k_all, k_cam = [], [], []
    for _ in range(reps + 1):   # the first round warms up
        t0 = time.perf_counter()
        _, _, info = prob.covariance(0, 0)
        wall.append((time.perf_counter() - t0) * 1e3)
        k_all.append(float(info[5]))
        _, _, info = prob.covariance(0, 0, frames=False)
        k_cam.append(float(info[5]))
    prob.close()
    n = 12 * C
    med = lambda v: float(np.median(v[1:]))   # noqa: E731
    frames_ms = med(k_all) - med(k_cam)
    rec_bytes = C * ((F + 63) // 64 * 64) * 72 * 8
    flops = 2.0 * 6 * F * n * n
    out = {"shape": shape, "n": n, "call_ms": med(wall), "kernel_ms": med(k_all), "k_cov_cam_ms": med(k_cam), "k_cov_frames_ms": frames_ms, "all_kernel_ms": k_all[1:], "all_call_ms": wall[1:],
           "record_bytes": rec_bytes, "hbm_fraction": rec_bytes / (frames_ms * 1e-3) / HBM_BYTES_PER_S, "gemm_flops": flops, "mfma_fraction": flops / (frames_ms * 1e-3) / FP64_MFMA_FLOPS,
           "lm_tick_us": LM_TICK_US.get(shape)}
    out["binding_roof"] = "HBM" if out["hbm_fraction"] >= out["mfma_fraction"] else "FP64 MFMA"
    print(json.dumps(out))


def design_block(results):
    lines = [BEGIN, "| shape | call (ms) | `k_cov_cam` (ms) | `k_cov_frames` (ms) | binding roof | fraction of it | one LM tick (us) |", "|---|---|---|---|---|---|---|"]
    for r in results:
        frac = max(r["hbm_fraction"], r["mfma_fraction"])
        lines.append(f"| {r['shape'].replace('x', ' x ')} | {r['call_ms']:.2f} | {r['k_cov_cam_ms']:.3f} | {r['k_cov_frames_ms']:.3f} | {r['binding_roof']} | {100 * frac:.1f} % | {r['lm_tick_us']:.0f} |")
    lines.append(END)
    return "\n".join(lines)


def write_design(path):
    results = json.load(open(path))
    design = os.path.join(ROOT, "DESIGN.md")
    text = open(design).read()
    if BEGIN not in text or END not in text:
        raise SystemExit("DESIGN.md has no covariance_timing block")
    a, b = text.index(BEGIN), text.index(END) + len(END)
    open(design, "w").write(text[:a] + design_block(results) + text[b:])


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def main():
    out_dir = arg("--out", os.path.join(ROOT, "build", "covariance_timing"))
    shapes = arg("--shapes", "6x10000x54,24x6250x200").split(",")
    reps = arg("--reps", "5")
    os.makedirs(out_dir, exist_ok=True)
    results = []
    for shape in shapes:
        r = subprocess.run(["timeout", "-k", "10", "420", sys.executable, __file__, "--child", shape, "--reps", reps], cwd=ROOT, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-3000:] + r.stderr[-3000:])
            raise SystemExit("step failed (exit %d): %s" % (r.returncode, shape))
        results.append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(json.dumps({k: v for k, v in results[-1].items() if not k.startswith("all_")}), flush=True)
        with open(os.path.join(out_dir, "covariance_timing.json"), "w") as fh:
            json.dump(results, fh, indent=1)
    print(design_block(results))


if __name__ == "__main__":
    if "--child" in sys.argv:
        child(arg("--child", "6x10000x54"), int(arg("--reps", "5")))
    elif "--design" in sys.argv:
        write_design(arg("--design", ""))
    else:
        main()
