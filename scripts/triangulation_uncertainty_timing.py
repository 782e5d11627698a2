"""Triangulation uncertainty on the MI355X: wall time of triangulation_uncertainty (the upload of the detections, the kernels, the copies out,
the host's unpacking) and kernel_ms of its kernels (HIP events), with a camera covariance (k_tricov_point + k_tricov_cal) and without one
(k_tricov_point + k_tricov_scale), at 2 M points x 6 cameras and at 200 k points x 24 cameras.  Warm, median of five.  The calibration term's
product Z = G Sigma_cc costs 2 * 3 * n^2 FP64 flops per point on the matrix cores (78.6 TFLOP/s); its share of that roof is reported, not gated.

  python scripts/triangulation_uncertainty_timing.py [--out DIR] [--shapes 2000000x6,200000x24] [--reps R]
  python scripts/triangulation_uncertainty_timing.py --child PxC --reps R        one measurement (JSON on stdout)
  python scripts/triangulation_uncertainty_timing.py --design JSON               rewrite the marked block of DESIGN.md section 8f-11 from a result file
  --weights: the same shapes again with a random weight plane (uniform in [0.1, 3]): the weighted kernel times beside the
  unweighted ones in the JSON and in the tricov block of DESIGN.md section 8f-13"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP64_MFMA_FLOPS = 78.6e12
BEGIN, END = "<!-- triangulation_uncertainty_timing:begin -->", "<!-- triangulation_uncertainty_timing:end -->"


def child(shape, reps, weights=False):
    import numpy as np

    sys.path.insert(0, ROOT)
    from multicam_calibration_amd import synth, triangulation_uncertainty

    P, C = (int(v) for v in shape.split("x"))
    p = synth.make_problem(C, 2, noise=0.0)
    cam = p["true_cam"]
    rng = np.random.default_rng(5)
    T = synth._T(p["true_poses"][0])
    X = rng.normal(0, 60, (P, 3)) @ T[:3, :3].T + T[:3, 3]
    uvs = [synth.project(cam[c:c + 1], np.zeros((1, 6)), X)[0, 0] + rng.normal(0, 0.3, (P, 2)) for c in range(C)]
    for u in uvs:
        u[rng.uniform(size=P) < 0.1] = np.nan
    intr = [(np.array([[c[0], 0, c[2]], [0, c[1], c[3]], [0, 0, 1.0]]), np.r_[c[4:6], 0, 0, 0]) for c in cam]
    ext = cam[:, 6:]
    n = 12 * C
    M = rng.normal(size=(n, n + 4))
    s = np.tile(np.r_[1.0, 1.0, 0.7, 0.7, 1e-3, 2e-3, 1e-3, 1e-3, 1e-3, 0.5, 0.5, 0.8], C)
    S = (M @ M.T) / (n + 4) * np.outer(s, s)
    S = 0.5 * (S + S.T)
    wall = {True: [], False: []}
    kern = {True: [], False: []}
    wkern = {True: [], False: []}
    W = rng.uniform(0.1, 3.0, (C, P)) if weights else None
    for _ in range(reps + 1):   # the first round warms up
        for with_cov in (True, False):
            t0 = time.perf_counter()
            u = triangulation_uncertainty(X, uvs, ext, intr, camera_covariance=S if with_cov else None, sigma=0.3)
            wall[with_cov].append((time.perf_counter() - t0) * 1e3)
            kern[with_cov].append(u.info["kernel_ms"])
            if weights:
                wkern[with_cov].append(triangulation_uncertainty(X, uvs, ext, intr, camera_covariance=S if with_cov else None, sigma=0.3, weights=W).info["kernel_ms"])
    med = lambda v: float(np.median(v[1:]))   # noqa: E731
    cal_ms = med(kern[True]) - med(kern[False])   # (k_tricov_cal against k_tricov_scale, which streams 96 bytes per point)
    flops = 2.0 * 3 * n * n * P
    out = {"shape": shape, "points": P, "cameras": C, "n": n, "usable_points": int((u.status == 1).sum()),
           "call_ms_with_covariance": med(wall[True]), "kernel_ms_with_covariance": med(kern[True]),
           "call_ms_detection_only": med(wall[False]), "kernel_ms_detection_only": med(kern[False]),
           "all_kernel_ms_with_covariance": kern[True][1:], "all_kernel_ms_detection_only": kern[False][1:],
           "gemm_flops": flops, "mfma_fraction": flops / (max(cal_ms, 1e-9) * 1e-3) / FP64_MFMA_FLOPS}
    if weights:
        out["weighted"] = {"kernel_ms_with_covariance": med(wkern[True]), "kernel_ms_detection_only": med(wkern[False]), "ratio_with_covariance": med(wkern[True]) / med(kern[True]),
                           "ratio_detection_only": med(wkern[False]) / med(kern[False])}
    print(json.dumps(out))


def design_block(results):
    lines = [BEGIN, "| points x cameras | call, with Σ_cc (ms) | kernels, with Σ_cc (ms) | call, detection term only (ms) | kernels, detection term only (ms) | `Z = G Σ_cc` against the FP64 matrix peak |",
             "|---|---|---|---|---|---|"]
    for r in results:
        lines.append(f"| {r['points']} x {r['cameras']} | {r['call_ms_with_covariance']:.1f} | {r['kernel_ms_with_covariance']:.2f} | {r['call_ms_detection_only']:.1f} | "
                     f"{r['kernel_ms_detection_only']:.2f} | {100 * r['mfma_fraction']:.1f} % |")
    lines.append(END)
    return "\n".join(lines)


W_BEGIN, W_END = "<!-- weights_timing:%s:begin -->", "<!-- weights_timing:%s:end -->"


def write_weights_block(key, header, rows):
    """rewrite this script's marked block of DESIGN.md section 8f-13 (weighted against unweighted kernel times from the same build)"""
    design = os.path.join(ROOT, "DESIGN.md")
    text = open(design).read()
    begin, end = W_BEGIN % key, W_END % key
    if begin not in text or end not in text:
        raise SystemExit("DESIGN.md has no weights_timing:%s block" % key)
    a, b = text.index(begin), text.index(end) + len(end)
    open(design, "w").write(text[:a] + "\n".join([begin, header, "|" + "---|" * (header.count("|") - 1)] + rows + [end]) + text[b:])


def weights_rows(results):
    return [f"| {r['points']} x {r['cameras']} | {r['kernel_ms_detection_only']:.2f} | {r['weighted']['kernel_ms_detection_only']:.2f} | {r['weighted']['ratio_detection_only']:.2f} | "
            f"{r['kernel_ms_with_covariance']:.2f} | {r['weighted']['kernel_ms_with_covariance']:.2f} | {r['weighted']['ratio_with_covariance']:.2f} |" for r in results if "weighted" in r]


W_HEADER = "| points x cameras | `k_tricov_point` + `k_tricov_scale` (ms) | weighted (ms) | ratio | `k_tricov_point` + `k_tricov_cal` (ms) | weighted (ms) | ratio |"


def write_design(path):
    results = json.load(open(path))
    design = os.path.join(ROOT, "DESIGN.md")
    text = open(design).read()
    if BEGIN not in text or END not in text:
        raise SystemExit("DESIGN.md has no triangulation_uncertainty_timing block")
    a, b = text.index(BEGIN), text.index(END) + len(END)
    open(design, "w").write(text[:a] + design_block(results) + text[b:])
    if any("weighted" in r for r in results):
        write_weights_block("tricov", W_HEADER, weights_rows(results))


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def main():
    out_dir = arg("--out", os.path.join(ROOT, "profiles"))
    shapes = arg("--shapes", "2000000x6,200000x24").split(",")
    reps = arg("--reps", "5")
    os.makedirs(out_dir, exist_ok=True)
    results = []
    for shape in shapes:
        r = subprocess.run(["timeout", "-k", "10", "420", sys.executable, __file__, "--child", shape, "--reps", reps] + (["--weights"] if "--weights" in sys.argv else []), cwd=ROOT, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-3000:] + r.stderr[-3000:])
            raise SystemExit("step failed (exit %d): %s" % (r.returncode, shape))
        results.append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(json.dumps({k: v for k, v in results[-1].items() if not k.startswith("all_")}), flush=True)
        with open(os.path.join(out_dir, "triangulation_uncertainty_timing.json"), "w") as fh:
            json.dump(results, fh, indent=1)
    print(design_block(results))
    if "--weights" in sys.argv:
        write_weights_block("tricov", W_HEADER, weights_rows(results))


if __name__ == "__main__":
    if "--child" in sys.argv:
        child(arg("--child", "2000000x6"), int(arg("--reps", "5")), "--weights" in sys.argv)
    elif "--design" in sys.argv:
        write_design(arg("--design", ""))
    else:
        main()
