"""Extrinsics refinement on the MI355X: wall time of refine_extrinsics (the upload of the detections, the Levenberg-Marquardt loop with its kernels
and host solves, the copies out) and the milliseconds per k_kpba_reduce pass and per k_kpba_step pass (HIP events around each launch, its finishing
kernel included), at 2 M points x 6 cameras and at 200 k points x 24 cameras with the resident reduction, and at 200 k x 24, 48 and 64 cameras with the tiled
one (k_kpba_factors + k_kpba_reduce_tiled; 200 k x 24 with both: the pair to compare).  Warm, median of five.  A pass reads 16 C P + 24 P bytes of detections and
points (the algorithmic traffic); its share of the 8 TB/s HBM roof is reported, not gated.

  python scripts/extrinsics_refinement_timing.py [--out DIR] [--shapes 2000000x6,200000x24,200000x24:tiled,...] [--reduction resident|tiled] [--reps R] [--nfev N]
  python scripts/extrinsics_refinement_timing.py --child PxC[:reduction] --reps R --nfev N      one measurement (JSON on stdout)
  A shape is PxC or PxC:reduction; --reduction names the reduction of the shapes that do not say.
  python scripts/extrinsics_refinement_timing.py --design JSON                      rewrite the marked block of DESIGN.md section 8f-12 from a result file
  --weights: the same shapes again with a random weight plane (uniform in [0.1, 3]): the weighted milliseconds per pass beside
  the unweighted ones in the JSON and in the kpba block of DESIGN.md section 8f-13"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_BYTES_PER_S = 8.0e12
BEGIN, END = "<!-- extrinsics_refinement_timing:begin -->", "<!-- extrinsics_refinement_timing:end -->"


DEFAULT_SHAPES = "2000000x6,200000x24,200000x24:tiled,200000x48:tiled,200000x64:tiled"


def child(shape, reps, nfev, weights=False, reduction="resident"):
    import numpy as np

    sys.path.insert(0, ROOT)
    from multicam_calibration_amd import synth, refine_extrinsics

    if ":" in shape:
        shape, reduction = shape.split(":")
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
    ext = cam[:, 6:].copy()
    ext[1:, :3] += rng.normal(0, 2e-3, (C - 1, 3))   # drifted cameras
    ext[1:, 3:] += rng.normal(0, 1.0, (C - 1, 3))
    X0 = X + rng.normal(0, 0.5, X.shape)
    wall, red, stp, kern, wred, wstp = [], [], [], [], [], []
    W = rng.uniform(0.1, 3.0, (C, P)) if weights else None
    for _ in range(reps + 1):   # the first round warms up
        t0 = time.perf_counter()
        r = refine_extrinsics(uvs, ext, intr, points=X0, loss="soft_l1", max_nfev=nfev, reduction=reduction)
        wall.append((time.perf_counter() - t0) * 1e3)
        red.append(r.info["reduce_ms"] / max(r.info["n_reduce"], 1))
        stp.append(r.info["step_ms"] / max(r.info["n_step"], 1))
        kern.append(r.info["kernel_ms"])
        if weights:
            rw = refine_extrinsics(uvs, ext, intr, points=X0, loss="soft_l1", max_nfev=nfev, weights=W, reduction=reduction)
            wred.append(rw.info["reduce_ms"] / max(rw.info["n_reduce"], 1))
            wstp.append(rw.info["step_ms"] / max(rw.info["n_step"], 1))
    med = lambda v: float(np.median(v[1:]))   # noqa: E731
    nbytes = 16.0 * C * P + 24.0 * P
    out = {"shape": shape, "points": P, "cameras": C, "reduction": reduction, "band_pairs": r.info["band_pairs"], "used_points": int((r.point_status == 1).sum()), "group": r.info["group"], "max_nfev": nfev, "nfev": r.nfev, "njev": r.njev,
           "n_reduce": r.info["n_reduce"], "n_step": r.info["n_step"], "status": r.status, "cost0": r.cost0, "cost": r.cost,
           "call_ms": med(wall), "kernel_ms": med(kern), "reduce_ms_per_pass": med(red), "step_ms_per_pass": med(stp), "all_reduce_ms_per_pass": red[1:], "all_step_ms_per_pass": stp[1:],
           "pass_bytes": nbytes, "reduce_hbm_fraction": nbytes / (med(red) * 1e-3) / HBM_BYTES_PER_S, "step_hbm_fraction": (nbytes + 24.0 * P) / (med(stp) * 1e-3) / HBM_BYTES_PER_S}
    if weights:
        out["weighted"] = {"reduce_ms_per_pass": med(wred), "step_ms_per_pass": med(wstp), "reduce_ratio": med(wred) / med(red), "step_ratio": med(wstp) / med(stp), "nfev": rw.nfev}
    print(json.dumps(out))


def design_block(results):
    lines = [BEGIN, "| points x cameras | reduction | points per group | reduce pass (ms) | of the HBM roof | `k_kpba_step` pass (ms) | of the HBM roof | whole call (ms), evaluations |",
             "|---|---|---|---|---|---|---|---|"]
    for r in results:
        lines.append(f"| {r['points']} x {r['cameras']} | {r.get('reduction', 'resident')} | {r['group']} | {r['reduce_ms_per_pass']:.2f} | {100 * r['reduce_hbm_fraction']:.1f} % | {r['step_ms_per_pass']:.2f} | "
                     f"{100 * r['step_hbm_fraction']:.1f} % | {r['call_ms']:.0f}, {r['nfev']} |")
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
    return [f"| {r['points']} x {r['cameras']} | {r['reduce_ms_per_pass']:.2f} | {r['weighted']['reduce_ms_per_pass']:.2f} | {r['weighted']['reduce_ratio']:.2f} | {r['step_ms_per_pass']:.2f} | "
            f"{r['weighted']['step_ms_per_pass']:.2f} | {r['weighted']['step_ratio']:.2f} |" for r in results if "weighted" in r]


W_HEADER = "| points x cameras | `k_kpba_reduce` pass (ms) | weighted (ms) | ratio | `k_kpba_step` pass (ms) | weighted (ms) | ratio |"


def write_design(path):
    results = json.load(open(path))
    design = os.path.join(ROOT, "DESIGN.md")
    text = open(design).read()
    if BEGIN not in text or END not in text:
        raise SystemExit("DESIGN.md has no extrinsics_refinement_timing block")
    a, b = text.index(BEGIN), text.index(END) + len(END)
    open(design, "w").write(text[:a] + design_block(results) + text[b:])
    if any("weighted" in r for r in results):
        write_weights_block("kpba", W_HEADER, weights_rows(results))


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def main():
    out_dir = arg("--out", os.path.join(ROOT, "profiles"))
    shapes = [sh if ":" in sh else sh + ":" + arg("--reduction", "resident") for sh in arg("--shapes", DEFAULT_SHAPES).split(",")]
    reps, nfev = arg("--reps", "5"), arg("--nfev", "6")
    os.makedirs(out_dir, exist_ok=True)
    results = []
    for shape in shapes:
        r = subprocess.run(["timeout", "-k", "10", "420", sys.executable, __file__, "--child", shape, "--reps", reps, "--nfev", nfev] + (["--weights"] if "--weights" in sys.argv else []), cwd=ROOT, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-3000:] + r.stderr[-3000:])
            raise SystemExit("step failed (exit %d): %s" % (r.returncode, shape))
        results.append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(json.dumps({k: v for k, v in results[-1].items() if not k.startswith("all_")}), flush=True)
        with open(os.path.join(out_dir, "extrinsics_refinement_timing.json"), "w") as fh:
            json.dump(results, fh, indent=1)
    print(design_block(results))
    if "--weights" in sys.argv:
        write_weights_block("kpba", W_HEADER, weights_rows(results))


if __name__ == "__main__":
    if "--child" in sys.argv:
        child(arg("--child", "2000000x6"), int(arg("--reps", "5")), int(arg("--nfev", "6")), "--weights" in sys.argv, arg("--reduction", "resident"))
    elif "--design" in sys.argv:
        write_design(arg("--design", ""))
    else:
        main()
