"""Camera refinement with free intrinsics on the MI355X: wall time of refine_cameras (the upload of the detections, the Levenberg-Marquardt loop with
its kernels and host solves, the copies out) and the milliseconds per k_kpcam_reduce pass and per k_kpcam_step pass (HIP events around each launch,
its finishing kernel included), at 200 k points x 6 and x 12 cameras, beside refine_extrinsics on the same input (same process, same scene, same
start: the yardstick; at 12 cameras too).  Warm, median of five.  No time is fixed in advance: what is reported is the ratio 12 rows / 6 rows per
pass -- the matrix-core work of the reduce is 4 x per point, the item work roughly 3 x (DESIGN.md section 8f-15 explains what is beyond that).

  python scripts/camera_refinement_timing.py [--out DIR] [--shapes 200000x6,200000x12] [--reps R] [--nfev N]
  python scripts/camera_refinement_timing.py --child PxC --reps R --nfev N      one measurement (JSON on stdout)"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_SHAPES = "200000x6,200000x12"


def child(shape, reps, nfev):
    import numpy as np

    sys.path.insert(0, ROOT)
    from multicam_calibration_amd import synth, refine_cameras, refine_extrinsics

    P, C = (int(v) for v in shape.split("x"))
    p = synth.make_problem(C, 2, noise=0.0)
    cam = p["true_cam"]
    rng = np.random.default_rng(5)
    T = synth._T(p["true_poses"][0])
    X = rng.normal(0, 60, (P, 3)) @ T[:3, :3].T + T[:3, 3]
    uvs = [synth.project(cam[c:c + 1], np.zeros((1, 6)), X)[0, 0] + rng.normal(0, 0.3, (P, 2)) for c in range(C)]
    for u in uvs:
        u[rng.uniform(size=P) < 0.1] = np.nan
    nominal = cam[:, :6] * (1 + np.r_[rng.normal(0, 2e-3, 2), np.zeros(4)])   # nominal focal lengths, 0.2 % off
    intr = [(np.array([[c[0], 0, c[2]], [0, c[1], c[3]], [0, 0, 1.0]]), np.r_[c[4:6], 0, 0, 0]) for c in nominal]
    ext = cam[:, 6:].copy()
    ext[1:, :3] += rng.normal(0, 2e-3, (C - 1, 3))   # drifted cameras
    ext[1:, 3:] += rng.normal(0, 1.0, (C - 1, 3))
    X0 = X + rng.normal(0, 0.5, X.shape)
    std = np.r_[0.005 * nominal[0, :2], 2.0, 2.0, 0.005, 0.005]
    runs = {"refine_cameras": lambda: refine_cameras(uvs, ext, intr, free_intrinsics=("focal", "principal", "distortion"), intrinsics_prior_std=std, points=X0, loss="soft_l1", max_nfev=nfev),
            "refine_extrinsics": lambda: refine_extrinsics(uvs, ext, intr, points=X0, loss="soft_l1", max_nfev=nfev)}
    out = {"shape": shape, "points": P, "cameras": C, "max_nfev": nfev}
    for key, run in runs.items():
        wall, red, stp, kern = [], [], [], []
        for _ in range(reps + 1):   # the first round warms up
            t0 = time.perf_counter()
            r = run()
            wall.append((time.perf_counter() - t0) * 1e3)
            red.append(r.info["reduce_ms"] / max(r.info["n_reduce"], 1))
            stp.append(r.info["step_ms"] / max(r.info["n_step"], 1))
            kern.append(r.info["kernel_ms"])
        med = lambda v: float(np.median(v[1:]))   # noqa: E731
        out[key] = {"group": r.info["group"], "nfev": r.nfev, "njev": r.njev, "n_reduce": r.info["n_reduce"], "n_step": r.info["n_step"], "status": r.status, "cost0": r.cost0, "cost": r.cost,
                    "call_ms": med(wall), "kernel_ms": med(kern), "reduce_ms_per_pass": med(red), "step_ms_per_pass": med(stp), "evaluation_ms": med(red) + med(stp),
                    "all_reduce_ms_per_pass": red[1:], "all_step_ms_per_pass": stp[1:], "all_call_ms": wall[1:]}
    a, b = out["refine_cameras"], out["refine_extrinsics"]
    out["ratio"] = {"reduce": a["reduce_ms_per_pass"] / b["reduce_ms_per_pass"], "step": a["step_ms_per_pass"] / b["step_ms_per_pass"], "evaluation": a["evaluation_ms"] / b["evaluation_ms"],
                    "call_per_evaluation": (a["call_ms"] / a["nfev"]) / (b["call_ms"] / b["nfev"])}
    print(json.dumps(out))


def table(results):
    lines = ["| points x cameras | call | points per group | reduce pass (ms) | step pass (ms) | evaluation (ms) | whole call (ms), evaluations |", "|---|---|---|---|---|---|---|"]
    for r in results:
        for key, name in (("refine_extrinsics", "`refine_extrinsics`"), ("refine_cameras", "`refine_cameras`")):
            v = r[key]
            lines.append(f"| {r['points']} x {r['cameras']} | {name} | {v['group']} | {v['reduce_ms_per_pass']:.2f} | {v['step_ms_per_pass']:.2f} | {v['evaluation_ms']:.2f} | {v['call_ms']:.0f}, {v['nfev']} |")
        q = r["ratio"]
        lines.append(f"| | ratio 12 rows / 6 rows | | {q['reduce']:.2f} | {q['step']:.2f} | {q['evaluation']:.2f} | {q['call_per_evaluation']:.2f} per evaluation |")
    return "\n".join(lines)


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def main():
    out_dir = arg("--out", os.path.join(ROOT, "profiles"))
    reps, nfev = arg("--reps", "5"), arg("--nfev", "6")
    os.makedirs(out_dir, exist_ok=True)
    results = []
    for shape in arg("--shapes", DEFAULT_SHAPES).split(","):
        r = subprocess.run(["timeout", "-k", "10", "420", sys.executable, __file__, "--child", shape, "--reps", reps, "--nfev", nfev], cwd=ROOT, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-3000:] + r.stderr[-3000:])
            raise SystemExit("step failed (exit %d): %s" % (r.returncode, shape))
        results.append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(json.dumps({k: (v if not isinstance(v, dict) else {q: w for q, w in v.items() if not q.startswith("all_")}) for k, v in results[-1].items()}), flush=True)
        with open(os.path.join(out_dir, "camera_refinement_timing.json"), "w") as fh:
            json.dump(results, fh, indent=1)
    print(table(results))


if __name__ == "__main__":
    if "--child" in sys.argv:
        child(arg("--child", "200000x6"), int(arg("--reps", "5")), int(arg("--nfev", "6")))
    else:
        main()
