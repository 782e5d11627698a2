"""The two hypothesis generators of the resection on the MI355X: writes profiles/p3p_resection_timing.json.
Per shape (cameras x points; by default 6 x 300, the size of the tests' six-camera scene, and 64 x 100 000) a fresh child process; in it, for 64,
256 and 1024 samples and for either solver, the kernel time per stage of mcba_resect_ransac / mcba_resect_ransac_p3p (HIP events: prepare,
hypotheses, score, finish, mask): the median of `reps` calls after one that warms up.  Scene: scripts/consensus_timing.py's (0.3 px noise, 10 %
of the detections missing, one detection displaced by N(0, 40^2) px on 15 % of the points); every camera is resected against the true points.

How to read it: the generator stage (k_rs3_hypotheses against k_rs_hypotheses) at equal sample count; the whole RANSAC at equal sample count,
where "p3p" fills and scores FOUR table slots per sample -- 4 x the work of k_hyp_score, k_hyp_finish and k_rs_winner -- so at equal sample count
it is the dearer call whenever the scorer dominates.  What "p3p" buys is that far fewer samples are needed.

  python scripts/p3p_resection_timing.py [--out DIR] [--reps R] [--big-reps R]"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
STAGES = ("prepare", "hypotheses", "score", "finish", "mask")
SHAPES = ((6, 300), (64, 100000))
SAMPLES = (64, 256, 1024)


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def child(C, P, reps):
    import numpy as np

    from consensus_timing import make_scene
    from multicam_calibration_amd import geometry

    uvs, ext, intr, X = make_scene(C, P, seed=16)
    centre = lambda e: -geometry.rodrigues(e[:3]).T @ e[3:]
    out = {"cameras": C, "points": P, "threshold_px": 2.5, "reps": reps, "runs": []}
    for H in SAMPLES:
        for solver in geometry.RESECTION_SOLVERS:
            kernels = []
            for _ in range(reps + 1):   # the first call warms up
                r = geometry.resect_cameras(X, uvs, intr, threshold=2.5, n_hypotheses=H, refine=False, solver=solver)
                kernels.append(r.info["kernel_ms"]["ransac"].copy())
            k = np.median(np.array(kernels[1:]), axis=0)
            out["runs"].append({"solver": solver, "samples": H, "table_slots": H * (4 if solver == "p3p" else 1), "ransac_kernel_ms": float(k[0]),
                                "stage_ms": {s: float(k[1 + i]) for i, s in enumerate(STAGES)}, "cameras_of_status_1": int((r.status == 1).sum()),
                                "least_inlier_share": float((r.n_inliers / r.n_usable).min()), "worst_centre_error_mm": float(max(np.linalg.norm(centre(r.extrinsics[c]) - centre(ext[c])) for c in range(C)))})
            print(f"{C} x {P}, {H} samples, {solver}: {k[0]:.3f} ms", file=sys.stderr, flush=True)
    print("RESULT " + json.dumps(out), flush=True)


def main():
    if "--child" in sys.argv:
        C, P, reps = (int(v) for v in sys.argv[sys.argv.index("--child") + 1: sys.argv.index("--child") + 4])
        return child(C, P, reps)
    out_dir, reps, big = arg("--out", os.path.join(ROOT, "profiles")), int(arg("--reps", "5")), int(arg("--big-reps", "5"))
    shapes = []
    for C, P in SHAPES:   # a fresh process per shape: nothing of one shape's allocations or warm-up reaches the next
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(C), str(P), str(reps if C * P < 10 ** 6 else big)], stdout=subprocess.PIPE, text=True, timeout=1100)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout)
            raise SystemExit(f"shape {C} x {P} failed with status {r.returncode}")
        shapes.append(json.loads(line[0][7:]))
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "p3p_resection_timing.json"), "w") as fh:
        json.dump({"shapes": shapes}, fh, indent=1)
    for sh in shapes:
        for run in sh["runs"]:
            print(sh["cameras"], "x", sh["points"], run["samples"], run["solver"], f"{run['ransac_kernel_ms']:.3f} ms:", " ".join(f"{s} {v:.3f}" for s, v in run["stage_ms"].items()))


if __name__ == "__main__":
    main()
