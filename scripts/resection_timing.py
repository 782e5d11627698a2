"""Camera resection on the MI355X: writes profiles/resection_timing.json.
Per shape (cameras x points x hypotheses; by default 6 x 200 000 x 512 and 24 x 20 000 x 256) a fresh child process: the call time of
resect_cameras with and without the polish, the kernel time of mcba_resect_ransac per stage (HIP events: prepare, hypotheses, score, finish, mask)
and the span and the evaluations of mcba_resect_refine; for the scorer (k_hyp_score with RsScore; key k_rs_score) the achieved FP64 rate from the operation count below.
Scene: scripts/consensus_timing.py's (0.3 px noise, 10 % of the detections missing, one detection displaced by N(0, 40^2) px on 15 % of the points);
every camera is resected against the true points.  The call does not exist in earlier versions: the numbers are recorded, nothing is compared.

  python scripts/resection_timing.py [--out DIR] [--reps R]"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
# FP64 operations of the scorer per (point, hypothesis), counted from the text of rs_error2 and tv_cost_term (a model, not a profile): three rows of
# K [R | t] 9 fma, fast_rcp 1 rcp + 3 fma, the two differences 2 fma, their squares 1 fma + 1 mul, the truncated sum 1 add:
# 15 fma + 1 mul + 1 add + 1 rcp = 18 instructions, 33 flops (an fma counts two)
SCORE_INSTRUCTIONS, SCORE_FLOPS = 18, 33
FP64_VECTOR_PEAK = 78.6e12   # flop/s, the figure DESIGN.md uses
STAGES = ("prepare", "hypotheses", "score", "finish", "mask")
SHAPES = ((6, 200000, 512), (24, 20000, 256))


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def child(C, P, H, reps):
    import numpy as np

    from consensus_timing import make_scene
    from multicam_calibration_amd import geometry

    uvs, ext, intr, X = make_scene(C, P)
    out = {"cameras": C, "points": P, "hypotheses": H, "threshold_px": 2.5}
    for refine in (False, True):
        calls, kernels, polish = [], [], []
        for _ in range(reps + 1):   # the first call warms up
            t0 = time.perf_counter()
            r = geometry.resect_cameras(X, uvs, intr, threshold=2.5, n_hypotheses=H, refine=refine)
            calls.append((time.perf_counter() - t0) * 1e3)
            kernels.append(r.info["kernel_ms"]["ransac"].copy())
            polish.append(r.info["kernel_ms"]["polish"])
        k = np.median(np.array(kernels[1:]), axis=0)
        centre = lambda e: -geometry.rodrigues(e[:3]).T @ e[3:]
        rec = {"call_ms": float(np.median(calls[1:])), "all_call_ms": calls[1:], "ransac_kernel_ms": float(k[0]), "stage_ms": {s: float(k[1 + i]) for i, s in enumerate(STAGES)},
               "status": [int(s) for s in r.status], "usable": [int(n) for n in r.n_usable], "inliers": [int(n) for n in r.n_inliers],
               "centre_error_mm": [float(np.linalg.norm(centre(r.extrinsics[c]) - centre(ext[c]))) for c in range(C)]}
        if refine:
            rec.update(polish_span_ms=float(np.median(polish[1:])), polish_evaluations=int(r.info.get("polish_evaluations", 0)), nfev=[int(n) for n in r.nfev], lm_status=[int(s) for s in r.lm_status])
        else:
            pairs = float(sum(r.n_usable)) * H
            score_s = k[1 + STAGES.index("score")] * 1e-3
            rec["k_rs_score"] = {"instructions_per_pair": SCORE_INSTRUCTIONS, "flops_per_pair": SCORE_FLOPS, "usable_point_hypothesis_pairs": pairs, "achieved_tflops": SCORE_FLOPS * pairs / score_s / 1e12,
                                 "share_of_fp64_vector_peak": SCORE_FLOPS * pairs / score_s / FP64_VECTOR_PEAK}
        out["polished" if refine else "ransac"] = rec
    print("RESULT " + json.dumps(out), flush=True)


def main():
    if "--child" in sys.argv:
        C, P, H, reps = (int(v) for v in sys.argv[sys.argv.index("--child") + 1: sys.argv.index("--child") + 5])
        return child(C, P, H, reps)
    out_dir, reps = arg("--out", os.path.join(ROOT, "profiles")), int(arg("--reps", "5"))
    shapes = []
    for C, P, H in SHAPES:   # a fresh process per shape: nothing of one shape's allocations or warm-up reaches the next
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(C), str(P), str(H), str(reps)], capture_output=True, text=True, timeout=600)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit(f"shape {C} x {P} x {H} failed with status {r.returncode}")
        shapes.append(json.loads(line[0][7:]))
        print(json.dumps(shapes[-1]), flush=True)
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "resection_timing.json"), "w") as fh:
        json.dump({"shapes": shapes}, fh, indent=1)


if __name__ == "__main__":
    main()
