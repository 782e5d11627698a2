"""Extrinsics from keypoints on the MI355X: writes profiles/two_view_timing.json.
  pair   one camera pair, 200 000 common points x 512 hypotheses: call time of estimate_relative_pose, kernel time of mcba_two_view_ransac per
         stage (HIP events: prepare, hypotheses, score, finish, pose), and for the scorer (k_hyp_score with TvScore; key k_tv_score) the achieved FP64 rate from the operation count below
  rig    a 6-camera rig at 200 000 points: call time of extrinsics_from_keypoints with and without the refinement, the two-view kernels' share
Scene: scripts/consensus_timing.py's (0.3 px noise, 10 % of the detections missing, one detection displaced by N(0, 40^2) px on 15 % of the points).

  python scripts/two_view_timing.py [--out DIR] [--points N] [--hypotheses H] [--reps R]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
# FP64 operations of the scorer per (point, hypothesis), counted from the text of tv_sampson2 and tv_cost_term (a model, not a profile):
# F x_a 6 fma, the first two of F^T x_b 4 fma, the numerator 2 fma, the denominator 3 fma + 1 mul, its square 1 mul, fast_rcp 1 rcp + 3 fma,
# the quotient 1 mul, the truncated sum 1 add: 18 fma + 3 mul + 1 add + 1 rcp = 23 instructions, 41 flops (an fma counts two)
SCORE_INSTRUCTIONS, SCORE_FLOPS = 23, 41
FP64_VECTOR_PEAK = 78.6e12   # flop/s, the figure DESIGN.md uses
STAGES = ("prepare", "hypotheses", "score", "finish", "pose")


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def main():
    import numpy as np

    from consensus_timing import make_scene
    from multicam_calibration_amd import geometry

    out_dir = arg("--out", os.path.join(ROOT, "profiles"))
    P, H, reps = int(arg("--points", "200000")), int(arg("--hypotheses", "512")), int(arg("--reps", "5"))
    uvs, ext, intr, _ = make_scene(6, P)
    threshold = 2.5
    # ---- one pair
    a, b = np.array(uvs[0]), np.array(uvs[1])
    both = np.isfinite(a).all(1) & np.isfinite(b).all(1)
    a, b = a[both][: P], b[both][: P]
    calls, kernels = [], []
    for _ in range(reps + 1):   # the first call warms up
        t0 = time.perf_counter()
        tr, inl, info = geometry.estimate_relative_pose(a, b, intr[0], intr[1], threshold=threshold, n_hypotheses=H, return_info=True)
        calls.append((time.perf_counter() - t0) * 1e3)
        kernels.append(info["kernel_ms"].copy())
    k = np.median(np.array(kernels[1:]), axis=0)
    M = info["n_common"]
    score_s = k[1 + STAGES.index("score")] * 1e-3
    pair = {"common_points": int(M), "hypotheses": H, "threshold_px": threshold, "inliers": int(info["n_inliers"]), "in_front": int(info["n_in_front"]), "status": int(info["status"]),
            "call_ms": float(np.median(calls[1:])), "all_call_ms": calls[1:], "kernel_ms": float(k[0]), "stage_ms": {s: float(k[1 + i]) for i, s in enumerate(STAGES)},
            "k_tv_score": {"instructions_per_pair": SCORE_INSTRUCTIONS, "flops_per_pair": SCORE_FLOPS, "fp64_flops": float(SCORE_FLOPS) * M * H,
                           "achieved_tflops": SCORE_FLOPS * M * H / score_s / 1e12, "share_of_fp64_vector_peak": SCORE_FLOPS * M * H / score_s / FP64_VECTOR_PEAK}}
    print(json.dumps(pair), flush=True)
    # ---- the rig
    rig = {"cameras": 6, "points": P, "hypotheses": H}
    for refine in (False, True):
        times = []
        for _ in range(3):
            t0 = time.perf_counter()
            r = geometry.extrinsics_from_keypoints(uvs, intr, threshold=threshold, n_hypotheses=H, refine=refine)
            times.append((time.perf_counter() - t0) * 1e3)
        key = "refined" if refine else "chain"
        rig[key] = {"call_ms": float(np.median(times[1:])), "all_call_ms": times[1:], "two_view_kernel_ms": r.info["kernel_ms"], "tree": r.tree, "scales": [e["scale"] for e in r.edges],
                    "inliers": [e["n_inliers"] for e in r.edges]}
        if refine:
            rig[key].update(refinement_kernel_ms=r.refinement.info["kernel_ms"], nfev=r.refinement.nfev, cost0=r.refinement.cost0, cost=r.refinement.cost, message=r.refinement.message)
    print(json.dumps(rig), flush=True)
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "two_view_timing.json"), "w") as fh:
        json.dump({"pair": pair, "rig": rig}, fh, indent=1)


if __name__ == "__main__":
    main()
