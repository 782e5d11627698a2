"""The two hypothesis generators of the two-view RANSAC side by side on the MI355X, at equal numbers of scored candidates: writes
profiles/two_view_5point_timing.json.
  per point count: solver="5point" with S samples scores n live candidates (about 4.3 S); solver="8point" is then run with n hypotheses.
  For both: call time of estimate_relative_pose, kernel time per stage (HIP events: prepare, hypotheses -- for "5point" with the compaction and
  the read-back of the packed count --, score, finish, pose), inliers.
Scene: the thin slab of SURVEY.md section 8f-17 (N(0, 1) x (60, 60, 5) mm where the board would be, 0.3 px noise), two cameras of synth.make_problem.

  python scripts/two_view_5point_timing.py [--out DIR] [--points N,N,...] [--samples S] [--reps R]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STAGES = ("prepare", "hypotheses", "score", "finish", "pose")


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def slab(P, seed=13, noise=0.3, zs=5.0):
    import numpy as np

    from multicam_calibration_amd import synth

    p = synth.make_problem(2, 2, seed=seed, noise=0.0)
    cam = p["true_cam"]
    rng = np.random.default_rng(seed + 7)
    T = synth._T(p["true_poses"][0])
    X = (rng.normal(0, 1, (P, 3)) * np.array([60.0, 60.0, zs])) @ T[:3, :3].T + T[:3, 3]
    uvs = np.stack([synth.project(cam[c:c + 1], np.zeros((1, 6)), X)[0, 0] for c in range(2)])
    uvs += rng.normal(0, noise, uvs.shape)
    intr = [(np.array([[c[0], 0, c[2]], [0, c[1], c[3]], [0, 0, 1.0]]), np.r_[c[4:6], 0, 0, 0]) for c in cam]
    return uvs, intr


def timed(fn, reps):
    import numpy as np

    calls, kernels, info = [], [], None
    for _ in range(reps + 1):   # the first call warms up
        t0 = time.perf_counter()
        _, _, info = fn()
        calls.append((time.perf_counter() - t0) * 1e3)
        kernels.append(info["kernel_ms"].copy())
    k = np.median(np.array(kernels[1:]), axis=0)
    return {"call_ms": float(np.median(calls[1:])), "kernel_ms": float(k[0]), "stage_ms": {s: float(k[1 + i]) for i, s in enumerate(STAGES)}, "scored": int(info["n_scored"]),
            "inliers": int(info["n_inliers"]), "common_points": int(info["n_common"]), "status": int(info["status"])}


def main():
    from multicam_calibration_amd import geometry

    out_dir = arg("--out", os.path.join(ROOT, "profiles"))
    points = [int(p) for p in arg("--points", "300,20000,200000").split(",")]
    S, reps = int(arg("--samples", "128")), int(arg("--reps", "5"))
    rows = []
    for P in points:
        uvs, intr = slab(P)
        five = timed(lambda: geometry.estimate_relative_pose(uvs[0], uvs[1], intr[0], intr[1], threshold=2.5, n_hypotheses=S, solver="5point", return_info=True), reps)
        H8 = min(five["scored"], geometry.MAX_HYPOTHESES)
        eight = timed(lambda: geometry.estimate_relative_pose(uvs[0], uvs[1], intr[0], intr[1], threshold=2.5, n_hypotheses=H8, solver="8point", return_info=True), reps)
        rows.append({"points": P, "samples_5point": S, "5point": five, "8point": eight})
        print(json.dumps(rows[-1]), flush=True)
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "two_view_5point_timing.json"), "w") as fh:
        json.dump({"threshold_px": 2.5, "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
