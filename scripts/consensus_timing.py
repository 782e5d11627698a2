"""Consensus triangulation on the MI355X: kernel_ms (HIP events) of mcba_triangulate_consensus and, from the same run and the same detections, of
mcba_triangulate_refine started from the median of pairs -- the same number of two-view null vectors --, their ratio, and the instruction-count
model (null vectors + hypotheses x cameras projections + refit) with the share of the FP64 vector rate it implies.  The shapes of
scripts/keypoint_timing.py: 2e6 points x 6 cameras and x 24 cameras (the wide rig); 0.3 px noise, 10 % of the detections missing, and one
detection displaced by N(0, 40^2) px on 15 % of the points.  With --forms: the kernel forms (MCBA_CONSENSUS_FORM, development only) side by
side on small rigs around the switch, each in a process of its own.

  python scripts/consensus_timing.py [--out DIR] [--cameras 6,24] [--points N] [--reps R] [--forms 6,8,9,12 --form-points N]
  python scripts/consensus_timing.py --child C --points N                        one measurement (JSON on stdout)"""
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP64_LANE_RATE = 78.6e12 / 2   # v_fma_f64 per second and lane, chip-wide: the 78.6 TFLOP/s FP64 vector peak DESIGN.md uses, one fma = two flops
# FP64 VALU instructions per unit of work (counted from the text of the per-lane headers; a model, not a profile):
I_NULL = 3000      # one 4 x 4 DLT system and its null vector: 7 sweeps x 6 rotations x ~70 (mcba_triangulate.hip quotes the same figure)
I_UNDISTORT = 160  # one detection, 5 rounds with one division each
I_PROJECT = 55     # rigid transform, reciprocal, five-coefficient distortion, distance (one square root), the inlier test
I_LINEARISE = 150  # one view of one linearisation of the refit: projection with its 2 x 3 Jacobian, weights, the packed 3 x 3 accumulation
I_SOLVE = 60       # the damped 3 x 3 Cholesky solve of one iteration


def make_scene(C, P, seed=1):
    import numpy as np

    import multicam_calibration_amd as m

    p = m.synth.make_problem(C, 2, seed=seed, noise=0.0)
    cam = p["true_cam"].copy()
    rng = np.random.default_rng(seed + 7)
    T = m.synth._T(p["true_poses"][0])
    X = rng.normal(0, 60, (P, 3)) @ T[:3, :3].T + T[:3, 3]
    uvs = np.stack([m.synth.project(cam[c:c + 1], np.zeros((1, 6)), X)[0, 0] for c in range(C)])
    uvs += rng.normal(0, 0.3, uvs.shape)
    uvs[rng.uniform(size=(C, P)) < 0.1] = np.nan
    bad = rng.choice(P, size=int(0.15 * P), replace=False)
    uvs[rng.integers(0, C, len(bad)), bad] += rng.normal(0, 40, (len(bad), 2))     # (a displaced unseen detection stays unseen)
    intr = [(np.array([[c[0], 0, c[2]], [0, c[1], c[3]], [0, 0, 1.0]]), np.r_[c[4:6], 0, 0, 0]) for c in cam]
    return list(uvs), cam[:, 6:], intr, X


def child(C, P, reps, threshold=2.5):
    import numpy as np

    sys.path.insert(0, ROOT)
    from multicam_calibration_amd import ops
    from multicam_calibration_amd.triangulation import _cam_blocks

    lib = ops.load_library()
    uvs, ext, intr, X = make_scene(C, P)
    cam, dist = _cam_blocks(ext, intr)
    U = np.ascontiguousarray(np.stack(uvs))
    ms = ctypes.c_double()
    a = ctypes.addressof(ms)
    pts, words, info, ref, rinfo = np.empty((P, 3)), np.zeros(P, dtype=np.uint64), np.empty((P, 8)), np.empty((P, 3)), np.empty((P, 4))
    t_cons, t_ref = [], []
    for _ in range(reps + 1):   # the first call warms up
        rc = lib.mcba_triangulate_consensus(C, P, U.ctypes.data, cam.ctypes.data, dist.ctypes.data, threshold, 2, 5, ops.LOSSES["linear"], 1.0, 100, 0, pts.ctypes.data, words.ctypes.data,
                                            info.ctypes.data, None, a)
        if rc != ops.OK:
            raise SystemExit(lib.mcba_last_error().decode())
        t_cons.append(ms.value)
        rc = lib.mcba_triangulate_refine(C, P, U.ctypes.data, cam.ctypes.data, dist.ctypes.data, None, 5, ops.LOSSES["linear"], 1.0, 100, 0, ref.ctypes.data, rinfo.ctypes.data, a)
        if rc != ops.OK:
            raise SystemExit(lib.mcba_last_error().decode())
        t_ref.append(ms.value)
    k_cons, k_ref = float(np.median(t_cons[1:])), float(np.median(t_ref[1:]))
    seen = ~np.isnan(U).any(-1)
    s = seen.sum(0).astype(np.int64)
    pairs = s * (s - 1) // 2
    fit = info[:, 7] >= 0
    n_in, its = info[fit, 0], info[fit, 6]
    work = {"null_vectors": int(pairs.sum()), "scoring_projections": int((pairs * s).sum()), "refit_view_linearisations": int(((1 + its) * n_in).sum()), "refit_iterations": int(its.sum())}
    instr = (work["null_vectors"] * (I_NULL + 2 * I_UNDISTORT) + work["scoring_projections"] * I_PROJECT + work["refit_view_linearisations"] * I_LINEARISE + work["refit_iterations"] * I_SOLVE)
    ok = fit & ~np.isnan(ref).any(1)
    flagged = (~(((words[None, :] >> np.arange(C, dtype=np.uint64)[:, None]) & np.uint64(1)).astype(bool)) & seen)[:, info[:, 7] != -1]

    def rms(A):
        return float(np.sqrt(np.mean(np.sum((A[ok] - X[ok]) ** 2, axis=1))))

    out = {"points": P, "cameras": C, "threshold_px": threshold, "form": os.environ.get("MCBA_CONSENSUS_FORM", "default"),
           "kernel_ms": {"mcba_triangulate_consensus": k_cons, "mcba_triangulate_refine_from_median_of_pairs": k_ref, "ratio": k_cons / k_ref, "all_consensus": t_cons[1:], "all_refine": t_ref[1:]},
           "work": work, "model_fp64_instructions": float(instr), "share_of_fp64_vector_rate": instr / (k_cons * 1e-3) / FP64_LANE_RATE,
           "refit": {"points_refitted": int(fit.sum()), "no_consensus": int((info[:, 7] == -2).sum()), "too_few_views": int((info[:, 7] == -1).sum()), "iterations_mean": float(its.mean()),
                     "iterations_max": int(its.max()), "iteration_limit_hit": int((info[fit, 7] == 0).sum())},
           "detections_flagged": int(flagged.sum()), "detections_seen": int(flagged.size),
           "rms_to_truth_mm": {"consensus": rms(pts), "least_squares_from_median_of_pairs": rms(ref)}}
    print(json.dumps(out))


def run(cmd, seconds, env=None):
    r = subprocess.run(["timeout", "-k", "10", str(seconds)] + cmd, cwd=ROOT, capture_output=True, text=True, env=env)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-3000:] + r.stderr[-3000:])
        raise SystemExit("step failed (exit %d): %s" % (r.returncode, " ".join(cmd)))
    return r.stdout


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def main():
    out_dir = arg("--out", os.path.join(ROOT, "build", "consensus_timing"))
    cams = [int(c) for c in arg("--cameras", "6,24").split(",") if c]
    forms = [int(c) for c in arg("--forms", "").split(",") if c]
    P, Pf, reps = arg("--points", "2000000"), arg("--form-points", "500000"), arg("--reps", "5")
    os.makedirs(out_dir, exist_ok=True)
    results = []

    def one(C, points, form=None):
        env = dict(os.environ)
        env.pop("MCBA_CONSENSUS_FORM", None)
        if form:
            env["MCBA_CONSENSUS_FORM"] = form
        res = json.loads(run([sys.executable, __file__, "--child", str(C), "--points", points, "--reps", reps], 600, env).strip().splitlines()[-1])
        results.append(res)
        brief = dict(res, kernel_ms={k: v for k, v in res["kernel_ms"].items() if not k.startswith("all_")})
        print(json.dumps(brief), flush=True)
        with open(os.path.join(out_dir, "consensus_timing.json"), "w") as fh:
            json.dump(results, fh, indent=1)

    for C in cams:
        one(C, P)
    for C in forms:
        for form in ("lane", "lane2", "wave"):
            one(C, Pf, form)


if __name__ == "__main__":
    if "--child" in sys.argv:
        child(int(arg("--child", "6")), int(arg("--points", "2000000")), int(arg("--reps", "5")))
    else:
        main()
