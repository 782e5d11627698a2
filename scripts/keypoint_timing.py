"""Keypoint projection, reprojection errors and triangulation refinement on the MI355X: the public calls end to end from host arrays (median of
7, warmed up), the kernel time of each call (HIP events), the algorithmic bytes of the streaming kernels against the measured copy rate, the
refinement's iteration counts, and rocprofv3 --kernel-trace --stats per kernel in a run of its own.  2e6 points x 6 cameras (the shape DESIGN.md
section 8f-4 times triangulate() at) and x 24 cameras (the rig of BASELINE configs[4]); 0.3 px noise, 10 % of the detections missing.

  python scripts/keypoint_timing.py [--out DIR] [--cameras 6,24] [--points N]   driver: every step a child process under its own `timeout -k`
  python scripts/keypoint_timing.py --child C --points N                        one measurement (JSON on stdout)
  --weights: also k_tri_refine's weighted instantiation on the same shapes with a random weight plane (uniform in [0.1, 3]; SURVEY.md section
  8f-13), its kernel time beside the unweighted one in the JSON, and -- with --out profiles -- the keypoint block of DESIGN.md section 8f-13"""
import ctypes
import glob
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COPY_RATE = 6.29e12   # bytes/s, measured float4 copy on this GPU


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
    intr = [(np.array([[c[0], 0, c[2]], [0, c[1], c[3]], [0, 0, 1.0]]), np.r_[c[4:6], 0, 0, 0]) for c in cam]
    return list(uvs), cam[:, 6:], intr


def child(C, P, reps, weights=False):
    import numpy as np

    sys.path.insert(0, ROOT)
    import multicam_calibration_amd as m
    from multicam_calibration_amd import ops
    from multicam_calibration_amd.triangulation import _cam_blocks

    lib = ops.load_library()
    uvs, ext, intr = make_scene(C, P)
    ms = ctypes.c_double()

    def timed(fn):
        fn()
        t = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(t))

    start, k_tri = m.triangulate(uvs, ext, intr, return_kernel_ms=True)
    out = {"points": P, "cameras": C}
    out["e2e_ms"] = {
        "triangulate": timed(lambda: m.triangulate(uvs, ext, intr)),
        "triangulate_refine": timed(lambda: m.triangulate(uvs, ext, intr, refine=True)),
        "refine_triangulation": timed(lambda: m.refine_triangulation(start, uvs, ext, intr)),
        "project_to_cameras": timed(lambda: m.project_to_cameras(start, ext, intr)),
        "keypoint_reprojection_errors": timed(lambda: m.keypoint_reprojection_errors(start, uvs, ext, intr)),
        "keypoint_reprojection_errors_medians_only": timed(lambda: m.keypoint_reprojection_errors(start, uvs, ext, intr, arrays=False)),
        "apply_rigid_transform": timed(lambda: m.apply_rigid_transform(ext[1], start)),
    }
    # kernel time of one call of each entry point (HIP events around the call's kernels)
    cam, dist = _cam_blocks(ext, intr)
    U = np.ascontiguousarray(np.stack(uvs))
    o2, o3, info, err, med = np.empty((C, P, 2)), np.empty((P, 3)), np.empty((P, 4)), np.empty((C, P)), np.empty(C)
    a = ctypes.addressof(ms)
    lib.mcba_project_points(C, P, start.ctypes.data, cam.ctypes.data, None, 0, o2.ctypes.data, a)
    k_proj = ms.value
    lib.mcba_project_points(C, P, start.ctypes.data, cam.ctypes.data, dist.ctypes.data, 0, o2.ctypes.data, a)
    k_proj5 = ms.value
    lib.mcba_keypoint_errors(C, P, start.ctypes.data, U.ctypes.data, cam.ctypes.data, dist.ctypes.data, 0, err.ctypes.data, med.ctypes.data, a)
    k_err = ms.value
    lib.mcba_triangulate_refine(C, P, U.ctypes.data, cam.ctypes.data, dist.ctypes.data, start.ctypes.data, 5, ops.LOSSES["soft_l1"], 1.0, 100, 0, o3.ctypes.data, info.ctypes.data, a)
    k_ref = ms.value
    ok = info[:, 3] >= 0
    evals = 1.0 + info[ok, 2]   # the linearisation of the start, then one per iteration
    out["kernel_ms"] = {"k_triangulate": k_tri, "k_project_radial2": k_proj, "k_project_opencv5": k_proj5, "k_keypoint_errors_plus_select": k_err, "k_tri_refine_soft_l1": k_ref}
    out["refine_iterations"] = {"mean": float(info[ok, 2].mean()), "max": int(info[ok, 2].max()), "iteration_limit_hit": int((info[ok, 3] == 0).sum()), "points_refined": int(ok.sum())}
    b_proj, b_err = P * (24 + 16 * C), P * (24 + 16 * C + 8 * C)
    b_ref = float(np.sum(24 + 16 * C * evals + 24)) + (P - ok.sum()) * (24 + 16 * C + 24)
    out["algorithmic_bytes"] = {"k_project": b_proj, "k_keypoint_errors": b_err, "k_tri_refine": b_ref}
    out["share_of_copy_rate"] = {"k_project_radial2": b_proj / (k_proj * 1e-3) / COPY_RATE, "k_project_opencv5": b_proj / (k_proj5 * 1e-3) / COPY_RATE}
    out["refine_bytes_per_s"] = b_ref / (k_ref * 1e-3)
    if weights:   # the same launch with the (C, P) plane beside the detections: 8 C more bytes per linearisation
        W = np.ascontiguousarray(np.random.default_rng(11).uniform(0.1, 3.0, (C, P)))
        winfo = np.empty((P, 4))
        lib.mcba_triangulate_refine_weighted(C, P, U.ctypes.data, W.ctypes.data, cam.ctypes.data, dist.ctypes.data, start.ctypes.data, 5, ops.LOSSES["soft_l1"], 1.0, 100, 0, o3.ctypes.data,
                                             winfo.ctypes.data, a)
        out["kernel_ms"]["k_tri_refine_soft_l1_weighted"] = ms.value
        wok = winfo[:, 3] >= 0
        out["weighted"] = {"k_tri_refine_ratio": ms.value / k_ref, "iterations_mean": float(winfo[wok, 2].mean()), "iterations_mean_unweighted": float(info[ok, 2].mean())}
    print(json.dumps(out))


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


def run(cmd, seconds):
    r = subprocess.run(["timeout", "-k", "10", str(seconds)] + cmd, cwd=ROOT, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-3000:] + r.stderr[-3000:])
        raise SystemExit("step failed (exit %d): %s" % (r.returncode, " ".join(cmd)))
    return r.stdout


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def main():
    out_dir = arg("--out", os.path.join(ROOT, "build", "keypoint_timing"))
    cams = [int(c) for c in arg("--cameras", "6,24").split(",")]
    P = arg("--points", "2000000")
    weighted = "--weights" in sys.argv
    os.makedirs(out_dir, exist_ok=True)
    results = []
    for C in cams:
        res = json.loads(run([sys.executable, __file__, "--child", str(C), "--points", P] + (["--weights"] if weighted else []), 900).strip().splitlines()[-1])
        results.append(res)
        print(json.dumps(res, indent=1), flush=True)
        with open(os.path.join(out_dir, "keypoint_timing.json"), "w") as fh:
            json.dump(results, fh, indent=1)
    if weighted:
        write_weights_block("keypoint", "| points x cameras | `k_tri_refine<soft_l1>` (ms) | weighted (ms) | ratio | iterations per point, mean (unweighted, weighted) |",
                            [f"| {r['points']} x {r['cameras']} | {r['kernel_ms']['k_tri_refine_soft_l1']:.2f} | {r['kernel_ms']['k_tri_refine_soft_l1_weighted']:.2f} | "
                             f"{r['weighted']['k_tri_refine_ratio']:.2f} | {r['weighted']['iterations_mean_unweighted']:.2f}, {r['weighted']['iterations_mean']:.2f} |" for r in results])
    if "--no-profile" in sys.argv:
        return
    for C in cams:   # kernel statistics, profiler in a run of its own (no counters)
        d = os.path.join(out_dir, "rocprof_%d" % C)
        run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "kp", "--", sys.executable, __file__, "--child", str(C), "--points", P, "--reps", "1"], 900)
        for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            print("== %d cameras: %s" % (C, os.path.relpath(f, out_dir)))
            for line in open(f):
                if line.startswith('"Name"') or any(k in line for k in ("k_project", "k_keypoint", "k_tri", "k_sel_")):
                    print(line.rstrip(), flush=True)


if __name__ == "__main__":
    if "--child" in sys.argv:
        child(int(arg("--child", "6")), int(arg("--points", "2000000")), int(arg("--reps", "7")), "--weights" in sys.argv)
    else:
        main()
