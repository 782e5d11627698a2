"""Per-iteration time and per-kernel split of the sparse-Schur handle (rigs of more than 40 cameras) on one GPU.

    python scripts/wide_rig_timing.py [--out DIR] [--shapes 64x10000,128x10000] [--k 8] [--iters 20] [--compare 40x10000]

For each C x F shape (synthetic rig, each frame seen by the k cameras nearest its board on the ring, 2 x 3 board): the device-resident LM
loop is run for a fixed number of ticks, once plain (wall time per tick, after one warm-up run) and once with the library's event profiling
(ms per kernel group per tick).  --compare adds shapes run with BOTH handles (dense and sparse) on the same problem.  Writes DIR/timing.json
(default build/wide_rig_timing) and prints a table."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import multicam_calibration_amd as m  # noqa: E402


def run(p, schur, iters, profile):
    x0 = m.serialize_params(p["extrinsics"], p["intrinsics"], p["poses"])
    prob = m.ops.Problem(p["uvs"], p["obj"], schur=schur)
    if profile:
        prob.profile_enable(True)
    prob.set_params(0, x0)
    prob.synchronize()
    t0 = time.perf_counter()
    # ftol = xtol = gtol = 0: no termination test fires, every tick does the whole work
    res = m.solver.lm_solve(prob, x0, ftol=0.0, xtol=0.0, gtol=0.0, max_nfev=iters + 1)
    prob.synchronize()
    dt = time.perf_counter() - t0
    prof = prob.profile_read() if profile else None
    prob.close()
    return dt, res, prof


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "wide_rig_timing"))
    ap.add_argument("--shapes", default="64x10000,128x10000")
    ap.add_argument("--compare", default="40x10000")
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    jobs = [(s, "sparse") for s in args.shapes.split(",") if s] + [(s, h) for s in args.compare.split(",") if s for h in ("dense", "sparse")]
    out = []
    for shape, schur in jobs:
        C, F = (int(v) for v in shape.split("x"))
        p = m.synth.make_problem(C, F, rows=2, cols=3, pitch=60.0, seed=11, visible_k=min(args.k, C))
        run(p, schur, 2, False)   # warm-up
        dt, res, _ = run(p, schur, args.iters, False)
        ticks = max(1, int(res.lm["steps"]))   # (ticks of the device loop: accepted, rejected and rebuild-only alike; res.lm["iterations"] counts accepted steps)
        _, _, prof = run(p, schur, args.iters, True)
        split = {k: ms / ticks for k, (ms, calls) in prof.items() if calls}
        rec = dict(C=C, F=F, k=min(args.k, C), schur=schur, ticks=ticks, accepted=int(res.lm["iterations"]), ms_per_tick=1e3 * dt / ticks, kernel_ms_per_tick=split)
        out.append(rec)
        print("%4d x %6d  %-6s  %7.3f ms / tick  (%d ticks, %d accepted)" % (C, F, schur, rec["ms_per_tick"], ticks, rec["accepted"]))
        for k, v in sorted(split.items(), key=lambda kv: -kv[1]):
            print("        %-18s %8.3f ms" % (k, v))
    with open(os.path.join(args.out, "timing.json"), "w") as fh:
        json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
