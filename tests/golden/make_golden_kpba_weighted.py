"""Writes tests/golden/kpba_weighted.npz: refine_extrinsics with per-detection weights.  Per case of
tests/weights_oracle.GOLDEN_CASES the weights (drawn from the levels 0, 1/4, 1, 4), the first start (ext0, pts0), scipy's optimum from it on the
virtual rig (weights_oracle.solve_virtual: kpba_oracle.solve's call, the virtual cameras of one physical camera tied by construction of the
parameter vector), the held mask and the spread between the optima of the two seeded starts, both rescaled to the first start's baseline.  A
case is `pinned` when that spread is within kpba_oracle.TWO_START_RULE on the extrinsics; the output says which are and which are not, and only
pinned cases are stored.

    python tests/golden/make_golden_kpba_weighted.py [case ...]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import conftest  # noqa: F401,E402  (makes the package importable as the tests see it)
import kpba_oracle as ko  # noqa: E402
import weights_oracle as wo  # noqa: E402


def main(names):
    out = {}
    if os.path.exists(wo.GOLDEN):
        out.update(np.load(wo.GOLDEN))
    for name in names:
        sc, loss = wo.GOLDEN_CASES[name]
        uvs, ext, intr, X, w = wo.golden_scene(name)
        runs = []
        for seed in ko.START_SEEDS:
            e0, p0 = ko.perturbed_start(ext, X, 0, seed)
            base = ko.baseline_of(runs[0][0], 0, runs[0][2]["scale_camera"]) if runs else None
            r = wo.solve_virtual(uvs, e0, intr, p0, w, loss=loss, scale_camera=runs[0][2]["scale_camera"] if runs else None, baseline=base)
            print(f"{name} start {seed}: cost {r['cost']:.15g} scipy status {r['scipy'].status} nfev {r['scipy'].nfev} optimality {r['scipy'].optimality:.3g}", flush=True)
            runs.append((e0, p0, r))
        (e0, p0, a), (_, _, b) = runs
        if not np.array_equal(a["held"], b["held"]):
            print(f"{name}: the two starts hold different scalars -- the spread below compares different gauges")
        se, sp = ko.relative_spread(a["extrinsics"], b["extrinsics"]), float(np.nanmax(np.abs(a["points"] - b["points"])))
        pinned = se <= ko.TWO_START_RULE
        print(f"{name} ({loss}): two-start spread extrinsics {se:.3g} relative, points {sp:.3g} absolute, costs {a['cost']:.15g} {b['cost']:.15g} -> {'PINNED' if pinned else 'NOT pinned'}", flush=True)
        for k in [k for k in out if k.startswith(name + "/")]:
            del out[k]
        if pinned:
            for k, v in dict(weights=w, ext0=e0, pts0=p0, extrinsics=a["extrinsics"], points=a["points"], cost=a["cost"], held=a["held"], scale_camera=a["scale_camera"], spread_ext=se,
                             spread_pts=sp, pinned=pinned).items():
                out[f"{name}/{k}"] = np.asarray(v)
        np.savez_compressed(wo.GOLDEN, **out)


if __name__ == "__main__":
    main(sys.argv[1:] or list(wo.GOLDEN_CASES))
