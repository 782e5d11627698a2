"""Writes tests/golden/kpcam.npz: per case of tests/kpcam_oracle.CASES the first start (ext0, pts0, theta0), the free mask and the prior's std, scipy's
optimum from it (extrinsics, theta6, points, cost, prior_cost), the held mask and the spread between the optima of the two seeded starts, both
rescaled to the first start's baseline.  A case is `pinned` when that spread is within 1e-7 relative on the extrinsics AND on the intrinsics
(SURVEY.md section 7); the output says which are and which are not.  The two starts of a case without a prior differ in extrinsics, points and
the free intrinsic scalars; those of a case with a prior share the intrinsics, which are the prior's centre.

    python tests/golden/make_golden_kpcam.py [--into FILE] [case ...]       (several processes may each write a file of their own)
    python tests/golden/make_golden_kpcam.py --merge FILE [FILE ...]        (into tests/golden/kpcam.npz)
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import conftest  # noqa: F401,E402  (makes the package importable as the tests see it)
import kpba_oracle as ko  # noqa: E402
import kpcam_oracle as kc  # noqa: E402


def main(names, target):
    out = {}
    if os.path.exists(target):
        out.update(np.load(target))
    for name in names:
        runs = []
        for seed in ko.START_SEEDS:
            i = kc.case_inputs(name, seed)
            first = runs[0][1] if runs else None
            t = time.time()
            r = kc.solve12(i["uvs"], i["ext0"], i["intr"], i["theta0"], i["pts0"], i["free"], i["prior_std"], loss=i["loss"], scale_camera=first["scale_camera"] if first else None,
                           baseline=ko.baseline_of(runs[0][0]["ext0"], 0, first["scale_camera"]) if first else None)
            print(f"{name} start {seed}: cost {r['cost']:.15g} (prior {r['prior_cost']:.6g}) scipy status {r['scipy'].status} nfev {r['scipy'].nfev} optimality {r['scipy'].optimality:.3g} "
                  f"{time.time() - t:.0f} s", flush=True)
            runs.append((i, r))
        (i, a), (_, b) = runs
        se, si = ko.relative_spread(a["extrinsics"], b["extrinsics"]), ko.relative_spread(a["theta6"], b["theta6"])
        sp = float(np.nanmax(np.abs(a["points"] - b["points"])))
        move = ko.relative_spread(kc.theta6_of(i["intr"]), a["theta6"])
        pinned = se <= ko.TWO_START_RULE and si <= ko.TWO_START_RULE and name not in kc.NEVER_PINNED
        print(f"{name} ({i['loss']}): two-start spread extrinsics {se:.3g} intrinsics {si:.3g} relative, points {sp:.3g} absolute; intrinsics moved {move:.3g} from the scene's own; "
              f"costs {a['cost']:.15g} {b['cost']:.15g} -> {'PINNED' if pinned else 'NOT pinned'}{' (never pinned: kpcam_oracle.NEVER_PINNED)' if name in kc.NEVER_PINNED else ''}", flush=True)
        std = np.full(i["free"].shape, np.inf) if i["prior_std"] is None else i["prior_std"]
        for k, v in dict(ext0=i["ext0"], pts0=i["pts0"], theta0=i["theta0"], free=i["free"], prior_std=std, extrinsics=a["extrinsics"], theta6=a["theta6"], points=a["points"], cost=a["cost"],
                         prior_cost=a["prior_cost"], held=a["held"], scale_camera=a["scale_camera"], spread_ext=se, spread_intr=si, spread_pts=sp, moved=move, pinned=pinned).items():
            out[f"{name}/{k}"] = np.asarray(v)
        np.savez_compressed(target, **out)


if __name__ == "__main__":
    args = sys.argv[1:]
    if args and args[0] == "--merge":
        merged = {}
        if os.path.exists(kc.GOLDEN):
            merged.update(np.load(kc.GOLDEN))
        for f in args[1:]:
            merged.update(np.load(f))
        for n in kc.NEVER_PINNED:
            if f"{n}/pinned" in merged:
                merged[f"{n}/pinned"] = np.asarray(False)
        np.savez_compressed(kc.GOLDEN, **{k: merged[k] for k in sorted(merged)})
        print(sorted({k.split("/")[0] for k in merged}))
    else:
        target = kc.GOLDEN
        if args and args[0] == "--into":
            target, args = args[1], args[2:]
        main(args or list(kc.CASES), target)
