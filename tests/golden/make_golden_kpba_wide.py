"""Writes tests/golden/kpba_wide.npz: per case of tests/kpba_wide.CASES (25 to 64 cameras) what make_golden_kpba.py writes per case of its own --
the first start (ext0, pts0), scipy's optimum from it (kpba_oracle.solve: trf, the exact solver, a 3-point Jacobian, ftol = xtol = 1e-15, its held
scalars and closing rescale), the held mask and the spread between the optima of the two seeded starts, both rescaled to the first start's
baseline.  A case is `pinned` when that spread is within 1e-7 relative on the extrinsics; the output says which are.

    python tests/golden/make_golden_kpba_wide.py [case ...]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import conftest  # noqa: F401,E402  (makes the package importable as the tests see it)
import kpba_oracle as ko  # noqa: E402
import kpba_wide as kw  # noqa: E402


def solve_case(name):
    """the entries of one case, keyed name/..."""
    loss = kw.CASES[name][3]
    uvs, ext, intr, X = kw.make_scene(name)
    runs = []
    for seed in ko.START_SEEDS:
        e0, p0 = ko.perturbed_start(ext, X, 0, seed)
        base = ko.baseline_of(runs[0][0], 0, runs[0][2]["scale_camera"]) if runs else None
        r = ko.solve(uvs, e0, intr, p0, loss=loss, scale_camera=runs[0][2]["scale_camera"] if runs else None, baseline=base)
        print(f"{name} start {seed}: cost {r['cost']:.15g} scipy status {r['scipy'].status} nfev {r['scipy'].nfev} optimality {r['scipy'].optimality:.3g}", flush=True)
        runs.append((e0, p0, r))
    (e0, p0, a), (_, _, b) = runs
    if not np.array_equal(a["held"], b["held"]):
        print(f"{name}: the two starts hold different scalars -- the spread below compares different gauges")
    se, sp = ko.relative_spread(a["extrinsics"], b["extrinsics"]), float(np.nanmax(np.abs(a["points"] - b["points"])))
    pinned = se <= ko.TWO_START_RULE
    print(f"{name} ({loss}): two-start spread extrinsics {se:.3g} relative, points {sp:.3g} absolute, costs {a['cost']:.15g} {b['cost']:.15g} -> {'PINNED' if pinned else 'NOT pinned'}", flush=True)
    return {f"{name}/{k}": np.asarray(v) for k, v in dict(ext0=e0, pts0=p0, extrinsics=a["extrinsics"], points=a["points"], cost=a["cost"], held=a["held"], scale_camera=a["scale_camera"],
                                                          spread_ext=se, spread_pts=sp, pinned=pinned).items()}


def main(names):
    out = {}
    if os.path.exists(kw.GOLDEN):
        out.update(np.load(kw.GOLDEN))
    for name in names:
        out.update(solve_case(name))
        np.savez_compressed(kw.GOLDEN, **out)


if __name__ == "__main__":
    main(sys.argv[1:] or list(kw.CASES))
