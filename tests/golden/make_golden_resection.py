"""Writes tests/golden/resection.npz: the optimum of the resection polish by scipy.optimize.least_squares on the six pose
scalars of one camera, the points fixed (the oracle's triangulation of the other cameras), every usable point in the mask, with the settings of
tests/kpba_oracle.solve, from two seeded starts (tests/resection_oracle.perturbed_start, seeds START_SEEDS).  A case is pinned only where its
two starts agree within the project's 1e-7 rule (kpba_oracle.TWO_START_RULE); the spreads are printed, and SURVEY.md section 8f-16 tabulates them.

    python tests/golden/make_golden_resection.py        (from the repository root; needs scipy)"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import keypoint_scenes as ks  # noqa: E402
import kpba_oracle as ko  # noqa: E402
import resection_oracle as ro  # noqa: E402


def solve(start, points, uv, mask, intr, loss):
    from scipy.optimize import least_squares

    use = mask & np.isfinite(points).all(1) & np.isfinite(uv).all(1)
    X, obs, d = points[use], uv[use], ro.d5(intr)

    def fun(x):
        return (obs - ks.project5(X, x, intr[0], d)).ravel()

    r = least_squares(fun, start, method="trf", tr_solver="exact", jac="3-point", x_scale="jac", ftol=1e-15, xtol=1e-15, gtol=1e-12, loss=loss, f_scale=1.0, max_nfev=200)
    return r.x, ro.robust_cost(r.x, points, uv, mask, intr, loss)


def main():
    out = {}
    for name, (sc, cam, loss) in ro.GOLDEN_CASES.items():
        c = ro.camera_of(sc, cam)
        sols = [solve(ro.perturbed_start(c["ext"], s), c["points"], c["uv"], c["usable"], c["intr"], loss) for s in ro.START_SEEDS]
        spread = ko.relative_spread(sols[0][0], sols[1][0])
        best = min(sols, key=lambda s: s[1])
        pinned = spread <= ko.TWO_START_RULE
        print(f"{name}: usable {int(c['usable'].sum())}; costs {sols[0][1]:.12g} {sols[1][1]:.12g}; two-start spread {spread:.3g}; pinned {pinned}")
        out[f"{name}/pose"], out[f"{name}/cost"], out[f"{name}/spread"], out[f"{name}/pinned"] = best[0], best[1], spread, pinned
    np.savez(ro.GOLDEN, **out)


if __name__ == "__main__":
    main()
