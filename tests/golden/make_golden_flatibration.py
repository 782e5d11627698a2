"""Golden vectors for floor-plane alignment FROM THE REFERENCE ITSELF (flatibration.py, with sklearn's RANSACRegressor).

Run where the reference and sklearn are installed:   python tests/golden/make_golden_flatibration.py <reference checkout>
Loads the reference's geometry.py and flatibration.py unmodified (an empty stub for cv2, which the functions recorded here never call)
and writes flatibration.npz: for every case of tests/flat_problem.py, after np.random.seed(global seed), flatibrate's transform, the
RANSAC fit's n_trials_ and inlier_mask_ and numpy's global RNG state after the call; center_arena with each centre method; flip_z_axis;
and the tutorial chain (get_floor_points -> flatibrate -> center_arena -> flip_z_axis) on seeded keypoints.  Only seeds and outputs
are stored; the inputs are regenerated from tests/flat_problem.py."""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.dont_write_bytecode = True

import flat_problem as fp  # noqa: E402


def load_reference(ref_root):
    src = os.path.join(ref_root, "multicam_calibration")
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    pkg = types.ModuleType("multicam_calibration")
    pkg.__path__ = [src]
    sys.modules["multicam_calibration"] = pkg
    mods = {}
    for name in ("geometry", "flatibration"):
        spec = importlib.util.spec_from_file_location(f"multicam_calibration.{name}", os.path.join(src, name + ".py"))
        m = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = m
        spec.loader.exec_module(m)
        mods[name] = m
    return mods["flatibration"]


def rng_state():
    s = np.random.get_state()
    return np.concatenate([s[1].astype(np.int64), [s[2], s[3]]]), s[4]


def main(ref_root):
    flat = load_reference(ref_root)
    from sklearn.linear_model import RANSACRegressor

    out = {}
    for name, (n, frac, seed, gseed) in fp.CASES.items():
        P = fp.case_points(name)
        np.random.seed(gseed)
        t = flat.flatibrate(P, residual_threshold=fp.THRESHOLD)
        out[f"{name}_transform"] = t
        out[f"{name}_state"], out[f"{name}_gauss"] = rng_state()
        np.random.seed(gseed)  # the same fit again, for the estimator's attributes (flatibrate does not return them)
        r = RANSACRegressor(residual_threshold=fp.THRESHOLD).fit(P[:, :2], P[:, 2])
        out[f"{name}_n_trials"] = r.n_trials_
        out[f"{name}_inliers"] = r.inlier_mask_
        out[f"{name}_coef"] = np.r_[r.estimator_.coef_, r.estimator_.intercept_]
        for method in ("midrange", "mean", "median"):
            out[f"{name}_center_{method}"] = flat.center_arena(t, P, center_method=method)
        out[f"{name}_center_midrange5"] = flat.center_arena(t, P, center_method="midrange", range_pctl=5)
        out[f"{name}_flip"] = flat.flip_z_axis(t)
        print(name, r.n_trials_, int(r.inlier_mask_.sum()))
    # the tutorial chain (docs/source/flatibration_tutorial.ipynb), z pointing down as there
    kp = -fp.keypoints(20000, 12, seed=21)
    fl = flat.get_floor_points(kp, z_points_down=True)
    fl = fl[np.isfinite(fl).all(axis=1)]
    np.random.seed(8)
    t = flat.flatibrate(fl)
    t = flat.center_arena(t, fl, center_method="midrange")
    out["tutorial_transform"] = flat.flip_z_axis(t)
    out["tutorial_state"], out["tutorial_gauss"] = rng_state()
    np.savez_compressed(os.path.join(HERE, "flatibration.npz"), **out)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit("usage: make_golden_flatibration.py <reference checkout (the directory that holds multicam_calibration/)>")
    main(sys.argv[1])
