"""Golden vectors for the geometry module FROM THE REFERENCE ITSELF (geometry.py) and from scipy on the reference's project_points.

Run where the reference and scipy are installed:   python tests/golden/make_golden_geometry.py <reference checkout>
Loads the reference's geometry.py unmodified (empty stubs for cv2 and tqdm, which the functions recorded here never call) and writes
geometry.npz:
  * project_points with and without dist_coefs, leading shapes (P, 3) and (T, K, 3), an all-zero extrinsic, five-element dist_coefs with
    non-zero p1, p2, k3 (ignored by the reference), points behind the camera and NaN points; apply_rigid_transform (6-vector and 4 x 4),
    get_projection_matrix, rodrigues / rodrigues_inv, the homogeneous helpers, rigid_transform_from_correspondences (a plain case and one
    that takes the reflection branch) -- inputs and the reference's outputs;
  * the refinement oracle: for the scenes of tests/keypoint_scenes.py the start (oracle/triangulate_oracle.triangulate) and, per point
    with at least two views, scipy.optimize.least_squares on the reference's project_points residuals (jac='3-point', x_scale='jac',
    ftol = xtol = 1e-15, gtol = 1e-12) for the losses listed there at f_scale = 1, FROM TWO STARTS: the median-of-pairs point, and that
    point plus N(0, 0.5^2 mm) noise -- and, for the redescending losses cauchy and arctan, from a third: the soft_l1 optimum of the point.
    The script refuses to write unless all starts agree to 5e-7 mm for every point; it stores the first and the largest disagreement
    (`<scene>_<loss>_spread`).  A scene that fails this has points with several minima (see tests/keypoint_scenes.py: OUTLIER_SEED).  Scene inputs are regenerated from tests/keypoint_scenes.py, not stored."""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.dont_write_bytecode = True

import keypoint_scenes as ks  # noqa: E402
from oracle import triangulate_oracle as tri  # noqa: E402

TWO_START_GATE = 5e-7   # mm


def load_reference(ref_root):
    src = os.path.join(ref_root, "multicam_calibration")
    for stub in ("cv2", "tqdm"):
        sys.modules.setdefault(stub, types.ModuleType(stub))
    pkg = types.ModuleType("multicam_calibration")
    pkg.__path__ = [src]
    sys.modules["multicam_calibration"] = pkg
    spec = importlib.util.spec_from_file_location("multicam_calibration.geometry", os.path.join(src, "geometry.py"))
    m = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = m
    spec.loader.exec_module(m)
    return m


def refine_point(geo, X0, obs, cams, loss):
    """scipy's optimum of one point: obs (n, 2) detections of the n cameras (extrinsics, K, dist) that see it."""
    from scipy.optimize import least_squares

    def fun(X):
        return np.concatenate([o - geo.project_points(X, e, K, d) for o, (e, K, d) in zip(obs, cams)])

    return least_squares(fun, X0, jac="3-point", x_scale="jac", ftol=1e-15, xtol=1e-15, gtol=1e-12, loss=loss, f_scale=1.0, max_nfev=2000)


def refinement_oracle(geo, out):
    for name in ks.SCENES:
        uvs, ext, intr, X = ks.make(name)
        start = tri.triangulate(uvs, ext, intr)
        out[f"{name}_start"] = start
        U = np.stack(uvs)
        seen = ~np.isnan(U).any(-1)
        rng = np.random.default_rng(77)
        jitter = rng.normal(0, 0.5, start.shape)
        for loss in ks.LOSSES[name]:
            best = np.full(start.shape, np.nan)
            spread, nfev = 0.0, 0
            for p in range(len(start)):
                cs = np.flatnonzero(seen[:, p])
                if cs.size < 2 or np.isnan(start[p]).any():
                    continue
                cams = [(ext[c], intr[c][0], intr[c][1]) for c in cs]
                a = refine_point(geo, start[p], U[cs, p], cams, loss)
                b = refine_point(geo, start[p] + jitter[p], U[cs, p], cams, loss)
                best[p] = a.x
                spread = max(spread, float(np.abs(a.x - b.x).max()))
                nfev = max(nfev, a.nfev, b.nfev)
                if loss in ("cauchy", "arctan"):   # redescending: the basin must not depend on which robust estimate the solver starts from
                    c = refine_point(geo, out[f"{name}_soft_l1"][p], U[cs, p], cams, loss)
                    spread = max(spread, float(np.abs(a.x - c.x).max()))
            print(f"{name:8s} {loss:8s} two-start spread {spread:.2e} mm, at most {nfev} evaluations, rms to truth: start {rms(start, X):.4f} refined {rms(best, X):.4f} mm")
            assert spread <= TWO_START_GATE, f"{name} / {loss}: the oracle's two starts disagree by {spread} mm"
            out[f"{name}_{loss}"] = best
            out[f"{name}_{loss}_spread"] = spread


def rms(A, B):
    d = A - B
    d = d[~np.isnan(d).any(1)]
    return float(np.sqrt(np.mean(np.sum(d * d, axis=1))))


def main(ref_root):
    geo = load_reference(ref_root)
    out = {}
    rng = np.random.default_rng(2024)
    K = np.array([[1180.0, 0.0, 655.0], [0.0, 1210.0, 498.0], [0.0, 0.0, 1.0]])
    ext = np.array([0.21, -0.33, 0.12, 35.0, -20.0, 900.0])
    pts = rng.normal(0, 120, (40, 3))
    pts[5, 2] = -1500.0      # behind the camera (z < 0 in its frame): the reference "just projects"
    pts[6, 2] = -2500.0
    pts[9] = np.nan
    pts[11, 1] = np.nan
    grid = rng.normal(0, 80, (5, 4, 3))
    grid[2, 1] = np.nan
    d2, d5 = np.array([-0.11, 0.04]), np.array([-0.11, 0.04, 2e-3, -1e-3, 0.02])
    out.update(pp_K=K, pp_ext=ext, pp_pts=pts, pp_grid=grid, pp_d2=d2, pp_d5=d5)
    out["pp_plain"] = geo.project_points(pts, ext, K)
    out["pp_dist2"] = geo.project_points(pts, ext, K, d2)
    out["pp_dist5"] = geo.project_points(pts, ext, K, d5)
    out["pp_grid_dist2"] = geo.project_points(grid, ext, K, d2)
    out["pp_zero_ext"] = geo.project_points(pts + np.array([0, 0, 800.0]), np.zeros(6), K, d2)
    t6 = np.array([-0.4, 0.25, 1.1, 12.0, -7.0, 33.0])
    T4 = geo.get_transformation_matrix(np.array([0.9, -0.2, 0.3, -5.0, 8.0, 2.0]))
    out.update(rt_t6=t6, rt_T4=T4)
    out["rt_vec"] = geo.apply_rigid_transform(t6, pts)
    out["rt_mat"] = geo.apply_rigid_transform(T4, grid)
    out["projection_matrix"] = geo.get_projection_matrix(ext, (K, d5))
    rv = np.vstack([np.zeros(3), rng.normal(0, 0.8, (6, 3)), [1e-9, -2e-9, 1e-9]])
    out.update(rod_r=rv, rod_R=geo.rodrigues(rv))
    out["rod_inv"] = geo.rodrigues_inv(out["rod_R"])
    out["hom"] = geo.euclidean_to_homogenous(grid)
    hom_in = rng.normal(2, 1, (7, 4))
    out.update(hom_in=hom_in, hom_back=geo.homogeneous_to_euclidean(hom_in))
    src = rng.normal(0, 50, (30, 3))
    tgt = geo.apply_rigid_transform(t6, src) + rng.normal(0, 0.5, src.shape)
    t, rmsd = geo.rigid_transform_from_correspondences(src, tgt)
    out.update(kabsch_src=src, kabsch_tgt=tgt, kabsch_t=t, kabsch_rmsd=rmsd)
    # a mirrored, nearly planar target: the best orthogonal map is a reflection, so the reference flips the last singular vector
    flat = src * np.array([1.0, 1.0, 0.02])
    mirrored = flat * np.array([1.0, 1.0, -1.0]) + rng.normal(0, 0.01, src.shape)
    Hm = (flat - flat.mean(0)).T @ (mirrored - mirrored.mean(0))
    U_, _, Vt_ = np.linalg.svd(Hm)
    assert np.linalg.det(Vt_.T @ U_.T) < 0, "the reflection case does not take the reflection branch"
    t, rmsd = geo.rigid_transform_from_correspondences(flat, mirrored)
    out.update(reflect_src=flat, reflect_tgt=mirrored, reflect_t=t, reflect_rmsd=rmsd)
    refinement_oracle(geo, out)
    np.savez_compressed(os.path.join(HERE, "geometry.npz"), **out)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit("usage: make_golden_geometry.py <reference checkout (the directory that holds multicam_calibration/)>")
    main(sys.argv[1])
