"""Seeded keypoint scenes shared by tests/golden/make_golden_geometry.py, the host check and the GPU tier of the keypoint kernels, and the numpy
restatements those tests compare against (the five-coefficient forward model, the robust cost)."""
import numpy as np

from test_triangulate_cpu import scene

# name -> (C, P, seed, noise, p_unseen) of tests/test_triangulate_cpu.scene
SCENES = {"six": (6, 300, 16, 0.3, 0.25), "three": (3, 200, 13, 0.3, 0.25), "twelve": (12, 100, 22, 0.5, 0.6), "outlier": (6, 300, 31, 0.3, 0.1)}
# the losses the refinement oracle was run with, per scene
LOSSES = {"six": ("linear",), "three": ("linear",), "twelve": ("linear",), "outlier": ("linear", "soft_l1", "huber", "cauchy", "arctan")}
# The displacement seed: the first of 1031, 1032, ... with which the refinement oracle (tests/golden/make_golden_geometry.py) passes its own check,
# the same optimum to 5e-7 mm from all of its starts for every point and loss.  1031 .. 1037 do not: with some a point seen by few cameras, one of
# them displaced, has several minima of the redescending losses tens of millimetres apart (1031, arctan: 33 mm between scipy from the median of
# pairs and scipy from the soft_l1 optimum) -- "the" optimum of such a point is whichever basin a solver's first steps fall into, nothing to hold a
# solver to --, with the others (1033, 1035) the plain least-squares optimum of such a point is flat enough that scipy's two starts end 1e-6 mm apart.
OUTLIER_FRACTION, OUTLIER_SIGMA, OUTLIER_SEED = 0.15, 40.0, 1038


def make(name, outlier_seed=None):
    """(uvs list, extrinsics (C, 6), intrinsics list, truth (P, 3)).  "outlier": for a seeded 15 % of the points the detection of one camera that
    sees the point is displaced by N(0, 40^2) px."""
    C, P, seed, noise, p_unseen = SCENES[name]
    uvs, ext, intr, X = scene(C=C, P=P, seed=seed, noise=noise, p_unseen=p_unseen)
    if name == "outlier":
        rng = np.random.default_rng(OUTLIER_SEED if outlier_seed is None else outlier_seed)
        seen = ~np.isnan(np.stack(uvs)).any(-1)
        for i in rng.choice(P, size=int(round(OUTLIER_FRACTION * P)), replace=False):
            cams = np.flatnonzero(seen[:, i])
            shift = rng.normal(0, OUTLIER_SIGMA, 2)
            if cams.size:
                uvs[int(rng.choice(cams))][i] += shift
    return uvs, ext, intr, X


def rodrigues(r):
    r = np.asarray(r, dtype=np.float64)
    th = np.linalg.norm(r)
    if th == 0:
        return np.eye(3)
    k = r / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def project5(X, ext, K, d):
    """The forward five-coefficient model (k1 k2 p1 p2 k3) in numpy: X (..., 3) -> (..., 2)."""
    d = np.r_[np.ravel(d), np.zeros(5)][:5]
    Xc = np.asarray(X, dtype=np.float64) @ rodrigues(ext[:3]).T + np.asarray(ext[3:], dtype=np.float64)
    x, y = Xc[..., 0] / Xc[..., 2], Xc[..., 1] / Xc[..., 2]
    r2 = x * x + y * y
    rad = 1 + r2 * (d[0] + r2 * (d[1] + r2 * d[4]))
    xd = x * rad + 2 * d[2] * x * y + d[3] * (r2 + 2 * x * x)
    yd = y * rad + d[2] * (r2 + 2 * y * y) + 2 * d[3] * x * y
    return np.stack([K[0, 0] * xd + K[0, 2], K[1, 1] * yd + K[1, 2]], axis=-1)


def errors(X, uvs, ext, intr):
    """(C, P) |detection - projection|, NaN where unseen."""
    return np.stack([np.linalg.norm(np.asarray(uvs[c]) - project5(X, ext[c], *intr[c]), axis=-1) for c in range(len(ext))])


def rho(z, loss):
    if loss == "linear":
        return z
    if loss == "soft_l1":
        return 2 * (np.sqrt(1 + z) - 1)
    if loss == "huber":
        return np.where(z <= 1, z, 2 * np.sqrt(np.maximum(z, 1e-300)) - 1)
    if loss == "cauchy":
        return np.log1p(z)
    return np.arctan(z)


def robust_cost(X, uvs, ext, intr, loss, f_scale=1.0):
    """(P,) 0.5 f_scale^2 sum rho((f / f_scale)^2) over the scalars of the cameras that see each point (scipy's cost, per point)."""
    f = np.stack([np.asarray(uvs[c]) - project5(X, ext[c], *intr[c]) for c in range(len(ext))])   # (C, P, 2)
    seen = ~np.isnan(f).any(-1)
    r = rho((np.where(seen[..., None], f, 0.0) / f_scale) ** 2, loss) * seen[..., None]
    return 0.5 * f_scale ** 2 * r.sum(axis=(0, 2))
