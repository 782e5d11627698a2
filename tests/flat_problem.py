"""Seeded inputs for the floor-plane alignment tests and tests/golden/make_golden_flatibration.py (shared, so the fixture stores seeds
and outputs, never the large inputs)."""
import numpy as np

# name -> (n_points, outlier fraction, data seed, global numpy seed before flatibrate).  The outlier fractions put sklearn's stop at about
# 10 trials (0.3), about 35 (0.5) and the cap of 100 (0.65); 50 and 299 points take the permutation draw, 300 and more the tracking draw.
CASES = {
    "n50": (50, 0.2, 11, 0),
    "n299": (299, 0.3, 12, 1),
    "n300": (300, 0.3, 13, 2),
    "n5000": (5000, 0.3, 14, 3),
    "n5000_o10": (5000, 0.1, 15, 4),
    "n5000_o50": (5000, 0.5, 16, 5),
    "n5000_o65": (5000, 0.65, 17, 6),
    "n100k": (100000, 0.3, 18, 7),
}
THRESHOLD = 10.0


def floor_points(n, outlier_frac, seed, noise=2.0):
    """(n, 3) points on a tilted floor z = 0.05 x - 0.03 y + 40 in a 600 x 400 arena (mm) with Gaussian noise; a fraction lifted
    20 .. 150 above it (animals' lowest keypoints off the floor)."""
    rng = np.random.default_rng(seed)
    xy = rng.uniform([-300.0, -200.0], [300.0, 200.0], size=(n, 2))
    z = 0.05 * xy[:, 0] - 0.03 * xy[:, 1] + 40.0 + rng.normal(0.0, noise, n)
    out = rng.uniform(size=n) < outlier_frac
    z[out] += rng.uniform(20.0, 150.0, out.sum())
    return np.column_stack([xy, z])


def case_points(name):
    n, frac, seed, _ = CASES[name]
    return floor_points(n, frac, seed)


def keypoints(n_frames, n_keypoints, seed, nan_frames=0.02, nan_entries=0.02, ties=True):
    """(F, K, 3) keypoints: an animal's body above a floor, some frames wholly NaN, some single NaN z, and (ties) z rounded to 1 mm so
    that equal minima are common."""
    rng = np.random.default_rng(seed)
    base = rng.uniform([-300.0, -200.0, 0.0], [300.0, 200.0, 5.0], size=(n_frames, 1, 3))
    kp = base + rng.normal(0.0, [30.0, 30.0, 20.0], size=(n_frames, n_keypoints, 3))
    if ties:
        kp[..., 2] = np.round(kp[..., 2])
    kp[rng.uniform(size=(n_frames, n_keypoints)) < nan_entries, 2] = np.nan
    kp[rng.uniform(size=n_frames) < nan_frames] = np.nan
    return kp
