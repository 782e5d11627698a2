"""Seeded thin-slab keypoint scenes: the cameras of tests/test_triangulate_cpu.scene, the cloud replaced by a slab in the
board frame -- N(0, 1) x (60, 60, zs) mm --, every point seen by every camera.  An animal on an arena floor looks like this, and the 8-point
generator of the two-view RANSAC fails on it without saying so (tests/test_fivepoint_oracle_cpu.py pins that)."""
import numpy as np

import multicam_calibration_amd as m

# name -> (C, P, seed, noise in px, zs in mm).  "thin3_1025": one point past a workgroup of the scorer (1024 + 1)
SCENES = {"thin3": (3, 200, 13, 0.3, 5.0), "thin6": (6, 300, 16, 0.3, 5.0), "thin3_1025": (3, 1025, 13, 0.3, 5.0)}


def slab(C, P, seed, noise, zs):
    """(uvs list, extrinsics (C, 6), intrinsics list, truth (P, 3)) -- test_triangulate_cpu.scene with the slab for its cloud"""
    p = m.synth.make_problem(C, 2, seed=seed, noise=0.0)
    cam = p["true_cam"].copy()
    rng = np.random.default_rng(seed + 7)
    T = m.synth._T(p["true_poses"][0])
    X = (rng.normal(0, 1, (P, 3)) * np.array([60.0, 60.0, zs])) @ T[:3, :3].T + T[:3, 3]
    uvs = np.stack([m.synth.project(cam[c:c + 1], np.zeros((1, 6)), X)[0, 0] for c in range(C)])
    uvs += rng.normal(0, noise, uvs.shape) if noise else 0.0
    intr = [(np.array([[c[0], 0, c[2]], [0, c[1], c[3]], [0, 0, 1.0]]), np.r_[c[4:6], 0, 0, 0]) for c in cam]
    return list(uvs), cam[:, 6:], intr, X


_cache = {}


def make(name):
    """the scene of that name, computed once; read-only"""
    if name not in _cache:
        _cache[name] = slab(*SCENES[name])
    return _cache[name]
