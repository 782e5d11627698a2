"""Seeded scenes of the P3P resection generator, the ones the 6-point generator fails on without saying so
(tests/test_p3p_oracle_cpu.py pins that):
  flat3   tests/thin_scenes.slab(3, 200, 13, 0.3, 0.0): an exactly planar cloud, 0.3 px noise
  hair3   the same cloud 0.05 mm deep
  swap6   slab(6, 300, 16, 0.3, 60.0) with 60 % wrong detections: every detection displaced with probability 0.6 by +-U(20, 200) px per
          coordinate from default_rng(99); the cameras in order, each drawing the mask, then the magnitudes, then the signs"""
import numpy as np

import thin_scenes as ts

SLABS = {"flat3": (3, 200, 13, 0.3, 0.0), "hair3": (3, 200, 13, 0.3, 0.05), "swap6": (6, 300, 16, 0.3, 60.0)}
SWAP_SHARE, SWAP_PX, SWAP_SEED = 0.6, (20.0, 200.0), 99

_cache = {}


def make(name):
    """(uvs list, extrinsics (C, 6), intrinsics list, truth (P, 3), clean (C, P) bool: the detections left as projected); computed once, read-only"""
    if name not in _cache:
        uvs, ext, intr, X = ts.slab(*SLABS[name])
        uvs = [np.array(u) for u in uvs]
        clean = np.ones((len(uvs), len(X)), bool)
        if name == "swap6":
            rng = np.random.default_rng(SWAP_SEED)
            for c in range(len(uvs)):
                wrong = rng.random(len(X)) < SWAP_SHARE
                size = rng.uniform(SWAP_PX[0], SWAP_PX[1], (int(wrong.sum()), 2))
                sign = rng.choice([-1.0, 1.0], (int(wrong.sum()), 2))
                uvs[c][wrong] += size * sign
                clean[c] = ~wrong
        for a in uvs + [ext, X, clean]:
            a.setflags(write=False)
        _cache[name] = (uvs, ext, intr, X, clean)
    return _cache[name]
