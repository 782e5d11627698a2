"""The wide rigs of refine_extrinsics(reduction="tiled"): the case table of tests/golden/kpba_wide.npz -- 25 to 64 cameras,
past what the resident reduction holds -- and the inputs of the one-evaluation tests of the tiled path.  Everything is built from the seeded
scene() of tests/test_triangulate_cpu.py and kpba_oracle.perturbed_start; the oracle and its bounds are kpba_oracle's, unchanged.

    name -> (cameras, points, seed, loss)      "w32_outlier": the scene of "w32" with a seeded 15 % of its present detections displaced by N(0, 40^2) px
"""
import os

import numpy as np

import kpba_oracle as ko
from test_triangulate_cpu import scene

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kpba_wide.npz")
CASES = {"w25": (25, 60, 51, "linear"), "w32": (32, 80, 52, "linear"), "w32_outlier": (32, 80, 52, "soft_l1"), "w64": (64, 96, 53, "linear")}
OUTLIER_FRACTION, OUTLIER_SIGMA, OUTLIER_SEED = 0.15, 40.0, 2038
NOISE, P_UNSEEN = 0.3, 0.5


def make_scene(name):
    C, P, seed, _ = CASES[name]
    uvs, ext, intr, X = scene(C=C, P=P, seed=seed, noise=NOISE, p_unseen=P_UNSEEN)
    uvs = [np.array(u) for u in uvs]
    if name.endswith("_outlier"):
        rng = np.random.default_rng(OUTLIER_SEED)
        seen = ~np.isnan(np.stack(uvs)).any(-1)
        hit = seen & (rng.uniform(size=seen.shape) < OUTLIER_FRACTION)
        shift = rng.normal(0, OUTLIER_SIGMA, seen.shape + (2,))
        for c in range(C):
            uvs[c][hit[c]] += shift[c][hit[c]]
    return uvs, ext, intr, X


_golden = None


def golden():
    global _golden
    if _golden is None:
        _golden = dict(np.load(GOLDEN, allow_pickle=False))
    return _golden


def pinned_cases():
    g = golden()
    return [n for n in CASES if f"{n}/extrinsics" in g and bool(g[f"{n}/pinned"])]


def unpinned_cases():
    g = golden()
    return [n for n in CASES if f"{n}/extrinsics" in g and not bool(g[f"{n}/pinned"])]


def case(name):
    """the inputs (scene and first start) and the stored optimum of a case, in the keys of kpba_oracle.case"""
    g = golden()
    uvs, ext, intr, X = make_scene(name)
    return dict(uvs=uvs, intr=intr, loss=CASES[name][3], ext0=g[f"{name}/ext0"], pts0=g[f"{name}/pts0"]), \
        dict(extrinsics=g[f"{name}/extrinsics"], points=g[f"{name}/points"], cost=float(g[f"{name}/cost"]), held=g[f"{name}/held"], spread_ext=float(g[f"{name}/spread_ext"]),
             spread_pts=float(g[f"{name}/spread_pts"]), scale_camera=int(g[f"{name}/scale_camera"]))


# ---------------------------------------------------------------- the inputs of the one-evaluation tests of the tiled path
# B = 16 cameras to a band, G = 16 points to a group, at most PARTIAL_CAP(C) partial systems (the rule of csrc/mcba_kpba_tiled.hip, restated).
BAND, GROUP, CHUNK = 16, 16, 256
CAMERA_COUNTS = tuple(dict.fromkeys((2, 6, BAND - 1, BAND, BAND + 1, 2 * BAND, 2 * BAND + 1, 24, 25, 33, 63, 64)))   # (2 B + 1 is 33: once)
GROUP_EDGES = (GROUP - 1, GROUP, GROUP + 1)
AGAINST_RESIDENT = (2, 6, BAND + 1, 24)


def partial_size(C):
    NP = (6 * C + 15) // 16 * 16
    return NP * NP + 33 * C + 4


def partial_cap(C):
    """the partials of a pass together take no more than the resident path's largest: 512 at 24 cameras.  A power of two below that, at most 512"""
    n = 512 * partial_size(24) // partial_size(C)
    cap = 1
    while cap * 2 <= min(n, 512):
        cap *= 2
    return cap


def launch_facts(C, P):
    nb = (C + BAND - 1) // BAND
    return dict(band=BAND, band_pairs=nb * (nb + 1) // 2, group=GROUP, workgroups=min((P + CHUNK - 1) // CHUNK, partial_cap(C)), NP=(6 * C + 15) // 16 * 16)


INPUTS = {f"c{C}": dict(C=C, P=70, seed=400 + C, p_unseen=0.4) for C in CAMERA_COUNTS}
INPUTS.update({f"g25_p{n}": dict(C=25, P=n, seed=500 + n, p_unseen=0.4) for n in GROUP_EDGES})
INPUTS.update({f"p{n}": dict(C=17, P=n, seed=600, p_unseen=0.4) for n in (255, 256, 257)})
INPUTS.update({"p600_gap": dict(C=17, P=600, seed=601, p_unseen=0.4, edit="gap"), "p257_last": dict(C=17, P=257, seed=602, p_unseen=0.0, edit="last"),
               "held": dict(C=33, P=70, seed=603, p_unseen=0.85, edit="held", loss="soft_l1", f_scale=1.5, lam=1e-2)})
# one more chunk than the partial cap: the first shape with the grid stride.  The seeds are ones with which the last point is a used one
# ("thin": seven of every eight points of the 64-camera one start NaN and take no part -- the oracle of all 16 385 takes most of a minute; the last point stays)
INPUTS.update({"stride64": dict(C=64, P=CHUNK * partial_cap(64) + 1, seed=604, p_unseen=0.5, edit="thin"), "stride3": dict(C=3, P=CHUNK * partial_cap(3) + 1, seed=304, p_unseen=0.25)})
LOSS_GRID = [(loss, fs, lam) for loss in ko.LOSS_NAMES for fs in (1.0, 3.0) for lam in (0.0, 1e-4, 1.0)]
INPUTS.update({f"outlier_{loss}_{fs}_{lam}": dict(C=25, P=70, seed=607, p_unseen=0.78, outliers=True, loss=loss, f_scale=fs, lam=lam) for loss, fs, lam in LOSS_GRID})
STRIDE = ("stride64", "stride3")

_cache = {}


def system_case(name):
    """(inputs, oracle) of one input of INPUTS, as kpba_oracle.system_case hands them out: computed once and shared, read-only"""
    if name in _cache:
        return _cache[name]
    sp = INPUTS[name]
    uvs, ext, intr, X = scene(C=sp["C"], P=sp["P"], seed=sp["seed"], noise=0.3, p_unseen=sp["p_unseen"])
    uvs = [np.array(u) for u in uvs]
    seed = sp["seed"]
    if sp.get("outliers"):
        rng = np.random.default_rng(8000 + seed)
        seen = ~np.isnan(np.stack(uvs)).any(-1)
        hit = seen & (rng.uniform(size=seen.shape) < OUTLIER_FRACTION)
        for c in range(sp["C"]):
            uvs[c][hit[c]] += rng.normal(0, OUTLIER_SIGMA, (int(hit[c].sum()), 2))
    ext0, pts0 = ko.perturbed_start(ext, X, 0, 5000 + seed)
    edit = sp.get("edit")
    if edit == "gap":
        pts0[256:512] = np.nan
    elif edit == "last":
        pts0[:255] = np.nan
    elif edit == "thin":
        pts0[np.arange(len(pts0)) % 8 != 0] = np.nan
    elif edit == "held":
        uvs[3][:] = np.nan
        uvs[20][:] = np.nan   # (a camera of the second band without detections)
    held, scale_camera = ko.held_mask(ext0, uvs, pts0, scale_camera=1 if edit == "held" else None)
    if edit == "held":
        held[2] = held[17] = held[32] = [False, True, False, True, False, True]   # 0b101010 in every band
        assert held[0].all() and held[3].all() and held[20].all() and held[1].sum() == 1
    rng = np.random.default_rng(7000 + seed)
    dtheta = np.concatenate([rng.normal(0, 1e-3, (len(ext0), 3)), rng.normal(0, 0.5, (len(ext0), 3))], axis=1) * ~held
    i = dict(uvs=uvs, ext0=ext0, intr=intr, pts0=pts0, held=held, loss=sp.get("loss", "linear"), f_scale=sp.get("f_scale", 1.0), lam=sp.get("lam", 1e-4), step=(ext0 + dtheta, dtheta))
    o = ko.block_system(uvs, ext0, intr, pts0, held, loss=i["loss"], f_scale=i["f_scale"], lam=i["lam"], step=i["step"])
    assert name not in STRIDE or o["used"][-1]
    if len(_cache) >= 8 or name in STRIDE:
        _cache.clear()
    _cache[name] = (i, o)
    return i, o
