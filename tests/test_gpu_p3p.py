"""mcba_resect_ransac_p3p (csrc/mcba_resect_p3p.hip) and `solver="p3p"` above it on the GPU, held to tests/p3p_oracle.py by the rules of that
module's docstring: the stages (candidates, costs and counts, winner, mask) on the compared scenes; the launch boundaries (samples around the
64-lane workgroup of the generator and, as 4 H slots, around a chunk of the scorer, up to the cap; points around a workgroup of the scorer);
cameras of different usable counts in one call; bitwise repeatability; the default solver against the former call sequence, bit for bit; and
the end-to-end bar on the scenes the 6-point generator fails on.  Output buffers start as sentinels."""
import numpy as np
import pytest

import keypoint_scenes as ks
import p3p_oracle as po
import p3p_scenes as ps
import resection_oracle as ro
from test_triangulate_cpu import scene
from multicam_calibration_amd import ops, resect_camera, resect_cameras, draw_resection_samples
from multicam_calibration_amd.geometry import _rotation_vector
from multicam_calibration_amd.triangulation import _cam_blocks

pytestmark = pytest.mark.gpu
THR = po.THRESHOLD
SLOTS, CAP, PPB = ops.RESECT_P3P_SLOTS, ops.RESECT_P3P_MAX_SAMPLES, ops.RESECT_POINTS_PER_BLOCK
TIGHT = dict(ftol=1e-15, xtol=1e-15, gtol=1e-10, max_nfev=200)
SENTINEL = 7.0
KEYS = ("rt12", "best", "mask", "pose", "cost", "count", "status")


def buffers(C, n, T):
    return dict(rt12=np.full((C, 12), SENTINEL), best=np.full((C, 4), SENTINEL), mask=np.full((C, n), 7, np.uint8), pose=np.full((C, T, 12), SENTINEL), cost=np.full((C, T), SENTINEL),
                count=np.full((C, T), 7, np.uint32), status=np.full((C, T), 7, np.int32), kernel_ms=np.full(6, SENTINEL))


def call3(points, uvs, intrs, samples, threshold):
    """mcba_resect_ransac_p3p through ops.call for C cameras; uvs (C, P, 2), samples (C, H, 3); tables of 4 H rows"""
    C, H = len(uvs), np.shape(samples)[1]
    cam, dist = _cam_blocks([np.zeros(6)] * C, intrs)
    points, uvs, smp = np.ascontiguousarray(points, dtype=np.float64), np.ascontiguousarray(uvs, dtype=np.float64), np.ascontiguousarray(samples, dtype=np.int32)
    g = buffers(C, len(points), SLOTS * H)
    ops.call("mcba_resect_ransac_p3p", C, len(points), points.ctypes.data, uvs.ctypes.data, cam.ctypes.data, dist.ctypes.data, H, smp.ctypes.data, float(threshold), 5, 0, g["rt12"].ctypes.data,
             g["best"].ctypes.data, g["mask"].ctypes.data, g["pose"].ctypes.data, g["cost"].ctypes.data, g["count"].ctypes.data, g["status"].ctypes.data, g["kernel_ms"].ctypes.data)
    g["inliers"] = g["mask"].astype(bool)
    return g


def call6(points, uvs, intrs, threshold, samples=None, poses_in=None):
    """mcba_resect_ransac, the existing entry: samples (C, H, 6), or a pose table (C, T, 12) handed in"""
    C = len(uvs)
    T = np.shape(samples)[1] if poses_in is None else np.shape(poses_in)[1]
    cam, dist = _cam_blocks([np.zeros(6)] * C, intrs)
    points, uvs = np.ascontiguousarray(points, dtype=np.float64), np.ascontiguousarray(uvs, dtype=np.float64)
    smp = None if samples is None else np.ascontiguousarray(samples, dtype=np.int32)
    pin = None if poses_in is None else np.ascontiguousarray(poses_in, dtype=np.float64)
    g = buffers(C, len(points), T)
    ops.call("mcba_resect_ransac", C, len(points), points.ctypes.data, uvs.ctypes.data, cam.ctypes.data, dist.ctypes.data, T, None if smp is None else smp.ctypes.data,
             None if pin is None else pin.ctypes.data, float(threshold), 5, 0, g["rt12"].ctypes.data, g["best"].ctypes.data, g["mask"].ctypes.data, g["pose"].ctypes.data, g["cost"].ctypes.data,
             g["count"].ctypes.data, g["status"].ctypes.data, g["kernel_ms"].ctypes.data)
    g["inliers"] = g["mask"].astype(bool)
    return g


def row(g, c):
    return {k: v[c] for k, v in g.items() if k != "kernel_ms"}


def check_own_winner(g, n_usable):
    """the call's winner, count and mask against its own tables"""
    own = int(np.lexsort((np.arange(len(g["cost"])), g["cost"]))[0])
    assert g["best"][3] == n_usable and g["best"][0] == own and g["best"][1] == g["cost"][own] and g["best"][2] == g["count"][own] == g["inliers"].sum()
    assert np.array_equal(g["rt12"], g["pose"][own], equal_nan=True)
    void = g["status"] < 0
    assert np.isinf(g["cost"][void]).all() and (g["count"][void] == 0).all() and np.isnan(g["pose"][void]).all() and np.isfinite(g["pose"][~void]).all()


def check_stages(tag, c, smp, o):
    """one camera: candidates; costs and counts (the oracle's table through the scorer; the call's own table through the scorer, bit for bit);
    winner; mask"""
    pts, uv, intr = c["points"], c["uv"], c["intr"]
    g = call3(pts, uv[None], [intr], smp[None], THR)
    assert (g["kernel_ms"] >= 0).all()
    g0 = row(g, 0)
    po.check_candidates(tag, g0["pose"], g0["status"], o["hyp"])
    check_own_winner(g0, o["n_usable"])
    s = call6(pts, uv[None], [intr], THR, poses_in=o["hyp"]["pose"][None])
    assert np.array_equal(s["pose"][0], o["hyp"]["pose"], equal_nan=True)
    ro.check_scores(tag, s["cost"][0], s["count"][0], o["hyp"], o["score"], subset=np.ones(len(o["hyp"]["pose"]), bool))
    same = call6(pts, uv[None], [intr], THR, poses_in=g["pose"])      # the table is scored in place by the same kernels
    for k in KEYS:
        assert np.array_equal(same[k], g[k], equal_nan=True), k
    if o["comparable"]:
        w = o["winner"]
        und = o["score"]["undecided"][w]
        assert g0["best"][0] == w and np.array_equal(g0["inliers"][~und], o["inliers"][~und]) and (np.abs(g0["rt12"] - o["rt12"]) <= o["hyp"]["tol"][w]).all()
    return g


_cache = {}


def case(name, cam, H, points="truth", seed=None):
    key = (name, cam, H, points, repr(seed))
    if key not in _cache:
        c = po.camera_of(name, cam, points)
        smp = po.samples_of(c["usable"], H, [0, cam] if seed is None else seed)
        _cache[key] = (c, smp, po.ransac(c["points"], c["uv"], c["intr"], smp, THR))
    return _cache[key]


# ---------------------------------------------------------------- stage by stage
@pytest.mark.parametrize("name,cam", [("six", 0), ("three", 1), ("flat3", 1)])
def test_stages_on_the_compared_scenes(name, cam):
    c, smp, o = case(name, cam, 64)
    assert po.left_out_share(o["hyp"]) <= po.LEFT_OUT_CAP and not o["score"]["undecided"].any() and o["comparable"]
    check_stages(f"{name} camera {cam}", c, smp, o)


# ---------------------------------------------------------------- launch edges
@pytest.fixture(scope="module")
def cap_table():
    """"three" camera 1, the cap of samples: the oracle's candidates, once"""
    c = po.camera_of("three", 1)
    smp = po.samples_of(c["usable"], CAP, [0, 1])
    return c, smp, po.hypotheses(c["points"], ro.prepare(c["points"], c["uv"], c["intr"]), smp)


@pytest.mark.parametrize("H", [1, 15, 16, 17, 63, 64, 65, CAP])
def test_samples_at_the_launch_boundaries(cap_table, H):
    c, smp, hyp = cap_table
    g = row(call3(c["points"], c["uv"][None], [c["intr"]], smp[None, :H], THR), 0)
    T = SLOTS * H
    ok = hyp["comparable"][:T]
    live = ok & (hyp["status"][:T] > 0)
    ratio = float((np.abs(g["pose"] - hyp["pose"][:T])[live] / hyp["tol"][:T][live]).max()) if live.any() else 0.0
    print(f"H {H}: {T} slots, pose error / tolerance {ratio:.3g} over {int(live.sum())} live slots; comparable samples {int(hyp['sample_comparable'][:H].sum())}")
    assert g["pose"].shape == (T, 12) and np.array_equal(g["status"][ok], hyp["status"][:T][ok]) and ratio <= 1
    check_own_winner(g, int(c["usable"].sum()))
    assert (g["count"] <= c["usable"].sum()).all() and (g["cost"][g["status"] > 0] <= THR ** 2 * c["usable"].sum()).all()


def edge_scene(P, seed=5):
    """camera 1 of a two-camera scene against the true points (0.3 px noise)"""
    uvs, ext, intr, X = scene(C=2, P=P, seed=seed, noise=0.3)
    uv = np.array(uvs[1])
    return dict(points=X, uv=uv, intr=intr[1], ext=ext[1], usable=np.ones(P, bool))


@pytest.mark.parametrize("P", [6, PPB - 1, PPB, PPB + 1])
def test_points_at_the_launch_boundaries(P):
    c = edge_scene(P)
    smp = po.samples_of(c["usable"], 17, P)
    o = po.ransac(c["points"], c["uv"], c["intr"], smp, THR)
    g = check_stages(f"P {P}", c, smp, o)
    if P > 6:
        assert g["best"][0, 2] >= 0.9 * P


# ---------------------------------------------------------------- cameras
def test_cameras_of_5_6_and_many_usable_points_in_one_call():
    uvs, ext, intr, X = scene(C=3, P=PPB + 37, seed=9, noise=0.3)
    uvs = [np.array(u) for u in uvs]
    uvs[0][5:] = np.nan
    uvs[1][6:] = np.nan
    kw = dict(threshold=THR, n_hypotheses=17, solver="p3p")
    singles = [resect_camera(X, uvs[c], intr[c], seed=[3, c], return_info=True, **kw) for c in range(3)]
    r = resect_cameras(X, uvs, intr, seed=3, **kw)
    for c in range(3):
        tr, inl, one = singles[c]
        assert np.array_equal(r.extrinsics[c], tr, equal_nan=True) and np.array_equal(r.inliers[c], inl) and r.status[c] == one.status[0] and np.array_equal(r.cost[c:c + 1], one.cost, equal_nan=True)
        assert r.n_usable[c] == one.n_usable[0] and r.n_inliers[c] == one.n_inliers[0] and r.hypothesis[c] == one.hypothesis[0] and r.nfev[c] == one.nfev[0]
        assert np.array_equal(r.refined_cost[c:c + 1], one.refined_cost, equal_nan=True)
    assert list(r.n_usable) == [5, 6, PPB + 37] and r.status[0] == -1 and np.isnan(r.extrinsics[0]).all() and not r.inliers[0].any() and r.hypothesis[0] == -1 and r.info["samples"][0] is None
    assert r.status[1] == -2 and r.status[2] == 1 and r.info["samples"][2].shape == (17, 3) and 0 <= r.hypothesis[2] < SLOTS * 17
    centre = lambda e: -ks.rodrigues(e[:3]).T @ e[3:]
    assert np.linalg.norm(centre(r.extrinsics[2]) - centre(ext[2])) < 2.0 and r.n_inliers[2] >= 0.97 * r.n_usable[2]
    # the raw call: the first camera's tables are void, the others' equal their own calls
    smp = np.zeros((3, 17, 3), np.int32)
    for c in (1, 2):
        smp[c] = r.info["samples"][c]
    g = call3(X, np.stack(uvs), intr, smp, THR)
    assert np.isnan(g["rt12"][0]).all() and g["best"][0, 0] == -1 and np.isnan(g["best"][0, 1]) and g["best"][0, 2] == 0 and g["best"][0, 3] == 5
    assert not g["inliers"][0].any() and (g["status"][0] == -1).all() and (g["count"][0] == 0).all() and np.isnan(g["pose"][0]).all() and np.isnan(g["cost"][0]).all()
    for c in (1, 2):
        one = call3(X, uvs[c][None], [intr[c]], smp[c][None], THR)
        for k in KEYS:
            assert np.array_equal(g[k][c], one[k][0], equal_nan=True), (c, k)


# ---------------------------------------------------------------- determinism and the default
def test_two_calls_return_the_same_bits():
    c, smp, o = case("swap6", 3, 256)
    np.random.seed(99)
    before = np.random.get_state()[1].copy()
    a, b = (call3(c["points"], c["uv"][None], [c["intr"]], smp[None], THR) for _ in range(2))
    for k in KEYS:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    uvs, ext, intr, X = po.scene("flat3")
    p, q = (resect_cameras(X, uvs, intr, threshold=THR, n_hypotheses=64, seed=4, solver="p3p") for _ in range(2))
    for f in ("extrinsics", "inliers", "status", "n_inliers", "cost", "hypothesis", "refined_cost", "optimality", "nfev", "lm_status"):
        assert np.array_equal(getattr(p, f), getattr(q, f), equal_nan=True), f
    assert np.array_equal(np.random.get_state()[1], before)


def test_the_default_solver_is_the_former_call_sequence_bit_for_bit():
    uvs, ext, intr, X = ks.make("three")
    c0 = ro.camera_of("three", 0)
    pts = c0["points"]      # (a NaN row or two among them)
    H, seed = 65, 4
    plain = resect_cameras(pts, uvs, intr, threshold=THR, n_hypotheses=H, seed=seed)
    named = resect_cameras(pts, uvs, intr, threshold=THR, n_hypotheses=H, seed=seed, solver="dlt6")
    for f in ("extrinsics", "inliers", "status", "n_inliers", "cost", "hypothesis", "refined_cost", "optimality", "nfev", "lm_status", "n_usable"):
        assert np.array_equal(getattr(plain, f), getattr(named, f), equal_nan=True), f
    # the former sequence: samples of six from [seed, c], one call of mcba_resect_ransac, the rotation vector of the winner
    U = np.stack([np.asarray(u, dtype=np.float64) for u in uvs])
    usable = np.isfinite(pts).all(1)[None] & np.isfinite(U).all(2)
    smp = np.stack([np.flatnonzero(usable[c]).astype(np.int32)[draw_resection_samples(int(usable[c].sum()), H, [seed, c])] for c in range(len(U))])
    g = call6(pts, U, intr, THR, samples=smp)
    for c in range(len(U)):
        assert np.array_equal(plain.info["samples"][c], smp[c]) and plain.info["samples"][c].shape == (H, 6)
        assert np.array_equal(plain.info["ransac_extrinsics"][c], np.r_[_rotation_vector(g["rt12"][c, :9].reshape(3, 3)), g["rt12"][c, 9:]])
        assert np.array_equal(plain.inliers[c], g["inliers"][c]) and plain.cost[c] == g["best"][c, 1] and plain.hypothesis[c] == g["best"][c, 0] and plain.n_inliers[c] == g["best"][c, 2]
    tr, inl = resect_camera(pts, uvs[1], intr[1], threshold=THR, n_hypotheses=H, seed=[seed, 1])
    assert np.array_equal(tr, plain.extrinsics[1]) and np.array_equal(inl, plain.inliers[1])


# ---------------------------------------------------------------- end to end
@pytest.mark.parametrize("name,cam,points,seed", [("flat3", 1, "truth", [0, 1]), ("hair3", 1, "others", [0, 1]), ("swap6", 3, "truth", 0)])
def test_end_to_end_where_the_six_point_generator_fails(name, cam, points, seed):
    """status 1, the oracle's mask, and a polish that ends where the polish started from the truth on the same mask ends (section 7's 1e-7).
    What the six-point generator does on the same inputs is pinned in tests/test_p3p_oracle_cpu.py."""
    c, smp, o = case(name, cam, 64, points, seed)
    tr, inl, r = resect_camera(c["points"], c["uv"], c["intr"], threshold=THR, n_hypotheses=64, seed=seed, solver="p3p", return_info=True, **TIGHT)
    assert np.array_equal(r.info["samples"][0], smp) and r.status[0] == 1 and r.hypothesis[0] // SLOTS < 64
    print(f"{name} camera {cam}: inliers {r.n_inliers[0]} of {r.n_usable[0]} (oracle {o['n_inliers']}, comparable {o['comparable']}); winning slot {r.hypothesis[0]} (oracle {o['winner']}); "
          f"polish nfev {r.nfev[0]} status {r.lm_status[0]}")
    if o["comparable"]:
        und = o["score"]["undecided"][o["winner"]]
        assert r.hypothesis[0] == o["winner"] and np.array_equal(inl[~und], o["inliers"][~und])
    if name == "swap6":
        assert np.array_equal(inl, ps.make("swap6")[4][3])
    cam12, dist = _cam_blocks([c["ext"]], [c["intr"]])
    pts, uv, mask = np.ascontiguousarray(c["points"]), np.ascontiguousarray(c["uv"]), np.ascontiguousarray(inl, dtype=np.uint8)
    ref, res = np.full((1, 6), SENTINEL), np.full((1, 8), SENTINEL)
    ops.call("mcba_resect_refine", 1, len(pts), pts.ctypes.data, uv.ctypes.data, mask.ctypes.data, cam12.ctypes.data, dist.ctypes.data, None, ops.LOSSES["soft_l1"], 1.0, TIGHT["ftol"], TIGHT["xtol"],
             TIGHT["gtol"], TIGHT["max_nfev"], 0, ref.ctypes.data, res.ctypes.data, None, None)
    err = np.abs(tr - ref[0]) / np.maximum(1.0, np.abs(ref[0]))
    dc, dr = po.pose_errors(np.r_[ks.rodrigues(tr[:3]).ravel(), tr[3:]], c["ext"])
    print(f"{name} camera {cam}: polished from the winner against polished from the truth {err.max():.3g} (bar 1e-7); cost {r.refined_cost[0]:.12g} against {res[0, 1]:.12g}; "
          f"centre {dc:.3g} mm and rotation {dr:.3g} degrees from the truth")
    assert err.max() <= 1e-7
