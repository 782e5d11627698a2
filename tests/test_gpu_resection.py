"""mcba_resect_ransac / mcba_resect_refine (csrc/mcba_resect.hip) and the public functions above them on the GPU, held to tests/resection_oracle.py by
the rules of that module's docstring: every stage on the compared scenes; the launch boundaries (fewer points than a sample, a sample exactly, a
workgroup of the scoring kernel +- 1; one hypothesis, a chunk +- 1, two chunks + 2; one to three cameras of different usable counts in one call);
points behind the camera; a coplanar set; the error paths; bitwise repeatability; the polish against the pinned goldens of
tests/golden/resection.npz; and the end-to-end bar: a camera resected against the triangulation of the others, then refine_extrinsics, reaches the
stored optimum of tests/golden/kpba.npz (kpba_oracle.check_result).  Output buffers start as sentinels."""
import numpy as np
import pytest

import kpba_oracle as ko
import keypoint_scenes as ks
import resection_oracle as ro
from test_triangulate_cpu import scene
from multicam_calibration_amd import ops, refine_extrinsics, triangulate, resect_camera, resect_cameras
from multicam_calibration_amd.triangulation import _cam_blocks

pytestmark = pytest.mark.gpu
THR = ro.THRESHOLD
CHUNK, PPB, CAP = ops.RESECT_CHUNK, ops.RESECT_POINTS_PER_BLOCK, ops.RESECT_MAX_HYPOTHESES
TIGHT = dict(ftol=1e-15, xtol=1e-15, gtol=1e-10, max_nfev=200)
SENTINEL = 7.0


def call(points, uvs, intrs, samples, threshold, poses_in=None, H=None, ext=None):
    """mcba_resect_ransac through ops.call for C cameras; every output starts as a sentinel.  uvs (C, P, 2), samples (C, H, 6) or poses_in (C, H, 12)"""
    C = len(uvs)
    cam, dist = _cam_blocks([np.zeros(6)] * C if ext is None else ext, intrs)
    points, uvs = np.ascontiguousarray(points, dtype=np.float64), np.ascontiguousarray(uvs, dtype=np.float64)
    n = len(points)
    H = (np.shape(samples)[1] if poses_in is None else np.shape(poses_in)[1]) if H is None else H
    g = dict(rt12=np.full((C, 12), SENTINEL), best=np.full((C, 4), SENTINEL), mask=np.full((C, n), 7, np.uint8), pose=np.full((C, max(H, 1), 12), SENTINEL), cost=np.full((C, max(H, 1)), SENTINEL),
             count=np.full((C, max(H, 1)), 7, np.uint32), status=np.full((C, max(H, 1)), 7, np.int32), kernel_ms=np.full(6, SENTINEL))
    call.last = g
    smp = None if samples is None else np.ascontiguousarray(samples, dtype=np.int32)
    pin = None if poses_in is None else np.ascontiguousarray(poses_in, dtype=np.float64)
    ops.call("mcba_resect_ransac", C, n, points.ctypes.data, uvs.ctypes.data, cam.ctypes.data, dist.ctypes.data, H, None if smp is None else smp.ctypes.data, None if pin is None else pin.ctypes.data,
             float(threshold), 5, 0, g["rt12"].ctypes.data, g["best"].ctypes.data, g["mask"].ctypes.data, g["pose"].ctypes.data, g["cost"].ctypes.data, g["count"].ctypes.data, g["status"].ctypes.data,
             g["kernel_ms"].ctypes.data)
    g["inliers"] = g["mask"].astype(bool)
    return g


def untouched(g):
    return all((g[k] == 7).all() for k in ("rt12", "best", "mask", "pose", "cost", "count", "status", "kernel_ms"))


def refine(points, uvs, masks, intrs, starts, loss="linear", f_scale=1.0, active=None, **kw):
    """mcba_resect_refine through ops.call"""
    kw = {**dict(ftol=1e-8, xtol=1e-8, gtol=1e-8, max_nfev=50), **kw}
    cam, dist = _cam_blocks(list(starts), list(intrs))
    C, n = len(cam), len(points)
    points, uvs = np.ascontiguousarray(points, dtype=np.float64), np.ascontiguousarray(np.stack(uvs), dtype=np.float64)
    masks = np.ascontiguousarray(np.stack(masks), dtype=np.uint8)
    act = None if active is None else np.ascontiguousarray(active, dtype=np.int32)
    g = dict(extrinsics=np.full((C, 6), SENTINEL), result=np.full((C, 8), SENTINEL), system=np.full((C, 29), SENTINEL), kernel_ms=np.full(2, SENTINEL))
    ops.call("mcba_resect_refine", C, n, points.ctypes.data, uvs.ctypes.data, masks.ctypes.data, cam.ctypes.data, dist.ctypes.data, None if act is None else act.ctypes.data, ops.LOSSES[loss],
             float(f_scale), kw["ftol"], kw["xtol"], kw["gtol"], int(kw["max_nfev"]), 0, g["extrinsics"].ctypes.data, g["result"].ctypes.data, g["system"].ctypes.data, g["kernel_ms"].ctypes.data)
    return g


_cache = {}


def case(name, cam, H):
    """(the camera's inputs, samples, the oracle's stages): computed once, read-only"""
    if (name, cam, H) not in _cache:
        c = ro.camera_of(name, cam)
        smp = ro.samples_of(c["usable"], H, [0, cam])
        _cache[(name, cam, H)] = (c, smp, ro.ransac(c["points"], c["uv"], c["intr"], smp, THR))
    return _cache[(name, cam, H)]


def check_camera(tag, g, c, o, with_hypotheses=True):
    """one camera's row of a call (already sliced) against the oracle's stages"""
    if with_hypotheses:      # (costs are compared with the oracle's own poses handed in: the bound covers the scoring, not a pose that differs within its tolerance)
        ro.check_hypotheses(tag, g["pose"], g["status"], o["hyp"])
    else:
        ro.check_scores(tag, g["cost"], g["count"], o["hyp"], o["score"], subset=np.ones(len(g["cost"]), bool))
    own = int(np.lexsort((np.arange(len(g["cost"])), g["cost"]))[0])
    assert g["best"][3] == o["n_usable"] and g["best"][0] == own and g["best"][1] == g["cost"][own] and g["best"][2] == g["count"][own] == g["inliers"].sum()
    assert np.array_equal(g["rt12"], g["pose"][own], equal_nan=True)
    if o["comparable"] if with_hypotheses else ro.winner(o["score"]["cost"])[1]:
        w = o["winner"]
        und = o["score"]["undecided"][w]
        assert g["best"][0] == w and np.array_equal(g["inliers"][~und], o["inliers"][~und])


def row(g, c):
    return {k: v[c] for k, v in g.items() if k != "kernel_ms"}


# ---------------------------------------------------------------- stage by stage
@pytest.mark.parametrize("name,cam,H", [("six", 0, 64), ("six", 5, 512), ("three", 1, 64)])
def test_stages_on_the_compared_scenes(name, cam, H):
    c, smp, o = case(name, cam, H)
    assert ro.left_out_share(o["hyp"]) <= ro.LEFT_OUT_CAP and not o["score"]["undecided"].any()
    g = call(c["points"], c["uv"][None], [c["intr"]], smp[None], THR)
    check_camera(f"{name} camera {cam} H {H}", row(g, 0), c, o)
    assert (g["kernel_ms"] >= 0).all()
    s = call(c["points"], c["uv"][None], [c["intr"]], None, THR, poses_in=o["hyp"]["pose"][None])
    assert np.array_equal(s["pose"][0], o["hyp"]["pose"], equal_nan=True)
    check_camera(f"{name} camera {cam} H {H}, poses handed in", row(s, 0), c, o, with_hypotheses=False)
    assert np.array_equal(s["count"][0], o["score"]["count"])


@pytest.mark.parametrize("name,cam", [("outlier", 1), ("twelve", 4)])
def test_scoring_and_winner_with_poses_handed_in(name, cam):
    c, smp, o = case(name, cam, 64)
    s = call(c["points"], c["uv"][None], [c["intr"]], None, THR, poses_in=o["hyp"]["pose"][None])
    check_camera(f"{name} camera {cam}", row(s, 0), c, o, with_hypotheses=False)
    assert not o["score"]["undecided"].any() and np.array_equal(s["count"][0], o["score"]["count"])


# ---------------------------------------------------------------- launch edges
def edge_scene(P, seed=5, behind=0):
    """camera 1 of a two-camera scene against the true points (0.3 px noise); `behind`: that many further points mirrored through the camera's
    centre, detected where their mirror images are -- usable, on the pixel, and behind the camera"""
    uvs, ext, intr, X = scene(C=2, P=P, seed=seed, noise=0.3)
    uv = np.array(uvs[1])
    if behind:
        R, t = ks.rodrigues(ext[1][:3]), ext[1][3:]
        centre = -R.T @ t
        X = np.r_[X, 2 * centre - X[:behind]]
        uv = np.r_[uv, uv[:behind]]
    return X, uv, intr[1], ext[1]


@pytest.mark.parametrize("P", [1, 5, 6, PPB - 1, PPB, PPB + 1])
def test_points_at_the_launch_boundaries(P):
    X, uv, intr, ext = edge_scene(P)
    if P < 6:
        g = call(X, uv[None], [intr], np.zeros((1, 3, 6), np.int32), THR)
        assert np.isnan(g["rt12"]).all() and g["best"][0, 0] == -1 and np.isnan(g["best"][0, 1]) and g["best"][0, 2] == 0 and g["best"][0, 3] == P
        assert not g["inliers"].any() and (g["status"] == -1).all() and (g["count"] == 0).all() and np.isnan(g["pose"]).all() and np.isnan(g["cost"]).all()
        tr, inl, r = resect_camera(X, uv, intr, threshold=THR, return_info=True)
        assert np.isnan(tr).all() and not inl.any() and r.status[0] == -1 and r.n_usable[0] == P and r.lm_status[0] == -1
        return
    smp = ro.samples_of(np.ones(P, bool), 65, P)
    o = ro.ransac(X, uv, intr, smp, THR)
    g = call(X, uv[None], [intr], smp[None], THR)
    check_camera(f"P {P}", row(g, 0), None, o)
    if P > 6:
        assert g["best"][0, 2] >= 0.97 * P


@pytest.mark.parametrize("H", sorted({1, 63, 64, 65, 130, CHUNK - 1, CHUNK + 1, 2 * CHUNK + 2}))
def test_hypotheses_at_the_launch_boundaries(H):
    c, smp, o = case("three", 1, 2 * CHUNK + 2)
    g = call(c["points"], c["uv"][None], [c["intr"]], smp[None, :H], THR)
    ok = o["hyp"]["comparable"][:H]
    ratio = float((np.abs(g["pose"][0] - o["hyp"]["pose"][:H])[ok] / o["hyp"]["tol"][:H][ok]).max()) if ok.any() else 0.0
    print(f"H {H}: pose error / tolerance {ratio:.3g}; comparable {int(ok.sum())}")
    assert np.array_equal(g["status"][0][ok], o["hyp"]["status"][:H][ok]) and ratio <= 1
    own = int(np.lexsort((np.arange(H), g["cost"][0]))[0])
    assert g["best"][0, 0] == own and g["best"][0, 1] == g["cost"][0, own] and g["best"][0, 2] == g["count"][0, own] == g["inliers"][0].sum() and np.isfinite(g["cost"][0][ok]).all()
    assert (g["count"][0][ok] <= o["n_usable"]).all() and (g["cost"][0][ok] <= THR ** 2 * o["n_usable"]).all()


def finish_scene():
    """(X, uvs (2, P, 2), intrs, poses (2, 5, 12)): cameras 1 and 2 of a three-camera scene (0.3 px noise) at 257 workgroups + 1 point; per camera
    the true pose and four perturbed ones (rotation vector by 1e-4 rad, translation by 0.5 scene units per coordinate, normal, seeded)"""
    uvs, ext, intr, X = scene(C=3, P=257 * PPB + 1, seed=5, noise=0.3)
    rng = np.random.default_rng(11)
    poses = np.empty((2, 5, 12))
    for a, c in enumerate((1, 2)):
        for h in range(5):
            e = ext[c] + (rng.normal(size=6) * np.r_[[1e-4] * 3, [0.5] * 3] if h else 0.0)
            poses[a, h] = np.r_[ks.rodrigues(e[:3]).ravel(), e[3:]]
    return X, np.stack([np.array(uvs[1]), np.array(uvs[2])]), [intr[1], intr[2]], poses


def test_finish_past_one_partial_per_lane_with_a_second_camera():
    """k_hyp_finish with more partials than lanes (257 workgroups + 1 point: lane 0 sums two) AND a camera index above 0, in one call: C = 2,
    H = 5 poses handed in.  Each camera's row is held to the oracle as in test_scoring_and_winner_with_poses_handed_in."""
    X, uvs, intrs, poses = finish_scene()
    g = call(X, uvs, intrs, None, THR, poses_in=poses)
    assert np.array_equal(g["pose"], poses)
    for a in range(2):
        o = ro.ransac(X, uvs[a], intrs[a], None, THR, poses_in=poses[a])
        check_camera(f"257 workgroups + 1 point, camera {a}", row(g, a), None, o, with_hypotheses=False)
        assert g["best"][a, 3] == len(X)


def test_cameras_of_different_usable_counts_in_one_call():
    """C = 1, 2, 3: the third camera sees 4 points (status -1, NaN, nothing launched for it), the second about half; every row equals its single-camera call bit for bit"""
    uvs, ext, intr, X = scene(C=3, P=PPB + 37, seed=9, noise=0.3)
    uvs = [np.array(u) for u in uvs]
    uvs[1][::2] = np.nan
    uvs[2][4:] = np.nan
    pts = X.copy()
    pts[10] = np.nan
    singles = [resect_camera(pts, uvs[c], intr[c], threshold=THR, n_hypotheses=65, seed=[3, c], return_info=True) for c in range(3)]
    for C in (1, 2, 3):
        r = resect_cameras(pts, uvs[:C], intr[:C], threshold=THR, n_hypotheses=65, seed=3)
        for c in range(C):
            tr, inl, one = singles[c]
            assert np.array_equal(r.extrinsics[c], tr, equal_nan=True) and np.array_equal(r.inliers[c], inl) and r.status[c] == one.status[0] and np.array_equal(r.cost[c:c + 1], one.cost, equal_nan=True)
            assert r.n_usable[c] == one.n_usable[0] and r.n_inliers[c] == one.n_inliers[0] and r.hypothesis[c] == one.hypothesis[0] and r.nfev[c] == one.nfev[0]
            assert np.array_equal(r.refined_cost[c:c + 1], one.refined_cost, equal_nan=True)
    assert list(r.status) == [1, 1, -1] and np.isnan(r.extrinsics[2]).all() and not r.inliers[2].any() and r.n_usable[2] == 4 and r.info["samples"][2] is None
    assert not r.inliers[:, 10].any() and r.n_usable[0] == PPB + 36
    for c in (0, 1):
        centre = lambda e: -ks.rodrigues(e[:3]).T @ e[3:]
        assert np.linalg.norm(centre(r.extrinsics[c]) - centre(ext[c])) < 2.0 and r.n_inliers[c] >= 0.97 * r.n_usable[c]


def test_points_behind_the_true_camera_are_not_inliers():
    P, nb = 300, 60
    X, uv, intr, ext = edge_scene(P, seed=6, behind=nb)
    pose = np.r_[ks.rodrigues(ext[:3]).ravel(), ext[3:]]
    o = ro.ransac(X, uv, intr, None, THR, poses_in=pose[None])
    assert o["n_usable"] == P + nb and not o["inliers"][P:].any() and o["inliers"][:P].mean() > 0.97 and not o["score"]["undecided"].any()
    s = call(X, uv[None], [intr], None, THR, poses_in=pose[None, None])
    check_camera("behind, the true pose handed in", row(s, 0), None, o, with_hypotheses=False)
    assert np.array_equal(s["inliers"][0], o["inliers"]) and s["cost"][0, 0] >= nb * THR ** 2
    tr, inl, r = resect_camera(X, uv, intr, threshold=THR, n_hypotheses=128, return_info=True)
    print(f"behind: inliers {inl[:P].sum()} of {P} in front, {inl[P:].sum()} of {nb} behind; status {r.status[0]}")
    assert r.status[0] == 1 and not inl[P:].any() and inl[:P].mean() > 0.97 and np.abs(tr - ext).max() < 0.5


def coplanar_scene(P=80, seed=0):
    """camera 1 of a two-camera scene whose points are pushed onto one plane (to rounding), detected with 0.3 px of noise"""
    uvs, ext, intr, X = scene(C=2, P=P, seed=seed, noise=0.0)
    n = np.array([0.3, 0.2, 1.0]) / np.linalg.norm([0.3, 0.2, 1.0])
    Xp = X - np.outer((X - X.mean(0)) @ n, n)
    return Xp, ks.project5(Xp, ext[1], *intr[1]) + np.random.default_rng(seed).normal(0, 0.3, (P, 2)), intr[1]


def test_a_coplanar_point_set_ends_in_status_minus_2():
    """Coplanar points end in status -2 and raise no exception: the 6-point DLT is degenerate for them (its normal matrix has a null space of
    four dimensions, eigen-gap at rounding level), a start that is not defined is void (RS_DLT_GAP_MIN), so every hypothesis is void, nothing
    has an inlier, and the polish has nothing to start from."""
    Xp, uv, intr = coplanar_scene()
    smp = ro.samples_of(np.ones(len(Xp), bool), 64, 1)
    o = ro.ransac(Xp, uv, intr, smp, THR)
    g = call(Xp, uv[None], [intr], smp[None], THR)
    print(f"coplanar: oracle's largest eigen-gap {o['hyp']['gap'].max():.3g}; void {int((g['status'][0] < 0).sum())} of 64")
    assert (o["hyp"]["status"] == -1).all() and (g["status"] == -1).all() and np.isinf(g["cost"]).all() and (g["count"] == 0).all() and np.isnan(g["pose"]).all()
    assert g["best"][0, 0] == 0 and np.isinf(g["best"][0, 1]) and g["best"][0, 2] == 0 and g["best"][0, 3] == len(Xp) and np.isnan(g["rt12"]).all() and not g["inliers"].any()
    tr, inl, r = resect_camera(Xp, uv, intr, threshold=THR, return_info=True)
    print(f"coplanar: status {r.status[0]}, inliers {r.n_inliers[0]} of {r.n_usable[0]}, lm_status {r.lm_status[0]}")
    assert r.status[0] == -2 and r.n_inliers[0] == 0 and not inl.any() and np.isnan(tr).all() and r.lm_status[0] == -1 and r.n_usable[0] == len(Xp)
    # beside a camera with points in general position, in one call: that camera is what it is alone
    X2, uv2, intr2, _ = edge_scene(len(Xp), seed=7)
    both = resect_cameras(X2, [uv2, uv2], [intr2, intr2], threshold=THR, n_hypotheses=64, seed=2)
    mixed = resect_cameras(Xp, [uv], [intr], threshold=THR, n_hypotheses=64, seed=2)
    assert list(both.status) == [1, 1] and mixed.status[0] == -2


# ---------------------------------------------------------------- error paths
def test_error_paths_leave_the_outputs_unwritten():
    c, smp, _ = case("three", 1, 64)
    twice = smp.copy()
    twice[17, 5] = twice[17, 2]
    beyond = smp.copy()
    beyond[3, 0] = len(c["points"])
    unusable = smp.copy()
    unusable[5, 1] = int(np.flatnonzero(~c["usable"])[0])
    a = (c["points"], c["uv"][None], [c["intr"]])
    for what, args in (("H = cap + 1", (*a, np.zeros((1, CAP + 1, 6), np.int32), THR)), ("a repeated index", (*a, twice[None], THR)), ("an index out of range", (*a, beyond[None], THR)),
                       ("a sampled point that is not usable", (*a, unusable[None], THR)), ("threshold = 0", (*a, smp[None], 0.0)),
                       ("65 cameras", (c["points"], np.repeat(c["uv"][None], 65, 0), [c["intr"]] * 65, np.repeat(smp[None], 65, 0), THR))):
        with pytest.raises(ops.McbaError) as e:
            call(*args)
        print(what, "->", e.value)
        assert e.value.code == ops.ERR_ARG and untouched(call.last), what
    for kw in (dict(loss_code=5), dict(f_scale=0.0), dict(max_nfev=0)):
        ext, res = np.full((1, 6), SENTINEL), np.full((1, 8), SENTINEL)
        cam, dist = _cam_blocks([c["ext"]], [c["intr"]])
        pts, uv, mask = np.ascontiguousarray(c["points"]), np.ascontiguousarray(c["uv"]), np.ascontiguousarray(c["usable"], dtype=np.uint8)
        with pytest.raises(ops.McbaError) as e:
            ops.call("mcba_resect_refine", 1, len(pts), pts.ctypes.data, uv.ctypes.data, mask.ctypes.data, cam.ctypes.data, dist.ctypes.data, None, kw.get("loss_code", 0), kw.get("f_scale", 1.0), 1e-8,
                     1e-8, 1e-8, kw.get("max_nfev", 50), 0, ext.ctypes.data, res.ctypes.data, None, None)
        assert e.value.code == ops.ERR_ARG and (ext == SENTINEL).all() and (res == SENTINEL).all()


# ---------------------------------------------------------------- determinism
def test_two_calls_return_the_same_bits_and_the_input_pose_is_never_read():
    c = ro.camera_of("outlier", 1)
    smp = ro.samples_of(c["usable"], 512, [0, 1])
    np.random.seed(99)
    before = np.random.get_state()[1].copy()
    garbage = [np.array([1e9, -3.0, np.nan, np.inf, 0.0, -1e-300])]
    a, b, k = (call(c["points"], c["uv"][None], [c["intr"]], smp[None], THR, ext=e) for e in (None, None, garbage))
    for key in ("rt12", "best", "mask", "pose", "cost", "count", "status"):
        assert np.array_equal(a[key], b[key], equal_nan=True) and np.array_equal(a[key], k[key], equal_nan=True), key
    uvs, ext, intr, _ = ks.make("three")
    pts = triangulate(uvs, ext, intr)
    p, q = (resect_cameras(pts, uvs, intr, threshold=THR, n_hypotheses=64, seed=4) for _ in range(2))
    for f in ("extrinsics", "inliers", "status", "n_inliers", "cost", "hypothesis", "refined_cost", "optimality", "nfev", "lm_status"):
        assert np.array_equal(getattr(p, f), getattr(q, f), equal_nan=True), f
    for cam in range(3):
        tr, inl = resect_camera(pts, uvs[cam], intr[cam], threshold=THR, n_hypotheses=64, seed=[4, cam])
        assert np.array_equal(tr, p.extrinsics[cam]) and np.array_equal(inl, p.inliers[cam]) and np.array_equal(p.info["samples"][cam][:, 0] >= 0, np.ones(64, bool))
    assert np.array_equal(np.random.get_state()[1], before)


# ---------------------------------------------------------------- the polish
@pytest.mark.parametrize("loss", ko.LOSS_NAMES)
def test_normal_system_matches_the_oracle(loss):
    c = ro.camera_of("outlier", 1)
    start = ro.perturbed_start(c["ext"], 5)
    g = refine(c["points"], [c["uv"]], [c["usable"]], [c["intr"]], [start], loss=loss, f_scale=1.5, max_nfev=1)
    assert g["result"][0, 5] == 0 and g["result"][0, 3] == 1 and np.array_equal(g["extrinsics"][0], start) and g["kernel_ms"][1] == 1
    ro.check_system(f"{loss}", g["system"][0], ro.normal_system(start, c["points"], c["uv"], c["usable"], c["intr"], loss, 1.5))


def test_normal_system_past_one_workgroup_of_points():
    X, uv, intr, ext = edge_scene(PPB + 1, seed=8)
    mask = np.ones(PPB + 1, bool)
    mask[::7] = False
    start = ro.perturbed_start(ext, 6)
    g = refine(X, [uv], [mask], [intr], [start], loss="soft_l1", max_nfev=1)
    ro.check_system("P 1025, masked", g["system"][0], ro.normal_system(start, X, uv, mask, intr, "soft_l1", 1.0))


@pytest.mark.parametrize("name", sorted(ro.GOLDEN_CASES))
def test_the_polish_reaches_the_goldens(name):
    i, o = ro.golden_case(name)
    g = refine(i["points"], [i["uv"]], [i["mask"]], [i["intr"]], [i["start"]], loss=i["loss"], **TIGHT)
    r = g["result"][0]
    print(f"{name}: two-start spread {o['spread']:.3g} pinned {o['pinned']}; status {int(r[5])} nfev {int(r[3])} evaluations {int(g['kernel_ms'][1])}")
    assert r[1] <= r[0] and r[5] in (0, 1, 2, 3)      # never worse than the start
    if o["pinned"]:
        ro.check_golden(name, g["extrinsics"][0], r[1], o)


def test_cameras_stop_on_their_own_and_inactive_ones_stay():
    a = ro.camera_of("six", 0)
    sa, sb = ro.perturbed_start(a["ext"], 1), ro.perturbed_start(a["ext"], 2)
    args = lambda n: (a["points"], [a["uv"]] * n, [a["usable"]] * n, [a["intr"]] * n)
    one_a, one_b = refine(*args(1), [sa]), refine(*args(1), [sb])
    both = refine(*args(3), [sa, sb, sa], active=[1, 0, 1])
    assert np.array_equal(both["extrinsics"][0], one_a["extrinsics"][0]) and np.array_equal(both["extrinsics"][2], one_a["extrinsics"][0]) and np.array_equal(both["result"][0], one_a["result"][0])
    assert np.array_equal(both["extrinsics"][1], sb) and np.isnan(both["result"][1]).all()
    # two cameras that need different numbers of evaluations: the one that stops first keeps its row, bit for bit, while the other goes on
    two = refine(*args(2), [sa, sb])
    print(f"nfev {two['result'][:, 3]}")
    for k, one in enumerate((one_a, one_b)):
        assert np.array_equal(two["extrinsics"][k], one["extrinsics"][0]) and np.array_equal(two["result"][k], one["result"][0]) and np.array_equal(two["system"][k], one["system"][0])
    assert two["kernel_ms"][1] >= max(one_a["kernel_ms"][1], one_b["kernel_ms"][1])


# ---------------------------------------------------------------- end to end on the stored optima
def into_gauge(ext, pts, o):
    """extrinsics and points moved, rigidly and by scale, to where camera 0 and the baseline to the scale camera are the stored optimum's"""
    Rg, tg = ks.rodrigues(o["extrinsics"][0][:3]), o["extrinsics"][0][3:]
    R0, t0 = ks.rodrigues(ext[0][:3]), ext[0][3:]
    A, b = Rg.T @ R0, Rg.T @ (t0 - tg)
    cg = -Rg.T @ tg
    Rs = [ks.rodrigues(e[:3]) @ A.T for e in ext]
    cs = [-(R.T @ (e[3:] - R @ b)) for R, e in zip(Rs, ext)]
    s = ko.baseline_of(o["extrinsics"], 0, o["scale_camera"]) / np.linalg.norm(cs[o["scale_camera"]] - cg)
    out = np.array([np.r_[ro.rodrigues_inv(R), -R @ (cg + s * (c - cg))] for R, c in zip(Rs, cs)])
    return out, cg + s * (pts @ A.T + b - cg)


@pytest.mark.parametrize("k", range(6))
def test_a_resected_camera_then_refine_extrinsics_reaches_the_stored_optimum(k):
    i, o = ko.case("six")
    others = [c for c in range(6) if c != k]
    pts = triangulate([i["uvs"][c] for c in others], i["ext0"][others], [i["intr"][c] for c in others])
    tr, inl, info = resect_camera(pts, i["uvs"][k], i["intr"][k], threshold=2.5, return_info=True)
    ext = np.array(i["ext0"])
    ext[k] = tr
    print(f"camera {k}: status {info.status[0]}, inliers {info.n_inliers[0]} of {info.n_usable[0]}, |resected - start| {np.abs(tr - i['ext0'][k]).max():.3g}, polish nfev {info.nfev[0]} status {info.lm_status[0]}")
    assert info.status[0] == 1
    r = refine_extrinsics(i["uvs"], ext, i["intr"], loss=i["loss"], gauge_camera=0, scale_camera=o["scale_camera"], **TIGHT)
    e, p = into_gauge(r.extrinsics, r.points, o)
    ko.check_result(f"six, camera {k} resected", e, p, r.cost, o)


def test_resection_in_the_outlier_scene_agrees_with_a_truth_start():
    uvs, ext, intr, _ = ks.make("outlier")
    ref = refine_extrinsics(uvs, ext, intr, loss="soft_l1", gauge_camera=0, scale_camera=1, **TIGHT)
    k = 3
    others = [c for c in range(6) if c != k]
    pts = triangulate([uvs[c] for c in others], ext[others], [intr[c] for c in others])
    tr, inl, info = resect_camera(pts, uvs[k], intr[k], threshold=2.5, loss="soft_l1", return_info=True)
    start = np.array(ext)
    start[k] = tr
    r = refine_extrinsics(uvs, start, intr, loss="soft_l1", gauge_camera=0, scale_camera=1, **TIGHT)
    err = np.abs(r.extrinsics - ref.extrinsics) / np.maximum(1.0, np.abs(ref.extrinsics))
    print(f"outlier, soft_l1, camera {k}: inliers {info.n_inliers[0]} of {info.n_usable[0]}; cost {r.cost:.12g} (truth start {ref.cost:.12g}); extrinsics {err.max():.3g} (bar 1e-6)")
    assert info.status[0] == 1 and err.max() <= 1e-6
