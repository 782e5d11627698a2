"""The keypoint kernels on the GPU (csrc/mcba_keypoints.hip): project_points / project_to_cameras / apply_rigid_transform against the reference's
outputs (tests/golden/geometry.npz), launch boundaries against numpy restatements, keypoint_reprojection_errors with its exact medians, and the
per-point refinement against the scipy optimum recorded by tests/golden/make_golden_geometry.py plus properties that need no oracle.

Refinement gate: max |dX| <= 5e-6 mm per point -- ten times the 5e-7 mm the golden script enforces on the oracle's own spread between starts,
because the stored optimum is only that good (3-point finite differences) while the kernel's Jacobian is analytic.  Measured on MI355X (this
file, -s): see DESIGN.md section 8f-8."""
import warnings

import numpy as np
import pytest

import multicam_calibration_amd as m

import keypoint_scenes as ks
from test_triangulate_cpu import scene

pytestmark = pytest.mark.gpu
GATE_MM = 5e-6


@pytest.fixture(scope="module")
def gold(golden):
    return golden("geometry.npz")


def rig(C, seed):
    """C cameras looking at a cloud near the origin, five-coefficient distortion with non-zero p1, p2, k3."""
    rng = np.random.default_rng(seed)
    ext = np.c_[rng.normal(0, 0.25, (C, 3)), rng.normal(0, 40, (C, 2)), rng.uniform(800, 1200, C)]
    intr = []
    for c in range(C):
        K = np.array([[rng.uniform(900, 1300), 0, rng.uniform(600, 700)], [0, rng.uniform(900, 1300), rng.uniform(450, 550)], [0, 0, 1.0]])
        intr.append((K, np.array([rng.normal(0, 0.08), rng.normal(0, 0.03), rng.normal(0, 1.5e-3), rng.normal(0, 1.5e-3), rng.normal(0, 0.01)])))
    return ext, intr


def cloud(P, seed):
    return np.random.default_rng(seed).normal(0, 70, (P, 3))


def project_ref(X, ext, K, d2):
    """The reference's project_points restated (k1, k2 only)."""
    return ks.project5(X, ext, K, np.r_[d2[:2], 0, 0, 0])


# ---------------------------------------------------------------- against the reference's outputs
def test_project_points_matches_the_reference(gold):
    K, ext = gold["pp_K"], gold["pp_ext"]
    cases = [(gold["pp_pts"], ext, None, "pp_plain"), (gold["pp_pts"], ext, gold["pp_d2"], "pp_dist2"), (gold["pp_pts"], ext, gold["pp_d5"], "pp_dist5"),
             (gold["pp_grid"], ext, gold["pp_d2"], "pp_grid_dist2"), (gold["pp_pts"] + np.array([0, 0, 800.0]), np.zeros(6), gold["pp_d2"], "pp_zero_ext")]
    for pts, e, d, key in cases:
        got = m.project_points(pts, e, K, d)
        assert got.shape == gold[key].shape and np.array_equal(np.isnan(got), np.isnan(gold[key])), key
        np.testing.assert_allclose(got, gold[key], rtol=1e-12, atol=1e-10, err_msg=key)


def test_project_to_cameras_is_project_points_per_camera(gold):
    ext, intr = rig(7, 3)
    pts = gold["pp_grid"]
    both = m.project_to_cameras(pts, ext, intr)
    assert both.shape == (7, 5, 4, 2)
    for c in range(7):
        assert np.array_equal(both[c], m.project_points(pts, ext[c], intr[c][0], intr[c][1]), equal_nan=True)
    five = m.project_to_cameras(pts, ext, intr, distortion="opencv5")
    for c in range(7):
        np.testing.assert_allclose(five[c], ks.project5(pts, ext[c], *intr[c]), rtol=1e-12, atol=1e-10)
    # with p1 = p2 = k3 = 0 the five-coefficient model is project_points'
    intr2 = [(K, np.r_[d[:2], 0, 0, 0]) for K, d in intr]
    np.testing.assert_allclose(m.project_to_cameras(pts, ext, intr2, distortion="opencv5"), m.project_to_cameras(pts, ext, intr2), rtol=1e-12, atol=1e-10)


def test_apply_rigid_transform_matches_the_reference(gold):
    got = m.apply_rigid_transform(gold["rt_t6"], gold["pp_pts"])
    assert np.array_equal(np.isnan(got), np.isnan(gold["rt_vec"]))
    np.testing.assert_allclose(got, gold["rt_vec"], rtol=1e-12, atol=1e-10)
    got = m.apply_rigid_transform(gold["rt_T4"], gold["pp_grid"])
    assert got.shape == (5, 4, 3) and np.array_equal(np.isnan(got), np.isnan(gold["rt_mat"]))
    np.testing.assert_allclose(got, gold["rt_mat"], rtol=1e-12, atol=1e-10)


# ---------------------------------------------------------------- launch boundaries
P_EDGES = [1, 63, 64, 65, 255, 256, 257, 100003]
C_EDGES = [1, 2, 8, 9, 40, 41, 64, 65, 130]


def edge_pairs(cs, seed):
    """A seeded selection of (P, C) pairs that covers every P and every C at least once (not the full product).  The 100 003-point case goes with
    at most 41 cameras -- beyond, it is a long copy, not another boundary --; a camera count it was drawn with gets 257 points instead."""
    rng = np.random.default_rng(seed)
    n = max(len(P_EDGES), len(cs))
    ps = list(rng.permutation(P_EDGES)) + list(rng.choice(P_EDGES[:-1], n - len(P_EDGES)))
    cc = list(rng.permutation(cs)) + list(rng.choice(cs, n - len(cs)))
    pairs = []
    for p, c in zip(ps, cc):
        if p == 100003 and c > 41:
            pairs += [(100003, int(min(cs[1], 9))), (257, int(c))]
        else:
            pairs.append((int(p), int(c)))
    return pairs


@pytest.mark.parametrize("P,C", edge_pairs(C_EDGES, 5) + [(257, 130), (65, 65)])
def test_projection_and_errors_at_launch_boundaries(P, C):
    ext, intr = rig(C, 100 + C)
    X = cloud(P, P)
    X[P // 2] = np.nan
    got = m.project_to_cameras(X, ext, intr, distortion="opencv5")
    want = np.stack([ks.project5(X, ext[c], *intr[c]) for c in range(C)])
    assert np.array_equal(np.isnan(got), np.isnan(want))
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-10)
    got2 = m.project_to_cameras(X, ext, intr)
    np.testing.assert_allclose(got2, np.stack([project_ref(X, ext[c], *intr[c]) for c in range(C)]), rtol=1e-12, atol=1e-10)
    rng = np.random.default_rng(P + C)
    uvs = want + rng.normal(0, 0.7, want.shape)
    uvs[rng.uniform(size=(C, P)) < 0.2] = np.nan
    if C > 2:
        uvs[C - 2] = np.nan                                            # a camera that sees nothing
    err, med = m.keypoint_reprojection_errors(X, list(uvs), ext, intr)
    werr = ks.errors(X, list(uvs), ext, intr)
    assert np.array_equal(np.isnan(err), np.isnan(werr))
    np.testing.assert_allclose(err, werr, rtol=0, atol=1e-10)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                # (numpy warns about the all-NaN row)
        wmed = np.nanmedian(err, axis=1)
    assert np.array_equal(med, wmed, equal_nan=True)
    if C > 2:
        assert np.isnan(med[C - 2])
    _, med2 = m.keypoint_reprojection_errors(X, list(uvs), ext, intr, arrays=False)
    assert _ is None and np.array_equal(med2, med, equal_nan=True)


@pytest.mark.parametrize("P,C", edge_pairs([2, 8, 9, 64], 9))
def test_refinement_at_launch_boundaries(P, C):
    ext, intr = rig(C, 200 + C)
    X = cloud(P, 7 * P + 1)
    rng = np.random.default_rng(P * 131 + C)
    uvs = np.stack([ks.project5(X, ext[c], *intr[c]) for c in range(C)]) + rng.normal(0, 0.4, (C, P, 2))
    uvs[rng.uniform(size=(C, P)) < (0.5 if C > 8 else 0.15)] = np.nan
    start = X + rng.normal(0, 0.3, X.shape)
    got, info = m.refine_triangulation(start, list(uvs), ext, intr, loss="soft_l1", return_info=True)
    views = (~np.isnan(uvs).any(-1)).sum(0)
    ok = views >= 2
    assert np.array_equal(np.isnan(got).any(1), ~ok) and np.all(info["status"][~ok] == -1) and np.all(info["status"][ok] == 1)
    assert np.all(info["cost"][ok] <= info["cost0"][ok])
    np.testing.assert_allclose(info["cost"][ok], ks.robust_cost(got, list(uvs), ext, intr, "soft_l1")[ok], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(info["cost0"][ok], ks.robust_cost(start, list(uvs), ext, intr, "soft_l1")[ok], rtol=1e-9, atol=1e-12)
    # a stationary point of the numpy cost: central differences of it vanish to their own accuracy
    idx = np.flatnonzero(ok)[:64]
    h = 1e-4
    for k in range(3):
        e = np.zeros(3)
        e[k] = h
        g = (ks.robust_cost(got + e, list(uvs), ext, intr, "soft_l1") - ks.robust_cost(got - e, list(uvs), ext, intr, "soft_l1"))[idx] / (2 * h)
        assert np.abs(g).max() < 1e-6, (k, np.abs(g).max())
    again = m.refine_triangulation(got, list(uvs), ext, intr, loss="soft_l1")
    assert not ok.any() or np.abs(again - got)[ok].max() < GATE_MM


# ---------------------------------------------------------------- errors on the golden scenes
@pytest.mark.parametrize("name", list(ks.SCENES))
def test_keypoint_errors_on_the_golden_scenes(gold, name):
    uvs, ext, intr, _ = ks.make(name)
    start = gold[f"{name}_start"]
    err, med = m.keypoint_reprojection_errors(start, uvs, ext, intr)
    want = ks.errors(start, uvs, ext, intr)
    assert np.array_equal(np.isnan(err), np.isnan(want))
    np.testing.assert_allclose(err, want, rtol=0, atol=1e-10)
    assert np.array_equal(med, np.nanmedian(err, axis=1))
    err2, med2 = m.keypoint_reprojection_errors(start, uvs, ext, intr, arrays=False)
    assert err2 is None and np.array_equal(med2, med)


# ---------------------------------------------------------------- refinement against the scipy optimum
@pytest.mark.parametrize("name,loss", [(n, l) for n in ks.SCENES for l in ks.LOSSES[n]])
def test_refinement_reaches_the_scipy_optimum(gold, name, loss):
    uvs, ext, intr, X = ks.make(name)
    start, want = gold[f"{name}_start"], gold[f"{name}_{loss}"]
    got, info = m.refine_triangulation(start, uvs, ext, intr, loss=loss, return_info=True)
    views = (~np.isnan(np.stack(uvs)).any(-1)).sum(0)
    ok = views >= 2
    assert np.array_equal(np.isnan(got).any(1), np.isnan(start).any(1)) and np.array_equal(np.isnan(got).any(1), ~ok)
    assert not np.isnan(want[ok]).any()                               # every point with two views has an optimum on record: none is left out
    diff = np.abs(got - want)[ok].max(axis=1)
    print(f"{name} {loss}: max |dX| {diff.max():.3e} mm (oracle's own spread {float(gold[f'{name}_{loss}_spread']):.1e}), iterations mean {info['n_iterations'][ok].mean():.1f} max {info['n_iterations'].max()}")
    assert diff.max() <= GATE_MM
    assert np.all(info["cost"][ok] <= info["cost0"][ok]) and np.all(info["status"][ok] == 1)
    again = m.refine_triangulation(got, uvs, ext, intr, loss=loss)
    assert np.abs(again - got)[ok].max() < GATE_MM


@pytest.mark.parametrize("name", list(ks.SCENES))
def test_every_loss_never_makes_a_point_worse(gold, name):
    uvs, ext, intr, _ = ks.make(name)
    start = gold[f"{name}_start"]
    ok = ~np.isnan(start).any(1)
    for loss in ("linear", "soft_l1", "huber", "cauchy", "arctan"):
        for f_scale in (1.0, 2.5):
            got, info = m.refine_triangulation(start, uvs, ext, intr, loss=loss, f_scale=f_scale, return_info=True)
            assert np.all(info["cost"][ok] <= info["cost0"][ok]), (loss, f_scale)
            np.testing.assert_allclose(info["cost"][ok], ks.robust_cost(got, uvs, ext, intr, loss, f_scale)[ok], rtol=1e-9, atol=1e-12)
            again = m.refine_triangulation(got, uvs, ext, intr, loss=loss, f_scale=f_scale)
            assert np.abs(again - got)[ok].max() < GATE_MM, (loss, f_scale)


def test_soft_l1_ends_nearer_the_truth_than_the_start_on_the_outlier_scene(gold):
    uvs, ext, intr, X = ks.make("outlier")
    start = gold["outlier_start"]
    got = m.refine_triangulation(start, uvs, ext, intr, loss="soft_l1")
    ok = ~np.isnan(start).any(1)

    def rms(A):
        return np.sqrt(np.mean(np.sum((A[ok] - X[ok]) ** 2, axis=1)))

    print(f"rms to truth: start {rms(start):.4f} soft_l1 {rms(got):.4f} mm")
    assert rms(got) < rms(start)


def test_noise_free_points_are_recovered():
    uvs, ext, intr, X = scene(C=5, P=777, seed=21)
    start = m.triangulate(uvs, ext, intr)                              # five undistortion rounds: good to 1e-6 only
    got = m.refine_triangulation(start, uvs, ext, intr, loss="linear")
    assert np.abs(got - X).max() < 1e-8
    # the same cloud through five-coefficient cameras (non-zero p1, p2, k3), detections made by the numpy forward model
    intr5 = [(K, np.r_[d[:2], 1.5e-3 * (-1) ** c, -8e-4, 0.015]) for c, (K, d) in enumerate(intr)]
    uvs5 = [ks.project5(X, ext[c], *intr5[c]) for c in range(len(ext))]
    start5 = m.triangulate(uvs5, ext, intr5)
    for loss in ("linear", "soft_l1"):
        got = m.refine_triangulation(start5, uvs5, ext, intr5, loss=loss)
        assert np.abs(got - X).max() < 1e-8, loss


# ---------------------------------------------------------------- triangulate(refine=...)
@pytest.mark.parametrize("name", ["six", "twelve", "outlier"])
def test_triangulate_refine_is_the_two_calls_back_to_back(name):
    uvs, ext, intr, _ = ks.make(name)
    base = m.triangulate(uvs, ext, intr)
    assert np.array_equal(m.triangulate(uvs, ext, intr, refine=False), base, equal_nan=True)
    for loss in ("soft_l1", "linear", "cauchy"):
        one = m.triangulate(uvs, ext, intr, refine=True, loss=loss)
        two = m.refine_triangulation(base, uvs, ext, intr, loss=loss)
        assert np.array_equal(one, two, equal_nan=True), loss
    pts, ms = m.triangulate(uvs, ext, intr, refine=True, return_kernel_ms=True)
    assert ms > 0 and np.array_equal(pts, m.refine_triangulation(base, uvs, ext, intr), equal_nan=True)
