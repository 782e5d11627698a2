"""The geometry module without a GPU: its host functions against the reference's outputs (tests/golden/geometry.npz), the package's exports, the
argument checks, the empty input, and the loud error where no device is visible."""
import ctypes

import numpy as np
import pytest

import multicam_calibration_amd as m
from multicam_calibration_amd import geometry, ops

import keypoint_scenes as ks

NAMES = ["project_points", "project_to_cameras", "apply_rigid_transform", "keypoint_reprojection_errors", "refine_triangulation", "rigid_transform_from_correspondences", "rodrigues",
         "rodrigues_inv", "get_transformation_matrix", "get_transformation_vector", "get_projection_matrix", "euclidean_to_homogenous", "homogeneous_to_euclidean"]


@pytest.fixture(scope="module")
def gold(golden):
    return golden("geometry.npz")


def no_gpu():
    n = ctypes.c_int()
    return not (ops.load_library().mcba_device_count(ctypes.byref(n)) == 0 and n.value > 0)


def test_the_package_exports_the_reference_namespace():
    for name in NAMES:
        assert getattr(m, name) is getattr(geometry, name) and name in m.__all__, name
    assert m.geometry is geometry
    from multicam_calibration_amd import calibration

    assert geometry.rodrigues is calibration.rodrigues and geometry.get_transformation_vector is calibration.get_transformation_vector


def test_host_helpers_match_the_reference(gold):
    K, ext = gold["pp_K"], gold["pp_ext"]
    np.testing.assert_allclose(m.get_projection_matrix(ext, (K, gold["pp_d5"])), gold["projection_matrix"], rtol=1e-12)
    np.testing.assert_allclose(m.rodrigues(gold["rod_r"]), gold["rod_R"], rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(m.rodrigues_inv(gold["rod_R"]), gold["rod_inv"], rtol=1e-12, atol=1e-300)
    hom = m.euclidean_to_homogenous(gold["pp_grid"])
    assert hom.shape == (5, 4, 4) and np.array_equal(hom, gold["hom"], equal_nan=True)
    np.testing.assert_allclose(m.homogeneous_to_euclidean(gold["hom_in"]), gold["hom_back"], rtol=1e-12)
    np.testing.assert_allclose(m.get_transformation_vector(gold["rt_T4"]), [0.9, -0.2, 0.3, -5.0, 8.0, 2.0], rtol=1e-12)


def test_rigid_transform_from_correspondences_matches_the_reference(gold):
    for case in ("kabsch", "reflect"):
        t, rmsd = m.rigid_transform_from_correspondences(gold[f"{case}_src"], gold[f"{case}_tgt"])
        np.testing.assert_allclose(t, gold[f"{case}_t"], rtol=1e-12, atol=1e-13)
        np.testing.assert_allclose(rmsd, gold[f"{case}_rmsd"], rtol=1e-12)
    # the reflection case really is one: without the flip the best orthogonal map has determinant -1
    s, g = gold["reflect_src"], gold["reflect_tgt"]
    U, _, Vt = np.linalg.svd((s - s.mean(0)).T @ (g - g.mean(0)))
    assert np.linalg.det(Vt.T @ U.T) < 0
    # (leading shapes are flattened, as in the reference)
    t2, _ = m.rigid_transform_from_correspondences(gold["kabsch_src"].reshape(5, 6, 3), gold["kabsch_tgt"].reshape(5, 6, 3))
    np.testing.assert_array_equal(t2, m.rigid_transform_from_correspondences(gold["kabsch_src"], gold["kabsch_tgt"])[0])
    # the one in flatibration.py keeps returning the vector alone
    from multicam_calibration_amd import flatibration

    assert np.shape(flatibration.rigid_transform_from_correspondences(gold["kabsch_src"], gold["kabsch_tgt"])) == (6,)


def test_empty_input_does_not_need_a_device(gold):
    K, ext = gold["pp_K"], gold["pp_ext"]
    intr = [(K, gold["pp_d5"])] * 3
    exts = [ext] * 3
    assert m.project_points(np.zeros((0, 3)), ext, K).shape == (0, 2)
    assert m.project_points(np.zeros((4, 0, 3)), ext, K, gold["pp_d2"]).shape == (4, 0, 2)
    assert m.project_to_cameras(np.zeros((0, 3)), exts, intr, distortion="opencv5").shape == (3, 0, 2)
    assert m.apply_rigid_transform(np.zeros(6), np.zeros((0, 3))).shape == (0, 3)
    err, med = m.keypoint_reprojection_errors(np.zeros((0, 3)), [np.zeros((0, 2))] * 3, exts, intr)
    assert err.shape == (3, 0) and med.shape == (3,) and np.isnan(med).all()
    pts, info = m.refine_triangulation(np.zeros((0, 3)), [np.zeros((0, 2))] * 3, exts, intr, return_info=True)
    assert pts.shape == (0, 3) and set(info) == {"cost", "cost0", "n_iterations", "status"} and all(v.shape == (0,) for v in info.values())


def test_argument_errors(gold):
    K, ext, d5 = gold["pp_K"], gold["pp_ext"], gold["pp_d5"]
    pts = np.ones((4, 3))
    uvs2 = [np.ones((4, 2))] * 2
    exts2, intr2 = [ext] * 2, [(K, d5)] * 2
    with pytest.raises(ValueError):
        m.project_points(np.ones((4, 2)), ext, K)
    with pytest.raises(ValueError):
        m.project_to_cameras(pts, exts2, intr2, distortion="fisheye")
    with pytest.raises(ValueError):
        m.apply_rigid_transform(np.zeros(7), pts)
    with pytest.raises(ValueError):
        m.keypoint_reprojection_errors(np.ones((5, 3)), uvs2, exts2, intr2)          # points and detections disagree
    with pytest.raises(ValueError):
        m.refine_triangulation(pts, uvs2, exts2, intr2, loss="tukey")
    with pytest.raises(ValueError):
        m.refine_triangulation(pts, uvs2, exts2, intr2, f_scale=0.0)
    with pytest.raises(ValueError):
        m.triangulate(uvs2, exts2, intr2, refine=True, loss="tukey")
    with pytest.raises(NotImplementedError):
        m.refine_triangulation(pts, [np.ones((4, 2))], [ext], [(K, d5)])              # one camera
    with pytest.raises(NotImplementedError):
        m.refine_triangulation(pts, [np.ones((4, 2))] * 65, [ext] * 65, [(K, d5)] * 65)
    skew = K.copy()
    skew[0, 1] = 0.3
    with pytest.raises(NotImplementedError):
        m.project_points(pts, ext, skew)
    with pytest.raises(NotImplementedError):
        m.project_to_cameras(pts, exts2, [(K, np.r_[d5, 0.0, 0.0, 1e-3])] * 2)
    # the C entry points check their arguments before any device call
    lib = ops.load_library()
    z = np.zeros(64)
    assert lib.mcba_project_points(0, 4, z.ctypes.data, z.ctypes.data, None, 0, z.ctypes.data, None) == ops.ERR_ARG
    assert lib.mcba_rigid_transform(4, None, z.ctypes.data, 0, z.ctypes.data) == ops.ERR_ARG
    assert lib.mcba_keypoint_errors(2, 4, z.ctypes.data, z.ctypes.data, z.ctypes.data, None, 0, None, None, None) == ops.ERR_ARG
    for C, loss, fs in ((1, 0, 1.0), (65, 0, 1.0), (2, 5, 1.0), (2, 0, 0.0)):
        assert lib.mcba_triangulate_refine(C, 4, z.ctypes.data, z.ctypes.data, None, None, 5, loss, fs, 10, 0, z.ctypes.data, None, None) == ops.ERR_ARG


def test_without_a_gpu_every_device_function_raises(gold):
    if not no_gpu():
        pytest.skip("a GPU is visible here")
    uvs, ext, intr, _ = ks.make("three")
    start = gold["three_start"]
    calls = [lambda: m.project_points(start, ext[0], intr[0][0], intr[0][1]), lambda: m.project_to_cameras(start, ext, intr), lambda: m.apply_rigid_transform(ext[1], start),
             lambda: m.keypoint_reprojection_errors(start, uvs, ext, intr), lambda: m.keypoint_reprojection_errors(start, uvs, ext, intr, arrays=False),
             lambda: m.refine_triangulation(start, uvs, ext, intr), lambda: m.triangulate(uvs, ext, intr, refine=True)]
    for call in calls:
        with pytest.raises(ops.McbaError):
            call()
