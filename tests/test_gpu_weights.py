"""Per-detection weights on the GPU: the keyword `weights=` of refine_triangulation and triangulate(refine=True) -- the
weighted instantiation of k_tri_refine through mcba_triangulate_refine_weighted -- against tests/weights_oracle.py, within the gate of
tests/test_gpu_keypoints.py (5e-6 mm); the identities that need no oracle; the refusals.  The covariance and the extrinsics refinement are in
tests/test_gpu_weights_tricov.py and tests/test_gpu_weights_kpba.py.

Cameras 2 (levels 1/4, 1, 4, nothing unseen), 6 and 16 (48 virtual cameras); 1, 255, 256, 257 points (around a workgroup); all five losses at 6
cameras; weights off the levels (uniform in [0.1, 3]) against the direct statement.  Every case has at least half of its points usable under the
oracle (weights_oracle asserts it)."""
import numpy as np
import pytest

import multicam_calibration_amd as m
import weights_oracle as wo

pytestmark = pytest.mark.gpu
GATE_MM = 5e-6   # tests/test_gpu_keypoints.py


def test_unknown_keyword_today():
    """the keyword exists on all five functions (a TypeError before this feature) and None is the unweighted call, bit for bit"""
    i, o = wo.refine_case("c6_p255")
    plain = m.refine_triangulation(i["start"], i["uvs"], i["ext"], i["intr"], loss=i["loss"])
    assert np.array_equal(m.refine_triangulation(i["start"], i["uvs"], i["ext"], i["intr"], loss=i["loss"], weights=None), plain, equal_nan=True)
    assert np.array_equal(m.triangulate(i["uvs"], i["ext"], i["intr"], refine=True, weights=None), m.triangulate(i["uvs"], i["ext"], i["intr"], refine=True), equal_nan=True)
    u = m.triangulation_uncertainty(plain, i["uvs"], i["ext"], i["intr"], weights=None)
    assert np.array_equal(u.covariance, m.triangulation_uncertainty(plain, i["uvs"], i["ext"], i["intr"]).covariance, equal_nan=True)
    s, _ = wo.system_case("c2_p70")
    kw = dict(points=s["pts0"], held=s["held"], lam=s["lam"], loss=s["loss"])
    assert np.array_equal(m.geometry.refine_extrinsics_system(s["uvs"], s["ext0"], s["intr"], weights=None, **kw)["system"], m.geometry.refine_extrinsics_system(s["uvs"], s["ext0"], s["intr"], **kw)["system"])
    r = m.refine_extrinsics(s["uvs"], s["ext0"], s["intr"], points=s["pts0"], loss="linear", weights=None, max_nfev=3)
    assert r.cost == m.refine_extrinsics(s["uvs"], s["ext0"], s["intr"], points=s["pts0"], loss="linear", max_nfev=3).cost


@pytest.mark.parametrize("name", list(wo.REFINE_CASES))
def test_refinement_reaches_the_oracle_minimiser(name):
    i, o = wo.refine_case(name)
    got, info = m.refine_triangulation(i["start"], i["uvs"], i["ext"], i["intr"], loss=i["loss"], f_scale=i["f_scale"], weights=i["weights"], return_info=True)
    ok = o["usable"]
    assert ok.mean() >= 0.5
    assert np.array_equal(np.isnan(got).any(1), ~ok) and np.all(info["status"][~ok] == -1) and np.all(info["status"][ok] == 1)
    diff = np.abs(got - o["points"])[ok].max()
    print(f"{name}: usable {ok.sum()} / {len(ok)}  max |dX| {diff:.3e} mm (gate {GATE_MM}), iterations max {info['n_iterations'].max()}")
    assert diff <= GATE_MM
    np.testing.assert_allclose(info["cost"][ok], wo.robust_cost_direct(got, i["uvs"], i["ext"], i["intr"], i["weights"], i["loss"], i["f_scale"])[ok], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(info["cost0"][ok], wo.robust_cost_direct(i["start"], i["uvs"], i["ext"], i["intr"], i["weights"], i["loss"], i["f_scale"])[ok], rtol=1e-9, atol=1e-12)
    assert np.all(info["cost"][ok] <= info["cost0"][ok])
    again = m.refine_triangulation(got, i["uvs"], i["ext"], i["intr"], loss=i["loss"], f_scale=i["f_scale"], weights=i["weights"])
    assert np.abs(again - got)[ok].max() < GATE_MM
    assert np.array_equal(m.refine_triangulation(i["start"], i["uvs"], i["ext"], i["intr"], loss=i["loss"], f_scale=i["f_scale"], weights=i["weights"]), got, equal_nan=True)   # the same bits


@pytest.mark.parametrize("name", ["c2_p257", "c6_p256", "c16_p33", "direct_c6_p65"])
def test_triangulate_refine_is_the_two_calls_back_to_back(name):
    """the median of pairs is unweighted and skips the detections of weight 0 / NaN; the refinement is the weighted one"""
    i, o = wo.refine_case(name)
    w = i["weights"].copy()
    w[0, 0] = np.nan   # a NaN weight: unseen
    base = m.triangulate(wo.masked(i["uvs"], w), i["ext"], i["intr"])
    one = m.triangulate(i["uvs"], i["ext"], i["intr"], refine=True, loss=i["loss"], f_scale=i["f_scale"], weights=w)
    two = m.refine_triangulation(base, i["uvs"], i["ext"], i["intr"], loss=i["loss"], f_scale=i["f_scale"], weights=w)
    assert np.array_equal(one, two, equal_nan=True)
    ok = ~np.isnan(two).any(1)
    ok[0] = False   # (point 0 lost a detection against the oracle's weights)
    assert ok.mean() >= 0.5 and np.abs(one - o["points"])[ok].max() <= GATE_MM


@pytest.mark.parametrize("loss", ["linear", "soft_l1"])
def test_identities(loss):
    i, o = wo.refine_case("c6_p257_" + loss)
    kw = dict(loss=loss, f_scale=i["f_scale"], return_info=True)
    plain, pinfo = m.refine_triangulation(i["start"], i["uvs"], i["ext"], i["intr"], **kw)
    ones, oinfo = m.refine_triangulation(i["start"], i["uvs"], i["ext"], i["intr"], weights=np.ones_like(i["weights"]), **kw)
    # all-ones weights: the unweighted problem (a multiplication by 1.0 is exact: the same bits)
    assert np.array_equal(ones, plain, equal_nan=True) and np.array_equal(oinfo["cost"], pinfo["cost"], equal_nan=True)
    # a 0/1 plane: the same mask written as NaN
    mask = i["weights"] > 0
    a = m.refine_triangulation(i["start"], i["uvs"], i["ext"], i["intr"], weights=mask.astype(np.float64), **kw)
    b = m.refine_triangulation(i["start"], wo.masked(i["uvs"], mask), i["ext"], i["intr"], **kw)
    assert np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1]["cost"], b[1]["cost"], equal_nan=True) and np.array_equal(a[1]["status"], b[1]["status"])
    if loss == "linear":   # a constant plane under the linear loss: the same points, the cost times w0
        c, cinfo = m.refine_triangulation(i["start"], i["uvs"], i["ext"], i["intr"], weights=np.full_like(i["weights"], 4.0), **kw)
        ok = ~np.isnan(plain).any(1)
        assert np.abs(c - plain)[ok].max() <= GATE_MM
        np.testing.assert_allclose(cinfo["cost"][ok], 4.0 * pinfo["cost"][ok], rtol=1e-9)


def test_refusals_say_why():
    i, o = wo.refine_case("c6_p255")
    w = i["weights"]
    args = (i["start"], i["uvs"], i["ext"], i["intr"])
    for bad, why in ((w[:, :-1], "weights must be"), (-w - 1, "not negative"), (np.where(w > 0, np.inf, w), "finite")):
        with pytest.raises(ValueError, match=why):
            m.refine_triangulation(*args, weights=bad)
        with pytest.raises(ValueError, match=why):
            m.triangulate(*args[1:], refine=True, weights=bad)
        with pytest.raises(ValueError, match=why):
            m.triangulation_uncertainty(*args, weights=bad)
        with pytest.raises(ValueError, match=why):
            m.refine_extrinsics(*args[1:], points=i["start"], weights=bad)
        with pytest.raises(ValueError, match=why):
            m.geometry.refine_extrinsics_system(*args[1:], points=i["start"], held=np.zeros(6, np.int32), lam=0.0, weights=bad)
    with pytest.raises(ValueError, match="refine=True"):
        m.triangulate(*args[1:], weights=w)
    with pytest.raises(ValueError, match="refine=True"):
        m.triangulate(*args[1:], refine=False, weights=w)
    # the C ABI refuses the same values
    lib, ops = m.ops.load_library(), m.ops
    uv = np.ascontiguousarray(np.stack(i["uvs"]))
    cam, dist = m.triangulation._cam_blocks(i["ext"], i["intr"])
    out, neg = np.empty((255, 3)), np.ascontiguousarray(-np.ones_like(w))
    rc = lib.mcba_triangulate_refine_weighted(6, 255, uv.ctypes.data, neg.ctypes.data, cam.ctypes.data, dist.ctypes.data, np.ascontiguousarray(i["start"]).ctypes.data, 0, 0, 1.0, 10, 0,
                                              out.ctypes.data, None, None)
    assert rc == ops.ERR_ARG
