"""The sparse-Schur handle (mcba_create_sparse; ops.Problem(..., schur="sparse")) on an MI355X: rigs of more than 40 cameras.
  * bundle_adjust() at 48 cameras against the reference's own tight optimum (tests/golden/make_golden_wide.py);
  * normal equations and Schur reduction against the oracle at 41 / 64 / 128 cameras;
  * the multi-workgroup blocked solve against LAPACK up to 12 x 256 rows, with a fixed mask, a numeric x_scale, and an indefinite system;
  * the sparse against the dense handle on the same problem (6 / 24 / 40 cameras), edge cases, reproducibility, frame shards."""
import contextlib
import io

import numpy as np
import pytest

from oracle import ba_oracle as orc

pytestmark = pytest.mark.gpu
WIDE_SHAPE = dict(n_cameras=48, n_frames=150, rows=2, cols=3, pitch=60.0, seed=7, perturb_seed=1, missing=0.1, visible_k=8)   # tests/golden/make_golden_wide.py


@pytest.fixture(scope="module")
def mc():
    import multicam_calibration_amd as m

    m.ops.load_library()
    return m


def _wide(mc, C, F, k=8, missing=0.1, seed=11):
    return mc.synth.make_problem(C, F, rows=2, cols=3, pitch=60.0, seed=seed, missing=missing, visible_k=min(k, C))


def _reduced(mc, p, lam, schur, x=None, **kw):
    x = orc.serialize_params(p["extrinsics"], p["intrinsics"], p["poses"]) if x is None else x
    prob = mc.ops.Problem(p["uvs"], p["obj"], schur=schur, **kw)
    prob.set_params(0, x)
    prob.linearize(0)
    prob.build_reduced(lam)
    red = {k: v.copy() for k, v in prob.get_reduced().items()}
    return prob, red


def _quiet(fn, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **kw)


# ------------------------------------------------------------------ bundle_adjust above 40 cameras: the reference's optimum
def test_bundle_adjust_48_cameras_matches_reference_golden(mc, golden):
    z = golden("wide_48x150.npz")
    p = mc.synth.make_problem(**WIDE_SHAPE)
    assert abs(float(z["uvs_checksum"]) - np.nansum(p["uvs"])) <= 1e-12 * abs(float(z["uvs_checksum"]))
    C = WIDE_SHAPE["n_cameras"]
    ext, intr, poses, use, res = _quiet(mc.bundle_adjust, p["uvs"], p["extrinsics"], p["intrinsics"], p["obj"], p["poses"], n_frames=None, outlier_threshold=1e30,
                                        ftol=1e-14, xtol=1e-14, gtol=1e-14, max_nfev=300)
    assert res.lm["reduced_solver"] == "device"
    assert np.array_equal(use, z["use"])
    cost_g = float(z["cost"])
    assert abs(res.cost - cost_g) <= 1e-10 * cost_g, (res.cost, cost_g)
    # intrinsics are gauge invariant; extrinsics and poses after moving the world frame onto the golden's camera 0
    cam, cam_g = res.x[:12 * C].reshape(C, 12), z["x"][:12 * C].reshape(C, 12)
    assert (np.abs(cam[:, :6] - cam_g[:, :6]) / np.abs(cam_g[:, :6])).max() < 1e-6
    ext_g, _, poses_g = orc.deserialize_params(z["x"], C)
    ext_a, poses_a = orc.gauge_align(ext, poses, ext_g[0])
    assert np.abs(ext_a - ext_g).max() < 1e-6 * np.abs(ext_g).max()
    Ta, Tg = orc.to_matrix(poses_a), orc.to_matrix(poses_g)
    assert np.abs(Ta - Tg)[..., :3, :3].max() < 1e-6
    assert np.abs(Ta - Tg)[..., :3, 3].max() < 1e-6 * np.abs(Tg[..., :3, 3]).max()


# ------------------------------------------------------------------ normal equations + Schur reduction against the oracle
@pytest.mark.parametrize("C", [41, 64, 128])
def test_schur_reduction_vs_oracle(mc, C):
    p = _wide(mc, C, 3 * C // 2 + 7)
    F = p["uvs"].shape[1]
    x = orc.serialize_params(p["extrinsics"], p["intrinsics"], p["poses"])
    lam = 1e-2
    prob, red = _reduced(mc, p, lam, "sparse", x)
    assert prob.is_sparse
    U, gc, V, gf, W, cost = orc.normal_equations(x, p["uvs"], p["obj"])
    Df2 = np.stack([np.where(np.diag(V[f]) > 0, np.diag(V[f]), 1.0) for f in range(F)])
    S, rhs = orc.schur_reduce(U, gc, V, gf, W, lam, np.zeros((C, 12)), Df2)
    assert np.abs(red["S0"] - S).max() <= 1e-10 * np.abs(S).max()
    assert np.abs(red["rhs"] - rhs).max() <= 1e-10 * np.abs(rhs).max()
    assert abs(red["scal"][0] - cost) <= 1e-12 * cost
    assert np.abs(prob.frame_gradient() - gf).max() <= 1e-10 * np.abs(gf).max()
    prob.close()


# ------------------------------------------------------------------ the blocked solve against LAPACK
def _device_solve(prob, red, lam, fixed=None):
    prob.lm_set_state(float(red["scal"][0]), lam, 2.0, 0)
    prob.lm_auto_config(0.0, 0.0, 0.0, 1e-12, 1e12, fixed)
    prob.lm_auto_solve(1)
    return prob.lm_auto_wait(1), prob.cam_step()


@pytest.mark.parametrize("C", [41, 64, 128, 256])
def test_blocked_solve_vs_lapack(mc, C):
    p = _wide(mc, C, max(60, C // 2), k=6, missing=0.0)
    lam = 1e-3
    prob, red = _reduced(mc, p, lam, "sparse")
    n = 12 * C
    st, dc = _device_solve(prob, red, lam)
    assert st[23] == 0 and st[14] == 0                                     # solve info ok, no rebuild
    D = np.where(red["diagU"] > 0, red["diagU"], 1.0)
    Sd = red["S0"] + lam * np.diag(D)
    Lc = np.linalg.cholesky(Sd)
    ref = np.linalg.solve(Sd, red["rhs"])
    r = Sd @ dc - red["rhs"]
    assert np.abs(r).max() <= 1e-11 * (np.abs(Sd).max() * np.abs(dc).max() + np.abs(red["rhs"]).max())
    assert np.abs(dc - ref).max() <= 1e-7 * np.abs(ref).max()
    assert np.isfinite(Lc).all() and dc.shape == (n,)
    assert abs(st[12] - dc @ dc) <= 1e-12 * (dc @ dc)                       # |d_c|^2 in the state
    assert abs(st[11] - dc @ (lam * D * dc - red["gc"])) <= 1e-9 * abs(st[11])
    prob.close()


def test_blocked_solve_fixed_mask_and_x_scale(mc):
    C = 48
    p = _wide(mc, C, 80, k=6)
    lam = 1e-2
    n = 12 * C
    rng = np.random.default_rng(3)
    fixed = np.zeros(n, bool)
    fixed[rng.choice(n, 40, replace=False)] = True
    fixed[:12] = True
    prob, red = _reduced(mc, p, lam, "sparse")
    st, dc = _device_solve(prob, red, lam, fixed=fixed)
    assert st[23] == 0
    D = np.where(red["diagU"] > 0, red["diagU"], 1.0)
    free = ~fixed
    Sd = (red["S0"] + lam * np.diag(D))[np.ix_(free, free)]
    ref = np.linalg.solve(Sd, red["rhs"][free])
    assert np.all(dc[fixed] == 0.0)
    assert np.abs(dc[free] - ref).max() <= 1e-7 * np.abs(ref).max()
    prob.close()
    # numeric x_scale: D_c = 1 / x_scale^2 instead of diag(U)
    F = p["uvs"].shape[1]
    xs = np.exp(rng.normal(0.0, 0.5, 12 * C + 6 * F))
    x = orc.serialize_params(p["extrinsics"], p["intrinsics"], p["poses"])
    prob = mc.ops.Problem(p["uvs"], p["obj"], schur="sparse")
    prob.set_x_scale(xs)
    prob.set_params(0, x)
    prob.linearize(0)
    prob.build_reduced(lam)
    red = {k: v.copy() for k, v in prob.get_reduced().items()}
    st, dc = _device_solve(prob, red, lam)
    assert st[23] == 0
    Sd = red["S0"] + lam * np.diag(1.0 / xs[:n] ** 2)
    ref = np.linalg.solve(Sd, red["rhs"])
    assert np.abs(dc - ref).max() <= 1e-7 * np.abs(ref).max()
    # ... and the frame blocks of that system were damped with the frames' x_scale (oracle Schur reduction)
    U, gc, V, gf, W, cost = orc.normal_equations(x, p["uvs"], p["obj"])
    S, rhs = orc.schur_reduce(U, gc, V, gf, W, lam, np.zeros((C, 12)), (1.0 / xs[n:] ** 2).reshape(F, 6))
    assert np.abs(red["S0"] - S).max() <= 1e-10 * np.abs(S).max()
    prob.close()


def test_blocked_solve_reports_an_indefinite_system(mc):
    """A negative damping makes S0 + lambda D indefinite: the factorisation must fail and say so the way k_solve_cam does --
    solve info 1, a rebuild-only next tick, the damping raised by nu."""
    C = 64
    p = _wide(mc, C, 70, k=6)
    prob, red = _reduced(mc, p, 1e-3, "sparse")
    lam = -1e3
    st, _ = _device_solve(prob, red, lam)
    assert st[23] == 1 and st[14] == 1
    assert st[1] == lam * 2.0 and st[2] == 4.0
    prob.close()


# ------------------------------------------------------------------ sparse against dense on the same problem
@pytest.mark.parametrize("C", [6, 24, 40])
def test_sparse_equals_dense(mc, C):
    p = mc.synth.make_problem(C, 300, rows=2, cols=3, pitch=60.0, seed=5, missing=0.2)
    lam = 1e-2
    _, rd = _reduced(mc, p, lam, "dense")
    prob, rs = _reduced(mc, p, lam, "sparse")
    for k in ("S0", "rhs", "diagU", "gc"):
        assert np.abs(rs[k] - rd[k]).max() <= 1e-12 * np.abs(rd[k]).max(), k
    assert np.array_equal(rs["scal"], rd["scal"])
    prob.close()
    out = {}
    for schur in ("dense", "sparse"):
        out[schur] = _quiet(mc.bundle_adjust, p["uvs"], p["extrinsics"], p["intrinsics"], p["obj"], p["poses"], n_frames=None, ftol=1e-12, xtol=1e-12, gtol=1e-12, schur=schur)[4]
    assert abs(out["sparse"].cost - out["dense"].cost) <= 1e-10 * out["dense"].cost


def test_dense_refuses_more_than_40_cameras(mc):
    p = _wide(mc, 41, 40)
    with pytest.raises(mc.ops.McbaError, match="at most 40"):
        _quiet(mc.bundle_adjust, p["uvs"], p["extrinsics"], p["intrinsics"], p["obj"], p["poses"], n_frames=None, schur="dense")


# ------------------------------------------------------------------ edge cases
def test_edge_cases_against_dense(mc):
    """A camera seen in no frame, a frame seen by one camera, a camera pair with no shared frame (visible_k = 2 on a ring of 12), and the
    6-wide camera block (fix_intrinsics) -- the sparse handle against the dense one on the same problem."""
    C = 12
    p = mc.synth.make_problem(C, 200, rows=2, cols=3, pitch=60.0, seed=9, visible_k=2)
    uvs = p["uvs"].copy()
    uvs[5] = np.nan                                                       # camera 5 sees nothing
    seen = ~np.isnan(uvs).all(axis=(2, 3))
    f1 = int(np.flatnonzero(seen.sum(0) == 2)[0])
    uvs[np.flatnonzero(seen[:, f1])[1], f1] = np.nan                      # frame f1: one camera
    seen = ~np.isnan(uvs).all(axis=(2, 3))
    assert (seen.sum(0) == 1).any() and not seen[5].any()
    assert not (seen[0] & seen[6]).any()                                  # a pair with no shared frame
    q = dict(p, uvs=uvs)
    lam = 1e-2
    _, rd = _reduced(mc, q, lam, "dense")
    prob, rs = _reduced(mc, q, lam, "sparse")
    for k in ("S0", "rhs"):
        assert np.abs(rs[k] - rd[k]).max() <= 1e-12 * np.abs(rd[k]).max(), k
    assert np.all(rs["S0"][0:12, 72:84] == 0.0)
    prob.close()
    for kw in ({}, dict(fix_intrinsics=True)):
        out = {}
        for schur in ("dense", "sparse"):
            out[schur] = _quiet(mc.bundle_adjust, uvs, p["extrinsics"], p["intrinsics"], p["obj"], p["poses"], n_frames=None, ftol=1e-12, xtol=1e-12, gtol=1e-12, schur=schur, **kw)[4]
        assert abs(out["sparse"].cost - out["dense"].cost) <= 1e-10 * out["dense"].cost, kw


# ------------------------------------------------------------------ reproducibility, shards
def test_bitwise_reproducible_at_64_cameras(mc):
    p = _wide(mc, 64, 400)
    runs = [_quiet(mc.bundle_adjust, p["uvs"], p["extrinsics"], p["intrinsics"], p["obj"], p["poses"], n_frames=None, ftol=1e-10)[4] for _ in range(2)]
    assert np.array_equal(runs[0].x, runs[1].x)
    assert runs[0].cost == runs[1].cost
    assert runs[0].cost < 0.05 * orc.robust_cost(orc.residuals(orc.serialize_params(p["extrinsics"], p["intrinsics"], p["poses"]), p["uvs"], p["obj"]))


def test_two_frame_shards_sum_to_the_whole(mc):
    C = 56
    p = _wide(mc, C, 180)
    F = p["uvs"].shape[1]
    x = orc.serialize_params(p["extrinsics"], p["intrinsics"], p["poses"])
    lam = 1e-2
    whole, rw = _reduced(mc, p, lam, "sparse", x)
    parts = []
    for sl in (slice(0, 70), slice(70, F)):
        q = dict(p, uvs=np.ascontiguousarray(p["uvs"][:, sl]))
        xs = np.concatenate([x[:12 * C], x[12 * C:].reshape(F, 6)[sl].ravel()])
        prob, r = _reduced(mc, q, lam, "sparse", xs)
        parts.append(r)
        prob.close()
    for k in ("S0", "rhs", "diagU", "gc"):
        s = parts[0][k] + parts[1][k]
        assert np.abs(s - rw[k]).max() <= 1e-12 * np.abs(rw[k]).max(), k
    assert abs(parts[0]["scal"][0] + parts[1]["scal"][0] - rw["scal"][0]) <= 1e-12 * rw["scal"][0]
    whole.close()


def test_reprojection_diagnostics_above_40_cameras(mc):
    """The diagnostics kernel runs in launch groups of 40 cameras: its medians at 44 cameras against the same four last cameras on their own."""
    from multicam_calibration_amd import diagnostics

    p = _wide(mc, 44, 60, k=10, missing=0.0)
    med = diagnostics.reprojection_errors(p["uvs"], p["extrinsics"], p["intrinsics"], p["obj"], p["poses"], arrays=False)[0]
    sub = diagnostics.reprojection_errors(p["uvs"][40:], p["extrinsics"][40:], p["intrinsics"][40:], p["obj"], p["poses"], arrays=False)[0]
    assert np.isfinite(np.asarray(med)[40:]).all()
    np.testing.assert_array_equal(np.asarray(med)[40:], np.asarray(sub))


def test_calibrate_calls_refuse_a_sparse_handle_above_40_cameras(mc):
    """calibrate()'s kernels hold at most 40 cameras (k_pose_chain's LDS tables); a sparse-Schur handle can have more, and every mcba_calib_*
    call on it must refuse with an argument error instead of running."""
    C = 41
    p = _wide(mc, C, 30, k=6, missing=0.0)
    prob = mc.ops.Problem(p["uvs"], p["obj"], schur="sparse")
    tree = np.stack([np.arange(C - 1), np.arange(1, C)], 1)
    intr9 = np.tile(np.r_[1150.0, 1150.0, 640.0, 512.0, -0.07, 0.02, 0.0, 0.0, 0.0], (C, 1))
    calls = [lambda: prob.calib_graph(tree, 0), lambda: prob.calib_complete(), lambda: prob.calib_pairwise(tree),
             lambda: prob.calib_consensus(np.zeros((C, 6))), lambda: prob.calib_poses(intr9)]
    for call in calls:
        with pytest.raises(mc.ops.McbaError, match="at most 40"):
            call()
    # ... and the handle still solves
    prob.set_params(0, orc.serialize_params(p["extrinsics"], p["intrinsics"], p["poses"]))
    prob.linearize(0)
    prob.build_reduced(1e-2)
    assert np.isfinite(prob.get_reduced()["S0"]).all()
    prob.close()
