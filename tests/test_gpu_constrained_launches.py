"""The XS instantiations of the LM core, one launch at a time (run with `-m gpu` on an MI355X): the kernels that run when a handle has a
`dscale` vector -- a numeric x_scale (mcba_set_x_scale) and / or frozen frame coordinates (mcba_set_frozen) -- and the box projection.
  1. k_syrk<.., XS> / k_sp_factor<true> + k_sp_y: reduced system, gradients and cost of ONE build_reduced against the CPU model
     (tests/fake_problem.py: OracleProblem), at the smallest shapes that reach every k_syrk shape, FS = 8 / 4 / 2, both camera block widths
     and the sparse handle; settings frozen / x_scale / both / neither;
  2. k_backsub: ONE step on the same handles -- frozen coordinates bitwise unmoved, the rest and the trial scalars against the model, and
     at C = 2, 8 against an independent dense solve of the whole damped system with the frozen columns deleted;
  3. k_clip: bounds half-way along the step are met to the bit, and lifting them gives the unclipped point back;
  4. the `dscale` index map of both reduced solves (12- and 6-wide) against LAPACK;
  5. k_syrk<.., DECIDE, XS>: scripted ticks against a replay of each tick's launches on a second handle;
  6. switching both off again gives the bits of a handle that never had them.
Every deviation is printed before it is asserted (run with -s to see the margins).  Measured on an MI355X: S0 <= 7.5e-14, right-hand side and
gradients <= 2.8e-13, cost <= 5.1e-14 (bounds 1e-10 .. 1e-12); the step <= 0.08 of its bound, its trial cost <= 8.1e-11 (bound 1e-10: the cost follows
the step's round-off along the weakly held rotation of a collinear board), the device solves 3.2e-12 from LAPACK, the ticks equal to their replay
to the bit."""
import numpy as np
import pytest
import scipy.linalg as sla
import scipy.sparse as sp

from fake_problem import OracleProblem
from oracle import ba_oracle as orc

pytestmark = pytest.mark.gpu

LAM = 3e-3                       # tests 1, 2, 3, 6 (test_gpu_parity.py::test_reduced_system_and_step_vs_oracle)
LAM_SOLVE = 1e-2                 # tests 4, 5 (test_gpu_shapes.py, test_gpu_sparse_schur.py)
RANK_SLOT = 3
BOARDS = {7: (1, 7), 33: (2, 3), 65: (2, 2), 130: (1, 5)}   # rows, cols per frame count: test_gpu_shapes.py::FRAMES_BOARDS, and the wide rig's 2 x 3
SETTINGS = ("frozen", "xscale", "both", "neither")


def _shapes():
    """(schur, camera block, C, F): k_syrk shape 1 (C = 2), 0 (8), 2 with FS 4 (14) and FS 2 (27), 4 (cw 6, C = 3), 3 (cw 6, C = 16); k_sp_factor / k_sp_y /
    k_sp_solve_pre at 3, 41 (12-wide) and 5 (6-wide).  7 frames: one ragged block; 65: two blocks, a second 32-frame super-stage; 130: three blocks."""
    out = []
    for schur, cw, C in (("dense", 12, 2), ("dense", 12, 8), ("dense", 6, 3), ("sparse", 12, 3), ("sparse", 6, 5)):
        out += [(schur, cw, C, F) for F in (7, 65, 130)]
    return out + [("dense", 12, 14, 65), ("dense", 12, 27, 33), ("dense", 6, 16, 65), ("sparse", 12, 41, 33)]


SHAPES = _shapes()


def _sid(shape):
    return "%s-cw%d-C%d-F%d" % shape


@pytest.fixture(scope="module")
def mc():
    import multicam_calibration_amd as m

    m.ops.load_library()
    return m


def _say(what, shape, setting, dev):
    print("DEV %s %s %s %s" % (what, shape if isinstance(shape, str) else _sid(shape), setting, " ".join("%s=%.2e" % kv for kv in dev.items())))


# ------------------------------------------------------------------ problems, masks, scales
_PROBLEMS = {}


def _frozen_mask(F, C, unseen, rng):
    """About 20 % of the frame coordinates at random, one whole frame, one coordinate each in frame 0, frame F - 1, a frame >= 64 (where there is one) and
    the frame no camera sees.  Camera entries clear (mcba_set_frozen ignores them: test 6)."""
    fr = np.zeros((F, 6), bool)
    n_random = int(round(0.2 * 6 * F))
    fr.ravel()[rng.choice(6 * F, n_random, replace=False)] = True
    fr[F // 2] = True
    fr[0, 1] = fr[F - 1, 4] = fr[unseen, 3] = True
    if F > 64:
        fr[64 + (F - 64) // 2, 2] = True
    return np.concatenate([np.zeros(12 * C, bool), fr.ravel()]), n_random


def _problem(mc, shape):
    """uvs (one frame blanked), board, start point, frozen mask, log-normal x_scale of a shape -- made once."""
    if shape in _PROBLEMS:
        return _PROBLEMS[shape]
    schur, cw, C, F = shape
    rows, cols = (2, 3) if C > 40 else BOARDS[F]
    wide =dict(visible_k=6, pitch=60.0) if C > 40 else dict(pitch=50.0)   # (41 cameras: the visibility of tests/test_gpu_sparse_schur.py::_wide)
    p = mc.synth.make_problem(C, F, rows=rows, cols=cols, seed=900 + 7 * C + F, missing=0.2, noise=0.3, **wide)
    rng = np.random.default_rng(1000 + 13 * C + F + cw)
    uvs = p["uvs"].copy()
    unseen = F // 3
    uvs[:, unseen] = np.nan
    mask, n_random = _frozen_mask(F, C, unseen, rng)
    # the properties a mask must have
    fr = mask[12 * C:].reshape(F, 6)
    assert not mask[:12 * C].any() and n_random <= fr.sum() <= n_random + 10 and abs(n_random / (6.0 * F) - 0.2) <= 0.5 / (6 * F)
    assert fr.all(1).any() and fr[0].any() and not fr[0].all() and fr[F - 1].any() and (F <= 64 or fr[64:].any())
    dark = np.isnan(uvs).all(axis=(0, 2, 3))
    assert dark[unseen] and fr[dark].any() and not fr.all()
    xs = np.exp(rng.normal(0.0, 0.5, 12 * C + 6 * F))
    x0 = orc.serialize_params(p["extrinsics"], p["intrinsics"], p["poses"])
    _PROBLEMS[shape] = dict(uvs=uvs, obj=p["obj"], x0=x0, mask=mask, xs=xs)
    return _PROBLEMS[shape]


def _handle(mc, shape, pr):
    schur, cw = shape[0], shape[1]
    prob = mc.ops.Problem(pr["uvs"], pr["obj"], schur=schur)
    assert prob.is_sparse == (schur == "sparse")
    if cw == 6:
        assert prob.set_camera_block(6) and prob.n == 6 * shape[2]
    return prob


def _copy(red):
    return {k: np.array(v, copy=True) for k, v in red.items()}


# ------------------------------------------------------------------ one build_reduced + one step per (shape, setting), shared by tests 1 and 2
_CASES = {}


def _case(mc, shape, setting):
    if (shape, setting) in _CASES:
        return _CASES[(shape, setting)]
    schur, cw, C, F = shape
    pr = _problem(mc, shape)
    x0 = pr["x0"]
    xs = pr["xs"] if setting in ("xscale", "both") else None
    mask = pr["mask"] if setting in ("frozen", "both") else None
    prob, model = _handle(mc, shape, pr), OracleProblem(pr["uvs"], pr["obj"])
    for q in (prob, model):
        q.set_x_scale(xs)
        q.set_frozen(mask)
        q.set_params(0, x0)
        q.linearize(0)
        q.build_reduced(LAM, rank_slot=RANK_SLOT)
    keep = np.asarray(prob.cam_index)
    red, gfd = _copy(prob.get_reduced()), prob.frame_gradient().copy()
    wide = model.get_reduced()                                       # the model's system is 12 wide: the 6-wide one is its rows / columns `cam_index`
    want = dict(S0=wide["S0"][np.ix_(keep, keep)], rhs=wide["rhs"][keep], diagU=wide["diagU"][keep], gc=wide["gc"][keep], scal=wide["scal"], gc_full=wide["gc"])
    # one step: the camera step from LAPACK on the model's damped system (D_c = 1 / x_scale^2 where x_scale is set, else diag(U), 1 where that is 0)
    Dc = 1.0 / xs[keep] ** 2 if xs is not None else np.where(want["diagU"] > 0, want["diagU"], 1.0)
    dc = np.linalg.solve(want["S0"] + LAM * np.diag(Dc), want["rhs"])
    dfull = np.zeros(12 * C)
    dfull[keep] = dc
    model.step(dfull, LAM, 0, 1)
    prob.step(dc, LAM, 0, 1)
    out = dict(red=red, gf=gfd, want=want, want_gf=model.frame_gradient(), keep=keep, dc=dc, x0=x0, x1=prob.get_params(1), t=prob.get_trial(), want_x1=model.get_params(1),
               want_t=model.get_trial(), mask=mask, xs=xs, pr=pr)
    prob.close()
    _CASES[(shape, setting)] = out
    return out


# ------------------------------------------------------------------ 1. the reduced system of one launch
@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_reduced_system_per_launch(mc, shape, setting):
    """k_syrk<SHAPE, false, XS> (k_sp_factor<XS> + k_sp_y on the sparse handle) + k_reduce_system against OracleProblem.build_reduced; tolerances of
    test_gpu_parity.py::test_reduced_system_and_step_vs_oracle.  scal[4 + slot] is the largest |g_f| over the FREE coordinates, frame_gradient() the
    true gradient, frozen entries included."""
    r = _case(mc, shape, setting)
    red, want = r["red"], r["want"]
    n = r["keep"].size
    assert red["S0"].shape == (n, n)
    scale = np.abs(want["S0"]).max()
    gmax, gfree = np.abs(r["want_gf"]).max(), want["scal"][4 + RANK_SLOT]
    live = want["diagU"] > 0
    dev = dict(S0=np.abs(red["S0"] - want["S0"]).max() / scale, sym=np.abs(red["S0"] - red["S0"].T).max() / scale,
               rhs=np.abs(red["rhs"] - want["rhs"]).max() / np.abs(want["rhs"]).max(), diagU=(np.abs(red["diagU"] - want["diagU"])[live] / want["diagU"][live]).max(),
               gc=np.abs(red["gc"] - want["gc"]).max() / np.abs(want["gc_full"]).max(), cost=abs(red["scal"][0] - want["scal"][0]) / want["scal"][0],
               gmax=abs(red["scal"][4 + RANK_SLOT] - gfree) / gfree, gf=np.abs(r["gf"] - r["want_gf"]).max() / gmax)
    _say("reduced", shape, setting, dev)
    assert dev["S0"] <= 1e-10 and dev["sym"] <= 1e-12
    assert dev["rhs"] <= 1e-10
    np.testing.assert_allclose(red["diagU"], want["diagU"], rtol=1e-11)
    assert dev["gc"] <= 1e-10
    assert dev["cost"] <= 1e-12
    assert red["scal"][2] == 0                                                     # every frame block factorised
    assert dev["gmax"] <= 1e-10
    assert np.all(np.delete(red["scal"][4:], RANK_SLOT) == 0)
    assert dev["gf"] <= 1e-10
    if r["mask"] is not None:   # (the largest free gradient is not the largest gradient: a kernel that reported the true maximum would be seen)
        assert gfree <= gmax


# ------------------------------------------------------------------ 2. one step of one launch
def _dense_step(pr, lam, xs, mask):
    """The LM step of the WHOLE damped system in one LAPACK solve: H = J^T w J from the oracle's Jacobian, D = 1 / x_scale^2 or diag(H) (1 where
    that is 0), the frozen columns deleted."""
    x, uvs, obj = pr["x0"], pr["uvs"], pr["obj"]
    J = orc.jacobian_csr(x, uvs, obj)
    f = orc.residuals(x, uvs, obj)
    js, _ = orc.robust_scales(f, "soft_l1")
    rho1 = orc.loss_rho(f ** 2, "soft_l1")[1]
    w = np.maximum(js * js, orc.CURV_FLOOR * rho1)                               # the LM's curvature weight (csrc/mcba_math.h)
    H = (J.T @ sp.diags(w) @ J).toarray()
    g = J.T @ (rho1 * f)
    D = 1.0 / xs ** 2 if xs is not None else np.where(np.diag(H) > 0, np.diag(H), 1.0)
    free = np.ones(x.size, bool) if mask is None else ~mask
    d = np.zeros(x.size)
    d[free] = np.linalg.solve((H + lam * np.diag(D))[np.ix_(free, free)], -g[free])
    return d


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_one_step_per_launch(mc, shape, setting):
    """k_backsub<CW> on the factors test 1 checked: frozen coordinates do not move by a bit, the intrinsics of the 6-wide block are copied, the rest and
    the trial scalars against OracleProblem.step (tolerances of test_reduced_system_and_step_vs_oracle); at C = 2 and 8 the step also against the
    dense solve of the whole system (1e-6, that test's: the model alone agrees with it to 2.4e-10 at these shapes).  Reordering the point sums
    of the model moves its own step by at most 0.07 of the bound on x (collinear boards under a numeric x_scale: the rotation about the board's
    line is held by lam / x_scale^2 alone), which is the round-off floor of this comparison."""
    schur, cw, C, F = shape
    r = _case(mc, shape, setting)
    x0, x1, want = r["x0"], r["x1"], r["want_x1"]
    step = want - x0
    if r["mask"] is not None:
        np.testing.assert_array_equal(x1[r["mask"]], x0[r["mask"]])
        assert np.all(want[r["mask"]] == x0[r["mask"]])                            # (and the model agrees that this is the step)
    if cw == 6:
        np.testing.assert_array_equal(x1[:12 * C].reshape(C, 12)[:, :6], x0[:12 * C].reshape(C, 12)[:, :6])
    t, wt = r["t"], r["want_t"]
    dev = dict(x=np.abs(x1 - want).max() / (1e-9 * np.abs(step).max() + 1e-13 * np.abs(x0).max()), t0=abs(t[0] - wt[0]) / wt[0], t1=abs(t[1] - wt[1]) / abs(wt[1]),
               t2=abs(t[2] - wt[2]) / wt[2], t3=abs(t[3] - wt[3]) / wt[3])
    _say("step (x: fraction of its bound)", shape, setting, dev)
    assert np.abs(x1 - want).max() <= 1e-9 * np.abs(step).max() + 1e-13 * np.abs(x0).max()
    assert dev["t0"] <= 1e-10 and dev["t1"] <= 1e-8 and dev["t2"] <= 1e-9 and dev["t3"] <= 1e-12
    assert t[4] == np.count_nonzero(~np.isnan(r["pr"]["uvs"]))
    if schur == "dense" and cw == 12 and C in (2, 8):
        full = _dense_step(r["pr"], LAM, r["xs"], r["mask"])
        dd = np.abs((x1 - x0) - full).max() / np.abs(full).max()
        _say("step vs dense solve", shape, setting, dict(model=np.abs(step - full).max() / np.abs(full).max(), gpu=dd))
        assert dd <= 1e-6


# ------------------------------------------------------------------ 3. the box projection
def _pick_bound_coordinates(s, ncam):
    """Among the coordinates whose step is above the median size: camera coordinates of both signs, frame coordinates of both signs below frame 64 and
    from frame 64 on."""
    big = np.abs(s) > np.median(np.abs(s))
    idx = np.arange(s.size)
    first = ncam + 6 * 64
    picked = []
    for zone, count in (((idx < ncam), 2), ((idx >= ncam) & (idx < first), 2), ((idx >= first), 1)):
        for sign in (1.0, -1.0):
            picked += list(idx[zone & big & (sign * s > 0)][:count])
    return np.array(sorted(picked))


@pytest.mark.parametrize("shape", [("dense", 12, 2, 130), ("sparse", 12, 3, 130)], ids=_sid)
def test_box_projection(mc, shape):
    """k_clip behind k_backsub: with a bound half-way along the step of a few coordinates, those end ON the bound to the bit, everything lies in the box,
    the rest and the cost (taken at the projected point) are the model's; without bounds the same call gives the unclipped point again; and the
    device-resident solve refuses to run while bounds are set (include/mcba.h)."""
    schur, cw, C, F = shape
    r = _case(mc, shape, "neither")
    pr, x0, dc, ncam = r["pr"], r["x0"], r["dc"], 12 * C
    s = r["want_x1"] - x0                                                           # the model's unclipped step
    picked = _pick_bound_coordinates(s, ncam)
    assert np.sum(picked < ncam) >= 2 and np.sum(picked >= ncam) >= 6 and np.any(picked >= ncam + 6 * 64)
    assert np.any(s[picked] > 0) and np.any(s[picked] < 0) and np.all(np.abs(s[picked]) > np.median(np.abs(s)))
    lo, hi = x0 - 10.0 * (1.0 + np.abs(x0)), x0 + 10.0 * (1.0 + np.abs(x0))
    up = picked[s[picked] > 0]
    down = picked[s[picked] < 0]
    hi[up] = x0[up] + 0.5 * s[up]
    lo[down] = x0[down] + 0.5 * s[down]
    bound = np.where(s[picked] > 0, hi[picked], lo[picked])

    prob, model = _handle(mc, shape, pr), OracleProblem(pr["uvs"], pr["obj"])
    for q in (prob, model):
        q.set_params(0, x0)
        q.linearize(0)
        q.build_reduced(LAM)
    dfull = np.zeros(ncam)
    dfull[r["keep"]] = dc
    prob.step(dc, LAM, 0, 1)
    free_point = prob.get_params(1)
    np.testing.assert_array_equal(free_point, r["x1"])                            # (the same launch as test 2's: the same bits)
    for q, d in ((prob, dc), (model, dfull)):
        q.set_bounds(lo, hi)
        q.step(d, LAM, 0, 1)
    x1, t, want, wt = prob.get_params(1), prob.get_trial(), model.get_params(1), model.get_trial()
    np.testing.assert_array_equal(x1[picked], bound)
    assert np.all(x1 >= lo) and np.all(x1 <= hi)
    assert np.all(want[picked] == bound) and not np.any(free_point[picked] == bound)
    dev = dict(x=np.abs(x1 - want).max() / (1e-9 * np.abs(s).max() + 1e-13 * np.abs(x0).max()), t0=abs(t[0] - wt[0]) / wt[0], t1=abs(t[1] - wt[1]) / abs(wt[1]),
               t2=abs(t[2] - wt[2]) / wt[2])
    _say("clipped step (x: fraction of its bound)", shape, "bounds", dev)
    assert np.abs(x1 - want).max() <= 1e-9 * np.abs(s).max() + 1e-13 * np.abs(x0).max()
    assert dev["t0"] <= 1e-10                                                     # the robust cost AT THE PROJECTED POINT
    assert dev["t1"] <= 1e-8 and dev["t2"] <= 1e-9                                # (the step's own scalars are those of the unclipped step)
    assert wt[0] != r["want_t"][0]                                                # ... which is another cost than the unclipped point's
    # the documented refusal of the device-resident solve
    prob.lm_set_state(float(prob.get_reduced()["scal"][0]), LAM, 2.0, 0)
    prob.lm_auto_config(0.0, 0.0, 0.0, 1e-12, 1e12, None)
    with pytest.raises(mc.ops.McbaError, match="box constraints are set"):
        prob.lm_auto_solve(1)
    # bounds lifted: the unclipped point again
    prob.set_bounds(None, None)
    prob.step(dc, LAM, 0, 1)
    np.testing.assert_array_equal(prob.get_params(1), free_point)
    assert np.abs(free_point - r["want_x1"]).max() <= 1e-9 * np.abs(s).max() + 1e-13 * np.abs(x0).max()
    prob.lm_auto_solve(1)                                                          # ... and the solve runs
    assert prob.lm_auto_wait(1)[23] == 0
    prob.close()


# ------------------------------------------------------------------ 4. x_scale in the reduced solves
def _patterned_x_scale(C, F, rng):
    """Twelve different values within a camera, neighbouring cameras on different levels: an index map that reads another entry reads another value."""
    cam = (0.6 + 0.1 * np.arange(12))[None, :] * (1.0 + 0.25 * ((7 * np.arange(C)) % 5))[:, None]
    return np.concatenate([cam.ravel(), np.exp(rng.normal(0.0, 0.5, 6 * F))])


@pytest.mark.parametrize("fixed", [False, True], ids=["free", "fixed"])
@pytest.mark.parametrize("shape", [("dense", 12, 3, 33), ("dense", 6, 3, 33), ("dense", 12, 10, 33), ("dense", 6, 10, 33), ("sparse", 6, 5, 33), ("sparse", 12, 41, 65)], ids=_sid)
def test_x_scale_in_the_reduced_solves(mc, shape, fixed):
    """The `dsc` branch of k_solve_cam (factor in LDS at 3 cameras, right-looking at 10) and of k_sp_solve_pre: D_c = 1 / x_scale[cam_index]^2 on the diagonal
    of the system that is factorised -- against LAPACK on S0 + lam D_c restricted to the free rows.  Tolerances of
    test_gpu_parity.py::test_device_reduced_solve_matches_lapack."""
    schur, cw, C, F = shape
    pr = _problem(mc, shape)
    rng = np.random.default_rng(40 + C + cw)
    xs = _patterned_x_scale(C, F, rng)
    lam = LAM_SOLVE
    prob = _handle(mc, shape, pr)
    n, keep = prob.n, np.asarray(prob.cam_index)
    mask = None
    if fixed:
        mask = np.zeros(n, bool)
        mask[:cw] = True                                                          # camera 0, and a few rows elsewhere
        mask[rng.choice(np.arange(cw, n), 5, replace=False)] = True
    prob.set_x_scale(xs)
    prob.set_params(0, pr["x0"])
    prob.linearize(0)
    prob.build_reduced(lam, rank_slot=0)
    red = _copy(prob.get_reduced())
    prob.lm_set_state(float(red["scal"][0]), lam, 2.0, 0)
    prob.lm_auto_config(0.0, 0.0, 0.0, 1e-12, 1e12, mask)
    prob.lm_auto_solve(1)
    st = prob.lm_auto_wait(1).copy()
    d = prob.cam_step()
    prob.close()

    D = 1.0 / xs[keep] ** 2
    S = red["S0"] + lam * np.diag(D)
    free = np.ones(n, bool) if mask is None else ~mask
    ref = np.zeros(n)
    ref[free] = sla.cho_solve(sla.cho_factor(S[np.ix_(free, free)]), red["rhs"][free])
    assert st[31] == 1 and st[23] == 0 and st[15] == 0 and st[14] == 0
    assert np.all(d[~free] == 0.0)
    back = S[np.ix_(free, free)] @ d[free] - red["rhs"][free]
    pred = float(ref @ (lam * D * ref - red["gc"]))
    dev = dict(backward=np.abs(back).max() / (np.abs(S).max() * np.abs(d).max() + np.abs(red["rhs"]).max()), lapack=np.abs(d - ref).max() / np.abs(ref).max(),
               pred=abs(st[11] - pred) / abs(pred), dn2=abs(st[12] - ref @ ref) / (ref @ ref))
    _say("solve", shape, "fixed" if fixed else "free", dev)
    assert dev["backward"] <= 1e-11
    assert dev["lapack"] <= 1e-7
    assert dev["pred"] <= 1e-6 and dev["dn2"] <= 1e-6


# ------------------------------------------------------------------ 5. the deciding instantiation
def _jacobian_x_scale(pr, C, rng):
    """A numeric x_scale on the scale scipy's 'jac' would find (1 / the column norms of J at the start), each entry off by a log-normal factor: the
    damped systems of the ticks stay as well conditioned as Marquardt's, so that two solves of one system agree far below the bound of the comparison."""
    U, gc, V, gf, W, cost = orc.normal_equations(pr["x0"], pr["uvs"], pr["obj"])
    d = np.concatenate([np.diag(U[c]) for c in range(C)] + [np.diag(V[f]) for f in range(V.shape[0])])
    return np.exp(rng.normal(0.0, 0.5, d.size)) / np.sqrt(np.where(d > 0, d, 1.0))


@pytest.mark.parametrize("shape", [("dense", 12, 2, 65), ("dense", 12, 8, 65), ("dense", 12, 14, 65), ("dense", 6, 3, 65)], ids=_sid)
def test_deciding_instantiation_replayed(mc, shape):
    """k_syrk<SHAPE, DECIDE, XS> inside lm_auto_tick (the default single-GPU tick): after every tick the current point, the damping and the cost of the
    posted state are taken to a second handle with the same x_scale, which repeats the tick's launches one call at a time -- linearize, build_reduced
    (the launch test 1 holds to the model), the device solve, step.  Its trial point must be the one the tick stored.  Up to 9 cameras the tick's solve
    stores the trial point itself (k_solve_backsub); beyond, the NEXT tick's back-substitution does, in the slot that was the trial slot then."""
    schur, cw, C, F = shape
    pr = _problem(mc, shape)
    x0 = pr["x0"]
    xs = _jacobian_x_scale(pr, C, np.random.default_rng(50 + C))
    tick, rep = _handle(mc, shape, pr), _handle(mc, shape, pr)
    for q in (tick, rep):
        q.set_x_scale(xs)
    tick.set_params(0, x0)
    tick.set_params(1, x0)
    tick.linearize(0)
    tick.build_reduced(LAM_SOLVE, rank_slot=0)
    tick.lm_set_state(float(tick.get_reduced()["scal"][0]), LAM_SOLVE, 2.0, 0)
    tick.lm_auto_config(0.0, 0.0, 0.0, 1e-12, 1e12, None)
    fused = tick.fuse_status()[1]                                                 # (by default: up to 9 cameras)
    rows = []

    def retire(seq):
        st = tick.lm_auto_wait(seq).copy()
        tick.synchronize()
        late, still = tick.fuse_status()
        if late != 0 or still != fused:
            pytest.fail("the fused launch of tick %d gave up waiting for its solve (fuse_status: %r, %r)" % (late, late, still))
        assert st[31] == seq and st[23] == 0 and st[15] == 0 and st[14] == 0
        rows.append((st, tick.get_params(0), tick.get_params(1)))

    tick.lm_auto_solve(1)
    retire(1)
    for seq in (2, 3):
        tick.lm_auto_tick(seq)
        retire(seq)
    assert rows[1][0][17] == 1 and rows[2][0][17] == 2                            # each tick took a decision on a trial point

    def replay(st, cur):
        rep.set_params(0, cur)
        rep.linearize(0)
        rep.build_reduced(float(st[1]), rank_slot=0)
        cost = float(rep.get_reduced()["scal"][0])
        rep.lm_set_state(cost, float(st[1]), float(st[2]), 0)
        rep.lm_auto_config(0.0, 0.0, 0.0, 1e-12, 1e12, None)
        rep.lm_auto_solve(1)
        assert rep.lm_auto_wait(1)[23] == 0
        rep.step(rep.cam_step(), float(st[1]), 0, 1)
        return cost, rep.get_params(1)

    checked = 0
    for k, (st, s0, s1) in enumerate(rows):                                       # k = seq - 1
        cur = int(st[3])
        here = (s0, s1)[cur]
        cost, want = replay(st, here)
        dcost = abs(st[0] - cost) / cost
        stored = None
        if fused and k >= 1:
            stored = (s0, s1)[1 - cur]
        elif not fused and k + 1 < len(rows):
            stored = rows[k + 1][1 + (1 - cur)]
        dev = dict(cost=dcost, lam=st[1])
        if stored is not None:
            bound = 1e-9 * np.abs(want - here).max() + 1e-13 * np.abs(here).max()
            dev["x"] = np.abs(stored - want).max() / bound
            checked += 1
        _say("tick %d (x: fraction of its bound)" % (k + 1), shape, "fused" if fused else "two launches", dev)
        assert dcost <= 1e-12
        if stored is not None:
            assert np.abs(stored - want).max() <= bound
            if cw == 6:
                np.testing.assert_array_equal(stored[:12 * C].reshape(C, 12)[:, :6], x0[:12 * C].reshape(C, 12)[:, :6])
    assert checked == 2
    tick.close()
    rep.close()


# ------------------------------------------------------------------ 6. switching back
@pytest.mark.parametrize("shape", [("dense", 12, 2, 65), ("sparse", 12, 3, 65)], ids=_sid)
def test_switching_back_gives_the_plain_bits(mc, shape):
    """set_frozen(None) + set_x_scale(None) return a handle to the XS = false instantiations: the same bits as a handle that never left them.  And the
    camera entries of a frozen mask do not count (include/mcba.h)."""
    schur, cw, C, F = shape
    pr = _problem(mc, shape)

    def system(q):
        q.set_params(0, pr["x0"])
        q.linearize(0)
        q.build_reduced(LAM)
        return _copy(q.get_reduced())

    a, b = _handle(mc, shape, pr), _handle(mc, shape, pr)
    a.set_x_scale(pr["xs"])
    a.set_frozen(pr["mask"])
    both = system(a)
    a.set_frozen(None)
    a.set_x_scale(None)
    back, plain = system(a), system(b)
    assert not np.array_equal(both["S0"], plain["S0"]) and not np.array_equal(both["rhs"], plain["rhs"])   # (they were in force)
    for k in ("S0", "rhs", "scal", "diagU", "gc"):
        np.testing.assert_array_equal(back[k], plain[k], err_msg=k)
    a.close()
    with_cams = pr["mask"].copy()
    with_cams[: 12 * C : 5] = True
    with_cams[:12] = True
    b.set_frozen(with_cams)
    set_, gset = system(b), b.frame_gradient().copy()
    b.set_frozen(pr["mask"])
    clear, gclear = system(b), b.frame_gradient().copy()
    c = _handle(mc, shape, pr)
    c.set_frozen(pr["mask"])
    fresh = system(c)
    for k in ("S0", "rhs", "scal", "diagU", "gc"):
        np.testing.assert_array_equal(set_[k], clear[k], err_msg=k)
        np.testing.assert_array_equal(fresh[k], clear[k], err_msg=k)
    np.testing.assert_array_equal(gset, gclear)
    assert not np.array_equal(clear["S0"], plain["S0"])
    b.close()
    c.close()
