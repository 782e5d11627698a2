"""The stretch of the LM tick from the reduced factorisation to the stored trial step (csrc/mcba_solve.hip, csrc/mcba_backsub.h):
  * the backward sweep that one wavefront runs alone, at the sizes where its block structure changes (three blocks; the right-hand-side row
    opening a block of its own; five blocks; the 6-wide camera block with identity rows behind the right-hand side) -- against LAPACK;
  * a solve that FAILS inside the fused launch (k_solve_backsub): the final release word alone tells the back-substitution workgroups not
    to store -- the trial slot stays as it was, the next tick rebuilds, a later tick proceeds, and every posted state, the current
    point and the stored trial points equal those of the two-launch path (MCBA_FUSE_BACKSUB=0) to the bit."""
import numpy as np
import pytest

from oracle import ba_oracle as orc

pytestmark = pytest.mark.gpu

LM_SKIP, LM_DONE, LM_SOLVE_INFO = 14, 15, 23   # csrc/mcba_lm_state.h


@pytest.fixture(scope="module")
def mc():
    import multicam_calibration_amd as m

    m.ops.load_library()
    return m


# ------------------------------------------------------------------ backward sweep at the block edges
@pytest.mark.parametrize("C,block6", [(3, False), (4, False), (5, False), (8, True), (9, True)])
def test_sweep_at_the_block_edges_matches_lapack(mc, C, block6):
    """Construction and tolerances of test_device_reduced_solve_matches_lapack (backward error 1e-11, 1e-7 against LAPACK), at sizes it does
    not have: C = 3 (37 rows with the right-hand side: three blocks of 16), C = 4 (49: the right-hand-side row opens a block of its own),
    C = 5 (61), and the 6-wide camera block (intrinsics held fixed) at C = 8 (n = 48: the right-hand side is row 48, identity rows behind
    it) and C = 9 (n = 54)."""
    import scipy.linalg as sla

    p = mc.synth.make_problem(C, 40, seed=60 + C, missing=0.1)
    x = orc.serialize_params(p["extrinsics"], p["intrinsics"], p["poses"])
    prob = mc.ops.Problem(p["uvs"], p["obj"])
    if block6:
        assert prob.set_camera_block(6)
    n = prob.n
    assert n == (6 if block6 else 12) * C
    prob.set_params(0, x)
    prob.linearize(0)
    lam = 2e-3
    prob.build_reduced(lam, rank_slot=0)
    red = {k: v.copy() for k, v in prob.get_reduced().items()}
    prob.lm_set_state(float(red["scal"][0]), lam, 2.0, 0)
    prob.lm_auto_config(1e-8, 1e-8, 1e-8, 1e-12, 1e12, None)
    prob.lm_auto_solve(1)
    st = prob.lm_auto_wait(1).copy()
    d_dev = prob.cam_step()
    prob.close()

    Dc = np.where(red["diagU"] > 0, red["diagU"], 1.0)
    S = red["S0"] + lam * np.diag(Dc)
    d_ref = sla.cho_solve(sla.cho_factor(S), red["rhs"])
    assert st[31] == 1 and st[LM_DONE] == 0 and st[LM_SKIP] == 0 and st[LM_SOLVE_INFO] == 0
    r = S @ d_dev - red["rhs"]
    assert np.abs(r).max() <= 1e-11 * (np.abs(S).max() * np.abs(d_dev).max() + np.abs(red["rhs"]).max())
    assert np.abs(d_dev - d_ref).max() <= 1e-7 * np.abs(d_ref).max()
    # the step scalars are taken from the sweep's result afterwards
    pred_cam = float(d_ref @ (lam * Dc * d_ref - red["gc"]))
    assert abs(st[11] - pred_cam) <= 1e-6 * abs(pred_cam)
    assert abs(st[12] - d_ref @ d_ref) <= 1e-6 * (d_ref @ d_ref)
    xc = x[:12 * C].reshape(C, 12)[:, 6:].ravel() if block6 else x[:12 * C]
    assert abs(st[13] - xc @ xc) <= 1e-13 * (xc @ xc)


# ------------------------------------------------------------------ a failed solve inside the fused launch
def _scripted_ticks(mc, p, fuse, monkeypatch):
    """solve (1), two ticks (2, 3), a NEGATIVE damping written into the device state together with SKIP = 1 (a rebuild-only tick takes no
    decision, and a decision would clamp the damping to lam_min), tick 4 (its solve must fail), a positive damping written back, ticks 5
    (rebuild-only), 6, 7.  Returns the posted states and both parameter slots after every tick."""
    monkeypatch.setenv("MCBA_FUSE_BACKSUB", fuse)
    x = orc.serialize_params(p["extrinsics"], p["intrinsics"], p["poses"])
    prob = mc.ops.Problem(p["uvs"], p["obj"])
    prob.set_params(0, x)
    prob.set_params(1, x)
    prob.linearize(0)
    lam = 1e-3
    prob.build_reduced(lam, rank_slot=0)
    cost = float(prob.get_reduced()["scal"][0])
    prob.lm_set_state(cost, lam, 2.0, 0)
    prob.lm_auto_config(0.0, 0.0, 0.0, 1e-12, 1e12, None)
    states, slots = [], []

    def retire(seq):
        st = prob.lm_auto_wait(seq).copy()
        prob.synchronize()
        states.append(st)
        slots.append((prob.get_params(0), prob.get_params(1)))
        return st

    def write_lambda(st, lam_new, nu):
        s = np.ascontiguousarray(st, dtype=np.float64).copy()
        s[1], s[2], s[LM_SKIP] = lam_new, nu, 1.0
        prob._chk(prob.lib.mcba_lm_set_state(prob.handle, mc.ops._p(s)))

    prob.lm_auto_solve(1)
    retire(1)
    for seq in (2, 3):
        prob.lm_auto_tick(seq)
        st = retire(seq)
    # H - |lambda| D is indefinite for every lambda < 0: the undamped normal equations are singular (the world frame is free), and the
    # frame blocks stay positive definite at this size of lambda, so it is the reduced factorisation that meets a negative pivot
    write_lambda(st, -1e-4, 2.0)
    prob.lm_auto_tick(4)
    st = retire(4)
    write_lambda(st, 1e-3, 2.0)
    for seq in (5, 6, 7):
        prob.lm_auto_tick(seq)
        retire(seq)
    prob.close()
    return states, slots


def test_failed_solve_in_the_fused_launch(mc, monkeypatch):
    p = mc.synth.make_problem(6, 130, seed=91)
    fused, fslots = _scripted_ticks(mc, p, "1", monkeypatch)
    apart, aslots = _scripted_ticks(mc, p, "0", monkeypatch)
    s3, s4, s5, s6 = fused[2], fused[3], fused[4], fused[5]
    # tick 4: the solve failed and said so; the damping was raised by nu; the trial slot (both slots, in fact: a tick writes parameters
    # only through its back-substitution) is what tick 3 left
    assert s4[LM_SOLVE_INFO] == 1 and s4[LM_SKIP] == 1 and s4[LM_DONE] == 0
    assert s4[1] == -2e-4 and s4[2] == 4.0 and s4[0] == s3[0] and s4[17] == s3[17]
    np.testing.assert_array_equal(fslots[3][0], fslots[2][0])
    np.testing.assert_array_equal(fslots[3][1], fslots[2][1])
    # tick 5 only rebuilt the system (no decision: cost and slot as before), its solve succeeded and its back-substitution stored a new trial point
    assert s5[LM_SOLVE_INFO] == 0 and s5[LM_SKIP] == 0 and s5[0] == s4[0] and s5[3] == s4[3] and s5[17] == s4[17] and s5[24] == 1
    trial = 1 - int(s5[3])
    assert not np.array_equal(fslots[4][trial], fslots[3][trial])
    np.testing.assert_array_equal(fslots[4][1 - trial], fslots[3][1 - trial])
    # tick 6 proceeds: a decision was taken on that trial point
    assert s6[LM_SOLVE_INFO] == 0 and s6[LM_DONE] == 0 and s6[17] == s5[17] + 1
    # ... and all of it is what the two separate launches do: every posted state, and the current point after every tick (the two-launch
    # path stores a tick's trial point at the start of the NEXT tick, so the trial slots are compared one tick apart)
    assert len(fused) == len(apart) == 7
    for a, b in zip(fused, apart):
        np.testing.assert_array_equal(a, b)
    for k, (fs, sa) in enumerate(zip(fslots, aslots)):
        cur = int(fused[k][3])
        np.testing.assert_array_equal(fs[cur], sa[cur])
    for k in (4, 5):   # the trial point ticks 5 and 6 stored, against what the two-launch ticks 6 and 7 stored for them
        tr = 1 - int(fused[k][3])
        np.testing.assert_array_equal(fslots[k][tr], aslots[k + 1][tr])
