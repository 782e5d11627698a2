"""The scalable reference routes of tests/trajectory_scale_oracle.py held to the dense oracles they replace, without a GPU: on the small cases of
smoothing_oracle, evidence_oracle, trajectory_refine_oracle and skeleton_trajectory_oracle every route agrees with the dense one within a quarter
of the bar the GPU tier (tests/test_gpu_trajectory_scale.py) applies to that quantity; and on the long and wide scenes themselves the conditions
under which those GPU tests mean anything: the banded reference's own error (reference_error) at most a quarter of 4 eps cond max|x|, the oracle's
own conjugate gradients done in half the library's cap, the lane, workgroup and level counts the shapes were chosen for, the wide scene's loop
decided for the oracle itself.  Every test prints the seconds its references took (DESIGN.md section 8f-25 records them)."""
import time

import numpy as np
import pytest

import evidence_oracle as eo
import skeleton_trajectory_oracle as sto
import smoothing_oracle as so
import trajectory_refine_oracle as tro
import trajectory_scale_oracle as tso

EPS, Q = so.EPS, 0.25
LINEAR = so.linear_cases()


def running_tracks(case):
    K = case["points"].shape[1]
    acc = np.broadcast_to(np.asarray(case["accel_std"], dtype=np.float64), (K,))
    return [(k, acc[k]) for k in range(K) if so.prepare(case["points"][:, k], case["cov"][:, k])[0].sum() >= 2]


@pytest.mark.parametrize("name", sorted(LINEAR))
def test_smoother_routes_against_the_dense_system(name):
    case = LINEAR[name]
    for k, a in running_tracks(case):
        pts, cov = case["points"][:, k], case["cov"][:, k]
        w = np.random.default_rng(k).choice(np.array([0.25, 1.0, 4.0]), size=len(pts))
        for weights in (None, w):
            dense = so.system(pts, cov, a, weights)
            r = tso.smooth_reference(pts, cov, a, weights)
            assert np.array_equal(tso.banded(tso.data_blocks(dense), a), dense["ab"]) and np.array_equal(so.banded_to_dense(r["sysd"]["ab"]), dense["A"])
            cnd = so.cond(dense)
            j = 1.0 / np.sqrt(np.diagonal(dense["A"]))
            xd = (np.linalg.solve(dense["A"] * np.outer(j, j), dense["b"] * j) * j).reshape(-1, 3)
            bar = so.BAR_K * EPS * cnd * np.abs(xd).max()
            assert np.abs(r["x"] - xd).max() <= Q * bar and r["ref_err"] <= Q * bar, (name, k, np.abs(r["x"] - xd).max(), r["ref_err"], bar)
            assert abs(r["cond"] - cnd) <= 1e-6 * cnd if len(pts) <= tso.WINDOW else r["cond"] >= 0.5 * cnd
            for loss in ("linear", "soft_l1"):
                c = so.objective(xd, pts, cov, a, loss)
                assert abs(tso.objective(xd, dense, a, loss) - c) <= Q * tso.cost_bar(c, cnd), (name, k, loss)
            us = dense["usable"]
            d2, d2l = so.mahalanobis2(xd, dense)[us], tso.mahalanobis2_ld(xd, dense)[us]
            assert (4 * np.abs(d2 - d2l) <= tso.d2_bar(d2l, cnd).astype(np.float64)).all(), (name, k)
            y = np.random.default_rng(0).standard_normal(dense["A"].shape[0])
            assert np.allclose(tso.banded_matvec(dense["ab"], y), dense["A"] @ y, rtol=0, atol=64 * EPS * np.abs(dense["A"]).sum(1).max() * np.abs(y).max())


def test_window_cond_is_not_below_half_the_dense_cond():
    """T400_default (a 40-frame gap), T333_seg2 of both oracles, T257 of trajectory_refine_oracle (a one-camera stretch, an unseen gap, unseen ends) and
    of evidence_oracle; and with a window shorter than the track, so that the two ends are really cut out: 200 of 400, 128 of 257, 160 of 333"""
    rows = []
    for name, window in (("T400_default", 400), ("T400_default", 200), ("T333_seg2", 400), ("T333_seg2", 160)):
        case = LINEAR[name]
        for k, a in running_tracks(case):
            s = so.system(case["points"][:, k], case["cov"][:, k], a)
            rows.append((f"smooth {name} track {k} window {window}", tso.window_cond(tso.data_blocks(s), a, window), so.cond(s)))
    for name, window in (("T257", 400), ("T333_seg2", 400)):
        case = tro.cases()[name]
        acc = np.broadcast_to(case["accel_std"], (case["start"].shape[1],))
        for k, ev in enumerate(tro.system_reference(name)):
            if ev is not None:
                rows.append((f"refine {name} track {k} window {window}", tso.window_cond(ev["H"], acc[k], window), so.cond(dict(A=ev["A"]))))
    c = eo.cases()["T257_seg3"]
    s = so.system(c["points"][:, 0], c["cov"][:, 0], eo.A_TRUE)
    rows.append(("evidence T257_seg3", tso.window_cond(tso.data_blocks(s), eo.A_TRUE), so.cond(s)))
    for what, wc, full in rows:
        print(f"{what}: window cond {wc:.4g}, dense cond {full:.4g}")
        assert wc >= 0.5 * full, (what, wc, full)


@pytest.mark.parametrize("name", sorted(eo.cases()))
def test_evidence_float64_route_against_the_longdouble_route(name):
    case = eo.cases()[name]
    K = case["points"].shape[1]
    for k in range(K):
        wk = None if case["weights"] is None else case["weights"][:, k]
        t = eo.Track(case["points"][:, k], case["cov"][:, k], wk)
        if not t.runs:
            continue
        for a in eo.EVAL_AT:
            ref, r = eo.reference((name, k, float(a)), case["points"][:, k], case["cov"][:, k], a, wk), tso.evidence_reference(t, a)
            assert r["cond"] == ref["cond"] or r["cond"] >= 0.5 * ref["cond"]
            assert abs(r["S"] - ref["S"]) <= 1e-9 * ref["S"] and r["N"] == t.neg2(a)
            for f in ("N", "data", "penalty", "log_det"):
                assert abs(r[f] - ref[f]) <= Q * ref["bars"][f], (name, k, a, f, r[f], ref[f], ref["bars"][f])


def test_evidence_float64_route_at_1301_frames_segment_two():
    """the shape of the GPU tier's second evidence case: Track's float64 terms within a quarter of evidence_oracle.bars of terms_banded (np.longdouble)"""
    case, a = tso.evidence_case(), eo.A_TRUE
    t0 = time.time()
    for k in (0, 2):
        ref = eo.reference(("T1301", k, float(a)), case["points"][:, k], case["cov"][:, k], a)
        r = tso.evidence_reference(eo.Track(case["points"][:, k], case["cov"][:, k]), a)
        fr = {f: abs(r[f] - ref[f]) / ref["bars"][f] for f in ("N", "data", "penalty", "log_det")}
        print(f"T1301 track {k}: dense cond {ref['cond']:.4g}, window cond {r['cond']:.4g}, float64 against longdouble, of the bars: {fr}")
        assert max(fr.values()) <= Q and r["cond"] >= 0.5 * ref["cond"]
    assert not eo.Track(case["points"][:, 1], case["cov"][:, 1]).runs
    print(f"references: {time.time() - t0:.1f} s")


@pytest.mark.parametrize("name", sorted(tro.cases()))
def test_refinement_routes_against_the_dense_oracle(name):
    case = tro.cases()[name]
    acc = np.broadcast_to(case["accel_std"], (case["start"].shape[1],))
    for k, ev in enumerate(tro.system_reference(name)):
        if ev is None:
            continue
        tc, x = tro.track_inputs(case, k), case["start"][:, k]
        r = tso.refine_evaluate(x, tc)
        assert np.array_equal(r["H"], ev["H"]) and r["data"] == ev["data"] and r["pen"] == ev["pen"]
        assert (np.abs(r["G"] - ev["G"]) <= Q * 1e-12 * ev["S"]).all() and (np.abs(r["S"] - ev["S"]) <= 1e-12 * ev["S"]).all(), (name, k)
        assert np.allclose(so.banded_to_dense(tso.banded(ev["H"], acc[k])), ev["A"], rtol=0, atol=4 * EPS * np.abs(ev["A"]).max())   # (einsum's H is symmetric to rounding only)
        d, cnd, own = tso.refine_step(ev["H"], ev["G"], acc[k])
        full = so.cond(dict(A=ev["A"]))
        bar = so.BAR_K * EPS * full * np.abs(ev["d"]).max()
        assert np.abs(d - ev["d"]).max() <= Q * bar and own <= Q * bar and cnd >= 0.5 * full, (name, k, np.abs(d - ev["d"]).max(), own, bar)
    T = case["start"].shape[0]
    P, y = tro.penalty_matrix(T), np.random.default_rng(1).standard_normal((T, 3))
    assert np.allclose(tso.penalty_apply(y), P @ y, rtol=0, atol=64 * EPS * np.abs(y).max()) and np.allclose(tso.penalty_apply(y, True), np.abs(P) @ np.abs(y), rtol=1e-14, atol=0)


@pytest.mark.parametrize("name", sorted(sto.cases()))
def test_skeleton_routes_against_the_dense_oracle(name):
    """the evaluation, the two operators, the sparse condition number and the matrix-free conjugate gradients against skeleton_trajectory_oracle's
    dense matrices (unknowns ordered (frame, running track, coordinate)); the step of the recurrence by check_system's own bar, a quarter of it"""
    case, ev = sto.cases()[name], sto.system_reference(name)
    run, apar = ev["run"], ev["apar"]
    idx = np.flatnonzero(run)
    x = np.where(run[None, :, None], case["start"], 0.0)
    r = tso.skeleton_evaluate(x, case)
    T = x.shape[0]
    for f in ("H", "u", "r"):
        assert np.array_equal(r[f], ev[f], equal_nan=True), (name, f)
    assert (r["data"], r["pen"], r["bone"]) == (ev["data"], ev["pen"], ev["bone"])
    assert (np.abs(r["G"][:, run] - ev["G"][:, run]).max(axis=(1, 2)) <= Q * 1e-12 * ev["S"][:, run].max(axis=(1, 2))).all() and np.allclose(r["S"][:, run], ev["S"][:, run], rtol=1e-12, atol=0)
    op = tso.SkeletonOperators(r["H"], r["u"], case, run, apar)
    flat = lambda v: v[:, idx].ravel()
    v = np.where(run[None, :, None], np.random.default_rng(2).standard_normal(x.shape), 0.0)
    scale = np.abs(ev["A"]).sum(1).max() * np.abs(v).max()
    assert np.abs(flat(op.A(v)) - ev["A"] @ flat(v)).max() <= 64 * EPS * scale and np.abs(flat(op.M(v)) - ev["M"] @ flat(v)).max() <= 64 * EPS * scale, name
    mi, mcond = np.linalg.solve(ev["M"], flat(v)), so.cond(dict(A=ev["M"]))
    assert np.abs(flat(op.Minv(v)) - mi).max() <= so.BAR_K * EPS * mcond * np.abs(mi).max(), name
    if run.all():
        sc = tso.sparse_cond(tso.skeleton_matrix(r["H"], r["u"], case, apar))
        assert abs(sc - ev["cond"]) <= 1e-6 * ev["cond"] and abs(tso.skeleton_window_cond(r["H"], r["u"], case, apar) - sc) <= 1e-6 * sc, (name, sc, ev["cond"])
    G = np.where(run[None, :, None], r["G"], 0.0)
    d, it, res = tso.pcg(op, G, sto.CG_TOL)
    dref = ev["d"][:, idx].ravel()
    ed = sto.a_norm(ev["A"], flat(d) - dref) / sto.a_norm(ev["A"], dref)
    bar = 2 * sto.CG_TOL * np.sqrt(ev["kappa"]) + 100 * EPS * ev["cond"]
    print(f"{name}: matrix-free CG {it} iterations to {res:.3g}, step {ed:.3g} in the A norm (bar {bar:.3g}), true residual {op.relative_residual(G, d):.3g}")
    assert ed <= Q * bar and it < tso.CG_MAX and res <= sto.CG_TOL
    rd = -(flat(G) + ev["A"] @ flat(d))
    true = float(np.sqrt(rd @ np.linalg.solve(ev["M"], rd) / (flat(G) @ np.linalg.solve(ev["M"], flat(G)))))
    assert abs(op.relative_residual(G, d) - true) <= Q * (2 * sto.CG_TOL + 100 * EPS * ev["cond"]), (name, op.relative_residual(G, d), true)
    assert abs(it - sto.pcg_iterations(ev["A"], ev["M"], G[:, idx].ravel(), tols=(sto.CG_TOL,))[0]) <= 1   # (an iteration's difference is round-off)


# ---------------------------------------------------------------- the long and the wide scenes themselves
def test_the_shapes_reach_what_they_were_chosen_for():
    T = tso.T_LONG
    assert T % 2 == 1 and tso.eval_blocks(T) >= 258   # (ceil(T / 256): smooth_eval_blocks of mcba_smooth_math.h, which smoothing_oracle.plan does not carry)
    assert len(so.plan(T, so.SEGMENT_DEFAULT, 2)) == 4 and len(so.plan(T, 2, 2)) == 10
    assert tso.evidence_lanes(T, so.SEGMENT_DEFAULT) == 2065 > 256 and tso.evidence_lanes(tso.T_EV, 2) == 329 > 256 and len(so.plan(tso.T_EV, 2, 3)) == 6
    assert (tso.T_SK * tso.K_SK + 255) // 256 == 301 >= 300
    assert so.expected_chunks(tso.T_W, tso.K_W, 3, 1.5 * so.chunk_doubles(tso.T_W, 1, 3, "smooth") * 8 / 1048576.0, "smooth")[:2] == (1, 131)
    assert tro.expected_chunks(tso.T_W, tso.K_W, 3, 3, 7.5 * tro.chunk_doubles(tso.T_W, 1, 3, 3) * 8 / 1048576.0)[:2] == (7, 19) and tso.K_W - 18 * 7 == 5
    L = tso.long_scene()
    us = np.isfinite(L["points"][:, :, 0])
    assert us.sum(0).tolist() == [T - 40 - 1 - 11] * 2 and not us[100:140].any() and not us[65990:].any() and not us[30000].any()


def test_long_smoother_and_evidence_references_are_better_than_a_quarter_of_the_bar():
    t0 = time.time()
    for weighted in (False, True):
        for k, r in enumerate(tso.long_smooth_reference(weighted)):
            bar = so.BAR_K * EPS * r["cond"] * np.abs(r["x"]).max()
            print(f"L {'weighted' if weighted else 'linear'} track {k}: window cond {r['cond']:.4g}, the reference's own error {r['ref_err']:.3g}, bar {bar:.3g}")
            assert r["ref_err"] <= Q * bar
            s = r["sysd"]
            us = s["usable"]
            d2, d2l = so.mahalanobis2(r["x"], s)[us], tso.mahalanobis2_ld(r["x"], s)[us]
            worst = float((np.abs(d2 - d2l) / tso.d2_bar(d2l, r["cond"])).max())
            print(f"    mahalanobis2 in float64 against np.longdouble: {float((np.abs(d2 - d2l) / d2l).max()):.3g} relative, {worst:.3g} of its bar; smallest d2 {d2.min():.3g}")
            assert 4 * worst <= 1.0
    t1 = time.time()
    for a in eo.EVAL_AT:
        for k, r in enumerate(tso.long_evidence_reference(a)):
            bar = so.BAR_K * EPS * r["cond"] * np.abs(r["x"]).max()
            print(f"L evidence a = {a} track {k}: window cond {r['cond']:.4g}, the reference's own error {r['ref_err']:.3g}, bar {bar:.3g}")
            assert r["ref_err"] <= Q * bar
    print(f"references: smoother (both sets of weights) {t1 - t0:.1f} s, evidence (three a) {time.time() - t1:.1f} s")


def test_long_refinement_reference_is_better_than_a_quarter_of_the_bar():
    t0 = time.time()
    case = tso.long_refine_case()
    nus, nsg, status = tro.counts(case)
    assert (status == 1).all() and (nsg >= 40).all()
    views = (~np.isnan(case["uvs"]).any(-1)).sum(0)
    assert (views[150:190] == 1).all() and (views[250:260] == 0).all()
    for k in range(2):
        tc = tro.track_inputs(case, k)
        ev = tso.refine_evaluate(case["start"][:, k], tc)
        d, cnd, own = tso.refine_step(ev["H"], ev["G"], tc["accel_std"])
        bar = so.BAR_K * EPS * cnd * np.abs(d).max()
        print(f"refine track {k}: window cond {cnd:.4g}, the reference's own error {own:.3g}, bar {bar:.3g}")
        assert own <= Q * bar
    print(f"references: {time.time() - t0:.1f} s")


def test_long_skeleton_oracle_converges_in_half_the_cap():
    t0 = time.time()
    case = tso.long_skeleton_case()
    ev = tso.skeleton_evaluate(case["start"], case)
    assert ev["run"].all() and (ev["apar"] >= 0).sum() == 6
    views = (~np.isnan(case["uvs"]).any(-1)).sum(0)
    assert (views[150:190, 1] == 1).all() and (views[250:260, 6] == 0).all()
    op = tso.SkeletonOperators(ev["H"], ev["u"], case, ev["run"], ev["apar"])
    d, it, res = tso.pcg(op, ev["G"], sto.CG_TOL)
    hist = []
    tso.pcg(op, ev["G"], sto.CG_TOL / 2, history=hist)
    lo, own, hi = tso.count_band(hist, sto.CG_TOL)
    print(f"skeleton: counts allowed {lo} .. {hi} around the oracle's {own}")
    assert own == it and lo <= own <= hi < tso.CG_MAX and hi - lo <= 4   # (a band that wide would guard nothing)
    cnd = tso.skeleton_window_cond(ev["H"], ev["u"], case, ev["apar"])
    true = op.relative_residual(ev["G"], d)
    print(f"skeleton: the oracle's CG {it} iterations to {res:.3g} (true residual {true:.3g}), window cond {cnd:.4g}; {time.time() - t0:.1f} s")
    assert 2 * it <= tso.CG_MAX and res <= sto.CG_TOL and true <= Q * (2 * sto.CG_TOL + 100 * EPS * cnd)


def test_wide_scene_is_decided_for_the_oracle_itself():
    """the cap of the robust tests, 10 left_out <= total, by the oracle alone; three distinct iteration counts or more among the running tracks;
    smoothing_oracle.check_robust passes on the oracle's own results, so the GPU tier's check can be met"""
    t0 = time.time()
    left_out, total, counts = tso.wide_smooth_oracle()
    print(f"W: {left_out} of {total} tracks undecided for the oracle, iteration counts {sorted(counts)}")
    assert total == 129 and 10 * left_out <= total and len(counts) >= 3
    case = tso.wide_smooth_case()
    res = [so.robust_reference(f"W_{k}", tso.wide_track(case, k))[0] if k not in (64, 65) else so.irls(case["points"][:, k], case["cov"][:, k], case["accel_std"][k], loss="soft_l1") for k in range(tso.K_W)]
    n = max(r["n_iterations"] for r in res)
    hist = np.full((n, tso.K_W, 2), np.nan)
    for k, r in enumerate(res):
        hist[:r["n_iterations"], k] = r["history"]
    got = dict({f: np.stack([r[f] for r in res], axis=1) for f in ("points", "weights", "mahalanobis2")}, history=hist, **{f: np.array([r[f] for r in res]) for f in ("status", "n_usable", "n_iterations")})
    assert tso.check_wide_smooth(case, got) == (0, 129)
    rc = tso.wide_refine_case()
    nus, nsg, status = tro.counts(rc)
    assert nus[64:67].tolist() == [0, 1, 2] and status[64:67].tolist() == [-1, -1, 1] and (status == 1).sum() == 129
    print(f"references: {time.time() - t0:.1f} s")
