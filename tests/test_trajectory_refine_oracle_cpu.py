"""tests/trajectory_refine_oracle.py alone: its derivatives against central differences, its loop by its own definition, what the joint fit gains
over the two-stage chain on the scenes of SURVEY.md section 8f-21, and that the cases of the other tiers keep the oracle's iteration counts
comparable."""
import numpy as np

import trajectory_refine_oracle as tro


def _noise_free(loss):
    s = tro.make_scene(3, 7, 2, seed=31, noise=0.0, p_drop=0.2, single=(3, 4))
    return tro.make_case(s, loss=loss, f_scale=2.0, pixel_std=np.array([0.5, 0.7, 0.4]), weights=tro.wo.draw_levels(3, 14, 77, (0.25, 1.0, 4.0)).reshape(3, 7, 2), start_noise=0.0)


def _data_cost(x, c):
    return tro.data_terms(x, c["uvs"], c["ext"], c["intr"], c["weff"], c["loss"], c["f_scale"])["cost"]


def test_gradient_against_central_differences():
    for loss in ("linear", "soft_l1", "huber"):
        c = _noise_free(loss)
        x = c["truth"] + np.random.default_rng(1).normal(0, 0.5, c["truth"].shape)   # residuals of a few pixel_std: both branches of huber
        d = tro.data_terms(x, c["uvs"], c["ext"], c["intr"], c["weff"], loss, c["f_scale"])
        h = 1e-5
        for e in range(3):
            dx = np.zeros(3)
            dx[e] = h
            num = (_data_cost(x + dx, c) - _data_cost(x - dx, c)) / (2 * h)
            assert np.abs(num - d["g"][..., e]).max() <= 1e-6 * max(1.0, np.abs(d["g"]).max()), (loss, e)
        assert (d["gabs"] >= np.abs(d["g"]) * (1 - 1e-12)).all()


def test_information_against_central_differences_of_the_gradient():
    """at residual-free detections the Hessian of the data term is its Gauss-Newton matrix, whatever the loss (rho' = 1, rho'' r^2 = 0 there)"""
    for loss in ("linear", "soft_l1", "huber"):
        c = _noise_free(loss)
        x = c["truth"]
        d = tro.data_terms(x, c["uvs"], c["ext"], c["intr"], c["weff"], loss, c["f_scale"])
        h = 1e-4
        for e in range(3):
            dx = np.zeros(3)
            dx[e] = h
            gp = tro.data_terms(x + dx, c["uvs"], c["ext"], c["intr"], c["weff"], loss, c["f_scale"])["g"]
            gm = tro.data_terms(x - dx, c["uvs"], c["ext"], c["intr"], c["weff"], loss, c["f_scale"])["g"]
            assert np.abs((gp - gm) / (2 * h) - d["H"][..., e]).max() <= 1e-5 * np.abs(d["H"]).max(), (loss, e)
        rank = np.linalg.matrix_rank(d["H"], tol=1e-9 * np.abs(d["H"]).max())
        assert np.array_equal(rank, np.where(d["views"] >= 2, 3, np.where(d["views"] == 1, 2, 0)))   # rank 2 on a single frame, 0 on an unseen one


def test_full_gradient_and_dense_matrix_are_the_objectives():
    c = tro.cases()["T3"]
    tc = tro.track_inputs(c, 0)
    x = np.array(c["start"][:, 0])
    ev = tro.evaluate(x, tc)
    h = 1e-5
    for t in range(3):
        for e in range(3):
            dx = np.zeros((3, 3))
            dx[t, e] = h
            num = (tro.objective(x + dx, tc) - tro.objective(x - dx, tc)) / (2 * h)
            assert abs(num - ev["G"][t, e]) <= 1e-5 * np.abs(ev["G"]).max()
    assert np.allclose(ev["A"] @ ev["d"].ravel(), -ev["G"].ravel(), rtol=0, atol=1e-9 * np.abs(ev["G"]).max())


def test_the_objective_never_rises_and_the_cases_keep_the_counts_comparable():
    undecided = total = 0
    for name in sorted(tro.cases()):
        for k, o in enumerate(tro.reference(name)):
            if o["status"] != tro.STATUS_OK:
                assert o["n_iterations"] == 0 and np.isnan(o["points"]).all()
                continue
            h = o["history"]
            assert (h[1:, 0] <= h[:-1, 0]).all() and o["n_iterations"] < 30, (name, k, h)
            assert tro.further_step(o["points"], tro.cases()[name], k) < 10 * 1e-8 * np.abs(o["points"]).max()
            total += 1
            undecided += not tro.decided(o)
    print(f"undecided tracks of the oracle alone: {undecided} of {total}")
    assert 10 * undecided <= total
    st = tro.counts(tro.cases()["T333_seg2"])[2]
    assert st[1] == tro.STATUS_TOO_FEW and st[3] == tro.STATUS_BAD_START and (st[[0, 2, 4]] == tro.STATUS_OK).all()


def _rms(x, truth, sl):
    return float(np.sqrt(np.mean(np.sum((x[sl] - truth[sl]) ** 2, axis=-1))))


def test_joint_fit_beats_the_two_stage_chain_inside_the_one_camera_stretch():
    """the measured pairs are quoted in SURVEY.md section 8f-21; only the inequality is asserted"""
    for name, case in (("stretch", tro.stretch_scene()), ("outliers", tro.outlier_scene())):
        two, _ = tro.two_stage(case)
        joint = tro.gauss_newton(dict(case, start=two), 0)
        assert joint["status"] == tro.STATUS_OK and (joint["history"][1:, 0] <= joint["history"][:-1, 0]).all()
        sl = slice(80, 120)
        a, b = _rms(two[:, 0], case["truth"][:, 0], sl), _rms(joint["points"], case["truth"][:, 0], sl)
        print(f"{name}: RMS inside the stretch two-stage {a:.3f} mm, joint {b:.3f} mm; whole track {_rms(two[:, 0], case['truth'][:, 0], slice(None)):.3f} / "
              f"{_rms(joint['points'], case['truth'][:, 0], slice(None)):.3f} mm; solves {joint['n_iterations']}")
        assert b < a
