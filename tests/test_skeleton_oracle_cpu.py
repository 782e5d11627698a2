"""tests/skeleton_oracle.py against itself and scipy: its loop reaches scipy least_squares' minimiser on the scenes, stays inside the cap of
undecided frames on the loop scenes and stops every frame before max_iterations; the dense matrix is the Jacobian's; and what the bones gain on
the issue's scene (4 cameras, a random tree of 12 keypoints, 60 frames, 0.5 px noise, 35 % of the detections dropped, bones of 8 .. 30 mm known to
0.5 mm), as inequalities -- the measured values are in SURVEY.md section 8f-22."""
import numpy as np

import skeleton_oracle as sko


def test_the_loop_reaches_scipys_minimiser():
    worst = 0.0
    for name in ("K2", "K3_chain", "two_pieces", "C2", "special"):
        case, cls = sko.cases()[name], sko.statuses(name)
        for t, o in enumerate(sko.reference(name)):
            if o is None or o["status"] == sko.NOTHING or t >= 5:
                continue
            x, cost = sko.scipy_minimiser(case, t, cls[t], o["points"])
            act = cls[t] > 0
            worst = max(worst, np.abs(x[act] - o["points"][act]).max())
            assert abs(cost - o["cost"]) <= 1e-9 * max(1.0, cost), (name, t, cost, o["cost"])
            assert np.abs(x[act] - o["points"][act]).max() < 1e-4, (name, t)   # (mm: ten thresholds xtol max|x| of the loop, and scipy's own stopping distance)
    print(f"largest distance from scipy's minimiser {worst:.3g} mm")


def test_the_loop_scenes_stay_inside_the_cap_and_stop_before_the_limit():
    left_out = total = 0
    for name in sko.LOOP_CASES:
        for o in sko.reference(name):
            if o is None or o["status"] == sko.NOTHING:
                continue
            total += 1
            left_out += not sko.decided(o)
            assert o["status"] == sko.CONVERGED and o["n_iterations"] < o["max_iterations"], name
            costs = [o["cost_start"]] + [h[0] for h in o["history"]]
            assert all(b <= a for a, b in zip(costs, costs[1:])) and o["cost"] == costs[-1], name
    print(f"undecided frames of the oracle alone {left_out} of {total}")
    assert 10 * left_out <= total, (left_out, total)


def test_the_dense_matrix_is_the_gauss_newton_matrix_of_the_residuals():
    """J^T J of the frame's residual vector (finite differences) against the matrix assembled from blocks and directions, linear loss"""
    name = "two_pieces"
    case, cls = sko.cases()[name], sko.statuses(name)
    for t in range(3):
        act = cls[t] > 0
        x = np.array(case["start"][t])
        ev = sko.evaluate(x, t, act, case, 0.0)
        idx = ev["idx"]

        def res(v):
            y = x.copy()
            y[idx] = v.reshape(-1, 3)
            C = len(case["ext"])
            sw = np.sqrt(case["weff"][:, t])
            uv = np.stack([case["uvs"][c][t] for c in range(C)])
            seen = ~np.isnan(uv).any(-1) & act[None]
            proj = np.stack([sko.ks.project5(np.nan_to_num(y), case["ext"][c], *case["intr"][c]) for c in range(C)])
            return np.r_[(np.where(seen[..., None], uv - proj, 0.0) * sw[..., None])[seen].ravel(), [b[3] for b in sko.bone_terms(y, act, case)]]

        v0, h = x[idx].ravel(), 1e-5
        J = np.stack([(res(v0 + h * e) - res(v0 - h * e)) / (2 * h) for e in np.eye(len(v0))], axis=1)
        assert np.abs(J.T @ J - ev["M"]).max() <= 1e-6 * np.abs(ev["M"]).max(), (t, np.abs(J.T @ J - ev["M"]).max())
        assert np.abs(J.T @ res(v0) - ev["G"][idx].ravel()).max() <= 1e-6 * np.abs(ev["S"][idx]).max()


def test_activity_rules():
    cls = sko.statuses("special")
    assert list(cls[0]) == [2, -1, 2, 2, 2, 2, 2] and list(cls[1]) == [2, 2, -1, -2, 2, 2, -2] and list(cls[5]) == [2, 2, 2, 2, 2, -1, 2]
    assert (sko.statuses("C1") == sko.NO_ANCHOR).all()


def test_what_the_bones_gain():
    """single-view keypoints come back finite with an RMS error below the bone length; the RMS error of the keypoints two cameras or more see is not
    above the per-keypoint fit's"""
    s = sko.make_scene(4, 60, sko.random_tree(12, 81), 12, seed=81, noise=0.5, p_drop=0.35, bone_jitter=0.5, max_single=None)
    case = sko.make_case(s, bone_std=0.5, pixel_std=0.5, start_noise=0.3, seed=81)
    cls, views = sko.classes(case)
    T, K = cls.shape
    P = T * K
    uv = [np.asarray(case["uvs"][c]).reshape(P, 2) for c in range(4)]
    alone = sko.wo.refine_direct(case["truth"].reshape(P, 3), uv, case["ext"], case["intr"], case["weff"].reshape(4, P), "linear", 3.0).reshape(T, K, 3)
    joint = np.stack([sko.lm(case, t, cls[t], max_iterations=100)["points"] for t in range(T)])
    usable, single = cls == sko.USABLE, cls == sko.SINGLE
    rms = lambda x, m: float(np.sqrt(((x[m] - case["truth"][m]) ** 2).sum(-1).mean()))
    print(f"usable keypoints {int(usable.sum())}: RMS error {rms(alone, usable):.4f} mm each alone, {rms(joint, usable):.4f} mm with the bones; "
          f"single-view keypoints {int(single.sum())}: RMS error {rms(joint, single):.4f} mm (NaN alone); without an anchor {int((cls == sko.NO_ANCHOR).sum())}")
    assert single.sum() > 20 and np.isfinite(joint[single]).all() and np.isnan(joint[cls < 0]).all()
    assert rms(joint, single) < case["bone_length"].min()
    assert rms(joint, usable) <= rms(alone, usable)
