"""tests/smoothing_oracle.py against itself: what the host-check and GPU tiers of smooth_trajectories are held to is right before anything is
held to it."""
import numpy as np

import smoothing_oracle as so


def test_banded_equals_dense():
    for T in (1, 2, 3, 4, 7, 30):
        s = so.scene(T, 1, seed=T, gaps=[(2, 4)] if T > 6 else [])
        w = np.random.default_rng(T).uniform(0.1, 1.0, T)
        d = so.system(s["points"][:, 0], s["cov"][:, 0], 0.07, w)
        assert np.allclose(so.banded_to_dense(d["ab"]), d["A"], rtol=1e-15, atol=0)
        if d["usable"].sum() >= 2:
            x = np.linalg.solve(d["A"], d["b"]).reshape(-1, 3)
            assert np.abs(so.solve(d) - x).max() <= 100 * so.EPS * so.cond(d) * np.abs(x).max()


def test_points_linear_in_time_come_back_unchanged():
    rng = np.random.default_rng(1)
    T = 40
    line = rng.standard_normal(3) + np.arange(T)[:, None] * rng.standard_normal(3)
    cov = so.random_cov(T, 1, rng)[:, 0]
    for a in (1e-3, 1.0):
        o = so.irls(line, cov, a)
        assert np.abs(o["points"] - line).max() <= 1e-9 * np.abs(line).max() and o["cost"] <= 1e-12


def test_loose_smoothness_returns_the_points():
    s = so.scene(50, 1, seed=2)
    o = so.irls(s["points"][:, 0], s["cov"][:, 0], 1e6)
    assert np.abs(o["points"] - s["points"][:, 0]).max() <= 1e-9


def test_a_gap_is_the_cubic_and_an_end_is_the_line():
    """tight data (sigma 1e-6) on a cubic in time: inside a gap the smoother's cubic through the neighbours is that cubic; past the last usable
    frame it continues the line of the last two frames' fit"""
    T = 40
    t = np.arange(T, dtype=np.float64)
    cubic = np.stack([1e-3 * t ** 3 - 0.02 * t ** 2 + t, 0.5 * t, 2.0 + 0 * t], axis=1)
    pts = cubic.copy()
    pts[15:22] = np.nan
    pts[34:] = np.nan
    cov = np.broadcast_to(np.eye(3) * 1e-12, (T, 3, 3))
    o = so.irls(pts, cov, 1.0)
    x = o["points"]
    # natural cubic spline through the usable frames: compare with scipy's
    from scipy.interpolate import CubicSpline
    us = np.isfinite(pts[:, 0])
    cs = CubicSpline(t[us][t[us] < 34], cubic[us][t[us] < 34], bc_type="natural")
    assert np.abs(x[15:22] - cs(t[15:22])).max() <= 1e-4
    end = x[33] + (t[34:, None] - 33.0) * (x[34] - x[33])
    assert np.abs(x[34:] - end).max() <= 1e-8 and np.abs(np.diff(x[32:], 2, axis=0)[1:]).max() <= 1e-8


def test_the_irls_objective_never_rises():
    for name, case in so.robust_cases().items():
        for k, o in enumerate(so.robust_reference(name, case)):
            h = o["history"][:, 0]
            assert (h[1:] <= h[:-1] * (1 + 1e-12)).all(), (name, k)
            assert so.further_step(o["points"], case, k) < 10 * 1e-8 * np.abs(o["points"]).max()
            assert so.decided(o), (name, k)


def test_robust_losses_beat_the_raw_points_and_the_linear_loss_does_not():
    s = so.outlier_scene()
    c = s["clean"][:, 0]

    def rms(x):
        return float(np.sqrt(np.mean(np.sum((x - s["truth"][:, 0])[c] ** 2, axis=1))))

    raw = rms(s["points"][:, 0])
    got = {loss: rms(so.irls(s["points"][:, 0], s["cov"][:, 0], s["accel_std"], loss=loss)["points"]) for loss in so.LOSSES}
    print(raw, got)
    assert got["soft_l1"] < raw and got["huber"] < raw and got["linear"] > raw


def test_unusable_frames_and_short_tracks():
    s = so.linear_cases()["bad_cov"]
    us = so.prepare(s["points"][:, 0], s["cov"][:, 0])[0]
    assert not us[[7, 8, 15]].any() and us.sum() == 27
    one = so.linear_cases()["one_usable"]
    o = so.irls(one["points"][:, 1], one["cov"][:, 1], 0.1)
    assert o["status"] == so.STATUS_TOO_FEW and o["n_usable"] == 1 and np.isnan(o["points"]).all()
