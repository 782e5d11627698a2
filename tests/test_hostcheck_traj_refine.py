"""csrc/mcba_traj_refine_math.h -- the per-lane text of k_traj_count, k_traj_linearise, k_traj_trial and k_traj_apply, the accept and stop rule,
the chunk rule -- and the right-hand-side mode of csrc/mcba_smooth_math.h, compiled with g++ -O2 (tests/hostcheck/traj_refine_hostcheck.cpp:
serial loops over the lanes in the kernels' order and the Gauss-Newton loop of the C call) and held to tests/trajectory_refine_oracle.py
without a GPU, on the cases and by the rules of the GPU tier (tests/test_gpu_traj_refine.py)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import trajectory_refine_oracle as tro

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck", "traj_refine_hostcheck.cpp")
V = ctypes.c_void_p
CASES = tro.cases()
LOSSES = {"linear": 0, "soft_l1": 1, "huber": 2}
SYM = np.array([[0, 1, 2], [1, 3, 4], [2, 4, 5]])


def build(tmp_path_factory):
    lib = str(tmp_path_factory.mktemp("traj_refine_hostcheck") / "libtraj_refine_hostcheck.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", lib, SRC])
    h = ctypes.CDLL(lib)
    h.hc_refine_trajectories.argtypes = [ctypes.c_int, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, V, V, V, V, V, V, V, ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_double, ctypes.c_int] + [V] * 16
    h.hc_refine_chunks.argtypes = [ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double, V]
    h.hc_weight_box.argtypes = [V, V, ctypes.c_int] + [ctypes.c_size_t] * 6 + [V]
    h.hc_weight_box.restype = None
    return h


@pytest.fixture(scope="module")
def hc(tmp_path_factory):
    return build(tmp_path_factory)


def run(hc, case, system=False, lag=False, max_iterations=30, xtol=1e-8, weights="case", uvs=None):
    uv = np.ascontiguousarray(case["uvs"] if uvs is None else uvs, dtype=np.float64)
    C, T, K = uv.shape[:3]
    cam, dist = tro.tco.camera_blocks(case["ext"], case["intr"])
    w = case["weights"] if isinstance(weights, str) else weights
    w = None if w is None else np.ascontiguousarray(w, dtype=np.float64)
    ps = np.ascontiguousarray(np.broadcast_to(np.asarray(case["pixel_std"], dtype=np.float64), (C,)))
    acc = np.ascontiguousarray(np.broadcast_to(np.asarray(case["accel_std"], dtype=np.float64), (K,)))
    start = np.ascontiguousarray(case["start"])
    x, h6, g, d = (np.full((T, K, n), 7.0) for n in (3, 6, 3, 3))
    st, nu, ns, ni = (np.full(K, 7, np.int32) for _ in range(4))
    cost, dc, pc, tc, hist, info = np.full(K, 7.0), np.full(K, 7.0), np.full(K, 7.0), np.full((K, 4), 7.0), np.full((max_iterations, K, 3), 7.0), np.full(8, 7.0)
    c6, l9 = (np.full((T, K, 6), 7.0), np.full((T - 1, K, 9), 7.0)) if lag else (None, None)
    p = lambda a: None if a is None else a.ctypes.data
    rc = hc.hc_refine_trajectories(int(system), T, K, C, p(uv), p(cam), p(dist), p(w), p(ps), p(start), p(acc), LOSSES[case["loss"]], case["f_scale"], max_iterations, xtol, case["segment"] or 0,
                                   p(x), p(h6), p(st), p(nu), p(ns), p(ni), p(cost), p(hist), p(c6), p(l9), p(g), p(d), p(dc), p(pc), p(tc), p(info))
    assert rc == 0
    out = dict(information=h6[..., SYM], status=st, n_usable=nu, n_single=ns, levels=int(info[0]))
    if system:
        out.update(gradient=g, step=d, data_cost=dc, penalty_cost=pc, trial_costs=tc)
    else:
        out.update(points=x, n_iterations=ni, cost=cost, history=hist[:max(int(ni.max()), 1)])
        if lag:
            out.update(covariance=c6[..., SYM], lag_covariance=l9.reshape(T - 1, K, 3, 3))
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_one_evaluation_against_the_oracle(hc, name):
    got = run(hc, CASES[name], system=True)
    tro.check_system(name, got)
    if name == "T333_seg2":
        assert got["levels"] == 5


def test_loop_against_the_oracle(hc):
    left_out = total = 0
    for name in sorted(CASES):
        got = run(hc, CASES[name], lag=True)
        lo, ran = tro.check_loop(name, got)
        tro.check_covariance(name, got)
        left_out, total = left_out + lo, total + ran
    print(f"undecided tracks {left_out} of {total}")
    assert 10 * left_out <= total, (left_out, total)


def test_unit_weights_are_no_weights_and_unseen_is_unseen(hc):
    case = CASES["T333_seg2"]
    plain = run(hc, case, weights=None)
    ones = run(hc, case, weights=np.ones(case["uvs"].shape[:3]))
    assert all(np.array_equal(plain[f], ones[f], equal_nan=True) for f in ("points", "information", "history", "cost", "n_iterations", "status"))
    rng = np.random.default_rng(5)
    hit = rng.uniform(size=case["uvs"].shape[:3]) < 0.1
    w = np.array(case["weights"])
    w[hit] = np.where(rng.uniform(size=int(hit.sum())) < 0.5, 0.0, np.nan)
    uv = np.array(case["uvs"])
    uv[hit] = np.nan
    a, b = run(hc, case, weights=w), run(hc, case, uvs=uv)
    assert all(np.array_equal(a[f], b[f], equal_nan=True) for f in ("points", "information", "history", "cost", "n_iterations", "status", "n_usable", "n_single"))


CHUNK_SHAPES = [(T, 2) for T in (1, 2, 3, 257, 333)] + [(400, None), (5000, None)]


@pytest.mark.parametrize("T,segment", CHUNK_SHAPES)
def test_chunk_rule_against_the_oracle(hc, T, segment):
    check_chunk_rule(hc, T, segment)


def check_chunk_rule(hc, T, segment):
    """the tracks-per-chunk rule and the byte count of the C call (mcba_traj_refine_math.h) against the oracle's count, which holds the
    detection and weight planes: T C 3 doubles per track"""
    for K in (1, 5, 20):
        for C in (2, 6, 64):
            for cov, lag in ((0, 0), (1, 0), (1, 1)):
                for budget in (8192.0, 0.5, 0.2, 0.001):
                    out4 = np.full(4, 7.0)
                    assert hc.hc_refine_chunks(T, K, C, segment or 0, cov, lag, budget, out4.ctypes.data) == 0
                    want = tro.expected_chunks(T, K, C, segment, budget, bool(cov), bool(lag))
                    assert tuple(int(v) for v in out4) == want, (K, C, budget, out4, want)
    a, b = tro.chunk_doubles(T, 1, 6, segment or 16), tro.chunk_doubles(T, 1, 7, segment or 16)
    assert b - a == 3 * T


WEIGHT_BOXES = {"last track chunk": (0, 3, 3, 2), "frame chunk": (1, 2, 0, 5), "whole": (0, 3, 0, 5), "one element": (2, 1, 4, 1)}   # t0, tc, k0, kc


@pytest.mark.parametrize("box", sorted(WEIGHT_BOXES))
@pytest.mark.parametrize("weighted", [False, True])
def test_weight_box_against_numpy_slicing(hc, box, weighted):
    """kp_weight_box (mcba_keypoint_math.h), the one place the C calls form sqrt(w) / pixel_std: every sub-box they ask for -- a block of tracks
    (the narrower last chunk of a chunking by two), a block of frames, everything, one element -- is the numpy slice of the whole plane, bit for
    bit; a zero or NaN weight gives 0, no weights means w = 1"""
    C, T, K = 2, 3, 5
    t0, tc, k0, kc = WEIGHT_BOXES[box]
    ps = np.array([0.7, 3.0])
    w = None
    if weighted:
        w = np.resize(np.array([0.0, np.nan, 0.25, 4.0, 1.3, 0.6, 2.0]), (C, T, K))   # (30 of them: each value four times or more)
    ww = np.ones((C, T, K)) if w is None else w
    with np.errstate(invalid="ignore"):
        want = np.where(ww > 0, np.sqrt(ww) * (1.0 / ps)[:, None, None], 0.0)[:, t0:t0 + tc, k0:k0 + kc]
    out = np.full((C, tc, kc), 7.0)
    hc.hc_weight_box(None if w is None else w.ctypes.data, ps.ctypes.data, C, T, K, t0, tc, k0, kc, out.ctypes.data)
    assert np.array_equal(out, want)
