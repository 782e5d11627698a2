"""csrc/mcba_skeltraj_math.h -- the per-lane text of the kernels of csrc/mcba_skeltraj.hip, the scalars of the conjugate-gradient recurrence, the
byte count of the budget -- and smooth_resolve_lane of csrc/mcba_smooth_math.h, compiled with g++ -O2 (tests/hostcheck/skeltraj_hostcheck.cpp: serial
loops over the lanes in the kernels' order, the recurrence and the Gauss-Newton loop of the C call) and held to tests/skeleton_trajectory_oracle.py
without a GPU, on the cases and by the rules of the GPU tier (tests/test_gpu_skeleton_trajectories.py).  A case of its own: the re-solve from the
stored factors against the fresh elimination on the same right-hand side, within 4 eps cond max|x|."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import skeleton_trajectory_oracle as sto
import smoothing_oracle as so
import trajectory_refine_oracle as tro

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck", "skeltraj_hostcheck.cpp")
V = ctypes.c_void_p
CASES = sto.cases()
LOSSES = {"linear": 0, "soft_l1": 1, "huber": 2}
SYM = np.array([[0, 1, 2], [1, 3, 4], [2, 4, 5]])


@pytest.fixture(scope="module")
def hc(tmp_path_factory):
    lib = str(tmp_path_factory.mktemp("skeltraj_hostcheck") / "libskeltraj_hostcheck.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", lib, SRC])
    h = ctypes.CDLL(lib)
    h.hc_refine_skeleton_trajectories.argtypes = [ctypes.c_int, ctypes.c_size_t, ctypes.c_int, ctypes.c_int] + [V] * 10 + [ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_double, ctypes.c_double,
                                                                                                                   ctypes.c_int, ctypes.c_int] + [V] * 22
    return h


def run(hc, case, system=False, max_iterations=30, xtol=1e-8, cg_tol=sto.CG_TOL, cg_max=200, weights="case", uvs=None, resolve=False):
    uv = np.ascontiguousarray(case["uvs"] if uvs is None else uvs, dtype=np.float64)
    C, T, K = uv.shape[:3]
    cam, dist = sto.tco.camera_blocks(case["ext"], case["intr"])
    w = case["weights"] if isinstance(weights, str) else weights
    w = None if w is None else np.ascontiguousarray(w, dtype=np.float64)
    ps = np.ascontiguousarray(np.broadcast_to(np.asarray(case["pixel_std"], dtype=np.float64), (C,)))
    acc = np.ascontiguousarray(np.broadcast_to(np.asarray(case["accel_std"], dtype=np.float64), (K,)))
    parent, L, s, start = np.ascontiguousarray(case["parent"], dtype=np.int32), np.ascontiguousarray(case["L"]), np.ascontiguousarray(case["s"]), np.ascontiguousarray(case["start"])
    x, h6, g, d, u = (np.full((T, K, n), 7.0) for n in (3, 6, 3, 3, 3))
    st, nu, ns = (np.full(K, 7, np.int32) for _ in range(3))
    conv, nit, cgi = (np.full(1, 7, np.int32) for _ in range(3))
    cost, cost0, cgr, dc, pc, bc, tc, hist, br, info = (np.full(n, 7.0) for n in (1, 1, 1, 1, 1, 1, 4, (max_iterations, 4), (T, K), 8))
    rs = np.full((2, T, K, 3), 7.0) if resolve else None
    p = lambda a: None if a is None else a.ctypes.data
    rc = hc.hc_refine_skeleton_trajectories(int(system), T, K, C, p(uv), p(cam), p(dist), p(w), p(ps), p(start), p(acc), p(parent), p(L), p(s), LOSSES[case["loss"]], case["f_scale"], max_iterations,
                                            xtol, cg_tol, cg_max, case["segment"] or 0, p(x), p(h6), p(st), p(nu), p(ns), p(conv), p(nit), p(cost), p(cost0), p(hist), p(br), p(u), p(g), p(d),
                                            p(cgi), p(cgr), p(dc), p(pc), p(bc), p(tc), p(info), p(rs))
    assert rc == 0
    out = dict(information=h6[..., SYM], direction=u, status=st, n_usable=nu, n_single=ns, levels=int(info[0]), device_bytes=int(info[6]), resolve=rs)
    if system:
        out.update(gradient=g, step=d, cg_iterations=int(cgi[0]), cg_residual=float(cgr[0]), data_cost=float(dc[0]), penalty_cost=float(pc[0]), bone_cost=float(bc[0]), trial_costs=tc)
    else:
        out.update(points=x, converged=bool(conv[0]), n_iterations=int(nit[0]), cost=float(cost[0]), cost_start=float(cost0[0]), history=hist[:int(nit[0])], bone_residual=br)
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_one_evaluation_against_the_oracle(hc, name):
    case = CASES[name]
    got = run(hc, case, system=True)
    sto.check_system(name, got)
    C, T, K = case["weff"].shape
    assert got["device_bytes"] == sto.chunk_doubles(T, K, C, case["segment"]) * 8 and got["levels"] == len(so.plan(T, case["segment"] or so.SEGMENT_DEFAULT, K))


@pytest.mark.parametrize("name", sorted(CASES))
def test_loop_against_the_oracle(hc, name):
    sto.check_loop(name, run(hc, CASES[name]))


@pytest.mark.parametrize("name", sto.RESOLVE_CASES)
def test_the_resolve_agrees_with_a_fresh_elimination(hc, name):
    sto.check_resolve(name, run(hc, CASES[name], system=True, resolve=True))


def test_one_track_without_a_bone_is_one_iteration_on_the_tracks_own_step(hc):
    sto.check_one_track(run(hc, CASES["K1"], system=True))


def test_a_bone_of_zero_length_at_the_start_is_status_minus_three(hc):
    case = sto.coincident_case()
    sto.check_coincident(run(hc, case), run(hc, case, system=True))


def test_unit_weights_are_no_weights_and_unseen_is_unseen(hc):
    case = CASES["T71_seg2"]
    fields = ("points", "information", "history", "cost", "n_iterations", "status", "n_usable", "n_single", "bone_residual", "direction")
    plain, ones = run(hc, case, weights=None), run(hc, case, weights=np.ones(case["uvs"].shape[:3]))
    assert all(np.array_equal(plain[f], ones[f], equal_nan=True) for f in fields)
    rng = np.random.default_rng(5)
    hit = rng.uniform(size=case["uvs"].shape[:3]) < 0.1
    w = np.array(case["weights"])
    w[hit] = np.where(rng.uniform(size=int(hit.sum())) < 0.5, 0.0, np.nan)
    uv = np.array(case["uvs"])
    uv[hit] = np.nan
    a, b = run(hc, case, weights=w), run(hc, case, uvs=uv)
    assert all(np.array_equal(a[f], b[f], equal_nan=True) for f in fields)
