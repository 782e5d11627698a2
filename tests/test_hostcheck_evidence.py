"""csrc/mcba_smooth_evidence_math.h over csrc/mcba_smooth_math.h -- the per-lane text of k_evidence_logdet and k_evidence_eval, the tree of
k_evidence_final and the search rule of mcba_estimate_accel_std -- compiled with g++ -O2 (tests/hostcheck/evidence_hostcheck.cpp: serial loops
over the lanes in the kernels' order) and held to tests/evidence_oracle.py without a GPU, on the cases and to the bars of the GPU tier
(tests/test_gpu_accel_estimation.py).  After every elimination the harness overwrites each slot of the factor storage that holds no factor with
NaN: a log-determinant that stays finite has read none of them."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import evidence_oracle as eo
import smoothing_oracle as so

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck", "evidence_hostcheck.cpp")
V = ctypes.c_void_p
CASES = eo.cases()
FIELDS = ("neg2_log_evidence", "data", "penalty", "log_det")


@pytest.fixture(scope="module")
def hc(tmp_path_factory):
    lib = str(tmp_path_factory.mktemp("evidence_hostcheck") / "libevidence_hostcheck.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", lib, SRC])
    h = ctypes.CDLL(lib)
    h.hc_smooth_evidence.argtypes = [ctypes.c_size_t, ctypes.c_int, V, V, V, V, ctypes.c_int, V, V, V, V]
    h.hc_estimate_accel_std.argtypes = [ctypes.c_size_t, ctypes.c_int, V, V, ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_double, V, V, ctypes.c_int] + [V] * 9
    return h


def evidence(hc, case, a):
    pts = np.ascontiguousarray(case["points"], dtype=np.float64)
    T, K = pts.shape[:2]
    c6 = so.pack6(case["cov"])
    acc = np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float64), (K,)))
    w = None if case["weights"] is None else np.ascontiguousarray(case["weights"], dtype=np.float64)
    out4, st, nu, fills = np.full((K, 4), 7.0), np.full(K, 7, np.int32), np.full(K, 7, np.int32), np.zeros(1, np.int64)
    assert hc.hc_smooth_evidence(T, K, pts.ctypes.data, c6.ctypes.data, acc.ctypes.data, None if w is None else w.ctypes.data, case["segment"] or 0, out4.ctypes.data, st.ctypes.data, nu.ctypes.data,
                                 fills.ctypes.data) == 0
    return dict(zip(FIELDS, out4.T), status=st, n_usable=nu, fills=int(fills[0]))


def estimate(hc, case, accel_range, n_grid, rtol, pool=None):
    pts = np.ascontiguousarray(case["points"], dtype=np.float64)
    T, K = pts.shape[:2]
    c6 = so.pack6(case["cov"])
    w = None if case["weights"] is None else np.ascontiguousarray(case["weights"], dtype=np.float64)
    units = None if pool is None else np.ascontiguousarray(eo.units_of(pool, K), dtype=np.int32)
    acc, ls, nb = np.full(K, 7.0), np.full(K, 7.0), np.full(K, 7.0)
    ed, st, nu, nev = np.full(K, 7, np.int32), np.full(K, 7, np.int32), np.full(K, 7, np.int32), np.zeros(1, np.int32)
    grid, ng = np.full(n_grid, 7.0), np.full((n_grid, K), 7.0)
    rc = hc.hc_estimate_accel_std(T, K, pts.ctypes.data, c6.ctypes.data, accel_range[0], accel_range[1], n_grid, rtol, None if w is None else w.ctypes.data,
                                  None if units is None else units.ctypes.data, case["segment"] or 0, acc.ctypes.data, ls.ctypes.data, ed.ctypes.data, st.ctypes.data, nu.ctypes.data, grid.ctypes.data,
                                  ng.ctypes.data, nb.ctypes.data, nev.ctypes.data)
    assert rc == 0
    return dict(accel_std=acc, log_std=ls, edge=ed, status=st, n_usable=nu, grid=grid, neg2_log_evidence_grid=ng, neg2_log_evidence=nb, n_evaluations=int(nev[0]))


@pytest.mark.parametrize("name", sorted(CASES))
def test_one_evaluation_meets_the_bars_with_every_unfactored_slot_nan(hc, name):
    case = CASES[name]
    worst = 0.0
    for a in eo.EVAL_AT:
        got = evidence(hc, case, a)
        assert got["fills"] > 0
        worst = max(worst, eo.check_evaluation(name, case, a, got))
    print(f"{name}: the largest fraction of a bar {worst:.3g}")


@pytest.mark.parametrize("name,pool", [("T71_K5", None), ("T257_seg3", None), ("T71_K5", "all"), ("T71_K5", np.array([4, 9, 4, 9, 9]))], ids=["T71_K5", "T257", "pool_all", "pool_labels"])
def test_estimator_against_the_oracle(hc, name, pool):
    case = CASES[name]
    got = estimate(hc, case, eo.RANGE, 9, 1e-3, pool)
    undecided, units, wa, ws = eo.check_estimate(name, case, got, eo.RANGE, 9, 1e-3, pool)
    print(f"{name}: {undecided} of {units} units undecided; the largest fraction of the bar of log a {wa:.3g}, of the log_std interval {ws:.3g}")
    assert 10 * undecided <= units
    again = estimate(hc, case, eo.RANGE, 9, 1e-3, pool)
    assert all(np.array_equal(got[f], again[f], equal_nan=True) for f in ("accel_std", "log_std", "edge", "neg2_log_evidence_grid", "neg2_log_evidence"))


def test_weights_none_is_a_plane_of_ones(hc):
    case = dict(CASES["T13"])
    a = evidence(hc, case, 0.1)
    case["weights"] = np.ones(case["points"].shape[:2])
    b = evidence(hc, case, 0.1)
    assert all(np.array_equal(a[f], b[f]) for f in FIELDS)


def test_lower_edge(hc):
    s = eo.linear_scene(40, seed=1)
    case = dict(points=s["points"], cov=s["cov"], segment=2, weights=None)
    got = estimate(hc, case, (0.01, 1.0), 9, 1e-3)
    undecided, units, _, _ = eo.check_estimate("linear40", case, got, (0.01, 1.0), 9, 1e-3)
    assert undecided == 0 and got["edge"][0] == -1 and got["accel_std"][0] == 0.01 and np.isnan(got["log_std"][0]) and got["status"][0] == 1


def test_refused_pivot_at_every_candidate_is_status_minus_two(hc):
    """a range whose inverse squares are finite while six times them is not: every candidate's diagonal is infinite and its pivot refused"""
    case = CASES["T7"]
    got = estimate(hc, case, (1e-154, 1.1e-154), 3, 1e-3)
    assert got["status"][0] == -2 and np.isnan(got["accel_std"][0]) and np.isnan(got["log_std"][0]) and np.isnan(got["neg2_log_evidence_grid"]).all() and got["edge"][0] == 0
    e = evidence(hc, case, 1e-154)
    assert e["status"][0] == -2 and all(np.isnan(e[f][0]) for f in FIELDS)
