"""The weighted paths of csrc/mcba_keypoint_math.h, csrc/mcba_tricov_math.h and csrc/mcba_kpba_math.h compiled with g++
(tests/hostcheck/weights_hostcheck.cpp, plain -O2) and held, without a GPU, to the cases and bars of the GPU tier (tests/test_gpu_weights*.py)
against tests/weights_oracle.py: the refinement within the gate of tests/test_gpu_keypoints.py (5e-6 mm), the covariance within
tricov_oracle.check_against_oracle and check_pooled, one evaluation of the extrinsics refinement within kpba_oracle.check_block and check_step, the
loop within kpba_oracle.check_result -- each on the virtual or the direct statement of the weighted problem.  No tolerance is set here."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import kpba_oracle as ko
import tricov_oracle as tco
import weights_oracle as wo

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck", "weights_hostcheck.cpp")
LOSSES = wo.LOSS_NAMES
GATE_MM = 5e-6   # tests/test_gpu_keypoints.py
MAX_NFEV = 200   # "outlier" (soft_l1, a quarter of the weights zero) takes 109 evaluations to the tight tolerances: the default 100 ends at status 0, 6e-10 above the optimum


def P(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


@pytest.fixture(scope="module")
def hc(tmp_path_factory):
    lib = str(tmp_path_factory.mktemp("weights_hostcheck") / "libweights_hostcheck.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-o", lib, SRC])
    h = ctypes.CDLL(lib)
    h.hc_w_refine.argtypes = [ctypes.c_int, ctypes.c_size_t] + [ctypes.c_void_p] * 5 + [ctypes.c_int, ctypes.c_double, ctypes.c_int] + [ctypes.c_void_p] * 2
    h.hc_w_tricov.argtypes = [ctypes.c_int, ctypes.c_size_t] + [ctypes.c_void_p] * 6 + [ctypes.c_int, ctypes.c_double, ctypes.c_double] + [ctypes.c_void_p] * 5
    h.hc_w_system.argtypes = [ctypes.c_int, ctypes.c_size_t] + [ctypes.c_void_p] * 6 + [ctypes.c_int, ctypes.c_double, ctypes.c_double] + [ctypes.c_void_p] * 8
    h.hc_w_kpba.argtypes = [ctypes.c_int, ctypes.c_size_t] + [ctypes.c_void_p] * 6 + [ctypes.c_int] * 3 + [ctypes.c_double] * 4 + [ctypes.c_int] + [ctypes.c_void_p] * 5 + [ctypes.c_int]
    return h


def planes(uvs, w):
    return np.ascontiguousarray(np.stack([np.asarray(u, dtype=np.float64) for u in uvs])), np.ascontiguousarray(w, dtype=np.float64)


def host_refine(hc, i, start=None):
    theta, d5 = tco.camera_blocks(i["ext"], i["intr"])
    uv, w = planes(i["uvs"], i["weights"])
    C, n = uv.shape[:2]
    start = np.ascontiguousarray(i["start"] if start is None else start)
    out, info = np.empty((n, 3)), np.empty((n, 4))
    assert hc.hc_w_refine(C, n, P(uv), P(w), P(theta), P(d5), P(start), LOSSES.index(i["loss"]), i["f_scale"], 100, P(out), P(info)) == 0
    return out, info


@pytest.mark.parametrize("name", list(wo.REFINE_CASES))
def test_refinement_reaches_the_oracle_minimiser(hc, name):
    i, o = wo.refine_case(name)
    got, info = host_refine(hc, i)
    ok = o["usable"]
    assert np.array_equal(np.isnan(got).any(1), ~ok) and np.all(info[~ok, 3] == -1) and np.all(info[ok, 3] == 1)
    diff = np.abs(got - o["points"])[ok].max()
    print(f"{name}: usable {ok.sum()} / {len(ok)}  max |dX| {diff:.3e} mm (gate {GATE_MM})")
    assert diff <= GATE_MM
    np.testing.assert_allclose(info[ok, 0], wo.robust_cost_direct(got, i["uvs"], i["ext"], i["intr"], i["weights"], i["loss"], i["f_scale"])[ok], rtol=1e-9, atol=1e-12)
    assert np.all(info[ok, 0] <= info[ok, 1])


def host_tricov(hc, i, with_cov=True, sigma=tco.SIGMA, weights=None, uvs=None):
    theta, d5 = tco.camera_blocks(i["ext"], i["intr"])
    uv, w = planes(i["uvs"] if uvs is None else uvs, i["weights"] if weights is None else weights)
    C, n = uv.shape[:2]
    pts = np.ascontiguousarray(i["points"])
    S = np.ascontiguousarray(i["camera_covariance"]) if with_cov else None
    det, cal, views, status, info = np.empty((n, 6)), np.empty((n, 6)) if with_cov else None, np.empty(n, np.int32), np.empty(n, np.int32), np.empty(8)
    assert hc.hc_w_tricov(C, n, P(pts), P(uv), P(w), P(theta), P(d5), P(S), LOSSES.index(i["loss"]), i["f_scale"], float("nan") if sigma is None else sigma ** 2, P(det), P(cal), P(views), P(status),
                          P(info)) == 0
    un = lambda a: None if a is None else a[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(-1, 3, 3)   # noqa: E731
    return dict(detection=un(det), calibration=un(cal), views=views, status=status, sigma2=float(info[0]), n_residuals=int(info[1]), n_free=int(info[2]), n_unusable=int(info[3]),
                n_degenerate=int(info[4]))


@pytest.mark.parametrize("name", list(wo.TRICOV_CASES))
def test_covariance_matches_the_oracle(hc, name):
    i, o = wo.tricov_case(name)
    tco.check_against_oracle(name, host_tricov(hc, i), o)
    tco.check_against_oracle(name + " (no camera covariance)", host_tricov(hc, i, with_cov=False), o, with_cov=False)


@pytest.mark.parametrize("name", wo.POOLED_CASES)
def test_pooled_sigma_matches_the_oracle(hc, name):
    i, o = wo.tricov_case(name)
    tco.check_pooled(name, host_tricov(hc, i, sigma=None), host_tricov(hc, i), o)


def test_the_two_statements_agree():
    """virtual cameras against the direct statement on a case with levels: the same usable points, the terms and sigma2 to 1e-13 relative"""
    i, o = wo.tricov_case("c6_p33")
    d = wo.uncertainty_direct(i["points"], i["uvs"], i["ext"], i["intr"], i["weights"], camera_covariance=i["camera_covariance"], sigma=None, loss=i["loss"], f_scale=i["f_scale"])
    v = wo.uncertainty_virtual(i["points"], i["uvs"], i["ext"], i["intr"], i["weights"], camera_covariance=i["camera_covariance"], sigma=None, loss=i["loss"], f_scale=i["f_scale"])
    ok = v["status"] == 1
    assert np.array_equal(v["status"], d["status"]) and np.array_equal(v["views"], d["views"])
    for k in ("detection", "calibration"):
        assert np.abs(v[k][ok] - d[k][ok]).max() <= 1e-13 * np.abs(d[k][ok]).max(), k
    assert abs(v["sigma2"] / d["sigma2"] - 1) <= 1e-13


def host_evaluation(hc, i, weights=None, uvs=None):
    theta, d5 = tco.camera_blocks(i["ext0"], i["intr"])
    uv, w = planes(i["uvs"] if uvs is None else uvs, i["weights"] if weights is None else weights)
    C, n = uv.shape[:2]
    NP = (6 * C + 15) // 16 * 16
    YY, acc, scal, status, trial, out3 = np.empty((NP, NP)), np.empty((C, 33)), np.empty(3), np.empty(n, np.int32), np.empty((n, 3)), np.empty(3)
    pts, hb = np.ascontiguousarray(i["pts0"]), ko.held_bits(i["held"])
    et, dth = (np.ascontiguousarray(a) for a in i["step"])
    assert hc.hc_w_system(C, n, P(uv), P(w), P(theta), P(d5), P(pts), P(hb), LOSSES.index(i["loss"]), i["f_scale"], i["lam"], P(et), P(dth), P(YY), P(acc), P(scal), P(status), P(trial), P(out3)) == 0
    return dict(YY=YY, acc=acc, cost=scal[0], count=scal[1], gmax=scal[2], tail=0.0, point_status=status, trial_points=trial, step4=np.r_[out3[0], out3[1], 0.0, out3[2]])


@pytest.mark.parametrize("name", list(wo.SYSTEM_CASES))
def test_one_evaluation_against_the_folded_block_oracle(hc, name):
    i, o = wo.system_case(name)
    wo.check_system(name, i, o, host_evaluation(hc, i))


def test_identities_of_one_evaluation(hc):
    """a 0/1 plane = the same mask written as NaN, bit for bit; a constant plane under the linear loss scales U, Y Y^T, g_c, Y z and the cost by
    w0 (a power of two: exactly) and leaves the point steps as they are"""
    i, o = wo.system_case("c3_p257")
    mask = i["weights"] > 0
    a = host_evaluation(hc, i, weights=mask.astype(np.float64))
    b = host_evaluation(hc, i, weights=np.ones_like(i["weights"]), uvs=wo.masked(i["uvs"], mask))
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    c = host_evaluation(hc, i, weights=4.0 * mask)
    assert np.array_equal(c["YY"], 4 * a["YY"]) and np.array_equal(c["acc"], 4 * a["acc"]) and c["cost"] == 4 * a["cost"] and c["gmax"] == 4 * a["gmax"]
    assert np.array_equal(c["trial_points"], a["trial_points"], equal_nan=True) and c["step4"][0] == 4 * a["step4"][0] and np.array_equal(c["step4"][1:], a["step4"][1:])


def host_loop(hc, i, o, **over):
    theta, d5 = tco.camera_blocks(i["ext0"], i["intr"])
    uv, w = planes(i["uvs"], over.pop("weights", i["weights"]))
    C, n = uv.shape[:2]
    pts0 = np.ascontiguousarray(i["pts0"])
    hb = ko.held_bits(o["held"])
    hb[o["held"].all(1)] = 0   # (the loop finds the gauge camera and the blind cameras itself)
    hb = np.ascontiguousarray(hb)
    ext, pts, status, res, hist = np.empty((C, 6)), np.empty((n, 3)), np.empty(n, np.int32), np.empty(8), np.zeros((MAX_NFEV + 8, 3))
    assert hc.hc_w_kpba(C, n, P(uv), P(w), P(theta), P(d5), P(pts0), P(hb), 0, o["scale_camera"], LOSSES.index(i["loss"]), 1.0, 1e-15, 1e-15, 1e-10, MAX_NFEV, P(ext), P(pts), P(status), P(res), P(hist),
                        len(hist)) == 0
    return dict(extrinsics=ext, points=pts, point_status=status, cost=res[0], cost0=res[1], status=int(res[5]), nfev=int(res[3]), held_bits=hb)


@pytest.mark.parametrize("name", list(wo.GOLDEN_CASES))
def test_host_loop_reaches_the_weighted_golden_optimum(hc, name):
    assert name in wo.pinned_cases(), f"{name} is not pinned in tests/golden/kpba_weighted.npz"
    i, o = wo.golden_case(name)
    got = host_loop(hc, i, o)
    print(f"{name}: status {got['status']} nfev {got['nfev']} cost {got['cost0']:.6g} -> {got['cost']:.15g}")
    assert np.array_equal(got["held_bits"], ko.held_bits(o["held"]))
    ko.check_result(name, got["extrinsics"], got["points"], got["cost"], o)
    assert got["cost"] <= got["cost0"] and got["status"] in (1, 2, 3)
    ref0, bound0 = wo.cost_virtual(i["ext0"], i["pts0"], i["uvs"], i["intr"], i["weights"], i["loss"])
    assert abs(got["cost0"] - ref0) <= bound0


def test_sanitized_stand_alone_program(tmp_path):
    """the three headers' weighted paths under AddressSanitizer + UBSan in a program of its own (its own main: 4 cameras x 11 points, zero and NaN
    weights, a camera that sees nothing, a point with one view of positive weight), run as a child process with the sanitizer runtime linked in"""
    exe = str(tmp_path / "weights_sanitized")
    subprocess.check_call(["g++", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-DWEIGHTS_MAIN", "-o", exe, SRC])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "weights hostcheck ok" in r.stdout
