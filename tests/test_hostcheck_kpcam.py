"""csrc/mcba_kpcam_math.h -- the arithmetic of the camera-refinement kernels (csrc/mcba_kpcam.hip) and the Levenberg-Marquardt loop of the C ABI,
prior included -- compiled with g++ (tests/hostcheck/kpcam_hostcheck.cpp, plain -O2) and held, without a GPU, to the bars of the GPU tier
(tests/test_gpu_kpcam.py, tests/test_gpu_kpcam_system.py) against tests/golden/kpcam.npz (scipy, tests/kpcam_oracle.py) and block_system12."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import kpba_oracle as ko
import kpcam_oracle as kc

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck", "kpcam_hostcheck.cpp")
LOSSES = ("linear", "soft_l1", "huber", "cauchy", "arctan")


def P(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


@pytest.fixture(scope="module")
def hc(tmp_path_factory):
    lib = str(tmp_path_factory.mktemp("kpcam_hostcheck") / "libkpcam_hostcheck.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-o", lib, SRC])
    h = ctypes.CDLL(lib)
    h.hc_kpcam.argtypes = [ctypes.c_int, ctypes.c_size_t] + [ctypes.c_void_p] * 6 + [ctypes.c_int] * 3 + [ctypes.c_double] * 4 + [ctypes.c_int] + [ctypes.c_void_p] * 5 + [ctypes.c_int]
    h.hc_kpcam_system.argtypes = [ctypes.c_int, ctypes.c_size_t] + [ctypes.c_void_p] * 5 + [ctypes.c_int, ctypes.c_double, ctypes.c_double] + [ctypes.c_void_p] * 4
    h.hc_kpcam_step.argtypes = [ctypes.c_int, ctypes.c_size_t] + [ctypes.c_void_p] * 4 + [ctypes.c_int, ctypes.c_double, ctypes.c_double] + [ctypes.c_void_p] * 4
    h.hc_kpcam_prior_cost.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 4
    h.hc_kpcam_prior_cost.restype = ctypes.c_double
    return h


def cam_blocks(ext, theta6, intr):
    """cam12 (C, 12) and dist5 (C, 5) with k1, k2 from theta6"""
    _, d5 = kc.tco.camera_blocks(ext, kc.intr_of(theta6, intr))
    return np.ascontiguousarray(np.concatenate([np.asarray(theta6), np.asarray(ext)], axis=1)), np.ascontiguousarray(d5)


def host_refine(hc, i, held, scale_camera, ftol=1e-15, xtol=1e-15, gtol=1e-10, max_nfev=100):
    cam12, d5 = cam_blocks(i["ext0"], i["theta0"], i["intr"])
    uv = np.ascontiguousarray(np.stack([np.asarray(u, dtype=np.float64) for u in i["uvs"]]))
    C, n = uv.shape[:2]
    pts0 = np.ascontiguousarray(i["pts0"], dtype=np.float64)
    hb = kc.held_bits12(held)
    pw = None if i["prior_std"] is None else np.ascontiguousarray(1.0 / i["prior_std"] ** 2)
    cams, pts, status, res, hist = np.empty((C, 12)), np.empty((n, 3)), np.empty(n, np.int32), np.empty(9), np.zeros((max_nfev + 8, 3))
    assert hc.hc_kpcam(C, n, P(uv), P(cam12), P(d5), P(pts0), P(hb), P(pw), 0, scale_camera, LOSSES.index(i["loss"]), 1.0, ftol, xtol, gtol, max_nfev, P(cams), P(pts), P(status), P(res), P(hist),
                       len(hist)) == 0
    return dict(extrinsics=cams[:, 6:], theta6=cams[:, :6], points=pts, point_status=status, cost=res[0], cost0=res[1], optimality=res[2], nfev=int(res[3]), njev=int(res[4]), status=int(res[5]),
                scale=res[6], history=hist[:int(res[7])], prior_cost=res[8], held_bits=hb)


def test_the_focal_only_linear_cases_are_pinned():
    assert {"three_focal", "six_focal"} <= set(kc.stored_cases(pinned=True))


@pytest.mark.parametrize("name", kc.stored_cases())
def test_host_loop_reaches_the_golden_optimum(hc, name):
    i, o = kc.case(name)
    held_in = o["held"].copy()
    held_in[0, 6:] = False   # (the gauge camera's extrinsics: the call's to hold)
    got = host_refine(hc, i, held_in, o["scale_camera"], max_nfev=1000)
    print(f"{name}: status {got['status']} nfev {got['nfev']} njev {got['njev']} optimality {got['optimality']:.3g} scale {got['scale']:.15g} prior {got['prior_cost']:.6g} (golden {o['prior_cost']:.6g})")
    assert np.array_equal(got["held_bits"], kc.held_bits12(o["held"]))
    kc.check_result12(name, got["extrinsics"], got["theta6"], got["points"], got["cost"], o)
    assert got["cost"] <= got["cost0"] and got["status"] in (0, 1, 2, 3)
    # the stated cost is the objective at the returned values (the rescale changes no projection)
    X = np.where(np.isnan(got["points"]), i["pts0"], got["points"])
    ref = ko.cost_of(got["extrinsics"], X, i["uvs"], kc.intr_of(got["theta6"], i["intr"]), i["loss"]) + kc.prior_cost(got["theta6"], i["theta0"], i["prior_std"], o["held"])
    assert abs(ref / got["cost"] - 1) <= 1e-10


def host_evaluation(hc, i):
    """one evaluation of the host build at an input of kpcam_oracle.system_case, in the keys of geometry.refine_cameras_system"""
    cam12, d5 = cam_blocks(i["ext0"], kc.theta6_of(i["intr"]), i["intr"])
    uv = np.ascontiguousarray(np.stack(i["uvs"]))
    C, n = uv.shape[:2]
    NP = (12 * C + 15) // 16 * 16
    YY, acc, scal, status, trial, out3 = np.empty((NP, NP)), np.empty((C, 102)), np.empty(3), np.empty(n, np.int32), np.empty((n, 3)), np.empty(3)
    pts, hb, loss = np.ascontiguousarray(i["pts0"]), kc.held_bits12(i["held"]), LOSSES.index(i["loss"])
    assert hc.hc_kpcam_system(C, n, P(uv), P(cam12), P(d5), P(pts), P(hb), loss, i["f_scale"], i["lam"], P(YY), P(acc), P(scal), P(status)) == 0
    ct, dth = (np.ascontiguousarray(a) for a in i["step"])
    assert hc.hc_kpcam_step(C, n, P(uv), P(cam12), P(d5), P(pts), loss, i["f_scale"], i["lam"], P(ct), P(dth), P(trial), P(out3)) == 0
    return dict(YY=YY, acc=acc, cost=scal[0], count=scal[1], gmax=scal[2], tail=0.0, point_status=status, trial_points=trial, step4=np.r_[out3[0], out3[1], 0.0, out3[2]])


HOST_WORST = {}


@pytest.mark.parametrize("name", [n for n in kc.SYSTEM_INPUTS if n not in kc.BIG])
def test_one_evaluation_against_the_block_oracle(hc, name):
    """the grid of tests/test_gpu_kpcam_system.py (the two large inputs apart) on the host build: the bounds hold on the reference path before
    any kernel is held to them"""
    i, o = kc.system_case(name)
    got = host_evaluation(hc, i)
    r = kc.check_block12(name, got, o)
    r.update(kc.check_step12(name, got["trial_points"], got["step4"], o, i["pts0"], i["uvs"], i["intr"], i["loss"], i["f_scale"]))
    ko.note_worst(HOST_WORST, r)
    print(ko.worst_line("host build so far", HOST_WORST))


def test_extrinsic_rows_agree_with_the_six_row_oracle():
    """with every intrinsic bit held, rows and columns 6 .. 11 of each camera's block of block_system12 are kpba_oracle.block_system's"""
    i, o = kc.system_case("intr_held")
    b = ko.block_system(i["uvs"], i["ext0"], i["intr"], i["pts0"], i["held"][:, 6:], loss=i["loss"], f_scale=i["f_scale"], lam=i["lam"])
    sel = np.flatnonzero(np.tile(np.r_[np.zeros(6, bool), np.ones(6, bool)], len(i["ext0"])))
    Ud = np.sqrt(np.diagonal(b["U"]))   # (both are long double sums rounded once: a few ulp of the uncancelled magnitude)
    for k in ("U", "YY"):
        assert (np.abs(o[k][np.ix_(sel, sel)] - b[k]) <= 8 * kc.EPS * np.outer(Ud, Ud)).all(), k
    for k in ("gc", "Yz"):
        assert (np.abs(o[k][sel] - b[k]) <= 8 * kc.EPS * Ud * b["fnorm"]).all(), k
    assert abs(o["cost"] - b["cost"]) <= 8 * kc.EPS * b["cost"] and np.array_equal(o["status"], b["status"])


def test_sanitized_stand_alone_program(tmp_path):
    """the header under AddressSanitizer + UBSan in a program of its own (its own main: 3 cameras x 14 points with a prior; 4 cameras x 16 points,
    soft_l1, a camera that sees nothing and a point with one view), run as a child process with the sanitizer runtime linked in"""
    exe = str(tmp_path / "kpcam_sanitized")
    subprocess.check_call(["g++", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-DKPCAM_MAIN", "-o", exe, SRC])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "kpcam hostcheck ok" in r.stdout
