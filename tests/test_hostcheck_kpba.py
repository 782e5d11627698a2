"""csrc/mcba_kpba_math.h -- the arithmetic of the free-point bundle-adjustment kernels (csrc/mcba_kpba.hip) and the Levenberg-Marquardt loop of the
C ABI -- compiled with g++ (tests/hostcheck/kpba_hostcheck.cpp, plain -O2) and held, without a GPU, to the bars of the GPU tier
(tests/test_gpu_kpba.py) against tests/golden/kpba.npz (scipy, tests/kpba_oracle.py): at ftol = xtol = 1e-15, gtol = 1e-10 every pinned case reaches
cost <= golden (1 + 1e-10), extrinsics within 1e-6 relative after the closing step, used points within max(1e-6 relative, 10 x the golden's own
two-start spread)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import kpba_oracle as ko
import tricov_oracle as tco

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck", "kpba_hostcheck.cpp")
LOSSES = ("linear", "soft_l1", "huber", "cauchy", "arctan")


def P(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


@pytest.fixture(scope="module")
def hc(tmp_path_factory):
    lib = str(tmp_path_factory.mktemp("kpba_hostcheck") / "libkpba_hostcheck.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-o", lib, SRC])
    h = ctypes.CDLL(lib)
    h.hc_kpba.argtypes = [ctypes.c_int, ctypes.c_size_t] + [ctypes.c_void_p] * 5 + [ctypes.c_int] * 3 + [ctypes.c_double] * 4 + [ctypes.c_int] + [ctypes.c_void_p] * 5 + [ctypes.c_int]
    h.hc_kpba_system.argtypes = [ctypes.c_int, ctypes.c_size_t] + [ctypes.c_void_p] * 5 + [ctypes.c_int, ctypes.c_double, ctypes.c_double] + [ctypes.c_void_p] * 4
    h.hc_kpba_step.argtypes = [ctypes.c_int, ctypes.c_size_t] + [ctypes.c_void_p] * 4 + [ctypes.c_int, ctypes.c_double, ctypes.c_double] + [ctypes.c_void_p] * 4
    h.hc_kpba_dense_solve.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 3
    return h


def bits(held):
    return np.ascontiguousarray((np.asarray(held, dtype=np.int32) << np.arange(6, dtype=np.int32)).sum(1), dtype=np.int32)


def host_refine(hc, uvs, ext0, intr, pts0, held, scale_camera, loss="linear", f_scale=1.0, ftol=1e-15, xtol=1e-15, gtol=1e-10, max_nfev=100):
    theta, d5 = tco.camera_blocks(ext0, intr)
    uv = np.ascontiguousarray(np.stack([np.asarray(u, dtype=np.float64) for u in uvs]))
    C, n = uv.shape[:2]
    pts0 = np.ascontiguousarray(pts0, dtype=np.float64)
    hb = bits(held)
    ext, pts, status, res, hist = np.empty((C, 6)), np.empty((n, 3)), np.empty(n, np.int32), np.empty(8), np.zeros((max_nfev + 8, 3))
    assert hc.hc_kpba(C, n, P(uv), P(theta), P(d5), P(pts0), P(hb), 0, scale_camera, LOSSES.index(loss), f_scale, ftol, xtol, gtol, max_nfev, P(ext), P(pts), P(status), P(res), P(hist),
                      len(hist)) == 0
    return dict(extrinsics=ext, points=pts, point_status=status, cost=res[0], cost0=res[1], optimality=res[2], nfev=int(res[3]), njev=int(res[4]), status=int(res[5]), scale=res[6],
                history=hist[:int(res[7])], held_bits=hb)


@pytest.mark.parametrize("name", ko.pinned_cases())
def test_host_loop_reaches_the_golden_optimum(hc, name):
    i, o = ko.case(name)
    got = host_refine(hc, i["uvs"], i["ext0"], i["intr"], i["pts0"], o["held"], o["scale_camera"], loss=i["loss"])
    print(f"{name}: status {got['status']} nfev {got['nfev']} njev {got['njev']} optimality {got['optimality']:.3g} scale {got['scale']:.15g}")
    assert np.array_equal(got["held_bits"], bits(o["held"]))
    ko.check_result(name, got["extrinsics"], got["points"], got["cost"], o)
    assert got["cost"] <= got["cost0"] and got["status"] in (1, 2, 3)
    base0 = ko.baseline_of(i["ext0"], 0, o["scale_camera"])
    assert abs(ko.baseline_of(got["extrinsics"], 0, o["scale_camera"]) / base0 - 1) <= 1e-12
    # the stated cost is the objective at the returned values (the rescale changes no projection)
    X = np.where(np.isnan(got["points"]), i["pts0"], got["points"])
    assert abs(ko.cost_of(got["extrinsics"], X, i["uvs"], i["intr"], i["loss"]) / got["cost"] - 1) <= 1e-10


@pytest.mark.parametrize("loss", ["cauchy", "arctan"])
def test_unpinned_losses_terminate_and_never_rise(hc, loss):
    i, o = ko.case("outlier")
    got = host_refine(hc, i["uvs"], i["ext0"], i["intr"], i["pts0"], o["held"], o["scale_camera"], loss=loss, ftol=1e-8, xtol=1e-8, gtol=1e-8, max_nfev=60)
    print(f"{loss}: cost {got['cost0']:.6g} -> {got['cost']:.6g}, status {got['status']}, nfev {got['nfev']}")
    assert got["cost"] <= got["cost0"] and got["status"] in (0, 1, 2, 3) and got["nfev"] <= 60


def test_start_at_the_optimum_ends_within_two_evaluations(hc):
    """at scipy's default tolerances (1e-8), from the golden optimum: at most the start and one trial, the cost unchanged to 1e-12"""
    for name in ("three", "six"):
        i, o = ko.case(name)
        X = np.where(np.isnan(o["points"]), i["pts0"], o["points"])
        got = host_refine(hc, i["uvs"], o["extrinsics"], i["intr"], X, o["held"], o["scale_camera"], ftol=1e-8, xtol=1e-8, gtol=1e-8)
        print(f"{name}: nfev {got['nfev']} status {got['status']} cost {got['cost']:.15g} golden {o['cost']:.15g}")
        assert got["nfev"] <= 2 and got["status"] > 0 and abs(got["cost"] / o["cost"] - 1) <= 1e-12


def test_camera_without_detections_and_points_that_take_no_part(hc):
    i, o = ko.case("six")
    uvs = [u.copy() for u in i["uvs"]]
    blind = next(c for c in range(1, len(uvs)) if c != o["scale_camera"])
    uvs[blind][:] = np.nan
    pts = i["pts0"].copy()
    pts[7, 2] = np.nan
    got = host_refine(hc, uvs, i["ext0"], i["intr"], pts, o["held"], o["scale_camera"], ftol=1e-8, xtol=1e-8, gtol=1e-8)
    assert got["held_bits"][blind] == 63 and np.array_equal(got["extrinsics"][blind], i["ext0"][blind]) and np.array_equal(got["extrinsics"][0], i["ext0"][0])
    used, _ = ko.used_points(uvs, pts)
    assert np.array_equal(got["point_status"] == 1, used) and got["point_status"][7] == -1 and np.isnan(got["points"][~used]).all()
    assert got["cost"] < got["cost0"]


def test_schur_system_against_the_dense_jacobian(hc):
    """A, columns 6 .. 11 of B and the assembled S, rhs at lambda = 0 on "three" at the start, against the oracle's dense J^T J Schur complement"""
    i, o = ko.case("three")
    theta, d5 = tco.camera_blocks(i["ext0"], i["intr"])
    uv = np.ascontiguousarray(np.stack(i["uvs"]))
    C, n = uv.shape[:2]
    NP = (6 * C + 15) // 16 * 16
    YY, acc, scal = np.empty((NP, NP)), np.empty((C, 33)), np.empty(3)
    pts = np.ascontiguousarray(i["pts0"])
    hb = bits(o["held"])
    assert hc.hc_kpba_system(C, n, P(uv), P(theta), P(d5), P(pts), P(hb), 0, 1.0, 0.0, P(YY), P(acc), P(scal), P(np.empty(n, np.int32))) == 0
    U = np.zeros((6 * C, 6 * C))
    tri = np.tril_indices(6)
    for c in range(C):
        blk = np.zeros((6, 6))
        blk[tri] = acc[c, :21]
        U[6 * c:6 * c + 6, 6 * c:6 * c + 6] = blk + np.tril(blk, -1).T
    S = U - YY[:6 * C, :6 * C]
    rhs = (acc[:, 27:33] - acc[:, 21:27]).ravel()
    d = ko.dense_system(i["uvs"], i["ext0"], i["intr"], i["pts0"], o["held"])
    free = d["free"]
    ko.check_schur("three", S[np.ix_(free, free)], rhs[free], d)
    assert abs(scal[0] / ko.cost_of(i["ext0"], i["pts0"], i["uvs"], i["intr"], "linear") - 1) <= 1e-12


def test_block_and_dense_oracles_agree():
    """two independent statements of the system (kpba_oracle.block_system: per-point blocks in long double; dense_system: the dense J^T J Schur
    complement) on "three" at linear loss and lambda = 0: S to 1e-12 relative to sqrt(U_ii U_jj), the right-hand side to 1e-12 sqrt(U_ii) |f|_2"""
    i, o = ko.case("three")
    d = ko.dense_system(i["uvs"], i["ext0"], i["intr"], i["pts0"], o["held"])
    b = ko.block_system(i["uvs"], i["ext0"], i["intr"], i["pts0"], o["held"], loss="linear", lam=0.0)
    free = d["free"]
    S, rhs = (b["U"] - b["YY"])[np.ix_(free, free)], (b["Yz"] - b["gc"])[free]
    Ud = np.sqrt(d["Udiag"])
    eS, er = (np.abs(S - d["S"]) / np.outer(Ud, Ud)).max(), (np.abs(rhs - d["rhs"]) / (Ud * d["fnorm"])).max()
    print(f"block against dense: S {eS:.3g}, rhs {er:.3g} (bar 1e-12); cond {b['cond'].max():.3g} / {d['cond']:.3g}, |f| {b['fnorm']:.15g} / {d['fnorm']:.15g}")
    assert eS <= 1e-12 and er <= 1e-12
    assert abs(b["cond"].max() / d["cond"] - 1) <= 1e-9 and abs(b["fnorm"] / d["fnorm"] - 1) <= 1e-12 and b["maxdet"] == d["maxdet"] and b["count"] == d["n_scalars"]
    assert abs(b["cost"] / ko.cost_of(i["ext0"], i["pts0"], i["uvs"], i["intr"], "linear") - 1) <= 1e-12


def host_evaluation(hc, i):
    """one evaluation of the host build at an input of kpba_oracle.system_case, in the keys of geometry.refine_extrinsics_system"""
    theta, d5 = tco.camera_blocks(i["ext0"], i["intr"])
    uv = np.ascontiguousarray(np.stack(i["uvs"]))
    C, n = uv.shape[:2]
    NP = (6 * C + 15) // 16 * 16
    YY, acc, scal, status, trial, out3 = np.empty((NP, NP)), np.empty((C, 33)), np.empty(3), np.empty(n, np.int32), np.empty((n, 3)), np.empty(3)
    pts, hb, loss = np.ascontiguousarray(i["pts0"]), ko.held_bits(i["held"]), LOSSES.index(i["loss"])
    assert hc.hc_kpba_system(C, n, P(uv), P(theta), P(d5), P(pts), P(hb), loss, i["f_scale"], i["lam"], P(YY), P(acc), P(scal), P(status)) == 0
    et, dth = (np.ascontiguousarray(a) for a in i["step"])
    assert hc.hc_kpba_step(C, n, P(uv), P(theta), P(d5), P(pts), loss, i["f_scale"], i["lam"], P(et), P(dth), P(trial), P(out3)) == 0
    return dict(YY=YY, acc=acc, cost=scal[0], count=scal[1], gmax=scal[2], tail=0.0, point_status=status, trial_points=trial, step4=np.r_[out3[0], out3[1], 0.0, out3[2]])


HOST_WORST = {}


@pytest.mark.parametrize("name", list(ko.SYSTEM_INPUTS))
def test_one_evaluation_against_the_block_oracle(hc, name):
    """the grid of tests/test_gpu_kpba_system.py (every input; the forced group sizes mean nothing here) on the host build: the bounds of
    kpba_oracle hold on the reference path before any kernel is held to them"""
    i, o = ko.system_case(name)
    got = host_evaluation(hc, i)
    r = ko.check_block(name, got, o)
    r.update(ko.check_step(name, got["trial_points"], got["step4"], o, i["pts0"], i["uvs"], i["intr"], i["loss"], i["f_scale"]))
    ko.note_worst(HOST_WORST, r)
    print(ko.worst_line("host build so far", HOST_WORST))


def test_dense_solve(hc):
    rng = np.random.default_rng(3)
    for n in (1, 5, 143):
        M = rng.normal(size=(n + 3, n)) * np.logspace(0, 3, n)
        A, b, x = np.ascontiguousarray(M.T @ M), rng.normal(size=n), np.empty(n)
        ref = np.linalg.solve(A, b)
        assert hc.hc_kpba_dense_solve(n, P(A.copy()), P(b), P(x)) == 1
        assert np.abs(x - ref).max() <= 1e-8 * np.abs(ref).max()
    A = -np.eye(3)
    assert hc.hc_kpba_dense_solve(3, P(A), P(np.ones(3)), P(np.empty(3))) == 0


def test_sanitized_stand_alone_program(tmp_path):
    """the header under AddressSanitizer + UBSan in a program of its own (its own main: 2 cameras x 8 points; 4 cameras x 11 points, soft_l1, a
    camera that sees nothing and a point with one view), run as a child process with the sanitizer runtime linked in"""
    exe = str(tmp_path / "kpba_sanitized")
    subprocess.check_call(["g++", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-DKPBA_MAIN", "-o", exe, SRC])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "kpba hostcheck ok" in r.stdout
