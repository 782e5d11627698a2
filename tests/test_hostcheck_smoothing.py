"""csrc/mcba_smooth_math.h -- the per-lane text of k_smooth_prepare, k_smooth_reduce, k_smooth_backsub and k_smooth_eval -- compiled with g++ -O2
(tests/hostcheck/smoothing_hostcheck.cpp: serial loops over the lanes in the kernels' order, every level, and the IRLS loop of the C call) and
held to tests/smoothing_oracle.py without a GPU, on the cases and by the rules of the GPU tier (tests/test_gpu_smoothing.py): a linear solve
within 4 eps cond max|x| of scipy's banded solve per track, the robust loop by its own definition.

MCBA_HOSTCHECK_SANITIZE=1 (opt-in, CPU only): the same harness is also built as a stand-alone program with its own main and
-fsanitize=address,undefined, reads a scene file written here and must exit 0 with the library build's answer.  Nothing is preloaded; the
shared object is never built with a sanitizer."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import smoothing_oracle as so

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck", "smoothing_hostcheck.cpp")
SANITIZE = os.environ.get("MCBA_HOSTCHECK_SANITIZE") == "1"
V = ctypes.c_void_p
LINEAR, ROBUST = so.linear_cases(), so.robust_cases()


@pytest.fixture(scope="module")
def hc(tmp_path_factory):
    lib = str(tmp_path_factory.mktemp("smoothing_hostcheck") / "libsmoothing_hostcheck.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", lib, SRC])
    h = ctypes.CDLL(lib)
    h.hc_smooth_trajectories.argtypes = [ctypes.c_size_t, ctypes.c_int, V, V, V, V, ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_double, ctypes.c_int, V, V, V, V, V, V, V, V]
    h.hc_smooth_chunks.argtypes = [ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_double, V, V, V]
    return h


def run(hc, points, cov, accel_std, loss="linear", f_scale=3.0, weights_in=None, max_iterations=50, xtol=1e-8, segment=None):
    pts = np.ascontiguousarray(points, dtype=np.float64)
    T, K = pts.shape[:2]
    c6 = so.pack6(cov)
    acc = np.ascontiguousarray(np.broadcast_to(np.asarray(accel_std, dtype=np.float64), (K,)))
    win = None if weights_in is None else np.ascontiguousarray(weights_in, dtype=np.float64)
    x, w, d2 = np.full((T, K, 3), 7.0), np.full((T, K), 7.0), np.full((T, K), 7.0)
    st, nu, ni = np.full(K, 7, np.int32), np.full(K, 7, np.int32), np.full(K, 7, np.int32)
    hist, info = np.full((max_iterations, K, 2), 7.0), np.full(8, 7.0)
    rc = hc.hc_smooth_trajectories(T, K, pts.ctypes.data, c6.ctypes.data, acc.ctypes.data, None if win is None else win.ctypes.data, so.LOSSES[loss], f_scale, max_iterations, xtol,
                                   0 if segment is None else segment, x.ctypes.data, w.ctypes.data, d2.ctypes.data, st.ctypes.data, nu.ctypes.data, ni.ctypes.data, hist.ctypes.data, info.ctypes.data)
    assert rc == 0
    return dict(points=x, weights=w, mahalanobis2=d2, status=st, n_usable=nu, n_iterations=ni, history=hist, levels=int(info[0]), segment=int(info[1]))


@pytest.mark.parametrize("name", sorted(LINEAR))
def test_linear_solve_meets_the_bar(hc, name):
    case = LINEAR[name]
    got = run(hc, case["points"], case["cov"], case["accel_std"], segment=case["segment"])
    worst = so.check_linear(name, case, got)
    print(f"{name}: levels {got['levels']}, segment {got['segment']}, largest error {worst:.3g} eps cond max|x|")
    if name == "T333_seg2":
        assert got["levels"] == 5


def test_default_segment_against_segment_two(hc):
    a, b = LINEAR["T400_default"], LINEAR["T400_seg2"]
    ga, gb = run(hc, a["points"], a["cov"], a["accel_std"]), run(hc, b["points"], b["cov"], b["accel_std"], segment=2)
    assert ga["segment"] == 16 and gb["segment"] == 2 and ga["levels"] < gb["levels"]
    for k, (o, c) in enumerate(so.linear_reference("T400_seg2", b)):
        err, bar = so.linear_bar(ga["points"][:, k], gb["points"][:, k], c)
        print(f"track {k}: default segment against segment 2: {err:.3g} (bar {bar:.3g})")
        assert err <= bar


@pytest.mark.parametrize("name", sorted(ROBUST))
def test_one_evaluation_with_converged_weights_meets_the_bar(hc, name):
    """max_iterations = 1 with the reference's converged weights: one linear solve with exactly those weights"""
    case = ROBUST[name]
    refs = so.robust_reference(name, case)
    win = np.stack([o["weights"] for o in refs], axis=1)
    got = run(hc, case["points"], case["cov"], case["accel_std"], loss=case["loss"], f_scale=case["f_scale"], weights_in=win, max_iterations=1, segment=case["segment"])
    for k in range(win.shape[1]):
        s = so.system(case["points"][:, k], case["cov"][:, k], case["accel_std"], win[:, k])
        err, bar = so.linear_bar(got["points"][:, k], so.solve(s), so.cond(s))
        print(f"{name} track {k}: err {err:.3g} bar {bar:.3g}")
        assert err <= bar and got["n_iterations"][k] == 1 and got["status"][k] == 1


def test_robust_loop(hc):
    left_out = total = 0
    for name, case in ROBUST.items():
        got = run(hc, case["points"], case["cov"], case["accel_std"], loss=case["loss"], f_scale=case["f_scale"], segment=case["segment"])
        left_out += so.check_robust(name, case, got)
        total += case["points"].shape[1]
        again = run(hc, case["points"], case["cov"], case["accel_std"], loss=case["loss"], f_scale=case["f_scale"], segment=case["segment"])
        assert all(np.array_equal(got[f], again[f], equal_nan=True) for f in ("points", "weights", "mahalanobis2", "history", "n_iterations"))
    assert 10 * left_out <= total, (left_out, total)


def test_refused_pivot_is_status_minus_two(hc):
    """an accel_std whose inverse square is finite but six times it is not: the diagonal of a block is infinite, its pivot is refused, the track
    is NaN with status -2 and its neighbour is untouched.  (With finite blocks the Jacobi-scaled pivots stay far above the threshold: the
    cases above reach 1e-3 of the noise and gaps of a whole segment.)"""
    s = so.scene(40, 2, seed=2)
    got = run(hc, s["points"], s["cov"], np.array([1e-154, 0.1]), segment=3)
    alone = run(hc, s["points"][:, 1:], s["cov"][:, 1:], 0.1, segment=3)
    print(got["status"], got["n_usable"])
    assert got["status"][0] == so.STATUS_PIVOT and np.isnan(got["points"][:, 0]).all() and np.isnan(got["mahalanobis2"][:, 0]).all() and (got["weights"][:, 0] == 0).all()
    assert got["status"][1] == 1 and np.array_equal(got["points"][:, 1], alone["points"][:, 0])


CHUNK_SHAPES = [(T, 2) for T in (1, 2, 3, 5, 333)] + [(400, None), (5000, None)]   # the shortest tracks, five levels, the default segment


@pytest.mark.parametrize("T,segment", CHUNK_SHAPES)
def test_chunk_rule_and_carve_against_the_oracle(hc, T, segment):
    """the tracks-per-chunk rule, the byte count and the level carve that the C call uses (mcba_smooth_math.h), against so.expected_chunks: one
    chunk, the budgets of the GPU tier, and one at which a chunk is a single track"""
    for K in (1, 5, 20):
        for budget in (8192.0, 0.5, 0.2, 0.001):
            out4, offs, total = np.full(4, 7.0), np.full(3 * so.MAX_LEVELS, 7, np.int64), np.full(1, 7, np.int64)
            assert hc.hc_smooth_chunks(T, K, segment or 0, budget, out4.ctypes.data, offs.ctypes.data, total.ctypes.data) == 0
            want = so.expected_chunks(T, K, segment, budget, "smooth")
            assert tuple(int(v) for v in out4) == want, (K, budget, out4, want)
            if budget == 8192.0:
                assert want[:2] == (K, 1)
            if budget == 0.001:
                assert want[:2] == (1, K)
            so.check_carve(so.plan(T, segment or so.SEGMENT_DEFAULT, want[0]), so.X_EXTRA, offs, int(total[0]))
            assert int(total[0]) == so.level_doubles(T, segment or so.SEGMENT_DEFAULT, want[0], so.X_EXTRA)


def test_stand_alone_program_under_sanitizers(hc, tmp_path):
    if not SANITIZE:
        pytest.skip("opt-in: MCBA_HOSTCHECK_SANITIZE=1")
    exe = str(tmp_path / "smoothing_hostcheck")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DSMOOTH_HOSTCHECK_MAIN", "-o", exe, SRC])
    for name, case in (("gaps_seg2", LINEAR["gaps_seg2"]), ("soft_l1_36", ROBUST["soft_l1_36"])):
        pts = np.ascontiguousarray(case["points"])
        T, K = pts.shape[:2]
        loss, seg = case.get("loss", "linear"), case["segment"] or 0
        path = str(tmp_path / f"{name}.bin")
        with open(path, "wb") as fh:
            fh.write(struct.pack("<qqqqqqdd", T, K, so.LOSSES[loss], 50, seg, 0, 3.0, 1e-8))
            fh.write(pts.tobytes())
            fh.write(so.pack6(case["cov"]).tobytes())
            fh.write(np.ascontiguousarray(np.broadcast_to(np.asarray(case["accel_std"], dtype=np.float64), (K,))).tobytes())
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
        print(r.stdout)
        assert r.returncode == 0 and "runtime error" not in r.stderr, r.stdout + r.stderr
        got = run(hc, case["points"], case["cov"], case["accel_std"], loss=loss, segment=case["segment"])
        for k in range(K):
            assert f"track {k} status {got['status'][k]} usable {got['n_usable'][k]} iterations {got['n_iterations'][k]} " in r.stdout
