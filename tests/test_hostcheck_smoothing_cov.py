"""csrc/mcba_smooth_cov_math.h -- the per-lane text of k_smooth_selinv, behind the elimination of mcba_smooth_math.h -- compiled with g++ -O2
(tests/hostcheck/smoothing_cov_hostcheck.cpp: serial loops over the lanes in the kernels' order, every level) and held to
tests/smoothing_cov_oracle.py without a GPU, on the cases and by the bar of the GPU tier (tests/test_gpu_smoothing_cov.py): per track
|zhat - zhat_ref| <= 4 eps cond max|zhat_ref| over Z_tt and Z_{t,t+1} in Jacobi-scaled units.

MCBA_HOSTCHECK_SANITIZE=1 (opt-in, CPU only): the same harness is also built as a stand-alone program with its own main and
-fsanitize=address,undefined, reads a scene file written here and must exit 0 with the library build's answer.  Nothing is preloaded; the
shared object is never built with a sanitizer."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import smoothing_cov_oracle as sc
import smoothing_oracle as so

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck", "smoothing_cov_hostcheck.cpp")
SANITIZE = os.environ.get("MCBA_HOSTCHECK_SANITIZE") == "1"
V = ctypes.c_void_p
LINEAR, ROBUST = so.linear_cases(), so.robust_cases()


@pytest.fixture(scope="module")
def hc(tmp_path_factory):
    lib = str(tmp_path_factory.mktemp("smoothing_cov_hostcheck") / "libsmoothing_cov_hostcheck.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", lib, SRC])
    h = ctypes.CDLL(lib)
    h.hc_smooth_covariance.argtypes = [ctypes.c_size_t, ctypes.c_int, V, V, V, V, ctypes.c_int, V, V, V, V, V]
    h.hc_smooth_chunks.argtypes = [ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_int, V, V, V]
    return h


def unpack(c6):
    i = np.array([[0, 1, 2], [1, 3, 4], [2, 4, 5]])
    return c6[..., i]


def run(hc, points, cov, accel_std, weights=None, lag=True, segment=None):
    pts = np.ascontiguousarray(points, dtype=np.float64)
    T, K = pts.shape[:2]
    c6 = so.pack6(cov)
    acc = np.ascontiguousarray(np.broadcast_to(np.asarray(accel_std, dtype=np.float64), (K,)))
    win = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
    oc, ol = np.full((T, K, 6), 7.0), np.full((T - 1, K, 9), 7.0)
    st, nu, info = np.full(K, 7, np.int32), np.full(K, 7, np.int32), np.full(8, 7.0)
    rc = hc.hc_smooth_covariance(T, K, pts.ctypes.data, c6.ctypes.data, acc.ctypes.data, None if win is None else win.ctypes.data, 0 if segment is None else segment, oc.ctypes.data,
                                 ol.ctypes.data if lag else None, st.ctypes.data, nu.ctypes.data, info.ctypes.data)
    assert rc == 0
    assert lag or (ol == 7.0).all()
    return dict(covariance=unpack(oc), lag_covariance=ol.reshape(T - 1, K, 3, 3) if lag else None, status=st, n_usable=nu, levels=int(info[0]), segment=int(info[1]))


@pytest.mark.parametrize("name", sorted(LINEAR))
def test_covariance_meets_the_bar(hc, name):
    case = LINEAR[name]
    got = run(hc, case["points"], case["cov"], case["accel_std"], segment=case["segment"])
    worst = sc.check_case(name, case, got)
    print(f"{name}: levels {got['levels']}, segment {got['segment']}, largest error {worst:.3g} eps cond max|zhat|")
    if name == "T333_seg2":
        assert got["levels"] == 5
    without = run(hc, case["points"], case["cov"], case["accel_std"], lag=False, segment=case["segment"])
    assert np.array_equal(got["covariance"], without["covariance"], equal_nan=True)


@pytest.mark.parametrize("name", sorted(ROBUST))
def test_covariance_at_converged_weights_meets_the_bar(hc, name):
    case = ROBUST[name]
    win = np.stack([o["weights"] for o in so.robust_reference(name, case)], axis=1)
    got = run(hc, case["points"], case["cov"], case["accel_std"], weights=win, segment=case["segment"])
    sc.check_case(name, case, got, weights=win)


def test_default_segment_against_segment_two(hc):
    """5000 frames x 7 tracks: the default segment against segment=2 within the sum of the two bars, the condition number and max|zhat| taken
    from the first 400 frames (the system is local: neither grows with the length of a stationary scene); that sub-case against the reference"""
    s = so.scene(5000, 7, seed=12, gaps=[(100, 140), (3000, 3001), (4990, 5000)])
    acc = np.linspace(0.03, 0.09, 7)
    sub = dict(points=s["points"][:400], cov=s["cov"][:400], accel_std=acc, segment=None)
    sc.check_case("T5000_sub400", sub, run(hc, sub["points"], sub["cov"], acc))
    a, b = run(hc, s["points"], s["cov"], acc), run(hc, s["points"], s["cov"], acc, segment=2)
    assert a["segment"] == 16 and b["segment"] == 2 and a["levels"] < b["levels"]
    for k, ref in enumerate(sc.case_reference("T5000_sub400", sub)):
        other = dict(diag=b["covariance"][:, k], lag=b["lag_covariance"][:, k], s=np.sqrt(so.system(s["points"][:, k], s["cov"][:, k], acc[k], dense=False)["ab"][8]))
        err, bar = sc.scaled_error(a["covariance"][:, k], a["lag_covariance"][:, k], other), 2 * sc.bar_of(ref)
        print(f"track {k}: cond {ref['cond']:.3g} default segment against segment 2: {err:.3g} (two bars {bar:.3g})")
        assert a["status"][k] == 1 and b["status"][k] == 1 and err <= bar


def test_refused_pivot_is_status_minus_two(hc):
    """an accel_std whose inverse square is finite but six times it is not (the case of tests/test_hostcheck_smoothing.py): status -2 and NaN
    throughout, the neighbour untouched"""
    s = so.scene(40, 2, seed=2)
    got = run(hc, s["points"], s["cov"], np.array([1e-154, 0.1]), segment=3)
    alone = run(hc, s["points"][:, 1:], s["cov"][:, 1:], 0.1, segment=3)
    assert got["status"][0] == so.STATUS_PIVOT and np.isnan(got["covariance"][:, 0]).all() and np.isnan(got["lag_covariance"][:, 0]).all()
    assert got["status"][1] == 1 and np.array_equal(got["covariance"][:, 1], alone["covariance"][:, 0]) and np.array_equal(got["lag_covariance"][:, 1], alone["lag_covariance"][:, 0])


CHUNK_SHAPES = [(T, 2) for T in (1, 2, 3, 5, 333)] + [(400, None), (5000, None)]   # the shortest tracks, five levels, the default segment


@pytest.mark.parametrize("T,segment", CHUNK_SHAPES)
def test_chunk_rule_and_carve_against_the_oracle(hc, T, segment):
    """the tracks-per-chunk rule, the byte count and the level carve that the C call uses (mcba_smooth_math.h, mcba_smooth_cov_math.h), against
    so.expected_chunks, with and without the lag plane: one chunk, the budgets of the GPU tier, and one at which a chunk is a single track"""
    for K in (1, 5, 20):
        for budget in (8192.0, 0.5, 0.2, 0.001):
            for lag in (False, True):
                out4, offs, total = np.full(4, 7.0), np.full(3 * so.MAX_LEVELS, 7, np.int64), np.full(1, 7, np.int64)
                assert hc.hc_smooth_chunks(T, K, segment or 0, budget, int(lag), out4.ctypes.data, offs.ctypes.data, total.ctypes.data) == 0
                want = so.expected_chunks(T, K, segment, budget, "cov", lag)
                assert tuple(int(v) for v in out4) == want, (K, budget, lag, out4, want)
                if budget == 8192.0:
                    assert want[:2] == (K, 1)
                if budget == 0.001:
                    assert want[:2] == (1, K)
                so.check_carve(so.plan(T, segment or so.SEGMENT_DEFAULT, want[0]), so.ZC_EXTRA, offs, int(total[0]))
                assert int(total[0]) == so.level_doubles(T, segment or so.SEGMENT_DEFAULT, want[0], so.ZC_EXTRA)


def test_stand_alone_program_under_sanitizers(hc, tmp_path):
    if not SANITIZE:
        pytest.skip("opt-in: MCBA_HOSTCHECK_SANITIZE=1")
    exe = str(tmp_path / "smoothing_cov_hostcheck")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DSMOOTH_COV_HOSTCHECK_MAIN", "-o", exe, SRC])
    for name in ("gaps_seg3", "T333_seg2", "S3_odd_seg2", "T1", "one_usable"):
        case = LINEAR[name]
        pts = np.ascontiguousarray(case["points"])
        T, K = pts.shape[:2]
        for lag in (1, 0):
            path = str(tmp_path / f"{name}_{lag}.bin")
            with open(path, "wb") as fh:
                fh.write(struct.pack("<qqqqq", T, K, case["segment"] or 0, 0, lag))
                fh.write(pts.tobytes())
                fh.write(so.pack6(case["cov"]).tobytes())
                fh.write(np.ascontiguousarray(np.broadcast_to(np.asarray(case["accel_std"], dtype=np.float64), (K,))).tobytes())
            r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
            print(r.stdout)
            assert r.returncode == 0 and "runtime error" not in r.stderr, r.stdout + r.stderr
            got = run(hc, case["points"], case["cov"], case["accel_std"], segment=case["segment"])
            for k in range(K):
                assert f"track {k} status {got['status'][k]} usable {got['n_usable'][k]} " in r.stdout
