"""csrc/mcba_consensus_math.h -- the per-lane text of the consensus triangulation kernels -- compiled with g++ (tests/hostcheck/consensus_hostcheck.cpp)
and held to the gates of the GPU tier (tests/test_gpu_consensus.py) without a GPU, against the numpy statement of the definition in
tests/consensus_oracle.py: mask, pair and status equal, the winning cost to rtol 1e-9, the points to the refinement gate 5e-6 mm.

Ambiguity rule (consensus_oracle.decided): a point is left out of the mask / pair comparison only when the oracle's two lowest costs are closer
than 1e-6 relative or one of the winner's errors is within 1e-6 px of the threshold, and never more than 1 % of a scene's points."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import consensus_oracle as co
import keypoint_scenes as ks
from multicam_calibration_amd import ops
from multicam_calibration_amd.triangulation import _cam_blocks

HERE = os.path.dirname(os.path.abspath(__file__))
GATE_MM = 5e-6   # the project's refinement gate (tests/test_hostcheck_keypoints.py)
SANITIZE = os.environ.get("MCBA_HOSTCHECK_SANITIZE") == "1"
SCENES = ["six", "three", "twelve", "outlier"]
THRESHOLDS = [1.0, 2.5]


def P(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


@pytest.fixture(scope="module")
def hc(tmp_path_factory):
    src = os.path.join(HERE, "hostcheck", "consensus_hostcheck.cpp")
    lib = str(tmp_path_factory.mktemp("consensus_hostcheck") / "libconsensus_hostcheck.so")
    flags = ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if SANITIZE else ["-O2"]
    subprocess.check_call(["g++"] + flags + ["-shared", "-fPIC", "-o", lib, src])
    h = ctypes.CDLL(lib)
    h.hc_consensus.argtypes = [ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_int,
                               ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    h.hc_consensus_hypothesis.argtypes = [ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    return h


def consensus(hc, uvs, ext, intr, threshold, min_views=2, loss="linear", f_scale=1.0, max_iterations=100, stride=1):
    cam, dist = _cam_blocks(ext, intr)
    U = np.ascontiguousarray(np.stack(uvs))
    C, n = U.shape[:2]
    out, words, info = np.empty((n, 3)), np.zeros(n, dtype=np.uint64), np.empty((n, 8))
    assert hc.hc_consensus(C, n, P(U), P(cam), P(dist), threshold, min_views, 5, ops.LOSSES[loss], f_scale, max_iterations, stride, P(out), P(words), P(info)) == 0
    inl = ((words[None, :] >> np.arange(C, dtype=np.uint64)[:, None]) & np.uint64(1)).astype(bool)
    return dict(points=out, inliers=inl, n_inliers=info[:, 0].astype(int), pair=info[:, 1:3].astype(int), hypothesis_cost=info[:, 3], cost=info[:, 4], cost0=info[:, 5], n_iterations=info[:, 6].astype(int),
                status=info[:, 7].astype(int))


def compare(got, o, label=""):
    return co.compare(got, o, GATE_MM, label)


@pytest.mark.parametrize("threshold", THRESHOLDS)
@pytest.mark.parametrize("name", SCENES)
def test_scenes_match_the_oracle(hc, name, threshold):
    uvs, ext, intr, _, o = co.scene_oracle(name, threshold)
    got = consensus(hc, uvs, ext, intr, threshold)
    ok = compare(got, o, f"{name} @ {threshold}")
    assert ok.all()   # the numpy prototype leaves out no point of these scenes: the ambiguity rule is a guard
    # the wavefront form's schedule (64 running bests, then the lexicographic minimum) picks the same winner, bit for bit
    wave = consensus(hc, uvs, ext, intr, threshold, stride=64)
    for key in ("points", "inliers", "pair", "hypothesis_cost", "status"):
        assert np.array_equal(got[key], wave[key], equal_nan=True), key


def test_exact_ties_go_to_the_lower_pair(hc):
    uvs, ext, intr, _ = co.duplicated_camera_scene()
    o = co.consensus(uvs, ext, intr, 2.5)
    for stride in (1, 64, 3):
        got = consensus(hc, uvs, ext, intr, 2.5, stride=stride)
        assert np.array_equal(got["pair"], o["pair"]) and np.array_equal(got["inliers"], o["inliers"]) and np.array_equal(got["status"], o["status"])
        np.testing.assert_allclose(got["hypothesis_cost"], o["hypothesis_cost"], rtol=1e-9)
        assert np.abs(got["points"] - o["points"]).max() <= GATE_MM
    tied = (o["pair"][:, 0] == 0) & (o["pair"][:, 1] >= 2)           # the winner (0, k) has the twin (1, k) of exactly the same cost
    print(f"{tied.sum()} of {len(tied)} winners have an exact-tie twin")
    assert tied.sum() >= 10 and not (got["pair"][:, 0] == 1).any()    # a pair starting at camera 1 never wins: its twin from camera 0 comes first


def test_outlier_scene_flags_exactly_the_displaced_detections(hc, golden):
    uvs, ext, intr, X, o = co.scene_oracle("outlier", 2.5)
    got = consensus(hc, uvs, ext, intr, 2.5)
    U = np.stack(uvs)
    seen = ~np.isnan(U).any(-1)
    off = ks.errors(X, uvs, ext, intr)                                # distance of each detection from the truth's projection
    displaced = seen & (off > 5.0)
    has = got["status"] != -1                                         # the points with a hypothesis
    assert displaced.sum() >= 40
    assert np.array_equal(~got["inliers"] & seen & has[None], displaced & has[None])
    ok = ~np.isnan(golden("geometry.npz")["outlier_start"]).any(1)
    assert np.array_equal(ok, has)

    def rms(A):
        return np.sqrt(np.mean(np.sum((A[ok] - X[ok]) ** 2, axis=1)))

    soft = rms(golden("geometry.npz")["outlier_soft_l1"])
    print(f"flagged {int((~got['inliers'] & seen & has[None]).sum())} of {int(seen[:, has].sum())} detections; rms to truth: consensus {rms(got['points']):.4f}, soft_l1 {soft:.4f} mm")
    assert rms(got["points"]) < soft


def test_zero_iterations_return_the_hypothesis(hc):
    uvs, ext, intr, _, o = co.scene_oracle("six", 2.5)
    got = consensus(hc, uvs, ext, intr, 2.5, max_iterations=0)
    fit = o["status"] == 1
    assert np.all(got["n_iterations"] == 0) and np.array_equal(got["cost"][fit], got["cost0"][fit]) and np.array_equal(got["status"] >= 0, fit)
    # bit for bit the winning pair's hypothesis, recomputed on its own
    cam, dist = _cam_blocks(ext, intr)
    U = np.ascontiguousarray(np.stack(uvs))
    pairs = np.ascontiguousarray(got["pair"], dtype=np.int32)
    X, kept = np.full((len(pairs), 3), np.nan), np.zeros(len(pairs), dtype=np.int32)
    hc.hc_consensus_hypothesis(len(cam), len(pairs), P(U), P(cam), P(dist), 5, P(pairs), P(X), P(kept))
    assert np.array_equal(kept == 1, fit) and np.array_equal(got["points"], X, equal_nan=True)
    np.testing.assert_allclose(X[fit], o["hypothesis"][fit], rtol=0, atol=1e-7)   # (the oracle's SVD and the Jacobi null vector)
    # the search does not depend on the refit
    full = consensus(hc, uvs, ext, intr, 2.5)
    assert np.array_equal(full["inliers"], got["inliers"]) and np.array_equal(full["pair"], got["pair"]) and np.array_equal(full["hypothesis_cost"], got["hypothesis_cost"], equal_nan=True)
    assert np.array_equal(full["cost0"], got["cost"], equal_nan=True)
    # the refit's linear cost at the hypothesis is the inliers' share of the truncated cost
    n_out = o["seen"].sum(0) - got["n_inliers"]
    np.testing.assert_allclose(0.5 * (got["hypothesis_cost"] - 2.5 ** 2 * n_out)[fit], got["cost"][fit], rtol=1e-9, atol=1e-12)


def test_few_views_and_min_views(hc):
    uvs, ext, intr, _, _ = co.scene_oracle("three", 2.5)
    U = np.stack(uvs).copy()
    a, b, c, d = np.flatnonzero((~np.isnan(U).any(-1)).all(0))[:4]
    U[1:, a] = np.nan                                                 # one camera sees point a
    U[:, b] = np.nan                                                  # nobody sees point b
    U[2, c] = np.nan                                                  # two cameras see point c, one detection displaced
    U[0, c] += 25.0
    U[2, d] = np.nan                                                  # two cameras see point d, both clean
    o = co.consensus(list(U), ext, intr, 2.5)
    got = consensus(hc, list(U), ext, intr, 2.5)
    compare(got, o, "few views")
    assert got["status"][a] == -1 and got["status"][b] == -1 and np.isnan(got["points"][[a, b]]).all() and not got["inliers"][:, [a, b]].any()
    assert got["status"][c] == o["status"][c] and got["status"][d] == 1 and got["n_inliers"][d] == 2
    print(f"two cameras, one displaced: status {got['status'][c]}, {got['n_inliers'][c]} inliers")
    # min_views above what agrees: no consensus, the mask still reported
    o3 = co.consensus(list(U), ext, intr, 2.5, min_views=3)
    got3 = consensus(hc, list(U), ext, intr, 2.5, min_views=3)
    compare(got3, o3, "min_views 3")
    two = (got3["n_inliers"] < 3) & (got3["status"] != -1)
    assert two.any() and np.all(got3["status"][two] == -2) and np.isnan(got3["points"][two]).all() and np.array_equal(got3["inliers"], got["inliers"])


@pytest.mark.parametrize("C,n", co.BOUNDARY_CASES)
def test_launch_boundary_scenes(hc, C, n):
    """The GPU tier's launch-boundary inputs, through the host text in both schedules."""
    uvs, ext, intr = co.boundary_case(C, n)
    o = co.consensus(uvs, ext, intr, 2.5)
    got = consensus(hc, uvs, ext, intr, 2.5)
    compare(got, o, f"C {C} P {n}")
    wave = consensus(hc, uvs, ext, intr, 2.5, stride=64)
    for key in ("points", "inliers", "pair", "hypothesis_cost", "status"):
        assert np.array_equal(got[key], wave[key], equal_nan=True), key


def test_consensus_hostcheck_under_sanitizers():
    """The same text with -fsanitize=address,undefined, every test of this file in a child process (the ASan runtime has to come first among the
    process' libraries)."""
    if SANITIZE:
        pytest.skip("this IS the sanitizer run")
    asan = subprocess.check_output(["gcc", "-print-file-name=libasan.so"], text=True).strip()
    if not os.path.isabs(asan) or not os.path.exists(asan):
        pytest.skip("libasan.so not found next to gcc")
    preload = " ".join(x for x in (asan, os.environ.get("LD_PRELOAD", "")) if x)
    env = dict(os.environ, MCBA_HOSTCHECK_SANITIZE="1", LD_PRELOAD=preload, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", os.path.abspath(__file__)], env=env, cwd=os.path.join(HERE, ".."), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "passed" in r.stdout and "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
