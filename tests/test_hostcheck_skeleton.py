"""csrc/mcba_skeleton_math.h -- everything k_skel_refine computes: skel_frame, the procedure of a frame phase by phase, the activity sweeps, the
accept and stop rule, the forest plan, the distance of estimate_bone_lengths -- compiled with g++ -O2 (tests/hostcheck/skeleton_hostcheck.cpp:
per phase a serial loop over the frame's lanes in the kernel's order) and held to tests/skeleton_oracle.py without a GPU, on the cases and by
the rules of the GPU tier (tests/test_gpu_skeleton.py)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import skeleton_oracle as sko

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck", "skeleton_hostcheck.cpp")
V = ctypes.c_void_p
CASES = sko.cases()
SYM = np.array([[0, 1, 2], [1, 3, 4], [2, 4, 5]])
MAX_ITERATIONS = 50


@pytest.fixture(scope="module")
def hc(tmp_path_factory):
    lib = str(tmp_path_factory.mktemp("skeleton_hostcheck") / "libskeleton_hostcheck.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", lib, SRC])
    h = ctypes.CDLL(lib)
    h.hc_refine_skeleton.argtypes = [ctypes.c_int, ctypes.c_size_t, ctypes.c_int, ctypes.c_int] + [V] * 9 + [ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_double, ctypes.c_double] + [V] * 17
    h.hc_skel_plan.argtypes = [ctypes.c_int] + [V] * 8
    h.hc_bone_distances.argtypes = [ctypes.c_size_t, ctypes.c_int, V, ctypes.c_int, V, V]
    return h


def run(hc, case, system=False, cov=False, lam=sko.SYSTEM_LAM, xtol=1e-8, weights="case", uvs=None, frames=None):
    sl = slice(None) if frames is None else frames
    uv = np.ascontiguousarray((case["uvs"] if uvs is None else uvs)[:, sl], dtype=np.float64)
    C, T, K = uv.shape[:3]
    cam, dist = sko.tco.camera_blocks(case["ext"], case["intr"])
    w = case["weights"] if isinstance(weights, str) else weights
    w = None if w is None else np.ascontiguousarray(np.asarray(w, dtype=np.float64)[:, sl])
    ps = np.ascontiguousarray(np.broadcast_to(np.asarray(case["pixel_std"], dtype=np.float64), (C,)))
    start = np.ascontiguousarray(case["start"][sl])
    parent, L, s = np.ascontiguousarray(case["parent"], dtype=np.int32), np.ascontiguousarray(case["L"]), np.ascontiguousarray(case["s"])
    x, g, d, u = (np.full((T, K, 3), 7.0) for _ in range(4))
    h6, c6 = np.full((T, K, 6), 7.0), np.full((T, K, 6), 7.0)
    kst, fst, nit = np.full((T, K), 7, np.int32), np.full(T, 7, np.int32), np.full(T, 7, np.int32)
    cost, cost0, dc, bc, tc = (np.full(T, 7.0) for _ in range(5))
    bres, hist, levels = np.full((T, K), 7.0), np.full((T, MAX_ITERATIONS), np.nan), ctypes.c_int(0)
    p = lambda a: None if a is None else a.ctypes.data
    wide = system or cov
    rc = hc.hc_refine_skeleton(int(system), T, K, C, p(uv), p(cam), p(dist), p(w), p(ps), p(start), p(parent), p(L), p(s), sko.LOSSES[case["loss"]], case["f_scale"], MAX_ITERATIONS, xtol, lam,
                               p(x), p(kst), p(fst), p(nit), p(cost), p(cost0), p(bres), p(c6) if cov else None, p(h6) if wide else None, p(u) if wide else None, p(g), p(d), p(dc), p(bc), p(tc),
                               p(hist), ctypes.addressof(levels))
    assert rc == 0
    out = dict(keypoint_status=kst, frame_status=fst, levels=levels.value)
    if system:
        out.update(information=h6[..., SYM], gradient=g, step=d, direction=u, data_cost=dc, bone_cost=bc, trial_cost=tc)
    else:
        out.update(points=x, n_iterations=nit, cost=cost, cost_start=cost0, bone_residual=bres, history=hist)
        if cov:
            out.update(covariance=c6[..., SYM], information=h6[..., SYM], direction=u)
    return out


@pytest.mark.parametrize("name", sko.SYSTEM_CASES)
def test_one_evaluation_against_the_oracle(hc, name):
    got = run(hc, CASES[name], system=True)
    sko.check_system(name, got)
    if name == "K64_chain":
        assert got["levels"] == 64
    if name == "K64_star":
        assert got["levels"] == 2


def test_loop_against_the_oracle(hc):
    left_out = total = 0
    for name in sko.LOOP_CASES:
        got = run(hc, CASES[name], cov=True)
        lo, ran = sko.check_loop(name, got, history=got["history"])
        sko.check_covariance(name, got)
        left_out, total = left_out + lo, total + ran
    print(f"undecided frames {left_out} of {total}")
    assert 10 * left_out <= total, (left_out, total)


def test_special_frames_have_the_statuses_their_comments_say(hc):
    got = run(hc, CASES["special"])
    st = got["keypoint_status"]
    assert list(st[0]) == [2, -1, 2, 2, 2, 2, 2]          # the tree split by the unseen keypoint 1: every piece holds a usable keypoint
    assert list(st[1]) == [2, 2, -1, -2, 2, 2, -2]        # {3, 6}: a piece of singles only
    assert list(st[2]) == [2, 2, 2, 2, 1, 2, 1] and list(st[3]) == [2, 1, 2, 2, 2, 2, 2] and list(st[4]) == [2, 2, 1, 1, 2, 2, 1]
    assert list(st[5]) == [2, 2, 2, 2, 2, -1, 2]
    assert np.isfinite(got["points"][st > 0]).all() and np.isnan(got["points"][st < 0]).all()
    assert np.isnan(got["bone_residual"][1, [0, 2, 3, 6]]).all() and np.isfinite(got["bone_residual"][1, [1, 4, 5]]).all()   # a root; the bones of what is not fitted


def test_a_frame_alone_gives_the_bits_it_gives_among_others(hc):
    case = CASES["K5"]
    full = run(hc, case, cov=True)
    for t in (0, 50, 153):
        one = run(hc, case, cov=True, frames=slice(t, t + 1))
        assert all(np.array_equal(one[f][0], full[f][t], equal_nan=True) for f in ("points", "covariance", "cost", "n_iterations", "keypoint_status", "bone_residual"))


def test_unit_weights_are_no_weights_and_unseen_is_unseen(hc):
    case = CASES["C6"]
    fields = ("points", "covariance", "information", "cost", "cost_start", "n_iterations", "keypoint_status", "frame_status", "bone_residual")
    plain = run(hc, case, cov=True, weights=None)
    ones = run(hc, case, cov=True, weights=np.ones(case["uvs"].shape[:3]))
    assert all(np.array_equal(plain[f], ones[f], equal_nan=True) for f in fields)
    rng = np.random.default_rng(5)
    hit = rng.uniform(size=case["uvs"].shape[:3]) < 0.1
    w = np.array(case["weights"])
    w[hit] = np.where(rng.uniform(size=int(hit.sum())) < 0.5, 0.0, np.nan)
    uv = np.array(case["uvs"])
    uv[hit] = np.nan
    a, b = run(hc, case, cov=True, weights=w), run(hc, case, cov=True, uvs=uv)
    assert all(np.array_equal(a[f], b[f], equal_nan=True) for f in fields)


FORESTS = {"chain": (64, sko.chain(64)), "star": (64, sko.star(64)), "two_pieces": (7, np.array([[0, 2], [2, 5], [1, 3], [3, 4], [3, 6]])), "random_64": (64, sko.random_tree(64, 3)),
           "single": (1, sko.chain(1))}


@pytest.mark.parametrize("name", sorted(FORESTS))
def test_forest_plan_against_the_oracle(hc, name):
    K, bones = FORESTS[name]
    parent, _ = sko.parents_of(bones, K)
    ref = sko.plan(parent)
    par = np.ascontiguousarray(parent, dtype=np.int32)
    one = np.ones(K)
    level, order, cs, ch, out2 = np.full(K, 7, np.int32), np.full(K, 7, np.int32), np.full(K + 1, 7, np.int32), np.full(K, 7, np.int32), np.full(2, 7, np.int32)
    assert hc.hc_skel_plan(K, par.ctypes.data, one.ctypes.data, one.ctypes.data, level.ctypes.data, order.ctypes.data, cs.ctypes.data, ch.ctypes.data, out2.ctypes.data) == 0
    assert np.array_equal(level, ref["level"]) and np.array_equal(order, ref["order"]) and out2[0] == ref["levels"] and out2[1] == 256 // K
    assert [list(ch[cs[k]:cs[k + 1]]) for k in range(K)] == ref["children"]
    assert all(level[parent[k]] == level[k] - 1 for k in range(K) if parent[k] >= 0)
    pos = np.argsort(order)
    assert all(pos[parent[k]] < pos[k] for k in range(K) if parent[k] >= 0)   # parents before children


def test_forest_plan_refuses_what_is_no_forest(hc):
    one = np.ones(4)
    bufs = [np.zeros(5, np.int32) for _ in range(5)]
    call = lambda parent, L=one, s=one: hc.hc_skel_plan(len(parent), np.ascontiguousarray(parent, dtype=np.int32).ctypes.data, L.ctypes.data, s.ctypes.data, *(b.ctypes.data for b in bufs))
    assert call([-1, 0, 1, 2]) == 0
    assert call([1, 2, 0, -1]) == 3 and call([1, 0, -1, -1]) == 3           # cycles
    assert call([-1, 1, 0, 0]) == 2 and call([-1, 4, 0, 0]) == 2 and call([-2, 0, 0, 0]) == 2
    assert call([-1, 0, 0, 0], L=np.array([1.0, 0.0, 1.0, 1.0])) == 4 and call([-1, 0, 0, 0], s=np.array([1.0, 1.0, -1.0, 1.0])) == 4 and call([-1, 0, 0, 0], s=np.array([1.0, 1.0, np.nan, 1.0])) == 4
    assert call([-1, 0, 0, 0], L=np.array([np.nan, 1.0, 1.0, 1.0])) == 0    # a root's entries are ignored


@pytest.mark.parametrize("T", [1, 6, 7])
def test_bone_distances_are_numpys(hc, T):
    rng = np.random.default_rng(T)
    pts = rng.normal(0, 50, (T, 5, 3))
    pts[rng.uniform(size=(T, 5)) < 0.2] = np.nan
    bones = np.ascontiguousarray([[0, 1], [1, 2], [4, 3], [2, 0]], dtype=np.int32)
    dist = np.full((4, T), 7.0)
    hc.hc_bone_distances(T, 5, pts.ctypes.data, 4, bones.ctypes.data, dist.ctypes.data)
    e = pts[:, bones[:, 0]] - pts[:, bones[:, 1]]
    ref = np.sqrt(e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1] + e[..., 2] * e[..., 2]).T
    assert np.array_equal(dist, ref, equal_nan=True)
