"""CPU tier of the sparse-Schur handle: the wide-rig visibility option of synth.make_problem, the public switches, the C-ABI additions."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT


def test_visible_k_leaves_every_other_output_unchanged():
    from multicam_calibration_amd import synth

    for kw in (dict(), dict(missing=0.2), dict(scalar_nans=7, outlier_frames=2), dict(frame_seed=3)):
        a = synth.make_problem(12, 40, rows=2, cols=3, **kw)
        b = synth.make_problem(12, 40, rows=2, cols=3, visible_k=12, **kw)   # every camera kept: byte-identical
        c = synth.make_problem(12, 40, rows=2, cols=3, visible_k=3, **kw)
        assert a["uvs"].tobytes() == b["uvs"].tobytes()
        for k in ("obj", "true_cam", "true_poses", "extrinsics", "poses"):
            assert a[k].tobytes() == c[k].tobytes(), k
        same = ~np.isnan(c["uvs"])
        assert np.array_equal(c["uvs"][same], a["uvs"][same])   # visibility only removes detections


def test_visible_k_keeps_the_k_nearest_cameras_on_the_ring():
    """Brute force: per frame, the cameras kept are the k of smallest azimuth gap to the board centre (recomputed from the generator's draws)."""
    from multicam_calibration_amd import synth

    C, F, k = 16, 60, 4
    p = synth.make_problem(C, F, rows=2, cols=3, visible_k=k)
    seen = ~np.isnan(p["uvs"]).all(axis=(2, 3))
    assert (seen.sum(0) == k).all()
    # the same draws as make_problem: camera azimuths, then (rotation, translation) of every frame
    rng = np.random.default_rng(0)
    phi = 2 * np.pi * (np.arange(C) + 0.25 * rng.uniform(-1, 1, C)) / C
    rng.uniform(1100, 1200, C); rng.uniform(0.99, 1.01, C); rng.uniform(-15, 15, C); rng.uniform(-15, 15, C); rng.uniform(-0.1, -0.05, C); rng.uniform(-0.005, 0.005, C)
    rng.normal(0, 0.6, (F, 3))
    tr = rng.normal(0, 60.0, (F, 3))
    for f in range(F):
        az = np.arctan2(tr[f, 1], tr[f, 0])
        gap = [abs((phi[c] - az + np.pi) % (2 * np.pi) - np.pi) for c in range(C)]
        assert set(np.flatnonzero(seen[:, f])) == set(np.argsort(gap, kind="stable")[:k]), f
    with pytest.raises(ValueError):
        synth.make_problem(4, 5, visible_k=5)


def test_header_declares_the_sparse_handle():
    src = open(os.path.join(ROOT, "include", "mcba.h")).read()
    for name in ("mcba_create_sparse", "mcba_is_sparse"):
        assert re.search(r"\b%s\s*\(" % name, src), name
    from multicam_calibration_amd import ops

    names = {s[0] for s in ops.SYMBOLS}
    assert {"mcba_create_sparse", "mcba_is_sparse"} <= names


def test_profiling_names_include_the_sparse_kernels():
    from multicam_calibration_amd import build, ops

    build.build()
    names = ops.load_library().mcba_profile_names().decode().split("\n")
    for k in ("k_sp_factor", "k_sp_pairs", "k_sp_solve_pre", "k_sp_potrf", "k_sp_trsm", "k_sp_update", "k_sp_finish"):
        assert k in names
    assert names[:10] == ["k_transpose_obs", "k_gram", "k_cost", "k_syrk", "k_reduce_system", "k_backsub", "k_sum_trial", "k_jacobian", "k_decide", "k_solve_cam"]


def test_schur_switch_is_checked_before_the_device():
    from multicam_calibration_amd import ops, synth
    import multicam_calibration_amd as m

    p = synth.make_problem(2, 3)
    with pytest.raises(ValueError, match="schur"):
        ops.Problem(p["uvs"], p["obj"], schur="banded")
    with pytest.raises(ValueError, match="schur"):
        m.bundle_adjust(p["uvs"], p["extrinsics"], p["intrinsics"], p["obj"], p["poses"], schur="banded", verbose=0)


def test_no_gpu_sparse_handle_is_a_loud_error():
    from multicam_calibration_amd import ops

    n = ctypes.c_int()
    rc = ops.load_library().mcba_device_count(ctypes.byref(n))
    if rc == 0 and n.value > 0:
        pytest.skip("a GPU is visible here")
    with pytest.raises(ops.McbaError):
        ops.Problem(np.zeros((64, 3, 4, 2)), np.zeros((4, 3)), schur="sparse")
    # the dense handle keeps refusing more than 40 cameras, and now names the way out
    with pytest.raises(ops.McbaError, match="at most 40.*sparse"):
        ops.Problem(np.zeros((41, 3, 4, 2)), np.zeros((4, 3)))


def _sparse_index(seen):
    """mcba_sparse_index (the sparse handle's visibility index, host code) -> its seven arrays."""
    from multicam_calibration_amd import ops

    lib = ops.load_library()
    C, F = seen.shape
    s = np.ascontiguousarray(seen, dtype=np.uint8)
    sizes = (ctypes.c_int * 4)()
    assert lib.mcba_sparse_index(s.ctypes.data, C, F, sizes, None, 0) == 0
    nent, npairs, nitems, nchunks = list(sizes)
    lens = [F + 1, nent, nent, 3 * nitems, 3 * nchunks, C * C, npairs + 1]
    out = np.zeros(sum(lens), dtype=np.int32)
    assert lib.mcba_sparse_index(s.ctypes.data, C, F, sizes, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), out.size) == 0
    parts = np.split(out, np.cumsum(lens)[:-1])
    return dict(zip(("frame_off", "ent_cam", "ent_frame", "items", "chunks", "pair_map", "pair_chunks"), parts)), (nent, npairs, nitems, nchunks)


@pytest.mark.parametrize("C,F,density,seed", [(1, 1, 1.0, 0), (5, 300, 0.5, 1), (41, 200, 0.15, 2), (64, 120, 0.05, 3), (7, 150, 1.0, 4)])
def test_visibility_index_against_brute_force(C, F, density, seed):
    """The host builder behind the sparse handle's reduction, against a direct O(C^2 F) construction: entries frame-major with cameras
    ascending, co-visible pairs (i <= j) in (i, j) order with their frames ascending, chunks of at most 64 frames in order."""
    rng = np.random.default_rng(seed)
    seen = rng.uniform(size=(C, F)) < density
    if C > 2:
        seen[2] = False                        # a camera seen in no frame
    x, (nent, npairs, nitems, nchunks) = _sparse_index(seen)
    # entries
    ent = [(c, f) for f in range(F) for c in range(C) if seen[c, f]]
    assert nent == len(ent)
    assert [(int(c), int(f)) for c, f in zip(x["ent_cam"], x["ent_frame"])] == ent
    assert list(x["frame_off"]) == [0] + list(np.cumsum(seen.sum(0)))
    eidx = {cf: e for e, cf in enumerate(ent)}
    # pairs, items
    pairs = [(i, j) for i in range(C) for j in range(i, C) if (seen[i] & seen[j]).any()]
    assert npairs == len(pairs)
    pm = x["pair_map"].reshape(C, C)
    expect_pm = -np.ones((C, C), int)
    for p, (i, j) in enumerate(pairs):
        expect_pm[i, j] = p
    assert np.array_equal(pm, expect_pm)
    items = [(eidx[(i, f)], eidx[(j, f)], f) for (i, j) in pairs for f in np.flatnonzero(seen[i] & seen[j])]
    assert nitems == len(items)
    assert [tuple(int(v) for v in t) for t in x["items"].reshape(-1, 3)] == items
    # chunks
    chunks, pc, start = [], [0], 0
    for i, j in pairs:
        cnt = int((seen[i] & seen[j]).sum())
        for s in range(0, cnt, 64):
            chunks.append((start + s, min(64, cnt - s), int(i == j)))
        start += cnt
        pc.append(len(chunks))
    assert nchunks == len(chunks)
    assert [tuple(int(v) for v in t) for t in x["chunks"].reshape(-1, 3)] == chunks
    assert list(x["pair_chunks"]) == pc


def test_visibility_index_output_too_small_is_refused():
    from multicam_calibration_amd import ops

    lib = ops.load_library()
    seen = np.ones((3, 4), np.uint8)
    sizes = (ctypes.c_int * 4)()
    out = np.zeros(5, np.int32)
    assert lib.mcba_sparse_index(seen.ctypes.data, 3, 4, sizes, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), out.size) == ops.ERR_ARG
