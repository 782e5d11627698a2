"""The kernels of csrc/mcba_kpcam.hip, one evaluation at a time: what k_kpba_status, k_kpcam_reduce + k_kpba_finish and k_kpcam_step wrote
(geometry.refine_cameras_system, the loop's own set-up and launches run once) against the long-double block statement of the same evaluation
(kpcam_oracle.block_system12), piece by piece and within kpba_oracle's bounds.  Nothing is iterated: a case is one evaluation (a reduction and a
step), or a few of them on one input where they are compared with each other.  tests/test_hostcheck_kpcam.py holds the host build to the same
oracle on the same inputs first.

Shapes (kpcam_oracle.SYSTEM_INPUTS):
  cameras   2 (NP 32), 3 (48: three tiles, 12 padding rows), 4 (48: no padding), 5 (64: 10 tiles, the last count with three tiles per wavefront),
            6 (80: 15 tiles, the first with twelve; the group falls to 32 by LDS), 11 and 12 (144: 45 tiles, the cap); 70 points, 40 % unseen, two
            calls the same bits
  groups    G - 1, G, G + 1 points for G = 16, 32, 64 at 6 cameras under every group size that fits there (16 and 32: the 80-row panel of 64
            points does not fit 160 KiB); a forced 16 at 2, 3 and 12 cameras; the three systems (16, 32, 64) of one 3-camera input within
            twice the bound of each other
  points    255, 256, 257 at 3 cameras; 600 with an all-NaN second chunk; 257 with one usable point per chunk; 131072 / 131073 at 2 cameras
            (512 and 513 chunks: the grid stride), the last point a used one
  losses    all five on "outlier" at f_scale 1, 1.5, 3 and damping 0, 1e-4, 1
  held      gauge camera 0xFC0, one scale bit, a camera at 0b101010101010, a camera without detections at 0xFFF; all intrinsic bits held;
            only fx free
  weights   levels 0, 1/4, 1, 4 on one 6-camera input against block_system12 with sqrt(w) folded into f, A, B
  cross     with all intrinsic bits held, rows 6 .. 11 of each camera's block against refine_extrinsics_system on the same input
Every case prints each error as a fraction of its bound before it asserts."""
import numpy as np
import pytest

import kpba_oracle as ko
import kpcam_oracle as kc
from multicam_calibration_amd.geometry import refine_cameras_system, refine_extrinsics_system

gpu = pytest.mark.gpu
LDS_LIMIT = 160 * 1024   # what a workgroup of the MI355X may ask for
WORST = {}


def fitting_groups(C):
    """the layout in the header comment of csrc/mcba_kpcam.hip: dynamic LDS 256 * 13 + 102 C + NP (3 G + 1) doubles, NP = 12 C rounded up to 16,
    12 KiB of static LDS counted with it"""
    NP = (12 * C + 15) // 16 * 16
    return [G for G in (64, 32, 16) if 8 * (256 * 13 + 102 * C + NP * (3 * G + 1)) + 12 * 1024 <= LDS_LIMIT]


def expected_group(C, forced=None):
    fits = fitting_groups(C)
    return forced if forced in fits else fits[0]


def evaluate(i, **over):
    kw = dict(points=i["pts0"], held=i["held"], lam=i["lam"], loss=i["loss"], f_scale=i["f_scale"], step=i["step"])
    kw.update(over)
    return refine_cameras_system(i["uvs"], i["ext0"], i["intr"], **kw)


def check(name, i, o, got, group=None, weights=None):
    C, P = len(i["ext0"]), len(i["pts0"])
    print(f"{name}: group {got['group']} workgroups {got['workgroups']} NP {got['NP']} kernel_ms {got['kernel_ms']:.3f}")
    assert got["group"] == expected_group(C, group) and got["workgroups"] == min((P + 255) // 256, 512) and got["NP"] == (12 * C + 15) // 16 * 16
    r = kc.check_block12(name, got, o)
    r.update(kc.check_step12(name, got["trial_points"], got["step4"], o, i["pts0"], i["uvs"], i["intr"], i["loss"], i["f_scale"], weights))
    ko.note_worst(WORST, r)
    print(ko.worst_line("kernels so far", WORST))
    return r


def same_bits(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in ("point_status", "system", "trial_points", "step4")) and (a["group"], a["workgroups"], a["NP"]) == (b["group"], b["workgroups"], b["NP"])


def test_the_groups_that_fit():
    assert fitting_groups(2) == [64, 32, 16] and fitting_groups(5) == [64, 32, 16] and fitting_groups(6) == [32, 16] and fitting_groups(12) == [32, 16]


@gpu
@pytest.mark.parametrize("C", kc.CAMERA_COUNTS)
def test_camera_counts(C):
    i, o = kc.system_case(f"c{C}")
    got = evaluate(i)
    check(f"c{C}", i, o, got)
    assert same_bits(got, evaluate(i))


@gpu
@pytest.mark.parametrize("C", [2, 3, 12])
def test_forced_group_of_16(monkeypatch, C):
    monkeypatch.setenv("MCBA_KPCAM_G", "16")
    i, o = kc.system_case(f"c{C}")
    check(f"c{C} (G = 16)", i, o, evaluate(i), group=16)


def compare_groups(name, got, o, C):
    cond = float(o["cond"].max())
    Ud = np.sqrt(np.diagonal(o["U"]))
    bM = 2 * ko.BOUND_FACTOR * cond * ko.EPS * np.outer(Ud, Ud)
    bv = 2 * ko.BOUND_FACTOR * ko.EPS * Ud * (cond * o["fnorm"] + o["maxdet"] * np.sqrt(o["count"]))
    n = 12 * C
    sizes = sorted(got)
    for x, a in enumerate(sizes):
        for b in sizes[x + 1:]:
            (Ua, ga, za), (Ub, gb, zb) = kc.unpack_acc12(got[a]["acc"]), kc.unpack_acc12(got[b]["acc"])
            r = [ko._ratio(np.abs(got[a]["YY"][:n, :n] - got[b]["YY"][:n, :n]), bM), ko._ratio(np.abs(Ua - Ub), bM), ko._ratio(np.abs(ga - gb), bv), ko._ratio(np.abs(za - zb), bv)]
            print(f"{name}: G = {a} against G = {b}: YY, U, gc, Yz differences / twice the bound", " ".join(f"{v:.3g}" for v in r))
            assert max(r) <= 1
            # the point steps do not depend on the group size
            assert np.array_equal(got[a]["trial_points"], got[b]["trial_points"], equal_nan=True) and np.array_equal(got[a]["step4"], got[b]["step4"])


@gpu
@pytest.mark.parametrize("n", kc.GROUP_EDGES)
def test_group_edges_at_six_cameras(monkeypatch, n):
    """G - 1, G, G + 1 points for G = 16, 32, 64, each under every group size that fits 6 cameras (a forced 64 falls back to 32: asserted)"""
    i, o = kc.system_case(f"g6_p{n}")
    got = {}
    for G in (16, 32, 64):
        monkeypatch.setenv("MCBA_KPCAM_G", str(G))
        g = evaluate(i)
        check(f"g6_p{n} (G = {G})", i, o, g, group=G)
        if G in fitting_groups(6):
            got[G] = g
        else:
            assert same_bits(g, got[32])
    compare_groups(f"g6_p{n}", got, o, 6)


@gpu
@pytest.mark.parametrize("name", ["c3", "p257"])
def test_three_group_sizes_of_one_input(monkeypatch, name):
    i, o = kc.system_case(name)
    got = {}
    for G in (16, 32, 64):
        monkeypatch.setenv("MCBA_KPCAM_G", str(G))
        got[G] = evaluate(i)
        check(f"{name} (G = {G})", i, o, got[G], group=G)
    compare_groups(name, got, o, 3)


@gpu
@pytest.mark.parametrize("name", ["p255", "p256", "p257", "p600_gap", "p257_last"])
def test_point_counts_around_a_chunk(name):
    i, o = kc.system_case(name)
    check(name, i, o, evaluate(i))


@gpu
@pytest.mark.parametrize("name", kc.BIG)
def test_512_and_513_chunks(name):
    i, o = kc.system_case(name)
    assert o["used"][-1]   # the one point of chunk 513 takes part, or a pass that never reaches it shows nowhere
    got = evaluate(i)
    check(name, i, o, got)
    if name.endswith("131073"):
        assert same_bits(got, evaluate(i))


@gpu
@pytest.mark.parametrize("loss,f_scale,lam", kc.LOSS_GRID)
def test_losses_scales_and_dampings(loss, f_scale, lam):
    name = f"outlier_{loss}_{f_scale}_{lam}"
    i, o = kc.system_case(name)
    check(name, i, o, evaluate(i))


@gpu
def test_held_bits():
    """rows and columns of held scalars of Y Y^T and their sum Y z are exactly zero (check_block12 asserts it for every case; here every kind of
    held camera is present), U and g_c of a held camera are not touched by the bits, and a camera without detections has a zero block"""
    i, o = kc.system_case("held")
    got = evaluate(i)
    check("held", i, o, got)
    bits = kc.held_bits12(i["held"])
    assert bits[0] == 0xFC0 and bits[2] == 0b101010101010 and bits[3] == 0xFFF and bin(bits[1]).count("1") == 1
    assert (got["acc"][3] == 0.0).all() and (got["acc"][0, 78:90] != 0.0).all() and (got["acc"][0, 96:] == 0.0).all() and (got["acc"][0, 90:96] != 0.0).all()
    assert same_bits(got, evaluate(i, held=bits))
    alone = evaluate(i, step=None)   # without a step: the same system, nothing else
    assert np.array_equal(alone["system"], got["system"]) and np.array_equal(alone["point_status"], got["point_status"]) and "trial_points" not in alone


@gpu
@pytest.mark.parametrize("name", ["intr_held", "fx"])
def test_held_intrinsics(name):
    i, o = kc.system_case(name)
    check(name, i, o, evaluate(i))


@gpu
def test_weights_against_the_folded_oracle():
    """levels 0, 1/4, 1, 4: the system and the step are those of block_system12 with sqrt(w) folded into f, A and B; a weight 0 is unseen"""
    i, _ = kc.system_case("c6")
    C, P = len(i["ext0"]), len(i["pts0"])
    w = np.random.default_rng(77).choice([0.0, 0.25, 1.0, 4.0], size=(C, P))
    o = kc.block_system12(i["uvs"], i["ext0"], i["intr"], i["pts0"], i["held"], loss=i["loss"], f_scale=i["f_scale"], lam=i["lam"], step=i["step"], weights=w)
    got = evaluate(i, weights=w)
    check("c6 weighted", i, o, got, weights=w)
    assert same_bits(got, evaluate(i, weights=w))
    ones = evaluate(i, weights=np.ones((C, P)))
    plain = evaluate(i)
    assert np.array_equal(ones["point_status"], plain["point_status"]) and np.array_equal(ones["system"], plain["system"])   # (times 1.0 is exact)


@gpu
def test_extrinsic_rows_agree_with_refine_extrinsics_system():
    """with all intrinsic bits held: rows and columns 6 .. 11 of each camera's block within the sum of both bounds of the six-row kernels' on the
    same input; point_status exactly"""
    i, o = kc.system_case("intr_held")
    got = evaluate(i)
    h6 = i["held"][:, 6:]
    six = refine_extrinsics_system(i["uvs"], i["ext0"], i["intr"], points=i["pts0"], held=h6, lam=i["lam"], loss=i["loss"], f_scale=i["f_scale"], step=(i["step"][0][:, 6:], i["step"][1][:, 6:]))
    C = len(i["ext0"])
    sel = np.flatnonzero(np.tile(np.r_[np.zeros(6, bool), np.ones(6, bool)], C))
    U12, g12, z12 = kc.unpack_acc12(got["acc"])
    U6, g6, z6 = ko.unpack_acc(six["acc"])
    cond = float(o["cond"].max())
    Ud = np.sqrt(np.diagonal(o["U"]))[sel]
    bM = 2 * ko.BOUND_FACTOR * cond * ko.EPS * np.outer(Ud, Ud)
    bv = 2 * ko.BOUND_FACTOR * ko.EPS * Ud * (cond * o["fnorm"] + o["maxdet"] * np.sqrt(o["count"]))
    r = dict(YY=ko._ratio(np.abs(got["YY"][np.ix_(sel, sel)] - six["YY"][:6 * C, :6 * C]), bM), U=ko._ratio(np.abs(U12[np.ix_(sel, sel)] - U6), bM), gc=ko._ratio(np.abs(g12[sel] - g6), bv),
             Yz=ko._ratio(np.abs(z12[sel] - z6), bv), cost=ko._ratio(abs(got["cost"] - six["cost"]), 2 * ko.cost_bound(o["cost"], o["fnorm"], o["maxdet"], o["count"])))
    print("12 rows against 6 rows, differences / sum of both bounds:", " ".join(f"{k} {v:.3g}" for k, v in r.items()))
    assert np.array_equal(got["point_status"], six["point_status"]) and got["count"] == six["count"]
    assert all(v <= 1 for v in r.values())
    # intrinsics held and no intrinsic step: the same point steps to the last bit is not promised (q sums 12 columns, six of them times zero), the bound is
    assert np.abs(got["trial_points"] - six["trial_points"])[o["used"]].max() <= 2 * (o["dX_bound"][o["used"]] + 4 * ko.EPS * np.abs(i["pts0"][o["used"]])).max()
