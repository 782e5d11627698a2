"""csrc/mcba_kpba_math.h on the wide rigs of refine_extrinsics(reduction="tiled") (25 to 64 cameras; tests/kpba_wide.py), without a GPU: the g++
build of tests/hostcheck/kpba_hostcheck.cpp -- the loop the C ABI runs, sized by vectors, no camera limit of its own -- held to the bars of
SURVEY.md section 8f-12 on every pinned case of tests/golden/kpba_wide.npz: at ftol = xtol = 1e-15, gtol = 1e-10 cost <= golden (1 + 1e-10),
extrinsics within 1e-6 relative after the closing step, used points within max(1e-6 relative, 10 x the golden's own two-start spread).  Then one
evaluation of the host build on every input of the tiled path's one-evaluation tests (tests/test_gpu_kpba_tiled.py) against
kpba_oracle.block_system, within kpba_oracle's bounds: they hold on the reference path before the tiled kernels are held to them.  The two inputs
of the grid stride are left to the GPU tier (a stride means nothing in plain loops, and their oracle takes half a minute)."""
import numpy as np
import pytest

import kpba_oracle as ko
import kpba_wide as kw
from test_hostcheck_kpba import P, bits, hc, host_evaluation, host_refine  # noqa: F401  (hc: the fixture that builds the host library)

HOST_WORST = {}


def test_every_wide_case_is_in_the_golden_file():
    g = kw.golden()
    assert all(f"{n}/extrinsics" in g for n in kw.CASES)
    for n in kw.CASES:
        print(f"{n}: two-start spread extrinsics {float(g[f'{n}/spread_ext']):.3g} relative, points {float(g[f'{n}/spread_pts']):.3g} absolute, pinned {bool(g[f'{n}/pinned'])}")
        assert bool(g[f"{n}/pinned"]) == (float(g[f"{n}/spread_ext"]) <= ko.TWO_START_RULE)
        assert g[f"{n}/ext0"].shape == (kw.CASES[n][0], 6) and g[f"{n}/pts0"].shape == (kw.CASES[n][1], 3)


@pytest.mark.parametrize("name", kw.pinned_cases())
def test_host_loop_reaches_the_golden_optimum(hc, name):  # noqa: F811
    i, o = kw.case(name)
    got = host_refine(hc, i["uvs"], i["ext0"], i["intr"], i["pts0"], o["held"], o["scale_camera"], loss=i["loss"])
    print(f"{name}: status {got['status']} nfev {got['nfev']} njev {got['njev']} optimality {got['optimality']:.3g} scale {got['scale']:.15g}")
    assert np.array_equal(got["held_bits"], bits(o["held"]))
    ko.check_result(name, got["extrinsics"], got["points"], got["cost"], o)
    assert got["cost"] <= got["cost0"] and got["status"] in (1, 2, 3)
    base0 = ko.baseline_of(i["ext0"], 0, o["scale_camera"])
    assert abs(ko.baseline_of(got["extrinsics"], 0, o["scale_camera"]) / base0 - 1) <= 1e-12
    X = np.where(np.isnan(got["points"]), i["pts0"], got["points"])
    assert abs(ko.cost_of(got["extrinsics"], X, i["uvs"], i["intr"], i["loss"]) / got["cost"] - 1) <= 1e-10


def test_start_at_the_optimum_ends_within_two_evaluations(hc):  # noqa: F811
    i, o = kw.case("w32")
    X = np.where(np.isnan(o["points"]), i["pts0"], o["points"])
    got = host_refine(hc, i["uvs"], o["extrinsics"], i["intr"], X, o["held"], o["scale_camera"], ftol=1e-8, xtol=1e-8, gtol=1e-8)
    print(f"w32: nfev {got['nfev']} status {got['status']} cost {got['cost']:.15g} golden {o['cost']:.15g}")
    assert got["nfev"] <= 2 and got["status"] > 0 and abs(got["cost"] / o["cost"] - 1) <= 1e-12


@pytest.mark.parametrize("name", [n for n in kw.INPUTS if n not in kw.STRIDE])
def test_one_evaluation_against_the_block_oracle(hc, name):  # noqa: F811
    i, o = kw.system_case(name)
    got = host_evaluation(hc, i)
    r = ko.check_block(name, got, o)
    r.update(ko.check_step(name, got["trial_points"], got["step4"], o, i["pts0"], i["uvs"], i["intr"], i["loss"], i["f_scale"]))
    ko.note_worst(HOST_WORST, r)
    print(ko.worst_line("host build on the wide inputs so far", HOST_WORST))


def test_dense_solve_of_377_rows(hc):  # noqa: F811
    """the free scalars of 64 cameras (6 x 64 - 6 - 1): nothing in kpba_dense_solve is sized by the resident reduction's 143"""
    rng = np.random.default_rng(5)
    n = 377
    M = rng.normal(size=(n + 3, n)) * np.logspace(0, 3, n)
    A, b, x = np.ascontiguousarray(M.T @ M), rng.normal(size=n), np.empty(n)
    ref = np.linalg.solve(A, b)
    assert hc.hc_kpba_dense_solve(n, P(A.copy()), P(b), P(x)) == 1
    assert np.abs(x - ref).max() <= 1e-8 * np.abs(ref).max()


def test_partial_cap_rule():
    """the cap of partial systems (kpba_wide.partial_cap, the restatement the GPU tier holds the launch facts to): together no more than 512
    partials of 24 cameras, a power of two; 64 at 64 cameras, 512 up to 24"""
    assert kw.partial_cap(64) == 64 and kw.partial_cap(24) == 512 and kw.partial_cap(2) == 512 and kw.partial_cap(25) == 256
    for C in range(2, 65):
        cap = kw.partial_cap(C)
        assert cap & (cap - 1) == 0 and cap * kw.partial_size(C) <= 512 * kw.partial_size(24) and (cap == 512 or 2 * cap * kw.partial_size(C) > 512 * kw.partial_size(24))
