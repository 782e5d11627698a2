"""k_triangulate<2..8> and k_triangulate_wave at every launch regime, held to the conditioning-scaled enclosure of tests/triangulate_bounds.py
(its docstring has the bound; tests/test_triangulate_bounds_cpu.py holds the bar itself and the host build to the same cases).  Inputs and
enclosures are made on the CPU; every case is a few points."""
import ctypes

import numpy as np
import pytest

import triangulate_bounds as tb

pytestmark = pytest.mark.gpu

SENTINEL = -7.25e77   # what the outputs hold before a call that reaches the C entry point directly


@pytest.fixture(scope="module")
def mc():
    import multicam_calibration_amd as m

    m.ops.load_library()
    return m


def _direct(mc, c):
    """mcba_triangulate itself, the output pre-filled with SENTINEL: dist5 = NULL (k1, k2 of the camera block count), or dist5 given beside
    other numbers in the camera block's k1, k2 (dist5 counts)"""
    uv = np.ascontiguousarray(np.stack(c.uvs), dtype=np.float64)
    C, P = uv.shape[:2]
    cam, dist = mc.triangulation._cam_blocks(c.ext, c.intr)
    if c.direct == "null_dist":
        assert not dist[:, 2:].any()
        dist_at = None
    else:
        cam[:, 4:6] = 0.3, -0.2
        dist_at = dist.ctypes.data
    out = np.full((P, 3), SENTINEL)
    ms = ctypes.c_double(0.0)
    mc.ops.call("mcba_triangulate", C, P, uv.ctypes.data, cam.ctypes.data, dist_at, int(c.iterations), 0, out.ctypes.data, ctypes.addressof(ms))
    assert not (out == SENTINEL).any(), c.label
    return out


def _run(mc, c):
    return _direct(mc, c) if c.direct else mc.triangulate(c.uvs, c.ext, c.intr, undistort_iterations=c.iterations)


@pytest.mark.parametrize("regime", tb.regimes())
def test_every_case_of_the_regime_lies_in_its_enclosure(mc, regime):
    """Register kernels: C = 2 .. 8 at 1, 255, 256 and 257 points.  Wave kernel: both ends of every points-per-workgroup row at 1, ppb - 1, ppb,
    ppb + 1 and 2 ppb + 1 points.  Views: every number of seeing cameras from 0 to C at C = 4, 8, 12, and a single missing coordinate.
    Undistortion: 0, 1, 5, 20 rounds, k1 k2 from the camera block against dist5, a detection past the model's valid radius, at C = 3 and 9."""
    cases = [c for c in tb.gpu_cases() if c.regime == regime]
    assert cases
    worst = 0.0
    for c in cases:
        lo, hi = tb.case_enclosure(c.label)
        assert tb.half_width_ratio(lo, hi) <= tb.HALF_WIDTH_MAX, c.label
        worst = max(worst, tb.check(c.label, _run(mc, c), lo, hi))
    print("GPU, %s: worst position %.3g of the half-width over %d cases" % (regime, worst, len(cases)))


@pytest.mark.parametrize("label", ["C=5 P=257", "C=43 P=5"])   # one lane per point; one wavefront per point
def test_two_calls_return_the_same_bits(mc, label):
    c = next(c for c in tb.gpu_cases() if c.label == label)
    first = _run(mc, c)
    assert not np.isnan(first).all()
    assert first.tobytes() == _run(mc, c).tobytes()
