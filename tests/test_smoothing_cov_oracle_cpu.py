"""The reference of trajectory_uncertainty (tests/smoothing_cov_oracle.py) held to itself, without a GPU: its two routes -- the inverse of the
Jacobi-scaled dense matrix in double, a banded Cholesky inverse in np.longdouble -- agree within a quarter of the bar on every case, so the
reference never eats the margin; an unusable frame has a finite, positive definite covariance that grows into a gap; and the library's recursion,
transcribed into numpy, meets the bar at segment 2 and 3."""
import numpy as np
import pytest

import smoothing_cov_oracle as sc
import smoothing_oracle as so

LINEAR = so.linear_cases()


def tracks(name):
    case = LINEAR[name]
    for k, ref in enumerate(sc.case_reference(name, case)):
        if ref is not None:
            yield k, ref


@pytest.mark.parametrize("name", sorted(LINEAR))
def test_the_two_routes_agree(name):
    n = 0
    for k, ref in tracks(name):
        diag, lag = sc.longdouble_band(ref["A"])
        err, bar = sc.scaled_error(diag.astype(np.float64), lag.astype(np.float64), ref), sc.bar_of(ref)
        print(f"{name} track {k}: cond {ref['cond']:.3g} routes differ by {err:.3g}, {err / bar:.3g} of the bar")
        assert err <= sc.ROUTES_AGREE * bar, (name, k, err, bar)
        assert abs(ref["zmax"] - np.abs(ref["diag"] * (ref["s"].reshape(-1, 3)[:, :, None] * ref["s"].reshape(-1, 3)[:, None, :])).max()) <= 1e-12 * ref["zmax"]   # the maximum is on the diagonal
        n += 1
    assert n >= 1 or name == "T1"


@pytest.mark.parametrize("name", ["gaps_seg2", "gaps_seg3", "bad_cov", "T400_default"])
def test_unusable_frames_have_a_positive_definite_covariance(name):
    seen = 0
    for k, ref in tracks(name):
        for t in np.flatnonzero(~ref["usable"]):
            assert np.isfinite(ref["diag"][t]).all() and np.linalg.eigvalsh(ref["diag"][t]).min() > 0, (name, k, t)
            seen += 1
    assert seen > 0


def test_the_uncertainty_grows_into_a_gap():
    """T400_default, frames 100 .. 139 missing: the middle of the gap is less certain than its edges"""
    for k, ref in tracks("T400_default"):
        assert not ref["usable"][100:140].any() and ref["usable"][99] and ref["usable"][140]
        tr = np.trace(ref["diag"], axis1=1, axis2=2)
        print(f"track {k}: trace at 99, 120, 140: {tr[99]:.3g} {tr[120]:.3g} {tr[140]:.3g}")
        assert tr[120] > tr[99] and tr[120] > tr[140]


@pytest.mark.parametrize("segment", [2, 3])
@pytest.mark.parametrize("name", sorted(LINEAR))
def test_the_recursion_meets_the_bar(name, segment):
    for k, ref in tracks(name):
        T = len(ref["diag"])
        diag, lag = sc.selinv_transcription(ref["A"], T, segment)
        assert np.isfinite(diag).all() and np.isfinite(lag).all()
        err, bar = sc.scaled_error(diag, lag, ref), sc.bar_of(ref)
        print(f"{name} segment {segment} track {k}: err {err:.3g} bar {bar:.3g} ratio to eps cond max|zhat| {err / (bar / sc.BAR_K):.3g}")
        assert err <= bar, (name, segment, k, err, bar)
