"""tests/p3p_oracle.py held to itself, and the reason for the P3P generator pinned on the two oracles: what the 6-point
generator of tests/resection_oracle.py does on a planar cloud, on a cloud 0.05 mm deep and under 60 % wrong detections, and what three points do.
No GPU, no library: numpy alone.

The 6-point samples are those of `resect_cameras` (seed [0, camera]) throughout, and so are the 3-point samples of the first two pins.  The
3-point samples of the outlier pin come from seed 0, the default of `resect_camera`: 5 of the 64 are clean (expected 64 x 0.4^3 = 4.1).  The
3-point draw of seed [0, 3] holds 3 clean samples, and the best of those three keeps 113 of the 120 clean points at 2.5 px (7.5 mm, 0.6 degrees
off; all 120 with 256 samples): the noise of a minimal sample, printed below, not asserted.  Nor is the 6-point failure a law: a draw of 256
six-point samples holds a clean one with probability 1 - (1 - 0.4^6)^256 = 65 %, and the draw of seed 0 does."""
import numpy as np
import pytest

import p3p_oracle as po
import p3p_scenes as ps
import resection_oracle as ro


def cameras_of(name):
    return range(len(po.scene(name)[1]))


@pytest.fixture(scope="module")
def cap_tables():
    """per (scene, camera) of the cap scenes: the inputs, the prepared points, the samples and the oracle's table by the first route"""
    out = {}
    for name in po.CAP_SCENES:
        for cam in cameras_of(name):
            c = po.camera_of(name, cam)
            prep = ro.prepare(c["points"], c["uv"], c["intr"])
            smp = po.samples_of(c["usable"], 64, [0, cam])
            out[(name, cam)] = (c, prep, smp, po.hypotheses(c["points"], prep, smp))
    return out


def test_left_out_samples_stay_under_the_cap(cap_tables):
    for (name, cam), (c, prep, smp, hyp) in cap_tables.items():
        share, live = po.left_out_share(hyp), int((hyp["status"] > 0).sum())
        print(f"{name} camera {cam}: live candidates {live} of 64 samples; non-void samples {int(hyp['sample_live'].sum())}; left out {share:.3%}")
        assert share <= po.LEFT_OUT_CAP and hyp["sample_live"].sum() >= 60
        assert 100 <= live <= 160      # about two candidates per sample


def test_the_two_routes_give_the_same_pose_sets_and_the_measured_multiple(cap_tables):
    worst, where = 0.0, None
    for (name, cam), (c, prep, smp, hyp) in cap_tables.items():
        m, same = po.route_multiple(c["points"], prep, smp)
        print(f"{name} camera {cam}: worst multiple of EPS cond between the routes {m:.3g}; pose sets of equal size {same}")
        assert same
        worst, where = (m, (name, cam)) if m > worst else (worst, where)
    print(f"worst multiple {worst:.3g} at {where}; K_P_MEASURED {po.K_P_MEASURED}, K_P {po.K_P}")
    assert abs(worst - po.K_P_MEASURED) <= 0.25 * po.K_P_MEASURED and 8 * worst <= po.K_P and po.K_P == max(64.0, 8 * po.K_P_MEASURED)


def test_five_iterations_settle_every_candidate(cap_tables):
    """the table behind MCBA_RESECT_P3P_POLISH: the share of live candidates whose step is still above 1e-10 after n iterations"""
    steps = np.array([s for (c, prep, smp, hyp) in cap_tables.values() for o in hyp["per_sample"] for s in o["steps"].values()])
    share = (steps > po.STEP_MAX).mean(0)
    print(f"{len(steps)} candidates; share not settled after 1 .. {po.POLISH} iterations: {np.array2string(share, precision=4)}; largest first step {steps[:, 0].max():.3g}")
    assert len(steps) > 1500 and share[0] > 0.0 and steps[:, 0].max() > 1e-6      # the closed form alone is not the root: the polish is needed
    assert share[-1] == 0.0 and share[-2] == 0.0                                   # ... and five iterations leave a margin of at least one


def test_roots_of_a_known_quartic_and_the_closed_form_on_exact_data():
    """noise-free detections: one candidate of every sample is the true pose, to rounding times the conditioning"""
    import keypoint_scenes as ks
    c = po.camera_of("six", 2)
    R, t = ks.rodrigues(c["ext"][:3]), c["ext"][3:]
    Xc = c["points"] @ R.T + t
    nx = Xc[:, :2] / Xc[:, 2:]
    truth = np.r_[R.ravel(), t]
    smp = po.samples_of(c["usable"], 16, 7)
    hyp = po.hypotheses(c["points"], dict(nx=nx), smp)
    for h in range(16):
        sl = slice(4 * h, 4 * h + 4)
        live = hyp["status"][sl] > 0
        err = np.abs(hyp["pose"][sl][live] - truth).max(1) / np.maximum(1.0, np.abs(truth).max())
        assert live.any() and err.min() <= 1e-9, (h, err)
    # slot order: ascending root
    A, aux = po.grunert(c["points"][smp[0]], po.bearings(nx[smp[0]]))
    real = np.sort(np.roots(A[::-1])[np.isreal(np.roots(A[::-1]))].real)
    assert len(real) in (2, 4) and (np.diff(real) > 0).all()


def test_degenerate_samples_are_void():
    c = po.camera_of("six", 0)
    prep = ro.prepare(c["points"], c["uv"], c["intr"])
    X = np.array(c["points"][:3])
    X[2] = X[0] + 2.5 * (X[1] - X[0])        # collinear world points
    o = po.sample(X, prep["nx"][:3])
    assert (o["status"] == -1).all() and np.isnan(o["pose"]).all()
    x = np.array(prep["nx"][:3])
    x[2] = x[0] + 0.3 * (x[1] - x[0])        # collinear image points
    o = po.sample(c["points"][:3], x)
    assert (o["status"] == -1).all()
    o = po.sample(np.full((3, 3), np.nan), prep["nx"][:3])
    assert (o["status"] == -1).all()


def test_planar_points_void_every_six_point_sample_and_p3p_keeps_all():
    for cam in cameras_of("flat3"):
        c = po.camera_of("flat3", cam)
        o6 = ro.ransac(c["points"], c["uv"], c["intr"], ro.samples_of(c["usable"], 64, [0, cam]), po.THRESHOLD)
        o3 = po.ransac(c["points"], c["uv"], c["intr"], po.samples_of(c["usable"], 64, [0, cam]), po.THRESHOLD)
        dc, dr = po.pose_errors(o3["rt12"], c["ext"])
        print(f"flat3 camera {cam}: 6-point live {int((o6['hyp']['status'] > 0).sum())} of 64, largest eigen-gap {o6['hyp']['gap'].max():.3g}; P3P keeps {o3['n_inliers']} of {o3['n_usable']}, "
              f"centre {dc:.3g} mm, rotation {dr:.3g} degrees")
        assert (o6["hyp"]["status"] == -1).all() and np.isnan(o6["rt12"]).all() and o6["n_inliers"] == 0
        assert o3["n_inliers"] == 200 == o3["n_usable"] and dc < 10.0 and dr < 1.0


def test_a_slab_thinner_than_the_noise_fools_the_six_point_winner():
    c = po.camera_of("hair3", 1, "others")
    o6 = ro.ransac(c["points"], c["uv"], c["intr"], ro.samples_of(c["usable"], 64, [0, 1]), po.THRESHOLD)
    dc, dr = po.pose_errors(o6["rt12"], c["ext"])
    print(f"hair3 camera 1: 6-point live {int((o6['hyp']['status'] > 0).sum())}, winner keeps {o6['n_inliers']} of {o6['n_usable']} (needs {ro.min_inliers(o6['n_usable'])}), centre {dc:.4g} mm, rotation {dr:.4g} degrees")
    assert o6["n_inliers"] >= ro.min_inliers(o6["n_usable"]) and dr > 90.0       # status 1, and wrong
    o3 = po.ransac(c["points"], c["uv"], c["intr"], po.samples_of(c["usable"], 64, [0, 1]), po.THRESHOLD)
    dc, dr = po.pose_errors(o3["rt12"], c["ext"])
    print(f"hair3 camera 1: P3P keeps {o3['n_inliers']} of {o3['n_usable']}, centre {dc:.3g} mm, rotation {dr:.3g} degrees")
    assert o3["n_inliers"] == 200 and dc < 10.0 and dr < 1.0


def test_sixty_percent_wrong_detections():
    c = po.camera_of("swap6", 3)
    clean = ps.make("swap6")[4][3]
    assert clean.sum() == 120
    o6 = ro.ransac(c["points"], c["uv"], c["intr"], ro.samples_of(c["usable"], 256, [0, 3]), po.THRESHOLD)
    o3 = po.ransac(c["points"], c["uv"], c["intr"], po.samples_of(c["usable"], 64, 0), po.THRESHOLD)
    other = po.ransac(c["points"], c["uv"], c["intr"], po.samples_of(c["usable"], 64, [0, 3]), po.THRESHOLD)
    print(f"swap6 camera 3, 3-point samples of seed [0, 3]: keeps {other['n_inliers']}")
    dc, dr = po.pose_errors(o3["rt12"], c["ext"])
    print(f"swap6 camera 3: best of 256 6-point hypotheses keeps {int(o6['score']['count'].max())}; 64 P3P samples keep {o3['n_inliers']} ({int((o3['inliers'] & clean).sum())} clean), centre {dc:.3g} mm, "
          f"rotation {dr:.3g} degrees")
    assert o6["score"]["count"].max() < 12 and o6["n_inliers"] < ro.min_inliers(300)
    assert o3["n_inliers"] == 120 and np.array_equal(o3["inliers"], clean)
