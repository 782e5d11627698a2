"""Golden for a WIDE rig (the sparse-Schur handle): the reference's own bundle_adjust() on 48 cameras x 150 frames x a 2 x 3 board, each frame
seen by the 8 cameras nearest its board on the ring (synth.make_problem(visible_k=8)) and 10 % of the remaining detections missing.

    python tests/golden/make_golden_wide.py <reference checkout (the directory that holds multicam_calibration/)>

The reference is loaded unmodified (an empty stub for cv2, which bundle_adjust never calls) and run with tight tolerances passed through
its **opt_kwargs to scipy's least_squares (LSMR with tight atol / btol, so that it does not stall short of the optimum), every frame kept (n_frames=None) and no outlier rejection.  Stored: x, cost, counters, the frame choice,
and a checksum of the inputs, which the test regenerates from the seed.  The point is then polished by scipy's least_squares on the
reference's own residual function (same loss and scaling) with the exact trust-region solve on the oracle's analytic Jacobian, until the
gradient is at round-off level.  -> wide_48x150.npz"""
import contextlib
import importlib.util
import io
import os
import sys
import time
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from multicam_calibration_amd import synth  # noqa: E402
from oracle import ba_oracle as orc  # noqa: E402
from scipy.optimize import least_squares  # noqa: E402

SHAPE = dict(n_cameras=48, n_frames=150, rows=2, cols=3, pitch=60.0, seed=7, perturb_seed=1, missing=0.1, visible_k=8)
TOL = dict(ftol=1e-14, xtol=1e-14, gtol=1e-14, max_nfev=300, tr_options=dict(atol=1e-15, btol=1e-15))


def load_reference(ref_root):
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    src = os.path.join(ref_root, "multicam_calibration")
    pkg = types.ModuleType("multicam_calibration")
    pkg.__path__ = [src]
    sys.modules["multicam_calibration"] = pkg
    mods = {}
    for name in ("geometry", "bundle_adjustment"):
        spec = importlib.util.spec_from_file_location(f"multicam_calibration.{name}", os.path.join(src, f"{name}.py"))
        m = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = m
        spec.loader.exec_module(m)
        mods[name] = m
    return mods["bundle_adjustment"]


def main(ref_root):
    ba = load_reference(ref_root)
    p = synth.make_problem(**SHAPE)
    buf = io.StringIO()
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(buf):
        ext, intr, poses, use, res = ba.bundle_adjust(p["uvs"], p["extrinsics"], p["intrinsics"], p["obj"], p["poses"], n_frames=None, outlier_threshold=1e30, verbose=0, **TOL)
    # polish (the reference's LSMR stops near |grad| ~ 1e-3): the same least_squares problem -- the reference's residual function, soft_l1,
    # x_scale 'jac' -- from its result, with the exact trust-region solve on the oracle's analytic Jacobian (dense at this size)
    uvs = p["uvs"][:, use]
    res = least_squares(ba.residuals, res.x, jac=lambda x, *a: orc.jacobian_csr(x, uvs, p["obj"]).toarray(), method="trf", loss="soft_l1", x_scale="jac", tr_solver="exact",
                        ftol=1e-15, xtol=1e-15, gtol=1e-15, max_nfev=100, args=(uvs, p["obj"]))
    dt = time.perf_counter() - t0
    print("reference: %.1f s, cost %.15g, nfev %d, status %d, |grad| %.3g" % (dt, res.cost, res.nfev, res.status, np.abs(res.grad).max()))
    np.savez_compressed(os.path.join(HERE, "wide_48x150.npz"), x=res.x, cost=np.array(res.cost), nfev=np.array(res.nfev), status=np.array(res.status), use=use,
                        grad_inf=np.array(np.abs(res.grad).max()), uvs_checksum=np.array(np.nansum(p["uvs"])), seconds=np.array(dt))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit("usage: make_golden_wide.py <reference checkout (the directory that holds multicam_calibration/)>")
    main(sys.argv[1])
