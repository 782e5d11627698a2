"""The bits of the trajectory and skeleton calls, for comparing two builds of the library: every call of trajectory.py and skeleton.py on the
cases of the oracles under tests/, one line per call, case and returned field -- the SHA-256 of the array's bytes, a scalar as it is, and of
`info` the integers only (no times).  Run it from the repository root once per build (MCBA_LIB names another build of the same ABI, as for
ops.py) and diff the two outputs: they must be identical, line for line.

The calls that run in chunks of tracks run a second time on every case of three tracks or more under a budget (MCBA_SMOOTH_BUDGET_MB) of two
tracks per chunk, so that the last chunk is narrower: two chunks at K = 3, three at K = 5, 34 at K = 67.  The smoothing oracle has no case
wider than three tracks, so smooth_trajectories and trajectory_uncertainty also run on the evidence oracle's cases (K = 5 and K = 67)."""
import dataclasses
import hashlib
import os
import sys

sys.path.insert(0, ".")   # run from the repository root
sys.path.insert(0, "tests")
import numpy as np

import evidence_oracle as eo
import skeleton_oracle as sko
import skeleton_trajectory_oracle as sto
import smoothing_oracle as so
import trajectory_refine_oracle as tro
import multicam_calibration_amd as m


def emit(call, case, result):
    for f in dataclasses.fields(result):
        v = getattr(result, f.name)
        if isinstance(v, dict):
            v = " ".join(f"{k}={x}" for k, x in sorted(v.items()) if isinstance(x, int))
        elif isinstance(v, np.ndarray):
            a = np.ascontiguousarray(v)
            v = f"{a.dtype} {a.shape} {hashlib.sha256(a.tobytes()).hexdigest()}"
        elif isinstance(v, float):
            v = v.hex()
        print(f"{call} {case} {f.name} {v}")


def chunked(call, case, K, run):
    """run() whole and, at an odd number of tracks from three on, again in chunks of two tracks.  The budget of two and a half tracks takes
    device_bytes as linear in K, which it is but for the levels' share; the assertion below holds it to the chunking it was meant to give.
    K = 3 makes two chunks; the cases of K = 5 and K = 67 give every chunking call three chunks or more with a narrower last one"""
    whole = run()
    emit(call, case, whole)
    if K < 3 or K % 2 == 0:
        return
    assert whole.info["chunks"] == 1 and whole.info["tracks_per_chunk"] == K
    os.environ["MCBA_SMOOTH_BUDGET_MB"] = repr(2.5 * whole.info["device_bytes"] / K / 1048576.0)
    try:
        parts = run()
    finally:
        del os.environ["MCBA_SMOOTH_BUDGET_MB"]
    assert parts.info["tracks_per_chunk"] == 2 and parts.info["chunks"] == (K + 1) // 2, (call, case, parts.info)
    emit(call + "[chunks]", case, parts)


def smoothing():
    cases = dict(so.linear_cases(), **so.robust_cases())
    cases.update({"evidence_" + n: dict(c, accel_std=0.1) for n, c in eo.cases().items() if c["points"].shape[1] >= 5})
    for name, c in sorted(cases.items()):
        K = c["points"].shape[1]
        kw = dict(accel_std=c["accel_std"], loss=c.get("loss", "linear"), f_scale=c.get("f_scale", 3.0), segment=c["segment"])
        chunked("smooth_trajectories", name, K, lambda: m.smooth_trajectories(c["points"], c["cov"], **kw))
        chunked("smooth_trajectories[lag]", name, K, lambda: m.smooth_trajectories(c["points"], c["cov"], uncertainty="lag", **kw))
        chunked("trajectory_uncertainty", name, K, lambda: m.trajectory_uncertainty(c["points"], c["cov"], accel_std=c["accel_std"], weights=c.get("weights"), lag=True, segment=c["segment"]))


def evidence():
    for name, c in sorted(eo.cases().items()):
        K = c["points"].shape[1]
        for a in eo.EVAL_AT:
            chunked(f"trajectory_evidence[{a}]", name, K, lambda: m.trajectory_evidence(c["points"], c["cov"], accel_std=a, weights=c["weights"], segment=c["segment"]))
        kw = dict(accel_range=eo.RANGE, n_grid=9, rtol=1e-3, weights=c["weights"], segment=c["segment"])
        chunked("estimate_accel_std", name, K, lambda: m.estimate_accel_std(c["points"], c["cov"], **kw))
        emit("estimate_accel_std[all]", name, m.estimate_accel_std(c["points"], c["cov"], pool="all", **kw))


def trajectories():
    for name, c in sorted(tro.cases().items()):
        K = c["uvs"].shape[2]
        kw = dict(accel_std=c["accel_std"], pixel_std=c["pixel_std"], loss=c["loss"], f_scale=c["f_scale"], weights=c["weights"], segment=c["segment"])
        scene = (c["start"], c["uvs"], c["ext"], c["intr"])
        chunked("refine_trajectories", name, K, lambda: m.refine_trajectories(*scene, **kw))
        chunked("refine_trajectories[lag]", name, K, lambda: m.refine_trajectories(*scene, uncertainty="lag", **kw))
        chunked("refine_trajectories_system", name, K, lambda: m.refine_trajectories_system(*scene, **kw))


def skeletons():
    for name, c in sorted(sko.cases().items()):
        kw = dict(bones=c["bones"], bone_length=c["bone_length"], bone_std=c["bone_std"], pixel_std=c["pixel_std"], loss=c["loss"], f_scale=c["f_scale"], weights=c["weights"])
        scene = (c["start"], c["uvs"], c["ext"], c["intr"])
        emit("refine_skeleton", name, m.refine_skeleton(*scene, **kw))
        emit("refine_skeleton[covariance]", name, m.refine_skeleton(*scene, covariance=True, **kw))
        emit("refine_skeleton_system", name, m.refine_skeleton_system(*scene, lam=sko.SYSTEM_LAM, **kw))
        if len(c["bones"]):
            emit("estimate_bone_lengths", name, m.estimate_bone_lengths(c["start"], c["bones"]))


def skeleton_trajectories():
    for name, c in sorted(sto.cases().items()):
        kw = dict(accel_std=c["accel_std"], bones=c["bones"], bone_length=c["bone_length"], bone_std=c["bone_std"], pixel_std=c["pixel_std"], loss=c["loss"], f_scale=c["f_scale"],
                  weights=c["weights"], segment=c["segment"], cg_tol=sto.CG_TOL)
        scene = (c["start"], c["uvs"], c["ext"], c["intr"])
        emit("refine_skeleton_trajectories", name, m.refine_skeleton_trajectories(*scene, **kw))
        emit("refine_skeleton_trajectories_system", name, m.refine_skeleton_trajectories_system(*scene, **kw))
        emit("refine_skeleton_trajectories_system[resolve_check]", name, m.refine_skeleton_trajectories_system(*scene, resolve_check=True, **kw))


if __name__ == "__main__":
    for family in (smoothing, evidence, trajectories, skeletons, skeleton_trajectories):
        family()
