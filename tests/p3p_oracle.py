"""Numpy statement of the P3P hypothesis generator of the resection (csrc/mcba_resect_p3p_math.h), the checker of the
host build (tests/test_hostcheck_p3p.py) and of the GPU tier (tests/test_gpu_p3p.py).  Scoring, winner and mask are tests/resection_oracle.py's,
imported: a P3P table is a pose table of 4 H slots.

A sample is three world points X_0 X_1 X_2 and their unit bearings j_i = (x_i, y_i, 1) / |.| from the prepared normalised coordinates.
  degenerate   |(X_1 - X_0) x (X_2 - X_0)| <= AREA_MIN |X_1 - X_0| |X_2 - X_0|, or the same of the bearings as points (x_i, y_i, 1) of the image
               plane (collinear image points: the camera centre lies in the triangle's plane): every slot void
  quartic      Grunert's (Haralick, Lee, Ottenberg, Noelle 1994, eqs. 9): a = |X_1 X_2|, b = |X_0 X_2|, c = |X_0 X_1|, cos alpha = j_1 . j_2,
               cos beta = j_0 . j_2, cos gamma = j_0 . j_1, depths s_1 = u s_0, s_2 = v s_0; A_4 v^4 + .. + A_0 = 0
  roots        np.roots; the real ones ascending, root k in slot k; the other slots void.  No finite Cauchy bound 1 + max |A_k| / |A_4|: all void
  candidate    u from v, s_0 = b / sqrt(1 + v^2 - 2 v cos beta); void when u <= 0 or v <= 0; the camera points Y_i = s_i j_i; R = F_Y F_X^T of
               the orthonormal frames (e_1 along 0 -> 1, e_3 the normal, e_2 = e_3 x e_1), t = Y_0 - R X_0
  polish       exactly POLISH Gauss-Newton iterations of tests/resection_oracle.py's step on the three points (6 residuals, 6 unknowns)
  void         anything not finite, or a sample point with z <= 0 after the polish; the pose is NaN

Two routes of different arithmetic: ("normal", points in order) and ("lstsq", the points rotated cyclically, X_1 X_2 X_0).  The rotated quartic
has other coefficients and other roots (v' = s_0 / s_1), its frames start at another vertex, its Gauss-Newton step goes through lstsq: the two
pose SETS must coincide on a comparable sample, candidate by nearest candidate.

A sample is COMPARABLE when no complex root of its quartic has |imag| < ROOT_GAP max(1, |v|), no two real roots are closer than
ROOT_GAP max(1, |v|), and every live candidate's last polish step is <= STEP_MAX = 1e-10 with an equilibrated cond_2(J^T J) < COND_MAX = 1e8
(`step` and `cond` as in tests/resection_oracle.py).  A degenerate sample is not comparable.  At most LEFT_OUT_CAP = 5 % of a camera's non-void
samples (those with a live slot) may be left out, asserted on the oracle alone (tests/test_p3p_oracle_cpu.py) for 64 samples, seed [0, camera],
on "six", "three", flat3 and "thin3" with true points, every camera.

Tolerance of a comparable candidate's pose: K_P EPS cond per entry of R, times max(1, |t|) per entry of t (section 8f-16's form).
K_P = max(64, 8 x the worst multiple of EPS cond between the two routes on those scenes), K_P_MEASURED below (the CPU test asserts it)."""
import numpy as np

import keypoint_scenes as ks
import resection_oracle as ro

EPS = ro.EPS
SAMPLE, SLOTS, POLISH = 3, 4, 5
AREA_MIN = 1e-6               # P3_AREA_MIN of csrc/mcba_resect_p3p_math.h: the sine of the triangle's angle at the first point
ROOT_GAP = 1e-6
STEP_MAX, COND_MAX, LEFT_OUT_CAP = ro.STEP_MAX, ro.COND_MAX, ro.LEFT_OUT_CAP
K_P_MEASURED = 2.48           # the worst multiple between the two routes (module docstring): "three" camera 0; "six" 1.02, "thin3" 0.34, flat3 0.11; so K_P = max(64, 19.8) = 64
K_P = max(64.0, 8 * K_P_MEASURED)
THRESHOLD = ro.THRESHOLD
CAP_SCENES = ("six", "three", "flat3", "thin3")   # the scenes of the left-out cap and of K_P_MEASURED, true points, 64 samples, seed [0, camera]


# ---------------------------------------------------------------- inputs
def draw_samples(M, H, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.choice(M, SAMPLE, replace=False) for _ in range(H)]).astype(np.int32)


def samples_of(usable, H, seed):
    idx = np.flatnonzero(usable)
    return idx[draw_samples(len(idx), H, seed)].astype(np.int32)


_scene_cache = {}


def scene(name):
    """(uvs, ext, intr, X) of a scene of keypoint_scenes, thin_scenes or p3p_scenes"""
    import p3p_scenes
    import thin_scenes
    if name in p3p_scenes.SLABS:
        return p3p_scenes.make(name)[:4]
    if name in thin_scenes.SCENES:
        return thin_scenes.make(name)
    return ks.make(name)


def camera_of(name, cam, points="truth"):
    """dict(points (P, 3), uv (P, 2), intr, ext, usable); points: "truth", or "others": the oracle's triangulation of the other cameras"""
    key = (name, cam, points)
    if key not in _scene_cache:
        uvs, ext, intr, X = scene(name)
        if points == "truth":
            pts = np.array(X, dtype=np.float64)
        else:
            from oracle import triangulate_oracle as tri
            others = [c for c in range(len(ext)) if c != cam]
            with np.errstate(all="ignore"):
                pts = tri.triangulate([uvs[c] for c in others], np.asarray(ext)[others], [intr[c] for c in others])
        uv = np.array(uvs[cam], dtype=np.float64)
        for a in (pts, uv):
            a.setflags(write=False)
        _scene_cache[key] = dict(points=pts, uv=uv, intr=intr[cam], ext=np.array(ext[cam]), usable=np.isfinite(pts).all(1) & np.isfinite(uv).all(1), n_cameras=len(ext))
    return _scene_cache[key]


# ---------------------------------------------------------------- the closed form
def bearings(nx):
    b = np.c_[nx, np.ones(len(nx))]
    return b / np.linalg.norm(b, axis=1)[:, None]


def collinear(A):
    d1, d2 = A[1] - A[0], A[2] - A[0]
    n = np.cross(d1, d2)
    return not (n @ n > AREA_MIN ** 2 * (d1 @ d1) * (d2 @ d2))


def grunert(X, j):
    """(A_0 .. A_4 ascending, the quantities that give u from v)"""
    a2, b2, c2 = ((X[1] - X[2]) ** 2).sum(), ((X[0] - X[2]) ** 2).sum(), ((X[0] - X[1]) ** 2).sum()
    ca, cb, cg = j[1] @ j[2], j[0] @ j[2], j[0] @ j[1]
    p, q = (a2 - c2) / b2, (a2 + c2) / b2
    A4 = (p - 1) ** 2 - 4 * c2 / b2 * ca ** 2
    A3 = 4 * (p * (1 - p) * cb - (1 - q) * ca * cg + 2 * c2 / b2 * ca ** 2 * cb)
    A2 = 2 * (p ** 2 - 1 + 2 * p ** 2 * cb ** 2 + 2 * (b2 - c2) / b2 * ca ** 2 - 4 * q * ca * cb * cg + 2 * (b2 - a2) / b2 * cg ** 2)
    A1 = 4 * (-p * (1 + p) * cb + 2 * a2 / b2 * cg ** 2 * cb - (1 - q) * ca * cg)
    A0 = (1 + p) ** 2 - 4 * a2 / b2 * cg ** 2
    return np.array([A0, A1, A2, A3, A4]), (p, ca, cb, cg, b2)


def frame(A):
    e1 = A[1] - A[0]
    e1 = e1 / np.linalg.norm(e1)
    e3 = np.cross(e1, A[2] - A[0])
    e3 = e3 / np.linalg.norm(e3)
    return np.stack([e1, np.cross(e3, e1), e3], axis=1)     # columns


def start_pose(X, j, v, aux):
    """(R, t) of the root v, or None where a depth ratio is not positive"""
    p, ca, cb, cg, b2 = aux
    u = ((p - 1) * v * v - 2 * p * cb * v + 1 + p) / (2 * (cg - v * ca))
    if not (u > 0 and v > 0):
        return None
    s0 = np.sqrt(b2 / (1 + v * v - 2 * v * cb))
    Y = np.array([s0, u * s0, v * s0])[:, None] * j
    R = frame(Y) @ frame(X).T
    return R, Y[0] - R @ X[0]


def gn_system(R, t, X, x):
    """resection_oracle.gn_system for any number of points"""
    Xc = X @ R.T + t
    z = Xc[:, 2]
    p = Xc[:, :2] / z[:, None]
    J = np.zeros((2 * len(X), 6))
    for k in range(len(X)):
        N = np.array([[1 / z[k], 0, -p[k, 0] / z[k]], [0, 1 / z[k], -p[k, 1] / z[k]]])
        J[2 * k:2 * k + 2, :3] = -N @ ro.skew(Xc[k])
        J[2 * k:2 * k + 2, 3:] = N
    return J, (p - x).ravel()


def polish(R, t, X, x, route, iterations):
    """(pose (12) or None, step of the last iteration, cond of its equilibrated J^T J, the steps of every iteration)"""
    step, cond, steps = np.inf, np.inf, []
    try:
        for _ in range(iterations):
            J, r = gn_system(R, t, X, x)
            y, cond = ro.gn_step(J, r, route)
            E = ks.rodrigues(y[:3])
            R, t = E @ R, E @ t + y[3:]
            step = max(np.linalg.norm(y[:3]), np.linalg.norm(y[3:]) / max(1.0, np.linalg.norm(t)))
            steps.append(step)
    except np.linalg.LinAlgError:
        return None, np.inf, np.inf, steps
    pose = np.r_[R.ravel(), t]
    if not (np.isfinite(pose).all() and ((X @ R.T + t)[:, 2] > 0).all()):
        return None, np.inf, np.inf, steps
    return pose, float(step), float(cond), steps


def sample(X, x, route="normal", order=(0, 1, 2), iterations=POLISH):
    """the four slots of one sample: dict(pose (4, 12), status (4), step (4), cond (4), roots: every root of the quartic (complex), clear: the
    root rule of a comparable sample holds, steps: per live slot the step of every iteration)"""
    out = dict(pose=np.full((SLOTS, 12), np.nan), status=np.full(SLOTS, -1, np.int32), step=np.full(SLOTS, np.inf), cond=np.full(SLOTS, np.inf), roots=np.zeros(0, complex), clear=False, steps={})
    X, x = np.asarray(X, dtype=np.float64)[list(order)], np.asarray(x, dtype=np.float64)[list(order)]
    with np.errstate(all="ignore"):
        j = bearings(x)
        if not (np.isfinite(X).all() and np.isfinite(j).all()) or collinear(X) or collinear(np.c_[x, np.ones(3)]):
            return out
        A, aux = grunert(X, j)
        if not np.isfinite(A).all() or not 1.0 + np.abs(A[:4]).max() / abs(A[4]) <= 1e300:
            return out
        roots = np.roots(A[::-1])
        out["roots"] = roots
        real = np.sort(roots[roots.imag == 0].real)
        cplx = roots[roots.imag != 0]
        scale = lambda v: ROOT_GAP * max(1.0, abs(v))
        out["clear"] = all(abs(r.imag) >= scale(r) for r in cplx) and all(real[k + 1] - real[k] >= scale(real[k]) for k in range(len(real) - 1))
        for k, v in enumerate(real[:SLOTS]):
            st = start_pose(X, j, v, aux)
            if st is None or not (np.isfinite(st[0]).all() and np.isfinite(st[1]).all()):
                continue
            pose, step, cond, steps = polish(st[0], st[1], X, x, route, iterations)
            if pose is not None:
                out["pose"][k], out["status"][k], out["step"][k], out["cond"][k], out["steps"][k] = pose, 1, step, cond, steps
    return out


def hypotheses(points, prep, samples, route="normal", order=(0, 1, 2), iterations=POLISH):
    """the table of 4 H slots: dict(pose (4 H, 12), status, step, cond (4 H), comparable (4 H): the slot's sample is comparable (void slots of it
    included: their status is compared), sample_comparable (H), sample_live (H): a live slot, tol (4 H, 12), per_sample: the dicts of `sample`)"""
    H = len(samples)
    per = [sample(np.asarray(points)[s], prep["nx"][s], route, order, iterations) for s in samples]
    out = {k: np.concatenate([o[k] for o in per]) for k in ("pose", "status", "step", "cond")}
    live = np.array([(o["status"] > 0).any() for o in per])
    comp = np.array([o["clear"] and all(o["step"][k] <= STEP_MAX and o["cond"][k] < COND_MAX for k in range(SLOTS) if o["status"][k] > 0) for o in per])
    out.update(sample_live=live, sample_comparable=comp, comparable=np.repeat(comp, SLOTS), per_sample=per)
    out["tol"] = ro.pose_tolerance(out["pose"], out["cond"], k=K_P)
    return out


def left_out_share(hyp):
    """the share of a camera's non-void samples that the element-wise comparison leaves out"""
    live = hyp["sample_live"]
    return float((live & ~hyp["sample_comparable"]).sum() / max(1, live.sum()))


def route_multiple(points, prep, samples):
    """(the worst |pose_a - pose_b| over EPS cond between the two routes, candidate by nearest candidate, over the samples comparable in both;
    whether the two pose sets coincide in number on every one of them)"""
    a, b = hypotheses(points, prep, samples, "normal", (0, 1, 2)), hypotheses(points, prep, samples, "lstsq", (1, 2, 0))
    worst, same = 0.0, True
    for h in np.flatnonzero(a["sample_comparable"] & b["sample_comparable"]):
        sl = slice(SLOTS * h, SLOTS * h + SLOTS)
        pa, pb = a["pose"][sl][a["status"][sl] > 0], b["pose"][sl][b["status"][sl] > 0]
        same = same and len(pa) == len(pb)
        if len(pa) == 0 or len(pb) == 0:
            continue
        unit = ro.pose_tolerance(pa, a["cond"][sl][a["status"][sl] > 0], k=1.0)
        ratio = np.abs(pa[:, None, :] - pb[None, :, :]) / unit[:, None, :]
        worst = max(worst, float(ratio.max(2).min(1).max()))
    return worst, same


def ransac(points, uv, intr, samples, threshold, iterations=5):
    """every stage on one camera, as resection_oracle.ransac: prep, hyp (4 H slots), score, winner (a slot), comparable, rt12, inliers, n_inliers,
    cost, n_usable"""
    points = np.asarray(points, dtype=np.float64)
    prep = ro.prepare(points, uv, intr, iterations)
    hyp = hypotheses(points, prep, samples)
    sc = ro.score(hyp["pose"], hyp["status"], points, prep, intr, threshold)
    w, comparable = ro.winner_comparable(sc, hyp)
    return dict(prep=prep, hyp=hyp, score=sc, winner=w, comparable=comparable, rt12=hyp["pose"][w], inliers=sc["inlier"][w], n_inliers=int(sc["count"][w]), cost=float(sc["cost"][w]),
                n_usable=int(prep["usable"].sum()))


def pose_errors(rt12, ext):
    """(distance of the camera centres, rotation angle in degrees) between a pose (12) and the truth (rotation vector, translation)"""
    R, t = rt12[:9].reshape(3, 3), rt12[9:]
    R0, t0 = ks.rodrigues(ext[:3]), ext[3:]
    c = np.clip((np.trace(R @ R0.T) - 1) / 2, -1, 1)
    return float(np.linalg.norm(R.T @ t - R0.T @ t0)), float(np.degrees(np.arccos(c)))


# ---------------------------------------------------------------- the rules, applied to what a build returns
def check_candidates(tag, pose, status, hyp):
    """status of every slot of a comparable sample; pose of every live one within its tolerance"""
    ok = hyp["comparable"]
    live = ok & (hyp["status"] > 0)
    pose, status = np.asarray(pose), np.asarray(status)
    ratio = float((np.abs(pose - hyp["pose"])[live] / hyp["tol"][live]).max()) if live.any() else 0.0
    print(f"{tag}: pose error / tolerance {ratio:.3g} over {int(live.sum())} live slots of {int(hyp['sample_comparable'].sum())} comparable samples of {len(hyp['sample_live'])}; "
          f"left out {left_out_share(hyp):.3%}; live slots {int((hyp['status'] > 0).sum())}")
    assert np.array_equal(status[ok], hyp["status"][ok]) and ratio <= 1
    assert np.isnan(pose[ok & (hyp["status"] < 0)]).all()
    return ratio
