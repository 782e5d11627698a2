"""References of the trajectory calls that scale to long tracks and wide chunks: the routes of smoothing_oracle,
evidence_oracle, trajectory_refine_oracle and skeleton_trajectory_oracle with every dense matrix replaced by the banded form of one track
(scipy.linalg.solveh_banded, cholesky_banded) or by a matrix-free operator, so that 66001 frames per track and 76808 (frame, keypoint) pairs
cost seconds.  tests/test_trajectory_scale_oracle_cpu.py holds every route here to the dense route it replaces on the small cases.

What stands in for the dense condition number: window_cond, the larger of the Jacobi-scaled dense condition numbers of the first and of the
last WINDOW frames taken as problems of their own (the system is local: smoothing_oracle's long-track test already relies on it); the scenes
here keep their longest gap and their one-camera stretches inside one of the two windows.  What says how good the banded reference itself
is: reference_error, one step of iterative refinement with the residual formed in np.longdouble.

The bar of mahalanobis2 at the RETURNED points (d2_bar): both sides evaluate d^T W d, d = x - p, at the same x in float64.  x and p are
exact inputs, so d carries one rounding, W = Sigma^-1 is formed twice (the library's Jacobi-scaled Cholesky inverse, numpy's inverse here)
with a relative difference of a few eps cond(Sigma), and the quadratic form of three terms adds a few eps sum |d_a W_ab d_b| <= eps
cond(Sigma) d^2: a relative error of about 10 eps cond(Sigma), 1e-13 at the scenes' cond(Sigma) <= 25.  The bar is 1e-9 d^2 (the cost
bar's relative part, four orders above that) plus 8 eps cond d^2 (twice the linear bar's relative error of x, what a comparison at the
reference's own points would have to allow); test_trajectory_scale_oracle_cpu.py measures the float64 formula against np.longdouble."""
import functools

import numpy as np
import scipy.linalg
import scipy.sparse
import scipy.sparse.linalg

import evidence_oracle as eo
import keypoint_scenes as ks
import skeleton_trajectory_oracle as sto
import smoothing_oracle as so
import trajectory_refine_oracle as tro

EPS, BAR_K, LD = so.EPS, so.BAR_K, np.longdouble
WINDOW = 400
CG_MAX = 200       # the library's default iteration cap of the inner solve


# ---------------------------------------------------------------- one track's banded system
def banded(W, accel_std):
    """the upper banded form (9, 3 T) of blockdiag(W_t) + a^-2 D2^T D2 (x) I3; W (T, 3, 3) symmetric: smoothing_oracle.system's ab from blocks"""
    T = len(W)
    ia2 = 1.0 / float(accel_std) ** 2
    dg, o1, o2 = so.penalty_bands(T)
    ab = np.zeros((9, 3 * T))
    for a in range(3):
        for b in range(a, 3):
            ab[8 + a - b, b::3] = W[:, a, b]
        ab[8, a::3] += ia2 * dg
        if T > 1:
            ab[5, 3 + a::3] = ia2 * o1[:T - 1]
        if T > 2:
            ab[2, 6 + a::3] = ia2 * o2[:T - 2]
    return ab


def banded_matvec(ab, x, dtype=np.float64):
    """A x of the symmetric matrix in upper banded form (9, n), in dtype, vectorised over the nine bands"""
    n = ab.shape[1]
    abl, xl = ab.astype(dtype), np.asarray(x).reshape(n).astype(dtype)
    y = abl[8] * xl
    for k in range(8):
        off = 8 - k
        if off >= n:
            continue
        v = abl[k, off:]
        y[:n - off] += v * xl[off:]
        y[off:] += v * xl[:n - off]
    return y


def reference_error(sysd, x):
    """the banded reference's own error at its solution x: the residual b - A x in np.longdouble, one more banded solve, max |e|"""
    r = sysd["b"].astype(LD) - banded_matvec(sysd["ab"], x, LD)
    return float(np.abs(scipy.linalg.solveh_banded(sysd["ab"], r.astype(np.float64), lower=False)).max())


def window_cond(W, accel_std, window=WINDOW):
    """the larger of the Jacobi-scaled dense condition numbers of the first and the last `window` frames, each a problem of its own:
    blockdiag(W_t) + a^-2 D2^T D2 (x) I3 over those frames; W (T, 3, 3) the weighted data blocks (w_t Sigma_t^-1, or the information H_t)"""
    T = len(W)
    ends = [W] if T <= window else [W[:window], W[T - window:]]
    return max(so.cond(dict(A=tro.dense_matrix(w, accel_std))) for w in ends)


def data_blocks(sysd):
    return sysd["winv"] * sysd["w"][:, None, None]


# ---------------------------------------------------------------- the smoother at length
def objective(x, sysd, accel_std, loss="linear", f_scale=3.0):
    """smoothing_oracle.objective from a system already prepared (prepare() is a loop over the frames)"""
    d = x - sysd["p"]
    us = sysd["usable"]
    d2 = np.einsum("ta,tab,tb->t", d, sysd["winv"], d)[us]
    f2 = float(f_scale) ** 2
    pen = np.sum((x[:-2] - 2.0 * x[1:-1] + x[2:]) ** 2) if len(x) >= 3 else 0.0
    return 0.5 * f2 * np.sum(so.rho(loss, d2 / f2)) + 0.5 / float(accel_std) ** 2 * pen


def mahalanobis2_ld(x, sysd):
    """smoothing_oracle.mahalanobis2 in np.longdouble (usable frames; NaN elsewhere)"""
    d = x.astype(LD) - sysd["p"].astype(LD)
    W = sysd["winv"].astype(LD)
    q = sum(d[:, a] * W[:, a, b] * d[:, b] for a in range(3) for b in range(3))
    return np.where(sysd["usable"], q, np.nan)


def smooth_reference(points, cov, accel_std, weights=None):
    """one track's linear solve with the given weights: dict(sysd, x, cond (window_cond), ref_err (reference_error))"""
    s = so.system(points, cov, accel_std, weights, dense=False)
    x = so.solve(s)
    return dict(sysd=s, x=x, cond=window_cond(data_blocks(s), accel_std), ref_err=reference_error(s, x))


def cost_bar(c, cnd):
    """section 8f-21's cost bar, the smoother's too"""
    return 1e-9 * max(1.0, c) + 100 * EPS * cnd * c


def d2_bar(d2, cnd):
    """the bar of mahalanobis2 at the returned points (the module's docstring)"""
    return 1e-9 * d2 + 8 * EPS * cnd * d2


def check_smooth(name, refs, accel_std, got, loss="linear", f_scale=3.0):
    """got: smooth_trajectories' fields after ONE solve (linear, or max_iterations=1 with weights_in); refs: per track smooth_reference() with
    those weights.  Points within 4 eps window_cond max|x| of the banded solve; cost, mahalanobis2 and weights against the objective, the
    distances and rho' evaluated here at the returned points; n_usable and status exact.  Returns the largest fraction of each bar"""
    worst = dict(points=0.0, cost=0.0, mahalanobis2=0.0, weights=0.0)
    f2 = float(f_scale) ** 2
    for k, r in enumerate(refs):
        s, us = r["sysd"], r["sysd"]["usable"]
        x = got["points"][:, k]
        assert got["status"][k] == so.STATUS_OK and got["n_usable"][k] == int(us.sum()) and got["n_iterations"][k] == 1 and np.isfinite(x).all(), (name, k)
        err, bar = so.linear_bar(x, r["x"], r["cond"])
        c = objective(x, s, accel_std[k], loss, f_scale)
        ec, bc = abs(got["cost"][k] - c), cost_bar(c, r["cond"])
        d2 = so.mahalanobis2(x, s)
        assert np.array_equal(np.isnan(got["mahalanobis2"][:, k]), ~us), (name, k)
        fd = float((np.abs(got["mahalanobis2"][us, k] - d2[us]) / d2_bar(d2[us], r["cond"])).max())
        w = so.drho(loss, d2[us] / f2)
        bw = 0.5 * (1e-9 + 8 * EPS * r["cond"]) + 4 * EPS   # w = rho'(z) of soft_l1 and huber: |dw| / w <= 0.5 |dz| / z, and its own roundings
        ew = float(np.abs(got["weights"][us, k] / w - 1.0).max())
        print(f"{name} track {k}: window cond {r['cond']:.3g}, points {err:.3g} (bar {bar:.3g}, the reference's own error {r['ref_err']:.3g}), cost {ec:.3g} (bar {bc:.3g}), "
              f"mahalanobis2 {fd:.3g} of its bar, weights {ew:.3g} relative (bar {bw:.3g})")
        assert err <= bar and ec <= bc and fd <= 1.0 and ew <= bw and (got["weights"][~us, k] == 0).all(), (name, k, err, bar, ec, bc, fd, ew)
        for f, v in (("points", err / bar), ("cost", ec / bc), ("mahalanobis2", fd), ("weights", ew / bw)):
            worst[f] = max(worst[f], v)
    return worst


# ---------------------------------------------------------------- the evidence at length
def evidence_terms(track, a):
    """evidence_oracle.Track.neg2's float64 route (scipy's banded Cholesky) with its terms laid open: dict(N, data, penalty, log_det, S, x)"""
    ia2 = 1.0 / float(a) ** 2
    ab = track.dat + ia2 * track.pen
    c = scipy.linalg.cholesky_banded(ab, lower=False)
    x = scipy.linalg.cho_solve_banded((c, False), track.s["b"]).reshape(-1, 3)
    data, pen = eo._terms(x, track.s, ia2)
    ll = 2.0 * np.log(c[8])
    log_det = float(ll.sum())
    return dict(N=float(data + pen + log_det + 6.0 * (track.T - 2) * np.log(a)), data=float(data), penalty=float(pen), log_det=log_det,
                S=float(np.abs(np.log(ab[8])).sum() + np.abs(ll).sum()), x=x, ab=ab)


def evidence_reference(track, a):
    """the terms of one track at a with their bars (evidence_oracle.bars at window_cond) and the reference's own error of x"""
    r = evidence_terms(track, a)
    r["cond"] = window_cond(data_blocks(track.s), a)
    r["bars"] = eo.bars(track.T, a, r, r["cond"], r["S"])
    r["ref_err"] = reference_error(dict(ab=r["ab"], b=track.s["b"]), r["x"])
    return r


def check_evidence(name, refs, got):
    """got: trajectory_evidence's fields at one a; refs: per track evidence_reference().  Returns the largest fraction of a bar"""
    worst = 0.0
    for k, r in enumerate(refs):
        assert got["status"][k] == so.STATUS_OK, (name, k)
        for f, key in (("log_det", "log_det"), ("data", "data"), ("penalty", "penalty"), ("neg2_log_evidence", "N")):
            err, bar = abs(got[f][k] - r[key]), r["bars"][key]
            worst = max(worst, err / bar)
            assert np.isfinite(got[f][k]) and err <= bar, (name, k, f, got[f][k], r[key], err, bar)
    return worst


# ---------------------------------------------------------------- trajectory refinement at length
def penalty_apply(x, absolute=False):
    """D2^T (D2 x) per coordinate of x (T, 3) from second differences; absolute: |D2|^T (|D2| |x|), which is |D2^T D2| |x| (the products that meet
    in one entry of D2^T D2 share their sign)"""
    y = np.zeros_like(x)
    if len(x) < 3:
        return y
    if absolute:
        x = np.abs(x)
        sd = x[:-2] + 2.0 * x[1:-1] + x[2:]
        y[1:-1] += 2.0 * sd
    else:
        sd = x[:-2] - 2.0 * x[1:-1] + x[2:]
        y[1:-1] -= 2.0 * sd
    y[:-2] += sd
    y[2:] += sd
    return y


def refine_evaluate(x, tc):
    """trajectory_refine_oracle.evaluate's H, G, S, data, pen of one track at x (T, 3) without a dense matrix; tc = tro.track_inputs(..)"""
    d = tro.data_terms(x[:, None], tc["uvs"], tc["ext"], tc["intr"], tc["weff"], tc["loss"], tc["f_scale"])
    ia2 = 1.0 / tc["accel_std"] ** 2
    return dict(H=d["H"][:, 0], G=d["g"][:, 0] + ia2 * penalty_apply(x), S=d["gabs"][:, 0] + ia2 * penalty_apply(x, True), data=float(d["cost"].sum()),
                pen=tro.penalty_cost(x, tc["accel_std"]))


def refine_step(H, G, accel_std):
    """(the step of (blockdiag(H) + a^-2 D2^T D2 (x) I3) d = -G by the banded solve, window_cond of that matrix, the solve's own error)"""
    ab = banded(H, accel_std)
    d = scipy.linalg.solveh_banded(ab, -G.ravel(), lower=False).reshape(-1, 3)
    return d, window_cond(H, accel_std), reference_error(dict(ab=ab, b=-G.ravel()), d)


def check_refine_system(name, case, got, dense=False):
    """trajectory_refine_oracle.check_system for a case that is not one of its own, by the same bars.  dense=False: the routes of this module
    (information and gradient against refine_evaluate, the step against the banded solve built from the returned information and gradient
    at window_cond, the costs against the oracle's objective at x + alpha d_returned); dense=True: tro.evaluate and the dense solve, the
    costs against the oracle's own trial points (check_system's rule).  Returns the largest fraction of each bar"""
    nus, nsg, status = tro.counts(case)
    K = len(status)
    acc = np.broadcast_to(np.asarray(case["accel_std"], dtype=np.float64), (K,))
    assert np.array_equal(got["status"], status) and np.array_equal(got["n_usable"], nus) and np.array_equal(got["n_single"], nsg), (name, got["status"], status)
    worst = dict(information=0.0, gradient=0.0, step=0.0, costs=0.0)
    for k in range(K):
        fields = [got[f][:, k] for f in ("information", "gradient", "step")] + [got[f][k] for f in ("data_cost", "penalty_cost", "trial_costs")]
        if status[k] != tro.STATUS_OK:
            assert all(np.isnan(f).all() for f in fields), (name, k)
            continue
        assert all(np.isfinite(f).all() for f in fields), (name, k)
        tc = tro.track_inputs(case, k)
        x, H, G, d = case["start"][:, k], got["information"][:, k], got["gradient"][:, k], got["step"][:, k]
        ev = tro.evaluate(x, tc) if dense else refine_evaluate(x, tc)
        eh = np.abs(H - ev["H"]).max() / np.abs(ev["H"]).max()
        eg = (np.abs(G - ev["G"]) / ev["S"]).max()
        if dense:
            A = tro.dense_matrix(H, acc[k])
            dref, cnd, own = np.linalg.solve(A, -G.ravel()).reshape(-1, 3), so.cond(dict(A=A)), np.nan
            trial = ev["trial"]
        else:
            dref, cnd, own = refine_step(H, G, acc[k])
            trial = np.array([tro.objective(x + a * d, tc) for a in tro.ALPHAS])
        ed, bar_d = np.abs(d - dref).max(), BAR_K * EPS * cnd * np.abs(dref).max()
        tol = cost_bar(ev["data"] + ev["pen"], cnd)
        ec = max(np.abs(got["trial_costs"][k] - trial).max(), abs(got["data_cost"][k] - ev["data"]), abs(got["penalty_cost"][k] - ev["pen"]))
        if not dense or k % 16 == 0:
            print(f"{name} track {k}: information {eh:.3g} (bar 1e-12), gradient {eg:.3g} of S (bar 1e-12), step {ed:.3g} (bar {bar_d:.3g}, cond {cnd:.3g}, the reference's own error "
                  f"{own:.3g}), costs {ec:.3g} (bar {tol:.3g})")
        assert eh <= 1e-12 and eg <= 1e-12 and ed <= bar_d and ec <= tol, (name, k, eh, eg, ed, bar_d, ec, tol)
        for f, v in (("information", eh / 1e-12), ("gradient", eg / 1e-12), ("step", ed / bar_d), ("costs", ec / tol)):
            worst[f] = max(worst[f], v)
    return worst


def check_refine_loop(name, case, got):
    """refine_trajectories after a few iterations on a long case: per running track the history never rises and `cost` is the oracle's objective
    at the returned points within the cost bar (window_cond of the returned information).  Returns the largest fraction of that bar"""
    status = tro.counts(case)[2]
    K = len(status)
    acc = np.broadcast_to(np.asarray(case["accel_std"], dtype=np.float64), (K,))
    assert np.array_equal(got["status"], status), (name, got["status"], status)
    worst = 0.0
    for k in np.flatnonzero(status == tro.STATUS_OK):
        x, nit = got["points"][:, k], int(got["n_iterations"][k])
        h = got["history"][:nit, k]
        assert nit >= 1 and np.isfinite(x).all() and np.isfinite(h).all() and np.isnan(got["history"][nit:, k]).all() and got["cost"][k] == h[-1, 0], (name, k)
        assert (h[1:, 0] <= h[:-1, 0]).all(), (name, k, h[:, 0])
        c = tro.objective(x, tro.track_inputs(case, k))
        cnd = window_cond(got["information"][:, k], acc[k])
        err, tol = abs(got["cost"][k] - c), cost_bar(c, cnd)
        print(f"{name} track {k}: iterations {nit}, cost {got['cost'][k]:.12g} (oracle at the returned points {c:.12g}: {err:.3g}, bar {tol:.3g}), alphas {h[:, 2]}")
        assert err <= tol, (name, k, err, tol)
        worst = max(worst, err / tol)
    return worst


# ---------------------------------------------------------------- skeleton trajectories at length
def skeleton_evaluate(x, case):
    """skeleton_trajectory_oracle.evaluate's H, G, S (NaN off the running tracks), u, r and costs at x (T, K, 3; zero off the running tracks)
    without M, B, A"""
    nus, nsg, status, run, apar = sto.running(case)
    T, K = x.shape[:2]
    dt = sto.data_terms(x, case)
    acc = np.broadcast_to(np.asarray(case["accel_std"], dtype=np.float64), (K,))
    G, S = np.full((T, K, 3), np.nan), np.full((T, K, 3), np.nan)
    for k in np.flatnonzero(run):
        G[:, k] = dt["g"][:, k] + penalty_apply(x[:, k]) / acc[k] ** 2
        S[:, k] = dt["gabs"][:, k] + penalty_apply(x[:, k], True) / acc[k] ** 2
    u, r = sto.bones_at(x, case, apar)
    for k in np.flatnonzero(apar >= 0):
        gb = u[:, k] * (r[:, k] / case["s"][k])[:, None]
        G[:, k] += gb
        G[:, apar[k]] -= gb
        S[:, k] += np.abs(gb)
        S[:, apar[k]] += np.abs(gb)
    data, pen, bone = sto.costs(x, case, run, apar)
    return dict(n_usable=nus, n_single=nsg, status=status, run=run, apar=apar, H=np.where(run[None, :, None, None], dt["H"], np.nan), G=G, S=S, u=u, r=r, data=data, pen=pen, bone=bone)


class SkeletonOperators:
    """A = M + B and M^-1 of one evaluation, matrix-free, on planes (T, K, 3) that are zero off the running tracks: M per running track banded
    (information H (T, K, 3, 3) and accel_std), B the active bones' rank-one terms from their directions u (T, K, 3) by child"""

    def __init__(self, H, u, case, run, apar):
        K = H.shape[1]
        acc = np.broadcast_to(np.asarray(case["accel_std"], dtype=np.float64), (K,))
        self.ab = {int(k): banded(H[:, k], acc[k]) for k in np.flatnonzero(run)}
        self.chol = {k: scipy.linalg.cholesky_banded(ab, lower=False) for k, ab in self.ab.items()}
        self.bones = [(int(k), int(apar[k]), u[:, k], 1.0 / case["s"][k] ** 2) for k in np.flatnonzero(apar >= 0)]

    def M(self, v):
        out = np.zeros_like(v)
        for k, ab in self.ab.items():
            out[:, k] = banded_matvec(ab, v[:, k]).reshape(-1, 3)
        return out

    def B(self, v):
        out = np.zeros_like(v)
        for k, p, u, is2 in self.bones:
            t = u * ((u * (v[:, k] - v[:, p])).sum(1) * is2)[:, None]
            out[:, k] += t
            out[:, p] -= t
        return out

    def A(self, v):
        return self.M(v) + self.B(v)

    def Minv(self, r):
        out = np.zeros_like(r)
        for k, c in self.chol.items():
            out[:, k] = scipy.linalg.cho_solve_banded((c, False), r[:, k].ravel()).reshape(-1, 3)
        return out

    def relative_residual(self, G, d):
        """sqrt(r^T M^-1 r / G^T M^-1 G), r = -(G + A d): the true preconditioned residual of a step d"""
        r = -(G + self.A(d))
        return float(np.sqrt(np.sum(r * self.Minv(r)) / np.sum(G * self.Minv(G))))


def pcg(op, G, cg_tol, cg_max=CG_MAX, history=None):
    """conjugate gradients on A d = -G preconditioned with M from d = 0, with the library's stopping rule (skt_scalars): it ends when r^T z is not
    positive at the start, when p^T A p is not positive, when r^T z <= cg_tol^2 r0^T z0 or after cg_max iterations.  (d, iterations, sqrt(r^T z /
    r0^T z0) when it ended); history: a list that receives that ratio after every iteration"""
    d, r = np.zeros_like(G), -G
    z = op.Minv(r)
    p, rz = z, float(np.sum(r * z))
    rz0, it = rz, 0
    done = not rz > 0.0
    while not done:
        y = op.A(p)
        pap = float(np.sum(p * y))
        if not pap > 0.0:
            break
        al = rz / pap
        d, r = d + al * p, r - al * y
        z = op.Minv(r)
        rzn = float(np.sum(r * z))
        beta, rz, it = rzn / rz, rzn, it + 1
        if history is not None:
            history.append(float(np.sqrt(rz / rz0)))
        done = not rz > cg_tol * cg_tol * rz0 or it >= cg_max
        p = z + beta * p
    return d, it, float(np.sqrt(rz / rz0)) if rz0 > 0 else 0.0


def sparse_cond(A):
    """lambda_max / lambda_min of the Jacobi-scaled symmetric positive definite sparse matrix A: Lanczos at both ends (shift-invert at 0)"""
    s = 1.0 / np.sqrt(A.diagonal())
    As = (scipy.sparse.diags(s) @ A @ scipy.sparse.diags(s)).tocsc()
    hi = scipy.sparse.linalg.eigsh(As, k=1, which="LA", return_eigenvectors=False)[0]
    lo = scipy.sparse.linalg.eigsh(As, k=1, sigma=0.0, which="LM", return_eigenvectors=False)[0]
    return float(hi / lo)


def skeleton_matrix(H, u, case, apar):
    """A = M + B of the frames H covers as a problem of their own, sparse, unknowns ordered (frame, track, coordinate)"""
    T, K = H.shape[:2]
    assert np.isfinite(H).all()   # (every track runs)
    acc = np.broadcast_to(np.asarray(case["accel_std"], dtype=np.float64), (K,))
    rows, cols, vals = [], [], []

    def add(I, J, blocks):   # the 3 x 3 blocks (n, 3, 3) at block rows I and block columns J (n,)
        e = np.arange(3)
        rows.append(np.broadcast_to(3 * I[:, None, None] + e[None, :, None], blocks.shape).ravel())
        cols.append(np.broadcast_to(3 * J[:, None, None] + e[None, None, :], blocks.shape).ravel())
        vals.append(blocks.ravel())

    t = np.arange(T)
    for k in range(K):
        add(t * K + k, t * K + k, H[:, k])
        if apar[k] >= 0:
            b = np.einsum("ta,tb->tab", u[:, k], u[:, k]) / case["s"][k] ** 2
            p = int(apar[k])
            add(t * K + k, t * K + k, b)
            add(t * K + p, t * K + p, b)
            add(t * K + k, t * K + p, -b)
            add(t * K + p, t * K + k, -b)
    B = scipy.sparse.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(3 * T * K, 3 * T * K))
    P = scipy.sparse.csr_matrix(tro.penalty_matrix(T))
    return (scipy.sparse.kron(P, scipy.sparse.kron(scipy.sparse.diags(1.0 / acc ** 2), scipy.sparse.identity(3))) + B).tocsc()


def skeleton_window_cond(H, u, case, apar, window=WINDOW):
    """window_cond of the joint system: the larger of the Jacobi-scaled condition numbers of A = M + B over the first and over the last `window` frames"""
    T = H.shape[0]
    ends = [slice(0, T)] if T <= window else [slice(0, window), slice(T - window, T)]
    return max(sparse_cond(skeleton_matrix(H[e], u[e], case, apar)) for e in ends)


def count_band(history, cg_tol, cg_max=CG_MAX):
    """(lo, own, hi): the iterations after which a residual history first falls to 2 cg_tol, cg_tol and cg_tol / 2 (cg_max where it never does).
    Two float64 runs of the same recurrence drift apart; the step's bar allows the drift a factor of 2 on the residual (2 cg_tol), and by
    the same factor a sound run's count lies in lo .. hi around the oracle's own"""
    first = lambda t: next((i + 1 for i, v in enumerate(history) if v <= t), cg_max)
    return first(2 * cg_tol), first(cg_tol), first(cg_tol / 2)


def check_skeleton_system(name, case, got, cg_tol, cg_max=CG_MAX):
    """got: refine_skeleton_trajectories_system's fields (direction by child) on a long case at cg_tol.  Information, gradient and direction by
    skeleton_trajectory_oracle.check_system's 1e-12 bars against skeleton_evaluate; the costs within the cost bar of sto.costs at x + alpha
    d_returned; the step by its true preconditioned residual under the oracle's own operators (its H and u, not the returned ones):
    sqrt(r^T M^-1 r / G^T M^-1 G) <= 2 cg_tol + 100 eps window_cond.  The scalars of the recurrence (alpha, beta, the done word), which no other
    field shows: the returned cg_residual is at most cg_tol and within that same bar of the true residual, and cg_iterations lies in count_band()
    of the oracle's own conjugate gradients, run on to cg_tol / 2.  Returns (the fractions, the oracle's own PCG count)"""
    x = case["start"]
    ev = skeleton_evaluate(x, case)
    run, apar = ev["run"], ev["apar"]
    has = apar >= 0
    assert np.array_equal(got["status"], ev["status"]) and np.array_equal(got["n_usable"], ev["n_usable"]) and np.array_equal(got["n_single"], ev["n_single"]), (name, got["status"])
    H, G, d, u = got["information"], got["gradient"], got["step"], got["direction"]
    assert np.isfinite(H).all() and np.isfinite(G).all() and np.isfinite(d).all() and np.isnan(u[:, ~has]).all() and np.isfinite(u[:, has]).all(), name
    eh = np.abs(H - ev["H"]).max() / np.abs(ev["H"]).max()
    eg = (np.abs(G - ev["G"]).max(axis=(1, 2)) / ev["S"].max(axis=(1, 2))).max()
    eu = np.abs(u[:, has] - ev["u"][:, has]).max()
    assert run.all()   # (the long case: every track runs)
    op = SkeletonOperators(ev["H"], ev["u"], case, run, apar)
    res = op.relative_residual(ev["G"], d)
    cnd = skeleton_window_cond(ev["H"], ev["u"], case, apar)
    bar_r = 2 * cg_tol + 100 * EPS * cnd
    cost = ev["data"] + ev["pen"] + ev["bone"]
    tol = cost_bar(cost, cnd)
    trial = np.array([sto.objective(x + a * d, case, run, apar) for a in tro.ALPHAS])
    ec = max(np.abs(got["trial_costs"] - trial).max(), abs(got["data_cost"] - ev["data"]), abs(got["penalty_cost"] - ev["pen"]), abs(got["bone_cost"] - ev["bone"]))
    hist = []
    pcg(op, ev["G"], cg_tol / 2, cg_max, hist)
    lo, own, hi = count_band(hist, cg_tol, cg_max)
    nit, cgr = int(got["cg_iterations"]), float(got["cg_residual"])
    print(f"{name}: information {eh:.3g} (bar 1e-12), gradient {eg:.3g} of max S (bar 1e-12), direction {eu:.3g} (bar 1e-12), true preconditioned residual of the step {res:.3g} (bar "
          f"{bar_r:.3g}, window cond {cnd:.3g}), CG iterations {nit} to {cgr:.3g} (the oracle's own: {own}, allowed {lo} .. {hi}), costs {ec:.3g} (bar {tol:.3g})")
    assert eh <= 1e-12 and eg <= 1e-12 and eu <= 1e-12 and res <= bar_r and ec <= tol and 1 <= nit < cg_max, name
    assert cgr <= cg_tol and abs(cgr - res) <= bar_r and lo <= nit <= hi, (name, cgr, res, nit, lo, own, hi)
    return dict(information=eh / 1e-12, gradient=eg / 1e-12, direction=eu / 1e-12, step=res / bar_r, costs=ec / tol), own


def check_skeleton_loop(name, case, got, total):
    """refine_skeleton_trajectories after a few iterations on a long case: the history never rises, `cost` is the oracle's objective at the
    returned points within the cost bar, the CG iterations of the history add up to `total` (info["cg_iterations_total"])"""
    nus, nsg, status, run, apar = sto.running(case)
    assert run.all() and np.array_equal(got["status"], status), (name, got["status"])   # (the long case: every track runs)
    x, nit, h = got["points"], int(got["n_iterations"]), got["history"]
    assert nit >= 1 and len(h) == nit and np.isfinite(x).all() and np.isfinite(h).all() and got["cost"] == h[-1, 0] and h[0, 0] <= got["cost_start"], name
    assert (h[1:, 0] <= h[:-1, 0]).all(), (name, h[:, 0])
    c = sto.objective(x, case, run, apar)
    cnd = skeleton_window_cond(got["information"], got["direction"], case, apar)
    err, tol = abs(got["cost"] - c), cost_bar(c, cnd)
    print(f"{name}: iterations {nit}, cost {got['cost']:.12g} (oracle at the returned points {c:.12g}: {err:.3g}, bar {tol:.3g}, window cond {cnd:.3g}), alphas {h[:, 2]}, CG iterations {h[:, 3]}")
    assert err <= tol and total == int(h[:, 3].sum()), (name, err, tol, total)
    return err / tol


# ---------------------------------------------------------------- the scenes
ACCEL_L = (0.03, 0.09)
GAPS_L = [(100, 140), (30000, 30001), (65990, 66001)]
T_LONG = 66001


@functools.lru_cache(maxsize=None)
def long_scene():
    """L: 66001 frames (odd: the phantom frame; 258 evaluation workgroups per track) x 2 tracks, a 40-frame gap inside the first window, one
    missing frame in the middle, the last 11 frames missing (inside the last window).  Shared and read-only"""
    s = so.scene(T_LONG, 2, seed=12, gaps=GAPS_L)
    return dict(points=s["points"], cov=s["cov"], accel_std=np.array(ACCEL_L))


@functools.lru_cache(maxsize=None)
def long_weights():
    """weights_in of L drawn from {0, 0.25, 1, 4}"""
    return np.random.default_rng(66).choice(np.array([0.0, 0.25, 1.0, 4.0]), size=(T_LONG, 2))


@functools.lru_cache(maxsize=None)
def long_smooth_reference(weighted):
    L = long_scene()
    w = long_weights() if weighted else None
    return [smooth_reference(L["points"][:, k], L["cov"][:, k], L["accel_std"][k], None if w is None else w[:, k]) for k in range(2)]


@functools.lru_cache(maxsize=None)
def long_tracks():
    """evidence_oracle.Track of every track of L"""
    L = long_scene()
    return [eo.Track(L["points"][:, k], L["cov"][:, k]) for k in range(2)]


@functools.lru_cache(maxsize=None)
def long_evidence_reference(a):
    return [evidence_reference(t, a) for t in long_tracks()]


T_EV = 1301


@functools.lru_cache(maxsize=None)
def evidence_case():
    """1301 frames x 3 tracks at segment 2: 329 elimination lanes per track over six levels; the middle track has one usable frame"""
    s = eo.matched_scene(T_EV, 3, eo.A_TRUE, seed=1301, gap=(200, 212))
    s["points"][1:, 1] = np.nan
    return dict(points=s["points"], cov=s["cov"], segment=2, weights=None)


def evidence_lanes(T, segment):
    """elimination lanes of one track over all levels (mcba_smooth_math.h: smooth_lanes): what k_evidence_final's second loop walks"""
    return sum(1 if m == n else n // (m + 1) + 1 for n, m, _, _ in so.plan(T, segment, 1))


def eval_blocks(T):
    """workgroups of 256 frames per track of the evaluation kernels: what the final kernels' first loop walks"""
    return (T + 255) // 256


@functools.lru_cache(maxsize=None)
def long_refine_case():
    """66001 frames x 2 tracks x 3 cameras, huber; frames 150 .. 189 seen by camera 0 only and 250 .. 259 by nobody, both inside the first window"""
    s = tro.make_scene(3, T_LONG, 2, seed=41, p_drop=0.15, single=(150, 190), unseen=(250, 260), outliers=0.03)
    return tro.make_case(s, accel_std=np.array([0.15, 0.3]), loss="huber", segment=None, seed=41)


T_SK, K_SK = 9601, 8
BONES_SK = np.array([[0, 1], [1, 2], [2, 3], [4, 5], [5, 6], [6, 7]])


@functools.lru_cache(maxsize=None)
def long_skeleton_case():
    """9601 frames x 8 keypoints in two chains of four, 3 cameras: 76808 lanes, 301 workgroups of 256; a one-camera stretch of keypoint 1 and an
    unseen gap of keypoint 6, both inside the first window"""
    s = sto.make_scene(3, T_SK, BONES_SK, K_SK, seed=51, p_drop=0.15, single=((1, 150, 190),), unseen=((6, 250, 260),))
    return sto.make_case(s, segment=None, seed=51)


T_W, K_W = 41, 131
ACCEL_W = np.exp(np.linspace(np.log(0.02), np.log(0.5), K_W))
SEEDS_W = 16   # candidate seeds per track


@functools.lru_cache(maxsize=None)
def wide_smooth_case():
    """W for the smoother: 41 frames x 131 tracks, segment 3, accel_std log-spaced 0.02 .. 0.5, noise 0.3 .. 0.9 with 8 % of the frames displaced by
    15 (the robust scenes of smoothing_oracle); track 64 has no usable frame, 65 one, 66 exactly two.  Every other track is drawn from the first
    of its own seeds 1000 + 16 k + (0 .. 15) at which the oracle's loop is decided (smoothing_oracle.decided: its count does not hinge on
    rounding) and ends before the iteration limit -- the rule by which trajectory_refine_oracle and skeleton_trajectory_oracle choose their starts.  A seed for the whole scene
    cannot do that: a loop that contracts by rho per solve stops inside decided()'s factor-4 band around the threshold with probability
    log 4 / log(1 / rho), a third at these scenes' rho of 0.1 to 0.2, whatever the seed.  Shared and read-only"""
    pts, cov, seeds = np.empty((T_W, K_W, 3)), np.empty((T_W, K_W, 3, 3)), np.zeros(K_W, int)
    for k in range(K_W):
        for seed in range(1000 + SEEDS_W * k, 1000 + SEEDS_W * (k + 1)):
            s = so.scene(T_W, 1, seed=seed, sigma=0.3, ratio=3.0, outliers=0.08, outlier_size=15.0)
            if k in (64, 65, 66):
                break
            o = so.irls(s["points"][:, 0], s["cov"][:, 0], ACCEL_W[k], loss="soft_l1", f_scale=3.0)
            if so.decided(o) and o["n_iterations"] < 50:   # (and it ends before the iteration limit)
                break
        else:
            raise AssertionError(f"no decided seed for track {k}")
        pts[:, k], cov[:, k], seeds[k] = s["points"][:, 0], s["cov"][:, 0], seed
    pts[:, 64] = np.nan
    pts[1:, 65] = np.nan
    keep = np.zeros(T_W, bool)
    keep[[12, 30]] = True
    pts[~keep, 66] = np.nan
    return dict(points=pts, cov=cov, accel_std=ACCEL_W, loss="soft_l1", f_scale=3.0, segment=3, seeds=seeds)


def wide_track(case, k):
    """track k of W as a case of its own (K = 1, a scalar accel_std): what smoothing_oracle.check_robust takes"""
    return dict(case, points=case["points"][:, k:k + 1], cov=case["cov"][:, k:k + 1], accel_std=float(case["accel_std"][k]))


def wide_smooth_oracle():
    """(tracks the oracle's own loop leaves undecided, running tracks, its distinct iteration counts) of W"""
    case = wide_smooth_case()
    left_out, counts = 0, set()
    running = [k for k in range(K_W) if k not in (64, 65)]
    for k in running:
        o = so.robust_reference(f"W_{k}", wide_track(case, k))[0]
        left_out += not so.decided(o)
        counts.add(o["n_iterations"])
    return left_out, len(running), counts


def check_wide_smooth(case, got):
    """smoothing_oracle.check_robust per running track of W; tracks 64 and 65 are status -1 and NaN.  Returns (tracks left out, running tracks)"""
    left_out = ran = 0
    for k in range(K_W):
        one = {f: got[f][:, k:k + 1] for f in ("points", "weights", "mahalanobis2", "history")}
        one.update({f: got[f][k:k + 1] for f in ("status", "n_usable", "n_iterations")})
        if k in (64, 65):
            assert got["status"][k] == so.STATUS_TOO_FEW and got["n_usable"][k] == k - 64 and got["n_iterations"][k] == 0 and np.isnan(got["points"][:, k]).all(), k
            continue
        left_out += so.check_robust(f"W_{k}", wide_track(case, k), one)
        ran += 1
    assert got["n_usable"][66] == 2
    return left_out, ran


@functools.lru_cache(maxsize=None)
def wide_refine_case():
    """W for refine_trajectories: 41 frames x 131 tracks x 3 cameras, segment 3, the same accel_std; track 64 has no usable frame, 65 one, 66 two"""
    s = tro.make_scene(3, T_W, K_W, seed=61, p_drop=0.15)
    s["uvs"][:, :, 64:67] = np.nan
    for t, k in ((20, 65), (12, 66), (30, 66)):   # two cameras see these frames and no other
        for c in range(2):
            s["uvs"][c, t, k] = ks.project5(s["truth"][t, k], s["ext"][c], *s["intr"][c])
    return tro.make_case(s, accel_std=ACCEL_W, loss="soft_l1", segment=3, seed=61)
