/* mcba.h -- C ABI of libmcba.so, the MI355X (gfx950) bundle-adjustment hot path.
 *
 * The reference (dattalab-6-cam/multicam-calibration) is pure Python and has no FFI: the path sits
 * behind two Python seams.  This header is the boundary a maintainer would
 * bind with ctypes in place of them (INTEGRATION.md shows the stub):
 *
 *   outer seam  multicam_calibration/bundle_adjustment.py:195-204,307-327  bundle_adjust(...)
 *   inner seam  scipy least_squares fun/jac callables:
 *               residuals()                       bundle_adjustment.py:66-98
 *               bundle_adjustment_sparsity()      bundle_adjustment.py:101-125  (structure is implicit here)
 *               scipy 2-point FD Jacobian         scipy/optimize/_numdiff.py:628-705 (replaced by analytic blocks)
 *               scipy TRF + LSMR linear algebra   scipy/optimize/_lsq/trf.py:401-560 (replaced by LM + Schur, incl. the
 *                                                 reduced solve and the termination tests: mcba_lm_auto_*)
 *
 * Conventions
 *   - plain C types only; every function returns an int status (0 = MCBA_OK), never throws;
 *     mcba_last_error() returns the message of the last failure on the calling thread.
 *   - parameter vector x: [C x (fx fy cx cy k1 k2 rx ry rz tx ty tz) | F x (rx ry rz tx ty tz)]  float64,
 *     exactly serialize_params() of the reference (bundle_adjustment.py:128-157).
 *   - observations: float64 (C,F,N,2) C-order, NaN = missing scalar (bundle_adjustment.py:82-84,97).
 *   - one handle = one GPU = one process (frames are sharded across processes by the caller);
 *     calls on a handle come from one host thread.  The library owns its device buffers until
 *     mcba_destroy(); host arrays belong to the caller.
 *   - all kernels are enqueued on the handle's stream (mcba_set_stream; default: the null stream) and
 *     functions that return host data synchronise that stream.
 */
#ifndef MCBA_H
#define MCBA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MCBA_OK 0
#define MCBA_ERR_HIP 1        /* a HIP runtime call failed */
#define MCBA_ERR_ARG 2        /* bad argument / wrong call order */
#define MCBA_ERR_NONFINITE 3  /* a used observation projects to NaN/inf (scipy: "Residuals are not finite") */
#define MCBA_ERR_NODEVICE 4   /* no usable gfx950 device */

/* scipy.optimize.least_squares `loss=` (least_squares.py:160-227) */
#define MCBA_LOSS_LINEAR 0
#define MCBA_LOSS_SOFT_L1 1
#define MCBA_LOSS_HUBER 2
#define MCBA_LOSS_CAUCHY 3
#define MCBA_LOSS_ARCTAN 4
#define MCBA_LOSS_TABLE 5   /* not a name for mcba_set_loss: what mcba_set_loss_table switches the handle to (least_squares' callable `loss`) */

typedef struct mcba_handle mcba_handle;
typedef struct mcba_buffer mcba_buffer;   /* a device array that outlives its handle (mcba_residuals_detach) */

/* ---- library ------------------------------------------------------------------------------- */
int mcba_abi_version(void);            /* 7.  Bumped when this header changes (the mcba_flat_* block at the end is ADDITIVE to ABI 7: new entry points only, none changed): 7 (round 6) ADDS the mcba_calib_* (incl. mcba_calib_start, mcba_calib_graph) / mcba_pose_* / mcba_create_views block below (calibrate() on the device) and leaves every ABI-6 entry point as it was; 6 (round 5) ADDED mcba_prefilter, mcba_prefilter_subset, mcba_lm_run, mcba_lm_history, mcba_lm_result, mcba_set_bounds / _frozen, mcba_set_loss_table, mcba_set_trial, mcba_calib_normal_equations (and the diagnostics / life-cycle helpers declared below as ABI 6) and leaves every
                                        * ABI-5 entry point as it was.  (ABI 5 gave LM-state slots 25 / 26 -- "reserved" before -- their meaning: curvature floor / switch
                                        * fraction; a caller that zeroes them gets the handle's floor, fixed.) */
const char* mcba_last_error(void);
int mcba_device_count(int* count);

/* ---- problem life cycle -------------------------------------------------------------------- */
/* n_cameras C, n_frames F (local shard), n_points N, HIP device ordinal. */
int mcba_create(mcba_handle** out, int n_cameras, int n_frames, int n_points, int device);
/* The sparse-Schur handle (ADDITIVE to ABI 7): any number of cameras -- mcba_create refuses more than 40.  The Schur reduction runs over the
 * camera pairs that share a frame (a visibility index built from the observations on first use after an upload), the reduced system is
 * factorised by a stream-ordered sequence of multi-workgroup launches, and the reduce buffer keeps the dense layout.  Every entry point of
 * this header that takes a handle works on it, except: the speculative reduction (mcba_lm_auto_reduce(h, 2, .)) and the solve that decides
 * (mcba_lm_auto_solve(h, ., 1)) return MCBA_ERR_ARG -- its frame-sharded ticks take two collectives; calibrate()'s mcba_calib_* calls
 * return MCBA_ERR_ARG on a handle of more than 40 cameras (their kernels hold at most 40).  mcba_is_sparse: 1 for such a handle, 0 otherwise. */
int mcba_create_sparse(mcba_handle** out, int n_cameras, int n_frames, int n_points, int device);
int mcba_is_sparse(const mcba_handle* h);
/* Its visibility index, computed on the host from a (C, F) mask (seen[c * F + f] != 0: camera c has a detection in frame f); needs no
 * device.  sizes[4]: entries (seen pairs), co-visible camera pairs, pair-frame items, chunks.  out (NULL: sizes only), `capacity` ints:
 * frame_off (F + 1) | ent_cam (entries, frame-major, cameras ascending) | ent_frame | items (3 per item: entry of camera i, entry of camera
 * j, frame; pairs (i <= j) in (i, j) order, frames ascending) | chunks (3 per chunk of <= 64 items: first item, count, i == j) |
 * pair_map (C x C: pair id of (i, j), i <= j, or -1) | pair_chunks (pairs + 1: each pair's first chunk). */
int mcba_sparse_index(const unsigned char* seen, int n_cameras, int n_frames, int* sizes, int* out, size_t capacity);
int mcba_destroy(mcba_handle* h);
/* Device and pinned buffers of destroyed handles are parked in a per-process pool and handed out again (hipMalloc / hipFree are
 * synchronising driver calls: 4 ms of a 16 ms bundle_adjust() at 6 x 10 000 x 54 before the pool).  MCBA_POOL_MB caps what is
 * parked (default 2048; 0 = no pool); this returns everything to the driver.  The solver's own buffers (records, partial sums,
 * reduce buffer, state ring) are allocated on the first call that needs them: a handle that only runs the pre-filter over all
 * frames of a long recording holds the observations and nothing else. */
int mcba_pool_trim(void);
/* Bytes of device memory the handle holds right now. */
size_t mcba_device_bytes(const mcba_handle* h);
/* Returns every device buffer to the pool except what defines the problem (observations in both layouts, board, parameter slots, the box of
 * mcba_set_bounds): solver buffers, pre-filter scores, Jacobian / residual blocks, calibrate()'s poses.  Calls that need them allocate them
 * again; a numeric x_scale / frozen set given before the trim is put back into the new buffers.  For handles that are parked so that
 * something can be produced from them later (the lazily attached result.jac): 0.26 -> 0.11 GB at 6 x 10 000 x 54.  Synchronises. */
int mcba_trim(mcba_handle* h);
/* The observations the handle holds, (C,F,N,2) doubles, back to the host (the values the solve saw). */
int mcba_download_observations(mcba_handle* h, double* uvs);
/* hipStream_t to enqueue on (e.g. torch.cuda.current_stream().cuda_stream); NULL = null stream. */
int mcba_set_stream(mcba_handle* h, void* hip_stream);
/* Observations (C,F,N,2) and board points (N,3), host pointers.  Re-laid out on the GPU as
 * [camera][point][frame] (u,v) pairs so that a wavefront reads 64 consecutive frames coalesced. */
int mcba_upload_observations(mcba_handle* h, const double* uvs, const double* objpoints);
/* Robust loss and f_scale of least_squares (default soft_l1, 1.0: bundle_adjustment.py:301-303). */
int mcba_set_loss(mcba_handle* h, int loss, double f_scale);
/* least_squares' CALLABLE `loss` -- rho(z) -> (rho, rho', rho'') (least_squares.py:160-227; the reference forwards it untouched: bundle_adjustment.py:301-313).
 * The function is the caller's, so are its values: tab3 = three (C,F,N,2) arrays in the order of the observations, evaluated at the residuals
 * (mcba_residuals) of the point that is linearised next: [0] 0.5 f_scale^2 rho(z), [1] rho'(z), [2] max(rho' + 2 rho'' z, EPS) (scipy's J_scale^2,
 * common.py:720-731); entries of missing observations are ignored.  mcba_linearize then builds the normal equations with these weights; the
 * trial cost of mcba_step is the caller's to evaluate (its function on the trial residuals); mcba_jacobian_eval returns unscaled rows;
 * mcba_step_linearize and the device-resident loops (mcba_lm_iterate, mcba_lm_auto_*, mcba_lm_run) refuse to run.  mcba_set_loss switches back. */
int mcba_set_loss_table(mcba_handle* h, const double* tab3);

/* Camera block width (round 4, ABI 5).  12 (default): all 12 parameters of every camera are variables, as in the reference
 * (bundle_adjustment.py:113,121-122,149-155).  6: the intrinsics (fx fy cx cy k1 k2) of EVERY camera are held fixed -- BASELINE
 * configs[1] ("intrinsics fixed: extrinsics + points only"; SURVEY section 8c-8: the reference has no entry point for it, its oracle is
 * a wrapper fun(y) = residuals(scatter(y, frozen intrinsics))).  With 6 the linearisation accumulates the (rho, t) blocks alone,
 * the reduced camera system is 6C x 6C -- row i is parameter 6 + i % 6 of camera i / 6 -- and EVERY camera-system quantity of this
 * ABI has 6 entries per camera: mcba_reduced_size / mcba_get_reduced (n = 6C), the camera step of mcba_step* / mcba_lm_* /
 * mcba_get_cam_step, the `fixed` flags of mcba_lm_auto_config.  The parameter vector x keeps the reference's layout (12 per camera;
 * the intrinsics are copied unchanged into every trial point).  Must be called before the first solver entry point of the handle
 * (MCBA_ERR_ARG afterwards, and for width 6 with more than 26 cameras: hold those with the `fixed` flags instead). */
int mcba_set_camera_block(mcba_handle* h, int width);
int mcba_get_camera_block(const mcba_handle* h);
/* Curvature weight of the linearisations enqueued from now on: w = max(rho' + 2 rho'' f^2, floor * rho'), 0 < floor <= 1.
 * 1 (default) = the IRLS weight rho' (monotone: the model for points far from the optimum); 0.1 = Triggs' second-order term with a
 * safety floor (fast at the optimum).  The reference has no counterpart: scipy's TRF always uses the Triggs weight clamped at EPS
 * (common.py:720-731); the stationary point does not depend on the choice, the number of evaluations does (16 -> 6 to the reference's
 * default tolerance at 6 x 10 000 x 54).  solver.py switches between ticks: IRLS, Triggs after an accepted step that gained < 1 %. */
int mcba_set_curvature_floor(mcba_handle* h, double floor);
double mcba_get_curvature_floor(const mcba_handle* h);

/* least_squares' numeric `x_scale` (forwarded verbatim by the reference: bundle_adjustment.py:301-313; scipy least_squares.py
 * :243, trf.py:415-420): 12C + 6F positive doubles in the layout of x -> the FIXED damping matrix D = diag(1 / x_scale^2) replaces
 * Marquardt's D = diag(J^T J) (which is x_scale = 'jac', the reference's default) in the frame blocks, the camera block and the
 * predicted reduction.  NULL returns to 'jac'.  MCBA_ERR_ARG with scipy's message if an entry is not positive and finite. */
int mcba_set_x_scale(mcba_handle* h, const double* x_scale);
/* Box constraints and the working set of an active-set method (round 5; the reference forwards `bounds` to scipy's least_squares:
 * bundle_adjustment.py:301-313, scipy trf_bounds).
 * mcba_set_bounds: lo <= x <= hi, 12C + 6F doubles each in the layout of x (-inf / +inf = none; both NULL = no constraints).  From then
 *   on the trial point of every mcba_step / mcba_step_linearize / mcba_step_fetch is projected onto the box before its cost is taken;
 *   the device-resident loops (mcba_lm_iterate, mcba_lm_auto_*, mcba_lm_run) refuse to run while bounds are set.
 * mcba_set_frozen: mask of 12C + 6F bytes (non-zero = frozen; NULL = none) -- a frozen FRAME coordinate gets a step of exactly 0 and
 *   nothing couples to it in the Schur reduction and the back-substitution (the reported frame gradient stays the true one); camera
 *   entries are ignored here (freeze camera parameters with the flags of mcba_lm_auto_config, or leave their rows out of a host solve).
 *   Takes effect with the next mcba_build_reduced. */
int mcba_set_bounds(mcba_handle* h, const double* lo, const double* hi);
int mcba_set_frozen(mcba_handle* h, const unsigned char* mask);

/* ---- parameter slots (two flat vectors live on the GPU: 0 and 1) ----------------------------- */
int mcba_set_params(mcba_handle* h, int slot, const double* x);   /* 12C+6F doubles, host */
int mcba_get_params(mcba_handle* h, int slot, double* x);
int mcba_copy_params(mcba_handle* h, int dst_slot, int src_slot);  /* device to device */

/* ---- residual / Jacobian evaluation (replaces residuals() and scipy's FD Jacobian) ----------- */
/* Robust cost 0.5*f_scale^2*sum rho((f/f_scale)^2) at x[slot]; *n_residuals = number of non-NaN scalars.
 * MCBA_ERR_NONFINITE if the cost is not finite. */
int mcba_cost(mcba_handle* h, int slot, double* cost, double* n_residuals);
/* Dense residual array (C,F,N,2), observed - predicted, 0 where the observation is NaN (host). */
int mcba_residuals(mcba_handle* h, int slot, double* res);
/* The same array -- with NaN instead of 0 where the observation is missing, so that it carries its own row mask (ABI 6) -- left
 * ON THE DEVICE as an object of its own (it outlives the handle): api.bundle_adjust hands it to the
 * OptimizeResult and downloads it when `result.fun` is first read -- scipy materialises `fun` (trf.py:557-560), but 52 MB of
 * device-to-host copy at 6 x 10 000 x 54 for a field few callers read was the largest single item of the call.
 * mcba_buffer_count: doubles in it; mcba_buffer_download: copy to host (synchronises); mcba_buffer_free: back to the pool. */
int mcba_residuals_detach(mcba_handle* h, int slot, mcba_buffer** out);
size_t mcba_buffer_count(const mcba_buffer* b);
int mcba_buffer_download(mcba_buffer* b, double* host);
int mcba_buffer_free(mcba_buffer* b);
/* Which scalars of the uploaded observations are present (not NaN), from the GPU's own copy: bits = numpy.packbits(~numpy.isnan(uvs))
 * over the (C, F, N, 2) array, (2 C F N + 7) / 8 bytes, host.  It is the row selection of the reference's residual vector and
 * Jacobian (bundle_adjustment.py:68-69 `mask = ~np.isnan(uvs)`, :101) without a pass over the caller's array; synchronises. */
int mcba_seen_bits(mcba_handle* h, unsigned char* bits);
/* Materialise residuals + analytic Jacobian blocks on the GPU: per scalar residual 18 doubles
 * [12 camera columns | 6 frame-pose columns] in (C,F,N,2,18) order = the CSR `data` array of the
 * reference's Jacobian when no observation is missing.  robust_scaled != 0 applies scipy's
 * sqrt(rho' + 2 rho'' f^2) row scaling (common.py:720-731).  Result stays on the GPU. */
int mcba_jacobian_eval(mcba_handle* h, int slot, int robust_scaled);
/* Copy the last mcba_jacobian_eval() result to the host: jac (C,F,N,2,18), res (C,F,N,2); either may be NULL. */
int mcba_jacobian_download(mcba_handle* h, double* jac, double* res);

/* ---- Levenberg-Marquardt building blocks (replace trf.py:450-551 + LSMR) ---------------------- */
/* Linearise at x[slot]: per (camera, frame) local Gram matrices expanded to W_cf (12x6), V_cf (6x6),
 * g_f and per-wave partial sums of U_c (12x12), g_c and the robust cost.  Kept on the GPU. */
int mcba_linearize(mcba_handle* h, int slot);
/* Schur-reduce the current linearisation with damping lambda (frame blocks damped by
 * lambda*diag(V_f)) into the reduce buffer (device), laid out as doubles, n = 12C:
 *   [0,n*n)      S0  = blockdiag(U_c) - sum_f W_f (V_f + lambda D_f)^-1 W_f^T      (undamped camera block)
 *   [n*n,+n)     rhs = -g_c + sum_f W_f (V_f + lambda D_f)^-1 g_f
 *   [..,+n)      diag(U)          [..,+n)  g_c
 *   [..,+16)     scalars: 0 cost, 1 number of (camera, frame) pairs with data, 2 n_cholesky_failures, 3 reserved,
 *                         4..15 per-rank slots: max |g_f| of THIS shard goes to slot 4+rank_slot, others 0
 * so that one all-reduce(SUM) of the whole buffer over the frame shards gives the global system. */
int mcba_build_reduced(mcba_handle* h, double lambda, int rank_slot);
size_t mcba_reduced_size(const mcba_handle* h);          /* doubles in the reduce buffer: system + 8 trial scalars + MCBA_LM_STATE */
/* Let the caller own the reduce buffer (device pointer, mcba_reduced_size() doubles), e.g. a torch
 * tensor handed to torch.distributed.all_reduce (RCCL).  NULL restores the internal buffer. */
int mcba_bind_reduce_buffer(mcba_handle* h, double* device_ptr);
int mcba_get_reduced(mcba_handle* h, double* host);      /* D2H of the system part (n*n+3n+16 doubles) */
/* Back-substitute: given the camera step (12C doubles, host) solve every frame step,
 * write x[dst_slot] = x[src_slot] + delta and evaluate the robust cost there.  Trial scalars
 * (8 doubles, appended to the reduce buffer at offset n*n+3n+16):
 *   0 cost(x_dst)  1 sum_f d_f^T (lambda D_f d_f - g_f)  2 sum |d_f|^2  3 sum |x_f|^2  4 n_residuals  5..7 reserved */
int mcba_step(mcba_handle* h, const double* delta_cam, double lambda, int src_slot, int dst_slot);
/* Same, but instead of a cost-only pass the trial point x[dst] is LINEARISED (as mcba_linearize) into the
 * handle's second linearisation buffer; its robust cost fills trial scalar 0 (scalar 4 = number of
 * (camera, frame) pairs with data).  If the step is accepted, mcba_accept_linearization() makes that buffer the
 * current one at no GPU cost -- an accepted LM iteration then needs ONE pass over the observations, not two. */
int mcba_step_linearize(mcba_handle* h, const double* delta_cam, double lambda, int src_slot, int dst_slot);
int mcba_accept_linearization(mcba_handle* h);
int mcba_get_trial(mcba_handle* h, double* host8);
int mcba_set_trial(mcba_handle* h, const double* host8);   /* the eight trial scalars, written back (a tabulated loss in a frame-sharded run: [the caller's cost of THIS shard's trial point, the step's other scalars], before the all-reduce) */
/* Convenience for the single-GPU loop (one ABI crossing instead of two):
 *   mcba_reduce_fetch     = mcba_build_reduced + mcba_get_reduced
 *   mcba_step_fetch       = mcba_step (linearize == 0) or mcba_step_linearize (linearize != 0) + mcba_get_trial */
int mcba_reduce_fetch(mcba_handle* h, double lambda, int rank_slot, double* host);
int mcba_step_fetch(mcba_handle* h, const double* delta_cam, double lambda, int src_slot, int dst_slot, int linearize, double* host8);
/* ---- device-resident LM iteration: ONE host synchronisation per iteration ----------------------------
 * The reduce buffer carries, behind the system (n*n+3n+16) and the 8 trial scalars, MCBA_LM_STATE = 32 doubles:
 *   0 cost  1 lambda  2 nu  3 sel (index of the current parameter slot AND linearisation buffer)  4 accepted
 *   5 cost_new  6 predicted reduction  7 ratio  8 step norm  9 x norm  10 actual reduction;
 *   11..24 belong to the device-resident solve below (0 for the host-solve entry points);
 *   25 curvature floor of the NEXT linearisations (1 = the IRLS weight rho', 0.1 = Triggs' term with a floor; 0 in the array handed to
 *      mcba_lm_set_state = the handle's value, mcba_set_curvature_floor)   26 switch fraction (> 0: the decision moves slot 25 -- Triggs
 *      after an accepted step that gained less than this fraction of the cost, IRLS after a rejection whose cost rose by more than 1e-9 of
 *      itself; 0: slot 25 stays)   27..31 reserved.
 * mcba_lm_set_state uploads it (after mcba_linearize(slot = sel) + mcba_build_reduced);
 * mcba_lm_trial            : back-substitute delta_cam from the current point, linearise the trial point
 *                            (other slot / buffer), sum its cost  -> trial scalars;  [all-reduce them when sharded]
 * mcba_lm_decide_reduce    : accept/reject (with a round-off guard for |dF| <= 32 EPS F) + Nielsen damping update (a rejection whose
 *                            cost rose by less than 1e-9 of itself doubles the damping without escalating) ON THE
 *                            GPU (same rule as the host driver, solver.py),
 *                            then Schur-reduce whichever linearisation is now current with the new lambda;
 *                            pred_cam = d_c^T(lambda D_c d_c - g_c), dcn2 = |d_c|^2, xcn2 = |x_c|^2 from the host solve;
 *                            [all-reduce the system when sharded]
 * mcba_lm_fetch            : D2H of system + trial scalars + state (mcba_reduced_size() doubles) and synchronise;
 * mcba_lm_iterate          : the three above in one call (single GPU);
 * mcba_lm_rebuild          : Schur-reduce again with the state's lambda (after the host changed it with set_state). */
#define MCBA_LM_STATE 32
int mcba_lm_set_state(mcba_handle* h, const double* state);
int mcba_lm_trial(mcba_handle* h, const double* delta_cam);
int mcba_lm_decide_reduce(mcba_handle* h, double pred_cam, double dcn2, double xcn2, double lam_min, double lam_max, int rank_slot);
int mcba_lm_rebuild(mcba_handle* h, int rank_slot);
int mcba_lm_fetch(mcba_handle* h, double* host);
int mcba_lm_iterate(mcba_handle* h, const double* delta_cam, double pred_cam, double dcn2, double xcn2, double lam_min, double lam_max, double* host);
/* ---- device-resident LM loop: NO host synchronisation per iteration --------------------------------------------
 * The reduced camera system is factorised and solved on the GPU as well (k_solve_cam: blocked FP64 Cholesky on
 * v_mfma_f64_16x16x4, one workgroup), the ftol / xtol / gtol tests of scipy (least_squares.py / trf.py:529-551) run
 * there, and the host only enqueues "ticks" and reads the state each tick posts to a host-mapped ring of 16 slots.
 *   state 11 pred_cam  12 |d_c|^2  13 |x_c|^2  14 skip (reduced solve failed: next tick only re-damps)  15 done (0 or
 *   the scipy status 1..4)  16 first-order optimality  17 trial evaluations  18 accepted steps  19 pending verdict
 *   20 lambda of the last trial  21 cost before it  22 ticks that did work  23 solve info (0 ok, 1 not positive
 *   definite, 2 a frame block failed)  24 last tick was a rebuild  31 (ring slots) sequence number.
 * mcba_lm_auto_config : tolerances, damping bounds, optional mask (n bytes, 1 = camera parameter held fixed);
 * mcba_lm_auto_solve  : optimality + termination verdict + solve of the system in the reduce buffer -> camera step on
 *                       the device, state posted to ring slot seq % 16 with sequence number `seq` (>= 1);
 *                       call once after mcba_build_reduced + mcba_lm_set_state (decide = 0), then once per tick;
 * mcba_lm_auto_trial  : back-substitute that step, linearise the trial point, sum its cost; decide > 0: accept/reject on
 *                       the same launch (single GPU);  [sharded: decide = 0, all-reduce the 8 trial scalars];  decide = -1:
 *                       no sums here -- the speculative reduction that follows (mcba_lm_auto_reduce(h, 2, .)) writes the trial
 *                       scalars itself, one launch less per tick;
 * mcba_lm_auto_reduce : decide = 0: Schur reduction of the current linearisation (the decision has been taken);
 *                       decide = 1: the stand-alone decision kernel first (sharded runs with TWO collectives: trial scalars,
 *                       then the system);  decide = 2: SPECULATIVE reduction (sharded runs with ONE collective): the trial
 *                       linearisation is reduced before the decision is known, on the prediction "accepted, lambda' =
 *                       max(lambda / 3, lambda_min)", and the 8 trial scalars [cost, pred_f, |d_f|^2, |x_f|^2, #pairs, stale, 0, 0]
 *                       are (re)written behind the system (stale = 1 if a back-substitution workgroup of this handle's previous fused
 *                       launch gave up waiting for its solve: the SUM over the shards is what the deciding solve tests, so that every
 *                       shard discards such a tick); the caller all-reduces [system | trial scalars] in one go
 *                       (offset 0, n*n + 3n + 16 + 8 doubles) and calls mcba_lm_auto_solve(seq, decide = 1), which takes
 *                       the decision and, if the prediction does not hold (rejected step, or another damping), marks the
 *                       next tick as a rebuild-only tick instead of solving;
 *                       With <= 9 cameras the solve's launch also carries the back-substitution of the NEXT trial step (after a
 *                       speculative reduction, or inside mcba_lm_auto_tick on one GPU): the following mcba_lm_auto_trial /
 *                       mcba_lm_auto_tick then starts with the linearisation of that trial point.  MCBA_FUSE_BACKSUB=0 disables it.
 * mcba_lm_auto_tick   : trial + reduce + solve in one call; with a direct RCCL communicator attached (mcba_comm_init) the
 *                       library issues the collective(s) itself -- one per tick (speculative), or two with MCBA_SPECULATE=0;
 * mcba_lm_auto_wait   : spin on the ring slot until tick `seq` has posted (falls back to a stream synchronisation after
 *                       50 ms) and copy its MCBA_LM_STATE doubles.  At most 15 ticks may be outstanding.
 * After termination (state 15 != 0) the kernels of later ticks return at once; such ticks still post their slot. */
int mcba_lm_auto_config(mcba_handle* h, double ftol, double xtol, double gtol, double lam_min, double lam_max, const unsigned char* fixed_mask);
/* Floor of Nielsen's damping factor on an accepted step, lambda *= max(floor, 1 - (2 ratio - 1)^3); 0 (the default of a new handle)
 * = the classical 1/3.  Applies to every decision the library takes (mcba_lm_decide_reduce, mcba_lm_iterate, the device-resident
 * loop) and to the prediction its speculative Schur reduction is built on.  The Python driver sets 1/10 (solver.py). */
int mcba_lm_set_decrease_floor(mcba_handle* h, double dec_floor);
int mcba_lm_auto_solve(mcba_handle* h, unsigned long long seq, int decide);
int mcba_lm_auto_trial(mcba_handle* h, int decide);
int mcba_lm_auto_reduce(mcba_handle* h, int decide, int rank_slot);
int mcba_lm_auto_tick(mcba_handle* h, unsigned long long seq, int rank_slot);
int mcba_lm_auto_wait(mcba_handle* h, unsigned long long seq, double* state);
/* ---- whole stages of bundle_adjust() per crossing (round 5, ABI 6) ----------------------------------------------
 * mcba_lm_run: the device-resident loop from start to finish in ONE call -- what the caller otherwise drives through
 * mcba_set_params, mcba_linearize, mcba_reduce_fetch, mcba_lm_set_state, mcba_lm_auto_config, mcba_lm_auto_solve and then
 * mcba_lm_auto_tick / mcba_lm_auto_wait per iteration (the loop scipy's trf_no_bounds runs on the host: trf.py:401-560).  Nothing waits
 * between the upload of x0 and the first tick: the start state is written on the device from the reduced system of the start point,
 * the first `depth` ticks are enqueued behind the first solve, then the host polls the state ring.  The ticks, their order and every
 * decision are those of the per-call sequence (the device decides; the host only keeps `depth` ticks in flight).
 *   x0      12C + 6F doubles, or NULL to start from what parameter slot 0 holds (mcba_create_subset gathers it on the device)
 *   opt     13 doubles: 0 ftol 1 xtol 2 gtol (0 = that test off) 3 lambda_0 4 lambda_min 5 lambda_max 6 floor of Nielsen's factor
 *           (0 = 1/3) 7 curvature floor of the first linearisations (mcba_set_curvature_floor) 8 curvature switch fraction (state slot
 *           26; 0 = fixed model) 9 max_nfev 10 max iterations (< 0: none) 11 ticks in flight (1..12) 12 rank slot (0 on one GPU)
 *   fixed   n bytes (1 = camera-system variable held fixed) or NULL
 *   summary 4 doubles out: 0 status (scipy's 1..4; 0 = a limit was reached) 1 rows recorded 2 rows consumed by the loop proper (the
 *           rest were retired by the final drain of ticks still in flight) 3 iterations
 * MCBA_ERR_NONFINITE: "Residuals are not finite in the initial point." (least_squares.py).  With a direct RCCL communicator attached the
 * start system is all-reduced and every tick carries its collective, as in mcba_lm_auto_tick.
 * mcba_lm_history: the MCBA_LM_STATE doubles every retired tick posted, row 0 = the solve of the start point (cost, optimality).
 * mcba_lm_result: x of parameter slot `slot` (12C + 6F doubles -> x_out) and the gradient J^T f there (OptimizeResult.grad: the camera
 * gradient g_c of the reduce buffer scattered to the parameter layout, 0 where a parameter is held fixed, then the frame gradients),
 * packed on the device.  grad_out != NULL: x_out must have room for 2 (12C + 6F) doubles and grad_out == x_out + 12C + 6F -- one copy
 * brings both; grad_dev != NULL (and grad_out NULL): the gradient stays on the device as a mcba_buffer of its own (mcba_buffer_download /
 * mcba_buffer_free), for callers that attach it lazily; both NULL: x alone. */
int mcba_lm_run(mcba_handle* h, const double* x0, const double* opt, const unsigned char* fixed, double* summary);
int mcba_lm_history(mcba_handle* h, double* rows, size_t capacity_rows);
int mcba_lm_result(mcba_handle* h, int slot, double* x_out, double* grad_out, mcba_buffer** grad_dev);
/* k_solve_backsub's back-substitution workgroups wait for the solve of the same launch with a BOUNDED poll (~0.5 s).  If one ever
 * runs out, it stamps the tick's number into a device word and a host-mapped word: the next tick's decision discards its (stale)
 * trial point and only rebuilds the system, and mcba_lm_auto_wait switches the handle to the two-launch path (k_solve_cam, then
 * k_backsub) for good.  *timeouts = number of the last tick in which that happened (0: never), *fused = the fused launch is still
 * in use.  MCBA_FUSE_MAX_POLLS=0 forces the event (tests). */
int mcba_lm_fuse_status(mcba_handle* h, double* timeouts, int* fused);
/* The waiting side of that protocol.  Default since round 6 (on != 0): the readers ACQUIRE the release word with an agent-scope fence -- the
 * form the HIP memory model asks for.  on == 0: the readers poll and read with agent-scope relaxed atomic loads and rely on gfx950's in-order
 * issue -- measured ~1.3 us per iteration faster (1.3 % at 6 x 10 000 x 54), stress-tested bit-identical, but a data race under the HIP
 * memory model.  Chosen at run time per handle; a new handle takes MCBA_STRICT_SYNC from the environment (unset = 1; mcba_create_subset /
 * mcba_create_views inherit their source's setting).  Results are identical to the bit. */
int mcba_set_strict_sync(mcba_handle* h, int on);
int mcba_get_strict_sync(const mcba_handle* h);
/* The camera step (12C doubles) the last mcba_lm_auto_solve left on the device; synchronises. */
int mcba_get_cam_step(mcba_handle* h, double* host);
/* ---- direct RCCL (optional; frame-sharded runs) ------------------------------------------------------------
 * The library dlopen()s the RCCL already loaded in the process (torch's) -- it is not linked against it.
 * Rank 0 calls mcba_comm_unique_id (128 bytes), the caller broadcasts them (e.g. torch.distributed), every rank
 * calls mcba_comm_init; mcba_comm_allreduce then enqueues ncclAllReduce(SUM, f64, in place) on `count` doubles of the
 * reduce buffer starting at `offset`, on the handle's stream (no host synchronisation, no Python dispatch). */
int mcba_comm_unique_id(unsigned char* out128);
int mcba_comm_init(mcba_handle* h, const unsigned char* id128, int rank, int world);
int mcba_comm_allreduce(mcba_handle* h, size_t offset, size_t count);
int mcba_comm_count(mcba_handle* h, int* count);   /* ranks of the attached communicator (ncclCommCount); 0 if none */
int mcba_comm_destroy(mcba_handle* h);
/* Frame part of the gradient J^T f of the last mcba_build_reduced(): (F,6) doubles, host.
 * (The camera part is the g_c block of the reduce buffer.)  Feeds OptimizeResult.grad (trf.py:557-560). */
int mcba_get_frame_gradient(mcba_handle* h, double* host);

/* ---- robust triangulation (reference geometry.py:361-433 `triangulate`) ------------------------
 * Stateless: uvs (C, P, 2) detections (NaN = unseen), cam12 (C, 12) camera blocks in the parameter layout above,
 * dist5 (C, 5) OpenCV distortion (k1 k2 p1 p2 k3) or NULL (then k1, k2 of cam12), iterations of the undistortion
 * fixed point (OpenCV's default: 5).  out (P, 3): per-coordinate nan-median over all camera pairs of the linear (DLT)
 * two-view triangulations, NaN where fewer than two cameras see the point.  2 <= C <= 64 (up to 8 cameras: one lane per point,
 * everything in registers; beyond: one wavefront per point, the camera pairs across its lanes).  kernel_ms (may be NULL)
 * receives the kernel time measured with HIP events. */
int mcba_triangulate(int n_cameras, size_t n_points, const double* uvs, const double* cam12, const double* dist5, int iterations, int device, double* out, double* kernel_ms);

/* ---- keypoints through a calibration (reference geometry.py:128-152, :277-325; additive to ABI 7) -------------
 * Stateless like mcba_triangulate: host arrays in and out, cam12 (C, 12) camera blocks, kernel_ms (may be NULL) the kernels' time.
 * No limit on the camera count unless stated: the kernels take the camera table in groups of 64.  n_points == 0 returns at once. */
/* `project_points` for every camera from one upload of points (P, 3): uvs_out (C, P, 2).  dist5 NULL: the reference's model, k1 and k2 of
 * cam12 (geometry.py:309); dist5 (C, 5): the forward five-coefficient model (k1 k2 p1 p2 k3), what cv2.undistortPoints inverts.  Nothing
 * special for points behind a camera; NaN in, NaN out. */
int mcba_project_points(int n_cameras, size_t n_points, const double* points, const double* cam12, const double* dist5, int device, double* uvs_out, double* kernel_ms);
/* `apply_rigid_transform`: out (P, 3) = R points + t, T12 = R (9, row-major) then t (3). */
int mcba_rigid_transform(size_t n_points, const double* points, const double* T12, int device, double* out);
/* Distance in pixels between each camera's detection uvs (C, P, 2) (raw, distorted; NaN = unseen) and the five-coefficient projection of
 * points (P, 3) (dist5 NULL: k1, k2 of cam12).  errors_out (C, P) or NULL: NaN where the camera does not see the point or the point has a NaN;
 * median_out (C): np.nanmedian of each row, exact (radix select on the device; NaN for a camera that sees nothing). */
int mcba_keypoint_errors(int n_cameras, size_t n_points, const double* points, const double* uvs, const double* cam12, const double* dist5, int device, double* errors_out, double* median_out,
                         double* kernel_ms);
/* Per point, Levenberg-Marquardt on 0.5 sum rho(f^2) over X, f = the raw detections minus the five-coefficient projection in the cameras that
 * see the point; rho / f_scale as scipy.optimize.least_squares, loss 0 .. 4 = linear soft_l1 huber cauchy arctan.  points_in (P, 3) is the
 * start, or NULL: the median of pairs of mcba_triangulate (with undistort_iterations), computed from the same upload of uvs.  2 <= C <= 64.
 * points_out (P, 3): NaN where fewer than two cameras see the point or the start has a NaN; never worse than the start in the robust cost.
 * info_out (P, 4) or NULL: cost at the result, cost at the start, iterations, status (1 converged, 0 iteration limit, -1 too few views). */
int mcba_triangulate_refine(int n_cameras, size_t n_points, const double* uvs, const double* cam12, const double* dist5, const double* points_in, int undistort_iterations, int loss, double f_scale,
                            int max_iterations, int device, double* points_out, double* info_out, double* kernel_ms);
/* Consensus triangulation (additive to ABI 7): which camera's detection of a point is wrong, and the point without it.  Per point,
 * every camera pair that sees it gives a hypothesis (the two-view DLT point of mcba_triangulate, undistort_iterations rounds); a camera that sees
 * the point is an inlier of a hypothesis when the point lies in front of it and its raw detection is within threshold (pixels, > 0) of the
 * five-coefficient projection; the hypothesis of lowest truncated cost (sum of e^2 for inliers, threshold^2 otherwise; an exact tie goes to
 * the first pair in the order (0,1), (0,2), ..., (1,2), ...) wins, and the point is refitted on its inliers alone as mcba_triangulate_refine
 * does (loss, f_scale, max_iterations; max_iterations 0 returns the hypothesis itself).  The mask is not voted again after the refit.
 * 2 <= C <= 64, min_views >= 2.  points_out (P, 3); inliers_out (P): bit c of word p set = camera c is an inlier of point p;
 * info_out (P, 8) or NULL: inlier count, winning pair (i, j), winning cost, refit cost at the result and at the start, iterations, status
 * (1 converged, 0 iteration limit, -1 too few views: no hypothesis, point NaN, empty mask, pair (-1, -1); -2 no consensus: fewer than min_views
 * inliers, point NaN, the mask still reported); errors_out (C, P) or NULL: as mcba_keypoint_errors at points_out. */
int mcba_triangulate_consensus(int n_cameras, size_t n_points, const double* uvs, const double* cam12, const double* dist5, double threshold, int min_views, int undistort_iterations, int loss,
                               double f_scale, int max_iterations, int device, double* points_out, unsigned long long* inliers_out, double* info_out, double* errors_out, double* kernel_ms);

/* ---- the wrapper's frame pre-filter (bundle_adjustment.py:265-285) and frame subsets ------------------------ */
/* Reprojection error |observed - predicted| of every detection at x[slot].  Host outputs, both (C,F) row-major:
 * mean_cf = np.nanmean over the board points (NaN where the camera does not see the frame), full_cf = number of
 * points with both coordinates present (== N  <=>  the detection is complete: bundle_adjustment.py:266).  The per-point
 * errors stay on the GPU for mcba_error_median. */
int mcba_frame_errors(mcba_handle* h, int slot, double* mean_cf, double* full_cf);
/* np.nanmedian of those per-point errors over the frames with frame_mask[f] != 0 (F bytes; NULL = all frames): the exact
 * order statistic (radix select), mean of the two middle values for an even count; *count = number of values. */
int mcba_error_median(mcba_handle* h, const unsigned char* frame_mask, double* median, double* count);
/* One pass of that radix select for a caller that holds only a SHARD of the frames (frame-sharded bundle_adjust: every rank runs
 * the pre-filter on its own slice): hist256[b] = number of per-point errors of the frames with frame_mask[f] != 0 (F bytes; NULL =
 * the mask of the previous call) whose leading `pass` bytes equal `prefix` and whose next byte is b (pass 0 = most significant
 * byte of the IEEE bit pattern; the errors are non-negative, so bit-pattern order is numeric order).  The caller sums the
 * histograms over the ranks, picks the bin that holds the wanted rank, extends the prefix and calls again: 8 passes give the exact
 * order statistic whatever the sharding.  Synchronises. */
int mcba_error_histogram(mcba_handle* h, const unsigned char* frame_mask, unsigned long long prefix, int pass, unsigned long long* hist256);
/* The whole pre-filter (bundle_adjustment.py:265-285) in ONE call and one host synchronisation (round 5, ABI 6): upload of the
 * observations + board (both NULL: those already uploaded) and of x (12C + 6F: the parameters every frame is scored at, slot 0),
 * re-layout, the reprojection errors, and -- on the device -- which frames are complete in at least two cameras (:266), the worst
 * camera's nan-mean error per frame (:279), the threshold (outlier_threshold, or NaN: 5 x np.nanmedian of the used frames' per-point
 * errors, :281-282, exact by radix select) and the comparison (:285).  status: F bytes out, bit 0 = frame used (:266), bit 1 = excluded
 * as an outlier, bit 2 = complete in every camera.  info: 8 doubles out, 0 threshold 1 median 2 number of values under the median
 * 3 (1 = the median's candidate list overflowed and the eight-pass select of mcba_error_median ran instead) 4 frames used 5 excluded
 * 6 kept frames that are incomplete in some camera.  The per-point errors and per-(camera, frame) statistics stay on the device as
 * after mcba_frame_errors(h, 0, ...). */
int mcba_prefilter(mcba_handle* h, const double* uvs, const double* objpoints, const double* x, double outlier_threshold, unsigned char* status, double* info8);
/* mcba_prefilter + the gather of the frames it kept, when no random draw stands in between (bundle_adjustment.py:292-296 draws the subsample from the
 * caller's global numpy RNG only if n_frames <= the number of frames kept; n_frames < 0 = None).  info8[7]: 0 nothing kept, 1 the caller must draw
 * (*sub stays NULL: mcba_create_subset of its draw), 2 every frame kept, in order (solve on h itself), 3 *sub = a new handle holding the kept frames
 * in order (as mcba_create_subset makes it: observations, board and the parameters of slot 0 gathered on the device).  The caller owns *sub. */
int mcba_prefilter_subset(mcba_handle* h, const double* uvs, const double* objpoints, const double* x, double outlier_threshold, int n_frames, unsigned char* status, double* info8,
                          mcba_handle** sub);
/* New handle on the same device / stream holding the observations of n_frames frames of `src` (indices into its frames,
 * any order, repeats allowed) -- gathered device to device: what bundle_adjust solves on after the pre-filter, without
 * a second host upload (the reference slices all_calib_uvs[:, use_frames]: bundle_adjustment.py:298,312).  Parameter slot 0 of the
 * new handle = the camera blocks of src's slot 0 + the poses of the chosen frames (ABI 6).  Does not synchronise. */
int mcba_create_subset(mcba_handle** out, mcba_handle* src, const int* frames, int n_frames);

/* ---- calibrate() on the device (ABI 7, round 6) ------------------------------------------------------------------------
 * The initialiser that produces bundle_adjust()'s inputs: reference multicam_calibration/calibration.py:280-373.  Its two OpenCV calls per
 * view (cv2.calibrateCamera :68 on <= 100 sampled views per camera, cv2.solvePnP :108 on every complete view) and its pose graph
 * (:116-277) run on the detections a handle already holds (mcba_upload_observations).  A call of calibrate() is
 *   mcba_calib_complete -> [host: np.random.choice per camera, as the reference draws it :57-60] -> mcba_calib_start (the sampled views'
 *   homographies, Zhang's closed form for every camera's K from them, the views' poses with that K and no distortion: one crossing; its
 *   first and last step alone are mcba_calib_homographies and mcba_calib_view_poses)
 *   -> mcba_create_views + mcba_lm_run + mcba_lm_result (EVERY camera's fx fy cx cy k1 k2 and its views' poses in one device-resident LM run)
 *   -> mcba_calib_poses (every (camera, frame): one launch, the poses stay on the device) -> [host: maximum spanning tree of the C x C
 *   co-detection counts :146-197] -> mcba_calib_graph (the tree's pairwise medians, the chain of C - 1 transforms :230-235 and the consensus in
 *   one crossing; its pieces alone: mcba_calib_pairwise, mcba_calib_consensus).
 * Views are (camera, frame) int pairs.  intr9 = C x (fx fy cx cy k1 k2 p1 p2 k3) (OpenCV's five-coefficient model; the reference's defaults
 * leave p1 = p2 = k3 = 0).  Poses are board -> camera 6-vectors (rotation vector, translation), NaN rows where there is none.  The board must
 * be planar (z = 0), as the reference's chessboards are.  cv2 is absent from the build image: parity with OpenCV's numbers is unpinned; the
 * kernels are checked against numpy restatements (oracle/calibration_oracle.py) and against exact recovery of synthetic truth. */
/* complete_cf (C, F) bytes: 1 = all 2 N scalars of the detection are present (what :55 samples from and :107 solves). */
int mcba_calib_complete(mcba_handle* h, unsigned char* complete_cf);
/* Board-plane -> pixel homographies, H[2][2] = 1, of the listed views (Hartley-normalised DLT, the smallest singular vector of the 2N x 9
 * system): H_out n_views x 9 row-major (NaN for an incomplete view), ok_out n_views bytes or NULL. */
int mcba_calib_homographies(mcba_handle* h, const int* views, int n_views, double* H_out, unsigned char* ok_out);
/* cv2.solvePnP's job for the listed views: undistort (undistort_iterations rounds of OpenCV's fixed point), homography start, pose from it,
 * Levenberg-Marquardt on the pixel reprojection error (at most max_evaluations linearisations per view, every view its own damping).
 * poses_out n_views x 6, ok_out n_views bytes or NULL. */
int mcba_calib_view_poses(mcba_handle* h, const int* views, int n_views, const double* intr9, int undistort_iterations, int max_evaluations, double* poses_out, unsigned char* ok_out);
/* The closed-form start of cv2.calibrateCamera (:68) for EVERY camera in one crossing: homographies of the listed views; Zhang's camera matrix
 * per camera from its views (image of the absolute conic with the skew held at zero: the null vector of a 6-column system, found as the
 * smallest eigenvector of its 6 x 6 normal matrix by cyclic Jacobi; image_sizes = C x (width, height) in pixels sets the normalisation and
 * the fallback f = max(w, h), c = ((w - 1) / 2, (h - 1) / 2) for a camera with fewer than two usable views or a non-positive-definite
 * estimate); then mcba_calib_view_poses' work with that K and zero distortion.  k4_out C x (fx fy cx cy); closed_out C bytes or NULL (1 = the
 * closed form was used); poses_out n_views x 6 (NaN rows = none); ok_out n_views bytes or NULL. */
int mcba_calib_start(mcba_handle* h, const int* views, int n_views, const double* image_sizes, int undistort_iterations, int max_evaluations, double* k4_out, unsigned char* closed_out,
                     double* poses_out, unsigned char* ok_out);
/* estimate_pose (:74-113) of EVERY camera at once.  The poses stay on the device for the two calls below; poses_out (C,F,6), ok_out (C,F)
 * bytes, evals_out (C,F) bytes (linearisations a view took) are optional -- with all three NULL the call does not synchronise. */
int mcba_calib_poses(mcba_handle* h, const double* intr9, int undistort_iterations, int max_evaluations, double* poses_out, unsigned char* ok_out, unsigned char* evals_out);
/* estimate_pairwise_camera_transform (:116-143) for camera pairs edges = n_edges x (c1, c2): transforms_out (n_edges, 6) = component-wise
 * median over the frames both cameras have a pose for of T2 T1^-1 (exact order statistics: radix select on the device; NaN if the pair shares
 * no frame); counts_out (n_edges) = frames shared, or NULL. */
int mcba_calib_pairwise(mcba_handle* h, const int* edges, int n_edges, double* transforms_out, double* counts_out);
/* consensus_calib_poses (:239-277): extrinsics (C,6) world -> camera; poses_out (F,6) = per-coordinate nan-median over the cameras of
 * T_ext^-1 T_pose; NaN rows for frames no camera has a pose for. */
int mcba_calib_consensus(mcba_handle* h, const double* extrinsics, double* poses_out);
/* The pose graph of calibrate() (:200-277) in ONE crossing: mcba_calib_pairwise's medians for the spanning tree's edges, chained from `root` into
 * the world -> camera extrinsics ON THE DEVICE (:226-235), and mcba_calib_consensus with them.  edges = n_edges x (c1, c2) ordered so that c1 is
 * `root` or the c2 of an earlier edge and every camera is reached exactly once (the reference's tree sorted by distance from the root; n_edges =
 * C - 1, none for one camera).  extrinsics_out (C, 6), the root's row exactly 0; poses_out (F, 6); transforms_out (n_edges, 6) and counts_out
 * (n_edges) or NULL. */
int mcba_calib_graph(mcba_handle* h, const int* edges, int n_edges, int root, double* extrinsics_out, double* poses_out, double* transforms_out, double* counts_out);
/* A new handle of C cameras x n_views frames: frame j holds view j's detection in ITS camera alone (NaN in the others) -- the sampled views of
 * every camera side by side, so that one LM run (12 C camera parameters of which the extrinsics are held fixed at 0, 6 per view) is
 * get_intrinsics of every camera.  Gathered device to device; does not synchronise. */
int mcba_create_views(mcba_handle** out, mcba_handle* src, const int* views, int n_views);
/* The two pose-graph steps for a caller's own pose array (C,F,6) (NaN rows = none): the reference's public functions of the same names take
 * exactly that.  Stateless: host arrays in, host arrays out. */
int mcba_pose_pairwise(int n_cameras, int n_frames, const double* poses, const int* edges, int n_edges, int device, double* transforms_out, double* counts_out);
int mcba_pose_consensus(int n_cameras, int n_frames, const double* poses, const double* extrinsics, int device, double* poses_out);

/* ---- geometry helpers and diagnostics around the solver ---------------------------------------- */
/* undistort_points (geometry.py:328-358 = cv2.undistortPoints(uvs, K, dist, None, K)): n_points (u,v) pairs, K4 = (fx fy cx cy),
 * dist5 = (k1 k2 p1 p2 k3) or NULL; fixed-point iteration, `iterations` rounds (OpenCV's default: 5).  NaN rows stay NaN. */
int mcba_undistort_points(size_t n_points, const double* uvs, const double* K4, const double* dist5, int iterations, int device, double* out);
/* Single-camera calibration with OpenCV's FIVE-coefficient distortion model (k1 k2 p1 p2 k3) -- what the reference's get_intrinsics() asks of
 * cv2.calibrateCamera when fix_k3 / zero_tangent_dist are False (calibration.py:11-71) and of cv2.solvePnP when such coefficients come back
 * (:74-113).  Stateless: uvs (V,N,2) detections of V views (NaN = missing), objpoints (N,3), intr9 = fx fy cx cy k1 k2 p1 p2 k3, poses (V,6)
 * board -> camera (rotation vector, translation).  out (V,136) per view: the upper triangle (row by row, 120) of the Gauss-Newton block J^T J over
 * the parameters [intr9 | pose6], the gradient J^T r (15), the cost 0.5 sum r^2, with r = observed - predicted.  Rows are differentiated by
 * forward-mode automatic differentiation on the GPU (csrc/mcba_calib.hip); the LM iteration around it is calibration.py's. */
int mcba_calib_normal_equations(int n_views, int n_points, const double* uvs, const double* objpoints, const double* intr9, const double* poses, int device, double* out);
/* Numeric core of plot_residuals (viz.py:166-186) at x[slot]: per (camera, frame) with a complete detection the
 * least-squares homography from the undistorted detections to the board plane, the distortion-free reprojection of the
 * board mapped through it, and per camera the median distance to the board points (board units).
 * dist5: (C,5) distortion used for undistorting (NULL: (k1, k2, 0, 0, 0) of x[slot]).  Host outputs: median_error (C);
 * reprojections (C,F,N,2) and transformed (C,F,N,2, NaN where the detection is incomplete) -- either may be NULL. */
int mcba_reprojection_diagnostics(mcba_handle* h, int slot, const double* dist5, int undistort_iterations, double* median_error, double* reprojections, double* transformed);

/* ---- measurement ----------------------------------------------------------------------------- */
/* When enabled kernel launches are bracketed by hipEvents on the handle's stream.  `on` = 0: off; 1: every
 * kernel; otherwise a bit mask over the kernels in mcba_profile_names() order, shifted left by one
 * (bit k+1 selects kernel k) -- e.g. time only the dominant kernel inside a measured region. */
int mcba_profile_enable(mcba_handle* h, int on);
/* Bracket only every `stride`-th launch of each selected kernel (event records put barrier packets on the stream:
 * sampling keeps a measured region undisturbed).  Reset to 1 by mcba_profile_enable. */
int mcba_profile_stride(mcba_handle* h, int stride);
/* on != 0: the fused k_gram kernel is timed by events attached to its dispatch (the kernel's own begin / end timestamps -- the
 * figure rocprofv3 reports) instead of event records around the launch; other kernels and k_gram's other launch variants are
 * bracketed as before.  Reset by mcba_profile_enable. */
int mcba_profile_exact(mcba_handle* h, int on);
/* Microseconds an event bracket reads with nothing between its two records, mean of `pairs` (<= 4096) brackets on the handle's stream:
 * the bracket's own share of an event-timed kernel (bench.py subtracts it: `roofline.avg_launch_us`).  Synchronises. */
int mcba_profile_bracket_overhead(mcba_handle* h, int pairs, double* us);
/* Drains the recorded events.  names: '\n'-separated kernel names in the order of ms[] / calls[]. */
int mcba_profile_read(mcba_handle* h, double* ms_total, int* calls, int capacity, int* n_kernels);
const char* mcba_profile_names(void);
/* Measurement aid (round 4): TFLOP/s of independent v_fma_f64 (2 flop each) that `device` sustains with one wavefront per SIMD on every
 * compute unit -- the occupancy and the operand pattern of k_gram's accumulate block.  bench.py reports k_gram's FP64 instruction stream
 * against it next to the datasheet peak (the reference has no counterpart: its arithmetic is numpy / scipy on the host). */
int mcba_fp64_issue_rate(int device, double* tflops);
int mcba_synchronize(mcba_handle* h);

/* ---- floor-plane alignment (reference flatibration.py; additive to ABI 7) -------------------------------
 * Stateless, like mcba_triangulate: host arrays in and out, one upload per call.  kernel_ms (may be NULL) receives the time of
 * the call's kernels measured with HIP events. */
#define MCBA_FLAT_MAX_HYPOTHESES 128   /* RANSAC hypotheses per mcba_flat_ransac call (sklearn's default max_trials is 100) */
#define MCBA_FLAT_MAX_KEYPOINTS 2048   /* keypoints per frame of mcba_flat_floor_points (a frame is staged whole in LDS) */
/* keypoints (F, K, 3) -> points_out (F, 3) = per frame the keypoint of smallest z (largest if z_points_down), index_out (F) ints or NULL:
 * np.argmin / np.argmax semantics (first index on ties, the first NaN wins, an all-NaN frame gives 0). */
int mcba_flat_floor_points(size_t n_frames, int n_keypoints, const double* keypoints, int z_points_down, int device, double* points_out, int* index_out, double* kernel_ms);
/* points (n, 3); planes (H, 3) = (a, b, c) of z = a x + b y + c; inlier = |z - (x a + y b + c)| <= threshold.  counts_out (H) = exact inlier
 * counts; moments_out (H, 9) = over the inliers, with dx = x - shift2[0], dy = y - shift2[1], r = the residual: sums of dx dy r dx^2 dx.dy dy^2
 * dx.r dy.r r^2, reduced in a fixed order (bitwise reproducible for a given n).  mask_out (n bytes, needs H == 1) or NULL. */
int mcba_flat_ransac(size_t n_points, const double* points, int n_hypotheses, const double* planes, double threshold, const double* shift2, int device,
                     unsigned long long* counts_out, double* moments_out, unsigned char* mask_out, double* kernel_ms);
/* points (n, 3) mapped by rt12 (R row-major 3x3, then t): x' = R p + t.  values_out (2, n_ranks) = the exact order statistics (0-based ranks,
 * at most 8) of x' and y' (radix select on the device, no sort); sums_out (2) = sums of x' and y'; nans_out (2) = NaN counts of x' and y'
 * (the order statistics of a coordinate that holds a NaN are meaningless). */
int mcba_flat_order_stats(size_t n_points, const double* points, const double* rt12, int n_ranks, const long long* ranks, int device, double* values_out, double* sums_out,
                          unsigned long long* nans_out, double* kernel_ms);

/* ---- chessboard detection (reference detection.py: detect_chessboard, reorder_chessboard_corners; additive to ABI 7) ----------------
 * Stateless: host arrays in and out.  Images are 8-bit, (H, W) grey or (H, W, 3) BGR, row-major; BGR is converted with OpenCV's
 * fixed-point formula.  Coordinates follow the pixel-centre convention (pixel (i, j) covers [j - 1/2, j + 1/2] x [i - 1/2, i + 1/2]).
 * A board of board_cols x board_rows inner corners (the reference's board_shape = (cols, rows)) is returned row-major: corner k is board
 * point x = k % board_cols, y = k / board_cols.  kernel_ms (may be NULL) receives the time of the call's kernels (HIP events). */
#define MCBA_DETECT_MAX_CANDIDATES 1024   /* saddle candidates per frame (more: status 3, the frame is not searched) */
#define MCBA_DETECT_MAX_CORNERS 512       /* board_cols * board_rows */
#define MCBA_DETECT_MAX_BOARD_SIDE 30     /* board_cols, board_rows */
#define MCBA_DETECT_MAX_WINDOW 15         /* cornerSubPix half-window (subpix_winSize) */
#define MCBA_DETECT_MAX_IMAGE_SIDE 4096   /* image width and height */
/* The whole pipeline for n_images frames of one size (grey -> saddle candidates -> lattice -> cornerSubPix -> anchor), in chunks whose
 * device memory stays within memory_budget bytes (0: 256 MiB).  scale_factor in (0, 1]: the search runs on the bilinear downscale, the
 * refinement on the full image.  Outputs per frame: status_out 0 no board, 1 accepted, 2 rejected (anchor ambiguous: best - second score
 * < match_score_min_diff), 3 more than MCBA_DETECT_MAX_CANDIDATES candidates; uvs_out (N, 2) float32, NaN unless status 1; scores_out (4)
 * sorted descending, NaN where no grid was assembled or reorder == 0.  reorder == 0: no anchor, status 1 for every assembled grid. */
int mcba_detect_chessboards(int n_images, int height, int width, int channels, const unsigned char* images, int board_cols, int board_rows, int win_w, int win_h,
                            double scale_factor, int reorder, double match_score_min_diff, size_t memory_budget, int device, float* uvs_out, double* scores_out,
                            signed char* status_out, double* kernel_ms);
/* cornerSubPix (half-window win_w x win_h, 30 iterations, eps 0.001, no zero zone) of n_corners float32 start points (n, 2) in one image */
int mcba_detect_subpix(int height, int width, int channels, const unsigned char* image, int n_corners, const float* start, int win_w, int win_h, int device, float* out,
                       double* kernel_ms);
/* the anchor test of reorder_chessboard_corners for uvs (N, 2) float32 in the reference's grid layout (board_rows x board_cols):
 * scores_out (4) unsorted correlations of the four regions, regions_out (4, 40, 40) uint8 or NULL, quads_out (4, 4, 2) float32 or NULL */
int mcba_detect_anchor(int height, int width, int channels, const unsigned char* image, int board_cols, int board_rows, const float* uvs, int device, double* scores_out,
                       unsigned char* regions_out, float* quads_out, double* kernel_ms);

/* ---- calibration uncertainty (no reference counterpart; additive to ABI 7) -----------------------------------------------------------
 * The Gauss-Newton (IRLS-weighted) covariance at x[slot], with the handle's loss, f_scale and camera block (mcba_set_camera_block):
 *   H = J^T diag(rho') J in blocks U_c, V_f, W_cf;  S = blockdiag(U) - sum_f W_f V_f^-1 W_f^T;  S_g = S with the six extrinsics of
 *   gauge_camera held (their rows and columns leave the system and are reported as exact zeros);
 *   cam_cov (n x n, n = 12 C, or 6 C with the 6-wide block; row i = the i-th variable of the camera system) = sigma2 S_g^-1;
 *   frame_cov (F x 6 x 6) = sigma2 V_f^-1 + Y_f cam_cov Y_f^T, Y_f = V_f^-1 W_f^T.  A frame without data gets a NaN block and leaves the
 *   count p; frames that hold data but whose V_f is not positive definite are refused (MCBA_ERR_ARG: leave them out).
 *   sigma2 = sigma2_in, or -- NaN -- sum rho' f^2 / (m - p) with m present scalars and p free parameters (NaN if m <= p).
 * The call linearises x[slot] with curvature floor 1 into the handle's own buffers and reduces with lambda = 0: a linearisation or reduced
 * system the caller had is gone afterwards (call mcba_linearize again); the handle's curvature floor, loss and parameters are untouched.
 * Either output may be NULL.  info8 = {sigma2, m, p, frames without data, failing pivot (-1 = none), kernel_ms of the covariance kernels,
 * frames per workgroup of k_cov_frames (8 or 4; 0 when frame_cov is NULL), ld (the row stride of the camera block on the device, n rounded up
 * to 64)}.  MCBA_ERR_NONFINITE with info8[4] >= 0: S_g is not positive definite at that pivot (the message names camera and parameter).
 * MCBA_ERR_ARG: a sparse-Schur handle, a tabulated loss, a numeric x_scale or frozen coordinates, gauge_camera out of range. */
int mcba_covariance(mcba_handle* h, int slot, int gauge_camera, double sigma2_in, double* cam_cov, double* frame_cov, double* info8);

/* ---- triangulation uncertainty (no reference counterpart; additive to ABI 7) ---------------------------------------------------------
 * The covariance of every triangulated point, in the Gauss-Newton (IRLS-weighted) convention of mcba_covariance.  Stateless like
 * mcba_triangulate_refine: points (P, 3) where to linearise (meaningful at a minimiser of that call's cost), uvs (C, P, 2) raw detections
 * (NaN = unseen), cam12 (C, 12), dist5 (C, 5) or NULL, 2 <= C <= 64, loss 0 .. 4, f_scale > 0.  Per point, over the cameras that see it:
 *   f = detection - five-coefficient projection, w = rho'((f / f_scale)^2) per scalar, A_c = d(u, v)/dX, B_c = d(u, v)/d(camera c's 12 of cam12);
 *   H = sum_c A_c^T W_c A_c, inverted through the Cholesky factor of its Jacobi-scaled form;
 *   det6 (P, 6) = sigma2 H^-1, packed 00 01 02 11 12 22;
 *   cal6 (P, 6) = G cam_cov G^T packed likewise, G = [G_0 .. G_{C-1}], G_c = H^-1 A_c^T W_c B_c (zero for a camera that does not see the
 *   point): how the re-triangulated point moves with the cameras.  cam_cov (12 C, 12 C) row-major, symmetric (mcba_covariance's, or any
 *   other), or NULL: the detection term alone; cal6 is required exactly when cam_cov is given.
 *   sigma2 = sigma2_in, or -- NaN -- sum w f^2 / (m - 3 P_u) over the P_u points of status 1 with their m present scalars, summed in a
 *   fixed order (NaN if m <= 3 P_u).
 * views_out (P): cameras that see the point.  status_out (P): 1 ok; -1 fewer than two views or a NaN in the point; -2 degenerate: a pivot of
 * the scaled factor whose square is below 1e-12 (two cameras with one centre, a point on the baseline).  Both terms are NaN unless the
 * status is 1, and such a point leaves the pooled sums.
 * info8 = {sigma2, m, 3 P_u, points of status -1, points of status -2, kernel_ms, points per workgroup of k_tricov_cal (16, 10 or 5; 0 without
 * cam_cov), ld (the row stride of the uploaded cam_cov, 12 C rounded up to 64)}; kernel_ms may be NULL.  n_points == 0 returns at once with
 * info8 = {sigma2_in, 0 ..}.
 * The environment variable MCBA_TRICOV_G (5, 10 or 16), read per call, forces the number of points a workgroup of the calibration term takes. */
int mcba_triangulation_covariance(int n_cameras, size_t n_points, const double* points, const double* uvs, const double* cam12, const double* dist5, const double* cam_cov, int loss, double f_scale,
                                  double sigma2_in, int device, double* det6, double* cal6, int* views_out, int* status_out, double* info8, double* kernel_ms);

/* ---- extrinsics refinement from keypoints: free-point bundle adjustment (no reference counterpart; additive to ABI 7) -----------------
 * Minimises 0.5 f_scale^2 sum rho((f / f_scale)^2), f = raw detection - five-coefficient projection, jointly over the rotation vector and
 * translation of every camera and every 3-D point; the intrinsics stay fixed.  Stateless: uvs (C, P, 2) raw detections (NaN = unseen), cam12
 * (C, 12) with the start extrinsics in columns 6 .. 11, dist5 (C, 5) or NULL, points (P, 3) the start, 2 <= C <= 24, P >= 1, loss 0 .. 4,
 * f_scale > 0, max_nfev >= 2.
 * held (C), in and out: bit i set = scalar i (0 .. 2 rotation vector, 3 .. 5 translation) of the camera is not free.  The call holds all six
 * of gauge_camera and of every camera that no used point sees and reports that here; the caller fixes the scale by holding one scalar of
 * scale_camera (a different camera).
 * Levenberg-Marquardt, Marquardt damping on cameras and points alike (from 1e-4, a tenth on an accepted trial, tenfold on a rejected one); a
 * trial is accepted when the robust cost does not rise.  Per evaluation the Schur reduction over the 3 x 3 point blocks and the
 * back-substitution run on the device, the reduced system (at most 143 rows) is solved on the host.  Afterwards camera centres and points are
 * rescaled about the gauge camera's centre so that its distance to scale_camera's is what it was at the start; no projection changes.
 * extrinsics_out (C, 6); points_out (P, 3), NaN rows unless point_status (P) is 1 (-1: fewer than two views or a NaN start; -2: a zero
 * diagonal in the point's 3 x 3 block).
 * result16 = {cost, cost at the start, optimality (inf-norm of the gradient over the free parameters), nfev, njev, status (scipy's: 0 max_nfev,
 * 1 gtol, 2 ftol, 3 xtol), scale of the closing step, evaluations recorded, kernel_ms, ms in k_kpba_reduce passes, their number, ms in
 * k_kpba_step passes, their number, points per group, 0, 0}.
 * history (history_rows, 3) or NULL with history_rows 0: per evaluation the cost, the damping and 1 if it was accepted; evaluations beyond
 * history_rows are counted in result16[7] and not stored.
 * No atomics: two calls on the same input return the same bits.  The environment variable MCBA_KPBA_G (16, 32 or 64), read per call, forces
 * the number of points in a group of k_kpba_reduce. */
int mcba_refine_extrinsics(int n_cameras, size_t n_points, const double* uvs, const double* cam12, const double* dist5, const double* points, int* held, int gauge_camera, int scale_camera, int loss,
                           double f_scale, double ftol, double xtol, double gtol, int max_nfev, int device, double* extrinsics_out, double* points_out, int* point_status, double* result16,
                           double* history, int history_rows);

/* One evaluation of mcba_refine_extrinsics laid open (additive to ABI 7): the very set-up, k_kpba_status, k_kpba_reduce + k_kpba_finish and -- with
 * ext_trial (C, 6) and dtheta (C, 6), both or neither -- k_kpba_step of the loop, once, at the extrinsics in cam12, the given points and the
 * damping lam (0 <= lam < 1e12), and what the kernels wrote as they wrote it.  For tests and diagnostics, as mcba_calib_normal_equations and
 * mcba_get_reduced are for the other solvers.  uvs, cam12, dist5, points, loss, f_scale and their refusals as above.
 * held (C) is taken as given: no gauge camera, no scale scalar and no rule for a camera without detections is applied.
 * point_status (P) as above.  system (NP NP + 33 C + 4 doubles, NP = 6 C rounded up to a multiple of 16): Y Y^T = sum_p Y_p Y_p^T (NP, NP)
 * row-major, rows and columns of held scalars and of the padding zero | per camera U_c packed lower (21: (i, j <= i) at i (i + 1) / 2 + j), g_c
 * (6), sum_p Y_cp z_p (6) | robust cost, present scalars of the used points, max |g_p|, 0.  The loop solves
 * (U + lam diag U - Y Y^T) dtheta = sum Y z - g_c over the free scalars.
 * With a step: trial_points (P, 3) = points + dX, dX_p = -(H_p + lam diag H_p)^-1 (g_p + sum_c W_cp^T dtheta_c) (a point that is not used
 * keeps its value, NaN included), and step4 = {robust cost at (ext_trial, trial_points), sum dX^2, 0, sum X^2 over the used points}.
 * info4 = {points per group, workgroups of a pass (= partial systems summed), NP, kernel_ms}.  MCBA_KPBA_G as above. */
int mcba_refine_extrinsics_system(int n_cameras, size_t n_points, const double* uvs, const double* cam12, const double* dist5, const double* points, const int* held, int loss, double f_scale,
                                  double lam, int device, const double* ext_trial, const double* dtheta, int* point_status, double* system, double* trial_points, double* step4, double* info4);

/* ---- per-detection confidence weights (no reference counterpart; additive to ABI 7) ------------------------------------
 * The four calls above with one more operand behind uvs: weights (C, P), w >= 0, the relative inverse variance of each detection (a pose
 * estimator's confidence), or NULL -- then the call is the one above, launch for launch (the unweighted entry points call these with NULL).
 * A detection of weight w enters every cost exactly as if it and fx, fy, cx, cy of its camera had been multiplied by sqrt(w): its residual
 * pair is scaled by sqrt(w) before the loss, and so is every derivative of its projection; distortion coefficients and extrinsics are
 * untouched.  w = 0 or NaN: the detection is unseen, exactly like a NaN detection; views, present scalars, "fewer than two views" and
 * point_status count the detections of positive weight.  A negative or infinite weight: MCBA_ERR_ARG.  The plane goes to the device once
 * per call, beside the detections (as sqrt(w)); the kernels are the weighted instantiations of the same templates, with the same launch
 * shapes and summation orders: two calls on the same input return the same bits.
 *   mcba_triangulate_refine_weighted         with points_in NULL the median of pairs is unweighted and skips the detections of weight 0 / NaN
 *   mcba_triangulation_covariance_weighted   H, G and the pooled sigma2 = sum rho' w f^2 / (m - 3 P_u) on the weighted problem; sigma2_in is the
 *                                            variance of a detection of weight 1
 *   mcba_refine_extrinsics_weighted          the blind-camera rule counts the detections of positive weight
 *   mcba_refine_extrinsics_system_weighted */
int mcba_triangulate_refine_weighted(int n_cameras, size_t n_points, const double* uvs, const double* weights, const double* cam12, const double* dist5, const double* points_in,
                                     int undistort_iterations, int loss, double f_scale, int max_iterations, int device, double* points_out, double* info_out, double* kernel_ms);
int mcba_triangulation_covariance_weighted(int n_cameras, size_t n_points, const double* points, const double* uvs, const double* weights, const double* cam12, const double* dist5,
                                           const double* cam_cov, int loss, double f_scale, double sigma2_in, int device, double* det6, double* cal6, int* views_out, int* status_out, double* info8,
                                           double* kernel_ms);
int mcba_refine_extrinsics_weighted(int n_cameras, size_t n_points, const double* uvs, const double* weights, const double* cam12, const double* dist5, const double* points, int* held,
                                    int gauge_camera, int scale_camera, int loss, double f_scale, double ftol, double xtol, double gtol, int max_nfev, int device, double* extrinsics_out,
                                    double* points_out, int* point_status, double* result16, double* history, int history_rows);
int mcba_refine_extrinsics_system_weighted(int n_cameras, size_t n_points, const double* uvs, const double* weights, const double* cam12, const double* dist5, const double* points, const int* held,
                                           int loss, double f_scale, double lam, int device, const double* ext_trial, const double* dtheta, int* point_status, double* system, double* trial_points,
                                           double* step4, double* info4);

/* ---- the tiled Schur reduction: extrinsics refinement for rigs of up to 64 cameras (additive to ABI 7) -------------------
 * The two weighted calls above with one more operand, reduction, behind weights (which may be NULL): MCBA_KPBA_RESIDENT (0) is the call above,
 * launch for launch (the entry points above call these with 0), with its 2 <= C <= 24.  MCBA_KPBA_TILED (1) takes 2 <= C <= 64 and delivers the
 * same system in the same layout by k_kpba_factors + k_kpba_reduce_tiled + k_kpba_finish (csrc/mcba_kpba_tiled.hip): the cameras in bands of 16,
 * the lower triangle of Y Y^T in band pairs, each a workgroup's own, groups of 16 points; the sums are in another order than the resident
 * reduction's, so the two agree within the rounding bound of either, not bit for bit.  The loop, the gauge rules, the closing step, the host's
 * solve (at most 377 free rows) and every refusal are the same.  Any other value of reduction: MCBA_ERR_ARG.  MCBA_KPBA_G is not read by the
 * tiled reduction.
 *   mcba_refine_extrinsics_reduction          result16[13 .. 15] = {points per group, cameras per band (0: resident), band pairs (0: resident)}
 *   mcba_refine_extrinsics_system_reduction   info8 = {points per group, partial systems summed, NP, kernel_ms, cameras per band (0: resident),
 *                                             band pairs (0: resident), reduction, 0} */
#define MCBA_KPBA_RESIDENT 0
#define MCBA_KPBA_TILED 1
int mcba_refine_extrinsics_reduction(int n_cameras, size_t n_points, const double* uvs, const double* weights, int reduction, const double* cam12, const double* dist5, const double* points, int* held,
                                     int gauge_camera, int scale_camera, int loss, double f_scale, double ftol, double xtol, double gtol, int max_nfev, int device, double* extrinsics_out,
                                     double* points_out, int* point_status, double* result16, double* history, int history_rows);
int mcba_refine_extrinsics_system_reduction(int n_cameras, size_t n_points, const double* uvs, const double* weights, int reduction, const double* cam12, const double* dist5, const double* points,
                                            const int* held, int loss, double f_scale, double lam, int device, const double* ext_trial, const double* dtheta, int* point_status, double* system,
                                            double* trial_points, double* step4, double* info8);

/* ---- camera refinement from keypoints, intrinsics free (no reference counterpart; additive to ABI 7) ---------------------
 * mcba_refine_extrinsics_weighted with 12 unknowns per camera, theta_c = (fx fy cx cy k1 k2 | rotation vector | translation), the layout of
 * cam12; p1, p2, k3 (dist5) stay constants.  2 <= C <= 12 (the reduced system is held to 144 rows); weights may be NULL.
 * held (C) in/out: 12 bits per camera in theta_c order, bit set = not free; bits 6 .. 11 mean what the bits 0 .. 5 of mcba_refine_extrinsics
 * mean.  The call sets the bits 6 .. 11 of gauge_camera and all 12 of a camera that no used point sees.
 * prior_weight (C, 6) or NULL: 1 / std^2 of a Gaussian prior on each intrinsic scalar about its input value, 0 = none.  The prior is the
 * host's alone: 0.5 sum prior_weight (theta - theta_0)^2 over the free intrinsic scalars is added to the cost (never through the loss),
 * prior_weight to the diagonal of the camera block before the damping, prior_weight (theta - theta_0) to the gradient.
 * Out: cameras_out (C, 12); points_out, point_status, history as mcba_refine_extrinsics; result16 = {cost (prior included), cost0,
 * optimality, nfev, njev, status, scale, evaluations, kernel_ms, reduce_ms, reductions, step_ms, steps, points per group, prior cost, 0}.
 * Kernels (csrc/mcba_kpcam.hip): k_kpba_status, k_kpcam_reduce, k_kpba_finish, k_kpcam_step; no atomics, two calls return the same bits.
 * MCBA_KPCAM_G (16, 32, 64; tests) forces the points per group where it fits.
 *   mcba_refine_cameras_system   one evaluation laid open, as mcba_refine_extrinsics_system: held as given, no prior; cameras_trial and
 *                                dtheta (C, 12 each) both or neither; system = Y Y^T (NP, NP; NP = 12 C rounded up to 16) | per camera U_c
 *                                packed lower (78), g_c (12), sum Y z (12) | cost, present scalars, max |g_p|, 0;
 *                                info4 = {points per group, partial systems summed, NP, kernel_ms} */
int mcba_refine_cameras(int n_cameras, size_t n_points, const double* uvs, const double* weights, const double* cam12, const double* dist5, const double* points, int* held, const double* prior_weight,
                        int gauge_camera, int scale_camera, int loss, double f_scale, double ftol, double xtol, double gtol, int max_nfev, int device, double* cameras_out, double* points_out,
                        int* point_status, double* result16, double* history, int history_rows);
int mcba_refine_cameras_system(int n_cameras, size_t n_points, const double* uvs, const double* weights, const double* cam12, const double* dist5, const double* points, const int* held, int loss,
                               double f_scale, double lam, int device, const double* cameras_trial, const double* dtheta, int* point_status, double* system, double* trial_points, double* step4,
                               double* info4);

/* ---- two-view RANSAC: relative pose from keypoints alone (no reference counterpart; additive to ABI 7) --------------------
 * Stateless.  uv_a, uv_b (M, 2): the detections of the M >= 8 points both cameras see, compacted by the caller (no NaN); cam12, dist5: two rows
 * each, camera a then camera b (of cam12 only fx fy cx cy are read); samples (H, 8) ints: the 8 correspondences of each hypothesis, drawn
 * by the caller.  Per hypothesis the 8-point essential matrix (Hartley-normalised, projected onto singular values 1, 1, 0, |E|_F = sqrt 2, the
 * entry of largest magnitude positive; x_b^T E x_a = 0 on normalised coordinates, row-major), status 1, or -1 (void: not finite, cost +inf);
 * every hypothesis is scored over all M points with the truncated squared Sampson distance of the undistorted pixels (undistort_iterations
 * rounds), sum min(e^2, threshold^2), inlier <=> e^2 <= threshold^2; the lowest (cost, index) wins.  Its four (R, t) are voted on by the
 * inliers in front of both cameras; the highest (count, -index) wins.  essential_in (H, 9) or NULL: the generator is skipped and these
 * matrices are scored (tests and diagnostics; samples may then be NULL).
 * Out: rt12 = R row-major, then t (|t| = 1), x_b = R x_a + t; best4 = {winning hypothesis, its cost, its inliers, inliers in front};
 * inliers (M bytes, 0 / 1); points (M, 3): the two-view point of every inlier in camera a's frame at unit baseline, NaN for the others;
 * optional tables essential_out (H, 9), cost_out (H), count_out (H), status_out (H); kernel_ms (6 doubles or NULL): the call's kernels, then
 * the stages prepare, hypotheses, score, finish, pose.  No sum uses atomics: two calls on the same input return the same bits.
 * MCBA_ERR_ARG, checked before any device is touched and with nothing written: M < 8, H < 1 or H > MCBA_TWOVIEW_MAX_HYPOTHESES, a sample
 * index outside 0 .. M - 1 or repeated within a sample, threshold <= 0. */
#define MCBA_TWOVIEW_MAX_HYPOTHESES 4096
#define MCBA_TWOVIEW_CHUNK 64               /* hypotheses per workgroup of the scoring kernel (its second grid dimension counts chunks) */
#define MCBA_TWOVIEW_POINTS_PER_BLOCK 1024  /* points per workgroup of the scoring kernel */
int mcba_two_view_ransac(size_t n_points, const double* uv_a, const double* uv_b, const double* cam12, const double* dist5, int n_hypotheses, const int* samples, const double* essential_in,
                         double threshold, int undistort_iterations, int device, double* rt12, double* best4, unsigned char* inliers, double* points, double* essential_out, double* cost_out,
                         unsigned* count_out, int* status_out, double* kernel_ms);

/* ---- the five-point hypothesis generator of the two-view RANSAC (additive to ABI 7) ------------------------------------------
 * mcba_two_view_ransac with another generator: samples (H, MCBA_TWOVIEW5_SAMPLE) ints, five correspondences each, drawn by the caller.  Per
 * sample the essential matrices of the five points in normalised coordinates -- the null space of the 5 x 9 epipolar matrix, the ten cubic
 * constraints, Gauss-Jordan, the degree-10 polynomial in one coordinate (and, in a second pass, in another), its real roots, a Gauss-Newton
 * polish -- at most MCBA_TWOVIEW5_SLOTS of them, in ascending order of the root, each in mcba_two_view_ransac's convention (singular values
 * 1, 1, 0, |E|_F = sqrt 2, the entry of largest magnitude positive) in the sample's leading slots; the other slots are void (status -1, E NaN).
 * A sample is void as a whole when anything is not finite, when sigma_5 / sigma_1 of the 5 x 9 matrix is below 1e-7 or when a pivot of the
 * elimination is below 1e-9 of the block's largest entry.  The live candidates are packed in slot order (a fixed-order prefix count, no
 * atomics) and scored, won and voted on by mcba_two_view_ransac's own stages: the lowest (cost, 10 sample + slot) wins.
 * Out as mcba_two_view_ransac, with best4[0] = 10 sample + slot of the winner and the optional tables in slot order: essential_out (10 H, 9),
 * cost_out (10 H; +inf for a void slot), count_out (10 H), status_out (10 H).  Nothing live: slot 0 "wins" with cost +inf, no inliers, a NaN
 * pose.  kernel_ms (6 doubles or NULL): the call's kernels, then prepare, hypotheses (with the compaction and the read-back of the packed
 * count), score, finish, pose.  Two calls on the same input return the same bits.
 * MCBA_ERR_ARG, checked before any device is touched and with nothing written: M < 8, H < 1 or H > MCBA_TWOVIEW5_MAX_SAMPLES, a sample index
 * outside 0 .. M - 1 or repeated within a sample, threshold <= 0. */
#define MCBA_TWOVIEW5_SAMPLE 5
#define MCBA_TWOVIEW5_SLOTS 10
#define MCBA_TWOVIEW5_MAX_SAMPLES 1024
int mcba_two_view_ransac5(size_t n_points, const double* uv_a, const double* uv_b, const double* cam12, const double* dist5, int n_samples, const int* samples, double threshold,
                          int undistort_iterations, int device, double* rt12, double* best4, unsigned char* inliers, double* points, double* essential_out, double* cost_out, unsigned* count_out,
                          int* status_out, double* kernel_ms);

/* ---- camera resection (the reference resects only a planar board, through cv2.solvePnP): the pose x_cam = R X + t of each
 * of C cameras from P known world points and that camera's own detections of them.  Stateless, host arrays in and out, a device ordinal.  Cameras
 * are independent problems; the camera index is a grid dimension of the kernels.
 * In: points (P, 3), a NaN row = unknown; uvs (C, P, 2) raw detections, NaN = unseen -- a point is usable for a camera when all five numbers are
 * finite; cam12 (C, 12) and dist5 (C, 5) as everywhere (mcba_resect_ransac reads the intrinsics alone: the pose in cam12 is never looked at;
 * mcba_resect_refine starts from it).
 *
 * mcba_resect_ransac: per camera H hypotheses from samples (C, H, MCBA_RESECT_SAMPLE) of indices into 0 .. P - 1, drawn by the caller.  A
 * hypothesis is the 6-point DLT pose (Hartley-normalised 12 x 12 normal matrix, its smallest eigenvector, the left block projected onto a
 * rotation) followed by exactly MCBA_RESECT_GN_ITERATIONS Gauss-Newton iterations on the same six points in normalised coordinates; it is void
 * when anything is not finite, when the eigen-gap lambda_2 / lambda_12 of the normal matrix is below 1e-10 (the DLT start is not defined: six
 * coplanar points) or when a sample point ends behind the camera.  Where every hypothesis of a camera is void, hypothesis 0 "wins" with cost
 * +inf, no inliers and a NaN pose.  Every hypothesis is scored over every usable point by the truncated
 * squared reprojection error of the undistorted pixels, sum min(e^2, threshold^2), a point with z <= 0 counting as e^2 = +inf; the lowest
 * (cost, index) wins; inlier <=> e^2 <= threshold^2 and z > 0.  poses_in (C, H, 12; R row-major then t) or NULL: the generator is skipped and
 * these poses are scored (tests and diagnostics; samples may then be NULL).
 * A camera with fewer than MCBA_RESECT_SAMPLE usable points takes no part: nothing is launched for it, its rt12, best4[1] and tables are NaN /
 * void (best4 = {-1, NaN, 0, usable}), its samples are not read.
 * Out: rt12 (C, 12); best4 (C, 4) = {winning hypothesis, its cost, its inliers, usable points}; inliers (C, P) bytes; optional tables pose_out
 * (C, H, 12), cost_out (C, H), count_out (C, H), status_out (C, H); kernel_ms (6 doubles or NULL): the call's kernels, then the stages prepare,
 * hypotheses, score, finish, mask.  No sum uses atomics: two calls on the same input return the same bits.
 * MCBA_ERR_ARG, checked before any device is touched and with nothing written: C < 1 or C > MCBA_RESECT_MAX_CAMERAS, P < 1, H < 1 or
 * H > MCBA_RESECT_MAX_HYPOTHESES, a sample index outside 0 .. P - 1, not usable or repeated within a sample, threshold <= 0.
 *
 * mcba_resect_refine: the pose-only polish.  Per camera with active[c] != 0 (NULL: every camera) Levenberg-Marquardt on the six pose scalars
 * over the points with mask[c, p] != 0 (and usable), the points fixed: f = detection - projection of the five-coefficient model on the raw
 * detections, robust loss and f_scale as mcba_refine_extrinsics, Marquardt damping with its tenfold rule, a 6 x 6 solve on the host, one
 * small device-to-host copy per evaluation.  Every camera has its own damping and stops on its own (scipy's status values: 1 gtol, 2 ftol,
 * 3 xtol, 0 max_nfev); a stopped camera is not evaluated again.
 * Out: extrinsics_out (C, 6) rotation vector, translation (an inactive camera: its start); result (C, 8) = {cost at the start, cost,
 * optimality, nfev, njev, status, detections used, damping}, NaN rows for inactive cameras; system_out (C, MCBA_RESECT_SYSTEM) or NULL: the
 * last linearisation -- upper triangle of J^T W J (21, row-major) | gradient (6) | robust cost | detections used; kernel_ms (2 doubles or
 * NULL): the span of the call's kernels and host solves, the number of evaluations.
 * MCBA_ERR_ARG: C outside 1 .. MCBA_RESECT_MAX_CAMERAS, P < 1, an unknown loss, f_scale <= 0, max_nfev < 1. */
#define MCBA_RESECT_MAX_HYPOTHESES 4096
#define MCBA_RESECT_MAX_CAMERAS 64
#define MCBA_RESECT_SAMPLE 6
#define MCBA_RESECT_GN_ITERATIONS 10
#define MCBA_RESECT_CHUNK 64               /* hypotheses per workgroup of the scoring kernel (its second grid dimension counts chunks) */
#define MCBA_RESECT_POINTS_PER_BLOCK 1024  /* points per workgroup of the scoring kernel */
#define MCBA_RESECT_SYSTEM 29
int mcba_resect_ransac(int n_cameras, size_t n_points, const double* points, const double* uvs, const double* cam12, const double* dist5, int n_hypotheses, const int* samples,
                       const double* poses_in, double threshold, int undistort_iterations, int device, double* rt12, double* best4, unsigned char* inliers, double* pose_out, double* cost_out,
                       unsigned* count_out, int* status_out, double* kernel_ms);
int mcba_resect_refine(int n_cameras, size_t n_points, const double* points, const double* uvs, const unsigned char* mask, const double* cam12, const double* dist5, const int* active, int loss,
                       double f_scale, double ftol, double xtol, double gtol, int max_nfev, int device, double* extrinsics_out, double* result, double* system_out, double* kernel_ms);

/* ---- the minimal generator of the resection: mcba_resect_ransac with P3P hypotheses, for point sets the 6-point DLT
 * cannot start from (coplanar and nearly coplanar points) and for detections so often wrong that six clean ones are rarely drawn together.
 * mcba_resect_ransac_p3p: the arguments of mcba_resect_ransac less poses_in.  samples (C, H, MCBA_RESECT_P3P_SAMPLE), H = n_hypotheses counts
 * SAMPLES, 1 .. MCBA_RESECT_P3P_MAX_SAMPLES.  A sample's three points and unit bearings give Grunert's quartic; each real root (ascending)
 * fills one of the sample's MCBA_RESECT_P3P_SLOTS slots with the pose of the two triangles' frames, settled by exactly MCBA_RESECT_P3P_POLISH
 * Gauss-Newton iterations on the three points.  A slot is void when there is no such root, when the world points or the bearings are collinear
 * (sine of the angle at the first point at most 1e-6), when a depth ratio is not positive, when anything is not finite or when a sample point
 * ends behind the camera.  Equal candidates are not merged.  The table of 4 H slots per camera is scored, and the winner and its mask are found,
 * exactly as mcba_resect_ransac does with 4 H hypotheses: best4[0] is the winning SLOT (its sample is best4[0] / 4), and the optional tables
 * pose_out (C, 4 H, 12), cost_out, count_out, status_out (C, 4 H) have 4 H rows per camera.  A camera takes part with at least
 * MCBA_RESECT_SAMPLE (6) usable points, as there.  kernel_ms: the same six slots.  Two calls on the same input return the same bits.
 * MCBA_ERR_ARG, checked before any device is touched and with nothing written: as mcba_resect_ransac, with H > MCBA_RESECT_P3P_MAX_SAMPLES. */
#define MCBA_RESECT_P3P_SAMPLE 3
#define MCBA_RESECT_P3P_SLOTS 4
#define MCBA_RESECT_P3P_POLISH 5
#define MCBA_RESECT_P3P_MAX_SAMPLES 1024
int mcba_resect_ransac_p3p(int n_cameras, size_t n_points, const double* points, const double* uvs, const double* cam12, const double* dist5, int n_hypotheses, const int* samples,
                           double threshold, int undistort_iterations, int device, double* rt12, double* best4, unsigned char* inliers, double* pose_out, double* cost_out, unsigned* count_out,
                           int* status_out, double* kernel_ms);

/* ---- Trajectory smoothing (Python: trajectory.smooth_trajectories).  Stateless.  Per track k of n_tracks (tracks are
 * independent), frames t = 0 .. n_frames - 1, unknowns x_t in R^3:
 *   minimise 0.5 f^2 sum_t rho(d_t^2 / f^2) + 0.5 / a_k^2 sum_{t=1}^{T-2} |x_{t-1} - 2 x_t + x_{t+1}|^2,  d_t^2 = (x_t - p_t)^T Sigma_t^-1 (x_t - p_t)
 * points (T, K, 3) = p, cov6 (T, K, 6) = Sigma packed 00 01 02 11 12 22, accel_std (K) = a (positive, finite), f = f_scale > 0, loss 0 linear,
 * 1 soft_l1, 2 huber (scipy's rho).  A frame is usable when p and Sigma are finite and Sigma is positive definite (every pivot of its
 * Jacobi-scaled 3 x 3 Cholesky factor has a square >= 1e-12, the rule of mcba_triangulation_covariance) with a finite inverse; an unusable frame
 * has no data term.  IRLS: weights w_t = rho'(d_t^2 / f^2) start at 1, or at weights_in (T, K; finite, >= 0; NULL = none); every iteration is
 * one solve of the block-pentadiagonal normal equations by a recursive partitioned elimination (separators of two consecutive frames, `segment`
 * pairs of frames between them: 0 = the default, else 2 .. 64) and one small download.  A track stops after solve number i >= 2 when
 * max |x_new - x_old| < xtol max |x_new|, or at max_iterations >= 1; the linear loss is one solve.  max_iterations == 1 with weights_in is one
 * evaluation laid open: one solve with exactly those weights.
 * out_points (T, K, 3): every frame filled for a track of status 1, NaN otherwise.  out_weights (T, K): rho' at the result, 0 on unusable frames.
 * out_d2 (T, K): d_t^2 at the result, NaN on unusable frames.  status (K): 1 ok, -1 fewer than two usable frames (never launched), -2 the square
 * of a pivot of a Jacobi-scaled 6 x 6 block fell below 1e-12.  n_usable, n_iterations (K).  history (max_iterations, K, 2): per solve the
 * objective at its result and its step max |x_new - x_old| (infinite for the first), NaN where a track no longer ran.
 * info8 = {levels, segment, tracks per chunk, chunks, kernel ms, most solves of a track, device bytes of a chunk, 0}: tracks are solved in chunks
 * that fit a device-memory budget (MCBA_SMOOTH_BUDGET_MB, default 8192; the result does not depend on it).  kernel_ms may be NULL.
 * Two calls on the same input return the same bits.  MCBA_ERR_ARG, checked before any device is touched and with nothing written: n_frames == 0
 * or above 2^31, n_tracks < 1, a NULL array, a loss outside 0 .. 2, f_scale or an accel_std not positive and finite, a negative or non-finite
 * weight, max_iterations < 1, xtol < 0, segment outside {0, 2 .. 64}. */
int mcba_smooth_trajectories(size_t n_frames, int n_tracks, const double* points, const double* cov6, const double* accel_std, const double* weights_in, int loss, double f_scale,
                             int max_iterations, double xtol, int segment, int device, double* out_points, double* out_weights, double* out_d2, int* status, int* n_usable, int* n_iterations,
                             double* history, double* info8, double* kernel_ms);

/* ---- Trajectory uncertainty (Python: trajectory.trajectory_uncertainty).  Stateless, additive to ABI 7.  Per track let
 *   A = blockdiag(w_t Sigma_t^-1) + a_k^-2 (D2^T D2 (x) I3)
 * be exactly the matrix of mcba_smooth_trajectories (same points, cov6, accel_std, usable-frame rule and segment; w_t = weights (T, K; finite,
 * >= 0), NULL = 1, and 0 on unusable frames whatever is passed) and Z = A^-1.  out_cov6 (T, K, 6) = Z_tt packed 00 01 02 11 12 22 for every
 * frame, unusable ones included (there: the interpolation uncertainty).  out_lag9 ((T - 1), K, 9; NULL = not computed) = Z_{t,t+1} row-major,
 * rows of frame t; it is not symmetric.  Cov(x_{t+1} - x_t) = Z_tt + Z_{t+1,t+1} - Z_{t,t+1} - Z_{t,t+1}^T is left to the caller: it cancels.
 * With weights = the out_weights of a robust solve this is the weighted-least-squares covariance at those weights, not a Hessian-based one (no
 * rho'' term).  One elimination of every level as in the smoother, then a selected inversion of every level top down; no atomics, two calls on
 * the same input return the same bits, and the chunking over tracks (MCBA_SMOOTH_BUDGET_MB) does not change them.
 * status (K): 1 ok, -1 fewer than two usable frames (never launched), -2 a refused pivot; a track of status -1 or -2 is NaN throughout.
 * n_usable (K).  info8 = {levels, segment, tracks per chunk, chunks, kernel ms, 1, device bytes of a chunk, kernel ms of the selected inversion
 * alone}.  kernel_ms may be NULL.  MCBA_ERR_ARG, checked before any device is touched and with nothing written: n_frames == 0 or above 2^31,
 * n_tracks < 1, a NULL array other than weights and out_lag9, an accel_std not positive and finite, a negative or non-finite weight, segment
 * outside {0, 2 .. 64}. */
int mcba_smooth_covariance(size_t n_frames, int n_tracks, const double* points, const double* cov6, const double* accel_std, const double* weights, int segment, int device,
                           double* out_cov6, double* out_lag9, int* status, int* n_usable, double* info8, double* kernel_ms);

/* ---- The smoother's evidence (Python: trajectory.trajectory_evidence, trajectory.estimate_accel_std).  Stateless,
 * additive to ABI 7.  Per track, with A(a) the matrix of mcba_smooth_covariance (same points, cov6, usable-frame rule, segment and weights) and
 * x(a) = A(a)^-1 b its linear solve,
 *   N(a) = sum_t w_t d_t^2(x) + a^-2 sum_t |x_{t-1} - 2 x_t + x_{t+1}|^2 + log det A(a) + 6 (T - 2) log a
 * is -2 x the log restricted marginal likelihood of a = accel_std up to a constant in a (T the true frame count; the prior is improper on the
 * motions linear in time).  log det A is summed from the Cholesky factors the elimination stores, one log per pivot, per-lane partials and a fixed
 * tree per track: no atomics, the same bits from any chunking (MCBA_SMOOTH_BUDGET_MB).
 * mcba_smooth_evidence: one evaluation at accel_std (K).  out4 (K, 4) = N, the data term, the penalty, log det A; status (K): 1, -1 fewer than
 * two usable frames, -2 a refused pivot -- such a track is NaN throughout; n_usable (K); info8 = {levels, segment, tracks per chunk, chunks,
 * kernel ms, 1, device bytes of a chunk, kernel ms of the per-level log-determinant kernels and the kernel of the final sums}.  MCBA_ERR_ARG as mcba_smooth_covariance. */
int mcba_smooth_evidence(size_t n_frames, int n_tracks, const double* points, const double* cov6, const double* accel_std, const double* weights, int segment, int device, double* out4,
                         int* status, int* n_usable, double* info8, double* kernel_ms);
/* mcba_estimate_accel_std: the a that minimises N, per unit: pool NULL = every track its own unit; else pool (K) labels in 0 .. K - 1, the tracks of
 * one label share one a and their unit's objective is the sum of its running tracks' N in track order (a NaN -- a pivot refused at that candidate
 * -- counts as +infinity).  The rule: (1) grid (n_grid = G >= 3 values, u_g = log lo + g (log hi - log lo) / (G - 1), a_g = exp(u_g), a_0 = lo,
 * a_{G-1} = hi) with g* the first argmin: every candidate NaN gives status -2; g* = 0 gives edge -1 and a = lo, g* = G - 1 edge +1 and a = hi, both
 * with log_std NaN; (2) otherwise a golden-section search in u = log a on [u_{g*-1}, u_{g*+1}], two first evaluations and then one per round, the
 * rounds -- the same for every unit -- ending when the bracket is narrower than rtol in [1e-6, 1); the estimate is the evaluated candidate with
 * the lowest objective, the grid included, the first on a tie; (3) N at u + 0.2 and u - 0.2 gives kappa = (N+ - 2 N0 + N-) / 0.04 and log_std =
 * sqrt(2 / kappa), NaN unless kappa > 0.  Every pass evaluates every track; n_evaluations (1) = G + 2 + rounds + 2 depends on the arguments alone.
 * Outputs (K each unless said): out_accel, out_log_std, out_edge, status, n_usable, n_best = the track's N at its estimate; grid (G); n_grid_out
 * (G, K); info8 as above with [5] = n_evaluations.  The detections are uploaded once per chunk, whatever the number of candidates.
 * MCBA_ERR_ARG, before any device is touched and with nothing written: the checks of mcba_smooth_evidence, n_frames < 3, not 0 < lo < hi with
 * finite inverse squares, n_grid < 3, rtol outside [1e-6, 1), a label outside 0 .. K - 1, and a pooled call that does not fit the budget
 * MCBA_SMOOTH_BUDGET_MB whole (a pool couples the tracks: it cannot run in chunks). */
int mcba_estimate_accel_std(size_t n_frames, int n_tracks, const double* points, const double* cov6, double accel_lo, double accel_hi, int n_grid, double rtol, const double* weights,
                            const int* pool, int segment, int device, double* out_accel, double* out_log_std, int* out_edge, int* status, int* n_usable, double* grid, double* n_grid_out,
                            double* n_best, int* n_evaluations, double* info8, double* kernel_ms);

/* ---- Trajectory refinement (Python: trajectory.refine_trajectories).  Stateless, additive to ABI 7.  Per track k of
 * n_tracks (tracks are independent), frames t = 0 .. T - 1, unknowns x_t in R^3:
 *   minimise 0.5 sum_t sum_{c sees (t,k)} f^2 [rho(ru^2 / f^2) + rho(rv^2 / f^2)] + 0.5 / a_k^2 sum_{t=1}^{T-2} |x_{t-1} - 2 x_t + x_{t+1}|^2,
 *   (ru, rv) = sqrt(w_ctk) (detection - projection_c(x_t)) / pixel_std_c
 * uvs (C, T, K, 2) raw detections (NaN = unseen), cam12 (C, 12), dist5 (C, 5) or NULL: the cameras of mcba_triangulate_refine (the
 * five-coefficient forward model), 1 <= C <= 64; weights (C, T, K) or NULL = 1: finite and >= 0, a zero or NaN weight = unseen; pixel_std (C)
 * positive; start (T, K, 3); accel_std (K) = a; loss 0 linear, 1 soft_l1, 2 huber (scipy's rho), f = f_scale in units of pixel_std.
 * A frame is usable when two cameras or more see it, single when exactly one does.  A track runs when it has two usable frames or more and a
 * finite start.  Gauss-Newton in step form: per iteration one linearisation (H_t with the curvature weights of mcba_triangulate_refine, the
 * gradient G of the whole objective), one solve (blockdiag(H_t) + a^-2 D2^T D2 (x) I3) d = -G by the elimination of mcba_smooth_trajectories
 * (`segment` as there), one evaluation of the objective at x + alpha d for alpha = 1, 1/2, 1/4, 1/8, and one small download: the largest alpha
 * whose objective is not above the current one is taken (none: the track stops where it is, alpha 0), and the track stops when
 * alpha max |d| < xtol max |x| or after max_iterations >= 1.  The objective never rises.
 * out_points (T, K, 3), information (T, K, 6) = H_t at the returned points packed 00 01 02 11 12 22; status (K): 1 ok, -1 fewer than two usable
 * frames, -2 a refused 6 x 6 pivot, -3 a non-finite start (-1 and -3: never launched); every track whose status is not 1 is NaN throughout.
 * n_usable, n_single, n_iterations (K); cost (K) the objective at the result; history (max_iterations, K, 3) = the objective after the
 * iteration, the accepted step alpha max |d|, alpha; NaN where a track no longer ran.  out_cov6 (T, K, 6) and out_lag9 (T - 1, K, 9), both or
 * the second may be NULL: Z_tt and Z_{t,t+1} of the inverse of the Gauss-Newton matrix at the returned points, as mcba_smooth_covariance
 * lays them out -- the covariance in units where pixel_std is the detection noise.  info8 = {levels, segment, tracks per chunk, chunks, kernel
 * ms, most iterations of a track, device bytes of a chunk, kernel ms of the covariance alone}; chunks as in mcba_smooth_trajectories
 * (MCBA_SMOOTH_BUDGET_MB).  No atomics: two calls return the same bits, whatever the chunking.  MCBA_ERR_ARG, checked before any device is
 * touched and with nothing written: n_frames == 0 or above 2^31, n_tracks < 1, n_cameras outside 1 .. 64, a NULL array other than dist5,
 * weights, out_cov6, out_lag9, kernel_ms (out_lag9 without out_cov6), a loss outside 0 .. 2, f_scale, a pixel_std or an accel_std not positive
 * and finite, a negative or infinite weight, max_iterations < 1, xtol < 0, segment outside {0, 2 .. 64}. */
int mcba_refine_trajectories(size_t n_frames, int n_tracks, int n_cameras, const double* uvs, const double* cam12, const double* dist5, const double* weights, const double* pixel_std,
                             const double* start, const double* accel_std, int loss, double f_scale, int max_iterations, double xtol, int segment, int device, double* out_points,
                             double* information, int* status, int* n_usable, int* n_single, int* n_iterations, double* cost, double* history, double* out_cov6, double* out_lag9, double* info8,
                             double* kernel_ms);
/* One evaluation of that loop laid open, at `points` and before anything is accepted: information (T, K, 6) = H, gradient (T, K, 3) = G,
 * step (T, K, 3) = d, data_cost and penalty_cost (K) = the two terms of the objective at the points, trial_costs (K, 4) = the objective at
 * x + alpha d for alpha = 1, 1/2, 1/4, 1/8; status, n_usable, n_single as above.  Arguments, errors and info8 as above. */
int mcba_refine_trajectories_system(size_t n_frames, int n_tracks, int n_cameras, const double* uvs, const double* cam12, const double* dist5, const double* weights, const double* pixel_std,
                                    const double* points, const double* accel_std, int loss, double f_scale, int segment, int device, double* information, double* gradient, double* step,
                                    int* status, int* n_usable, int* n_single, double* data_cost, double* penalty_cost, double* trial_costs, double* info8, double* kernel_ms);

/* ---- Skeleton-constrained keypoint refinement (Python: skeleton.refine_skeleton).  Stateless, additive to ABI 7.  Frames
 * are independent.  The skeleton is a forest over the n_keypoints = K keypoints, 1 <= K <= 64, passed as parent (K) in the caller's numbering
 * (-1 = root) with bone_length (K) = L_k and bone_std (K) = s_k of the bone (k, parent[k]), both positive and finite, in the points' unit; the
 * entries of a root are ignored.  The call checks that the parents form a forest and derives the processing order, the depth levels and the child
 * lists itself.  Per frame, over the positions x_k of its active keypoints:
 *   minimise 0.5 sum_k sum_{c sees k} f^2 [rho(ru^2 / f^2) + rho(rv^2 / f^2)] + 0.5 sum_{active bones} ((|x_k - x_parent(k)| - L_k) / s_k)^2,
 *   (ru, rv) = sqrt(w_ctk) (detection - projection_c(x_k)) / pixel_std_c
 * uvs (C, T, K, 2) raw detections (NaN = unseen), cam12 (C, 12), dist5 (C, 5) or NULL: the cameras of mcba_triangulate_refine (the
 * five-coefficient forward model), 1 <= C <= 64; weights (C, T, K) or NULL = 1: finite and >= 0, a zero or NaN weight = unseen; pixel_std (C)
 * positive; start (T, K, 3); loss 0 .. 4 = linear, soft_l1, huber, cauchy, arctan (scipy's rho), f = f_scale in units of pixel_std; the bone
 * term is always quadratic.
 * A keypoint is usable in a frame with two views or more and a finite start, single with exactly one view and a finite start; with no view or a
 * non-finite start it is out of the frame and its bones are dropped there, which may split a tree.  A connected piece of what is left is fitted
 * when it holds a usable keypoint.  keypoint_status (T, K): 2 fitted as usable, 1 fitted as single, -1 out of the frame, -2 in a piece without a
 * usable keypoint; every keypoint not fitted is NaN in every output.  A single keypoint has two solutions (its ray meets the sphere about its
 * neighbour twice): the fit goes to the one near the start.
 * Levenberg-Marquardt per frame, the iteration of mcba_triangulate_refine with the frame's whole objective: Marquardt's damping lam diag(H) from
 * 1e-4, divided by 10 on acceptance (floor 1e-12), times 10 on rejection; a trial is accepted when the objective is not larger (NaN compares
 * false, a refused 3 x 3 pivot is a rejected step), so the result is never worse than the start.  The Gauss-Newton matrix of a bone with
 * direction u is + u u^T / s^2 on both diagonal blocks and - u u^T / s^2 off the diagonal (its second-order term is left out); the system is
 * eliminated leaf to root on the forest, without fill.  A frame stops, frame_status (T) = 1, when a step has max |d| < xtol max |x| over its
 * active keypoints (accepted or not) or the damping reaches 1e12; at max_iterations >= 1 trials, frame_status = 0; -1: nothing to fit.
 * out_points (T, K, 3); n_iterations (T) trials made; cost, cost_start (T) the objective at the result and at the start; bone_residual (T, K) =
 * (|x_k - x_parent(k)| - L_k) / s_k at the result, NaN for a root and for a bone dropped in the frame.  out_cov6, information (T, K, 6) and
 * direction (T, K, 3): all three or none (NULL).  information = the diagonal block of the Gauss-Newton matrix at the result, bones included,
 * undamped, packed 00 01 02 11 12 22; direction = u of the bone (k, parent[k]), NaN where dropped; out_cov6 = the keypoint's 3 x 3 block of the
 * inverse of that matrix (selected inversion root to leaf), in units where pixel_std is the detection noise; a refused pivot there makes the
 * piece's blocks NaN.  info8 = {levels of the forest, frames per workgroup, frames per chunk, chunks, kernel ms, most iterations of a frame,
 * device bytes of a chunk, 0}.  No atomics: two calls return the same bits, and a frame's result does not depend on the frames around it.
 * MCBA_ERR_ARG, checked before any device is touched and with nothing written: n_frames == 0 or above 2^31, n_keypoints outside 1 .. 64,
 * n_cameras outside 1 .. 64, a NULL array other than dist5, weights, kernel_ms and the three optional outputs, a parent outside -1 .. K - 1 or
 * equal to its keypoint, a cycle, a bone_length or bone_std of a keypoint with a parent not positive and finite, a loss outside 0 .. 4, f_scale
 * or a pixel_std not positive and finite, a negative or infinite weight, max_iterations < 1, xtol < 0. */
int mcba_refine_skeleton(size_t n_frames, int n_keypoints, int n_cameras, const double* uvs, const double* cam12, const double* dist5, const double* weights, const double* pixel_std,
                         const double* start, const int* parent, const double* bone_length, const double* bone_std, int loss, double f_scale, int max_iterations, double xtol, int device,
                         double* out_points, int* keypoint_status, int* frame_status, int* n_iterations, double* cost, double* cost_start, double* bone_residual, double* out_cov6,
                         double* information, double* direction, double* info8, double* kernel_ms);
/* One evaluation of that loop laid open, at `points` with the damping lam >= 0 and before anything is accepted: information (T, K, 6) and
 * direction (T, K, 3) as above, gradient (T, K, 3) of the whole objective, step (T, K, 3) = the solution d of the damped system, data_cost and
 * bone_cost (T) = the two terms of the objective at the points, trial_cost (T) = the objective at x + d; keypoint_status as above, frame_status
 * 1 or -1.  Arguments, errors and info8 as above. */
int mcba_refine_skeleton_system(size_t n_frames, int n_keypoints, int n_cameras, const double* uvs, const double* cam12, const double* dist5, const double* weights, const double* pixel_std,
                                const double* points, const int* parent, const double* bone_length, const double* bone_std, int loss, double f_scale, double lam, int device, double* information,
                                double* gradient, double* direction, double* step, int* keypoint_status, int* frame_status, double* data_cost, double* bone_cost, double* trial_cost,
                                double* info8, double* kernel_ms);
/* Bone lengths from located keypoints (Python: skeleton.estimate_bone_lengths).  Stateless, additive to ABI 7.  points (T, K, 3), NaN = missing;
 * bones (E, 2) pairs of keypoints, 1 <= E <= 65535.  One kernel writes the (E, T) plane of distances sqrt(dx dx + dy dy + dz dz) -- plain
 * products and sums in that order, no fused multiply-add --, NaN where an end has a NaN; the exact radix select of mcba_keypoint_errors then runs
 * twice.  length (E) = the exact nan-median of the bone's distances (the mean of the two middle values for an even count), std (E) = 1.4826 times
 * the exact nan-median of |distance - length|, count (E) = the frames that have both ends; a bone with none has NaN, NaN, 0.  MCBA_ERR_ARG,
 * checked before any device is touched and with nothing written: n_frames == 0 or above 2^31, n_keypoints < 1, n_bones outside 1 .. 65535, a NULL
 * array other than kernel_ms, a bone's keypoint outside 0 .. K - 1. */
int mcba_bone_lengths(size_t n_frames, int n_keypoints, const double* points, int n_bones, const int* bones, int device, double* length, double* std, int* count, double* kernel_ms);

/* ---- skeleton trajectories (Python: skeleton.refine_skeleton_trajectories) -------------------------------------
 * Stateless, additive to ABI 7.  The tracks of mcba_refine_trajectories joined inside every frame by the bones of mcba_refine_skeleton: one problem
 * per call over x_{t,k}, t < n_frames, of the running tracks (two usable frames or more and a finite start, as there),
 *   the data term and the second-difference prior of mcba_refine_trajectories + 0.5 sum_t sum_{active bones} ((|x_tk - x_tp| - L_k) / s_k)^2,
 * a bone (k, parent[k]) being active, in every frame, when both its tracks run.  Arrays as mcba_refine_trajectories (uvs (C, T, K, 2), start
 * (T, K, 3), accel_std (K), weights (C, T, K) or NULL, pixel_std (C), loss 0 .. 2) and mcba_refine_skeleton (parent, bone_length, bone_std (K):
 * a forest over at most 64 keypoints).  Gauss-Newton in step form on the call's objective: per iteration the system (M + B) d = -G -- M the
 * tracks' block-pentadiagonal matrices, B the bones' Gauss-Newton terms -- is solved by conjugate gradients preconditioned with M (one
 * elimination of the smoother per iteration, one re-solve from its factors per CG iteration) until r^T z <= cg_tol^2 r0^T z0 or cg_max
 * iterations; the largest alpha of 1, 1/2, 1/4, 1/8 whose objective is not above the current one is taken (none: the call stops where it is), and
 * the call stops when alpha max |d| < xtol max |x| or after max_iterations.
 * Outputs: out_points (T, K, 3); information (T, K, 6) = H of the data term at the returned points, packed 00 01 02 11 12 22; status, n_usable,
 * n_single (K) as mcba_refine_trajectories (1, -1, -2, -3; a start whose objective is not finite gives every running track -3); converged (1) =
 * the call stopped on a small step or on nothing accepted; n_iterations (1); cost, cost_start (1); history (max_iterations, 4) = objective,
 * accepted step, alpha, CG iterations of that solve, NaN beyond n_iterations (an iteration that ends on a refused pivot or on an objective that
 * is not finite accepts nothing and is not counted, in n_iterations or in the CG total); bone_residual (T, K) and direction (T, K, 3) of bone (k, parent[k])
 * at the returned points, NaN where the bone is not active; info8 = levels, segment, running tracks, CG iterations in all, kernel ms, outer
 * iterations, device bytes, 0.  Whatever belongs to a track that is not 1 is NaN.
 * MCBA_ERR_ARG, before any device is touched and with nothing written: the checks of the two calls above, cg_tol outside (0, 1), cg_max < 1, and a
 * call that does not fit the budget MCBA_SMOOTH_BUDGET_MB whole (bones couple the tracks: it cannot run in chunks). */
int mcba_refine_skeleton_trajectories(size_t n_frames, int n_keypoints, int n_cameras, const double* uvs, const double* cam12, const double* dist5, const double* weights,
                                      const double* pixel_std, const double* start, const double* accel_std, const int* parent, const double* bone_length, const double* bone_std, int loss,
                                      double f_scale, int max_iterations, double xtol, double cg_tol, int cg_max, int segment, int device, double* out_points, double* information, int* status,
                                      int* n_usable, int* n_single, int* converged, int* n_iterations, double* cost, double* cost_start, double* history, double* bone_residual,
                                      double* direction, double* info8, double* kernel_ms);
/* One evaluation of that loop laid open, at `points` and before anything is accepted: information and direction as above, gradient (T, K, 3) of the
 * whole objective, step (T, K, 3) = the iterate of the preconditioned recurrence for (M + B) d = -G when it ended, cg_iterations (1), cg_residual
 * (1) = sqrt(r^T z / r0^T z0) of the recurrence then, data_cost, penalty_cost, bone_cost (1 each) = the three terms of the objective at the points,
 * trial_costs (4) = the objective at x + alpha d for alpha = 1, 1/2, 1/4, 1/8.  resolve_check: NULL, or (2, T, K, 3) for tests -- the solution of
 * M z = -G by the elimination and back-substitution, then by the re-solve from the stored factors and the same back-substitution after the
 * right-hand-side halves of every stored record were overwritten with NaN (tracks that do not run: unwritten).  Arguments, errors and info8 as
 * above. */
int mcba_refine_skeleton_trajectories_system(size_t n_frames, int n_keypoints, int n_cameras, const double* uvs, const double* cam12, const double* dist5, const double* weights,
                                             const double* pixel_std, const double* points, const double* accel_std, const int* parent, const double* bone_length, const double* bone_std,
                                             int loss, double f_scale, double cg_tol, int cg_max, int segment, int device, double* information, double* gradient, double* direction,
                                             double* step, int* status, int* n_usable, int* n_single, int* cg_iterations, double* cg_residual, double* data_cost, double* penalty_cost,
                                             double* bone_cost, double* trial_costs, double* resolve_check, double* info8, double* kernel_ms);

#ifdef __cplusplus
}
#endif
#endif /* MCBA_H */
