// mcba_lm_api.hip -- the device-resident Levenberg-Marquardt entry points of include/mcba.h: the per-iteration chain with the decision
// on the GPU (mcba_lm_set_state .. mcba_lm_iterate), the ticks of the device-resident loop (mcba_lm_auto_*), the whole loop in one call
// (mcba_lm_run / _history / _result), and what the host reads back from them.
#include <atomic>
#include <chrono>

#include "mcba_handle.h"

using namespace mcba_internal;

extern "C" {

// ---------------------------------------------------------------------------------------------------------
// Device-resident LM iteration: the accept/reject decision and the damping update happen on the GPU (k_decide), so
// backsub -> gram(trial) -> sum -> decide -> frame_factor -> syrk -> reduce is ONE stream-ordered chain.
// Convention while it is in use: parameter slot i and linearisation buffer i belong together; state[3] = current i.
int mcba_lm_set_state(mcba_handle* h, const double* state) {
  if (!h || !state) return fail(MCBA_ERR_ARG, "mcba_lm_set_state: bad argument");
  int sel = (int)state[3];
  if (sel != 0 && sel != 1) return fail(MCBA_ERR_ARG, "mcba_lm_set_state: state[3] must be 0 or 1");
  HIPCHK(hipSetDevice(h->device));
  NEED_SOLVER(h);
  double* stage = h->pinned + h->nsys + 8;
  memcpy(stage, state, MCBA_LMS * sizeof(double));
  if (!(stage[MCBA_LM_CFL] > 0.0)) stage[MCBA_LM_CFL] = h->curv_floor;  // (a caller that fills the first four entries only: the handle's model, fixed)
  HIPCHK(hipMemcpyAsync(h->red + h->nsys + 8, stage, MCBA_LMS * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (sel != h->lin) {
    // the accepted linearisation must live in buffer `sel`: swap the buffer pointers instead of copying 48 MB
    std::swap(h->rec2[0], h->rec2[1]);
    std::swap(h->gpart2[0], h->gpart2[1]);
    h->lin = sel;
  }
  h->trial_ready = false;
  return MCBA_OK;
}

static int lm_trial_impl(mcba_handle* h, const double* delta_cam, const mcba::DecideArgs& da) {
  if (!h || !delta_cam) return fail(MCBA_ERR_ARG, "mcba_lm_trial: bad argument");
  if (h->have_bounds) return fail(MCBA_ERR_ARG, "box constraints are set (mcba_set_bounds): drive the steps with mcba_step / mcba_step_linearize (the host-driven loop)");
  if (h->loss == mcba::LOSS_TABLE) return fail(MCBA_ERR_ARG, "a tabulated loss is set (mcba_set_loss_table): the device-resident loops cannot call the caller's function -- use the host-driven loop");
  if (!h->have_lin) return fail(MCBA_ERR_ARG, "mcba_lm_trial: no linearisation");
  HIPCHK(hipSetDevice(h->device));
  int rc;
  if ((rc = backsub_launch(h, dev_sel(h, 0), 0, 1, 0, 1, delta_cam))) return rc;
  if ((rc = gram_launch(h, dev_sel(h, 1), h->x[0], h->x[1], 0, 1))) return rc;  // trial point = the OTHER slot / buffer
  return trial_sum(h, dev_sel(h, 1), 0, 1, da);
}

int mcba_lm_trial(mcba_handle* h, const double* delta_cam) {
  return lm_trial_impl(h, delta_cam, mcba::DecideArgs{0, 0.0, 0.0, 0.0, 0.0, 0.0, nullptr});
}

// decide_here: k_syrk itself sums the trial scalars and takes the accept / reject decision (single-GPU ticks); it reads the
// state the previous tick left and publishes the decided state to the second buffer, which the rest of the tick reads.
static int lm_reduce_chain(mcba_handle* h, int rank_slot, bool spec = false, bool decide_here = false, unsigned long long seq = 0) {
  int rc;
  const mcba::Sel sl = spec ? spec_sel(h) : dev_sel(h, 0);
  mcba::SyrkFuse fz = no_fuse();
  if (decide_here) {
    fz.decide = 1;
    fz.cp0 = h->gpart2[0] + (size_t)90 * h->nfb;
    fz.cp1 = h->gpart2[1] + (size_t)90 * h->nfb;
    const mcba::GramCostSlots cs = h->gram.cost_slots();   // where the linearisation's launches left the trial cost
    fz.cstride = cs.cstride; fz.cinner = cs.cinner; fz.cdense = cs.cdense;
    fz.couter = (size_t)MCBA_GP * h->nfb;
    fz.ncp = h->C * fz.cinner;
    fz.bpart = h->bpart;
    fz.nbp = h->nbblocks;
    fz.trial_out = h->red + h->nsys;
    fz.lms_post = post_state(h);
    fz.da = mcba::DecideArgs{2, 0.0, 0.0, 0.0, h->lam_min, h->lam_max, nullptr, h->ftol, h->xtol, h->dec_floor};
    fz.timeout_word = timeout_word(h);
    fz.seq_prev = seq > 0 ? (double)(seq - 1) : 0.0;
  }
  if ((rc = syrk_launch(h, sl, fz))) return rc;
  if ((rc = reduce_launch(h, decide_here ? post_sel(h) : sl, rank_slot, spec))) return rc;
  h->have_red = true;
  h->spec_copy_ready = spec;
  return MCBA_OK;
}

int mcba_lm_decide_reduce(mcba_handle* h, double pred_cam, double dcn2, double xcn2, double lam_min, double lam_max, int rank_slot) {
  if (!h || rank_slot < 0 || rank_slot > 11) return fail(MCBA_ERR_ARG, "mcba_lm_decide_reduce: bad argument");
  HIPCHK(hipSetDevice(h->device));
  {
    Scope sc(h, K_DECIDE);
    mcba::launch_decide(h->stream, h->red + h->nsys, mcba::DecideArgs{1, pred_cam, dcn2, xcn2, lam_min, lam_max, h->red + h->nsys + 8, 0.0, 0.0, h->dec_floor});
  }
  int rc = check_launch();
  if (rc) return rc;
  return lm_reduce_chain(h, rank_slot);
}

int mcba_lm_rebuild(mcba_handle* h, int rank_slot) {
  if (!h || rank_slot < 0 || rank_slot > 11) return fail(MCBA_ERR_ARG, "mcba_lm_rebuild: bad argument");
  HIPCHK(hipSetDevice(h->device));
  return lm_reduce_chain(h, rank_slot);
}

int mcba_lm_fetch(mcba_handle* h, double* host) {
  if (!h || !host) return fail(MCBA_ERR_ARG, "mcba_lm_fetch: bad argument");
  size_t cnt = h->nsys + 8 + MCBA_LMS;
  HIPCHK(hipMemcpyAsync(h->pinned, h->red, cnt * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  memcpy(host, h->pinned, cnt * sizeof(double));
  int sel = (int)host[h->nsys + 8 + 3];
  if (sel == 0 || sel == 1) h->lin = sel;  // keep the host-selected entry points consistent with the device state
  h->have_spec = false;
  return MCBA_OK;
}

int mcba_lm_iterate(mcba_handle* h, const double* delta_cam, double pred_cam, double dcn2, double xcn2, double lam_min, double lam_max, double* host) {
  if (!h) return fail(MCBA_ERR_ARG, "NULL handle");
  // single rank: the decision rides on k_sum_trial (no separate launch, nothing to all-reduce in between)
  int rc = lm_trial_impl(h, delta_cam, mcba::DecideArgs{1, pred_cam, dcn2, xcn2, lam_min, lam_max, h->red + h->nsys + 8, 0.0, 0.0, h->dec_floor});
  if (rc) return rc;
  rc = lm_reduce_chain(h, 0);
  if (rc) return rc;
  return mcba_lm_fetch(h, host);
}


// ---------------------------------------------------------------------------------------------------------
// Device-resident LM loop: the reduced camera system is solved on the GPU too (k_solve_cam), the termination tests run
// there, and the host only enqueues "ticks" and reads the 32-double state each one posts to a host-mapped ring:
//   one GPU:        tick = k_gram(trial) -> k_syrk (trial sums + decision + frame factors + SYRK) -> k_reduce_system -> k_solve_backsub (solve + the
//                   back-substitution of the next trial step; k_backsub / k_solve_cam apart for the first tick, > 9 cameras, MCBA_FUSE_BACKSUB=0)
//   frame-sharded:  tick = k_backsub -> k_gram(trial) -> k_syrk (speculative) -> k_reduce_system (+ trial scalars) -> all-reduce -> k_solve_cam (decides)
//                   (MCBA_SPECULATE=0: k_sum_trial -> all-reduce -> k_decide -> k_syrk -> k_reduce_system -> all-reduce -> k_solve_cam)
// No host synchronisation inside or between ticks; after termination the remaining ticks return immediately.
int mcba_lm_auto_config(mcba_handle* h, double ftol, double xtol, double gtol, double lam_min, double lam_max, const unsigned char* fixed) {
  if (!h || !(lam_min > 0.0) || !(lam_max > lam_min)) return fail(MCBA_ERR_ARG, "mcba_lm_auto_config: bad argument");
  HIPCHK(hipSetDevice(h->device));
  NEED_SOLVER(h);
  h->ftol = ftol; h->xtol = xtol; h->gtol = gtol; h->lam_min = lam_min; h->lam_max = lam_max;
  h->have_fixed = fixed != nullptr;
  if (fixed) {
    HIPCHK(hipMemcpyAsync(h->fixed, fixed, (size_t)h->n, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  memset(h->ring, 0, (size_t)kRing * MCBA_LMS * sizeof(double));
  HIPCHK(hipMemsetAsync(h->dcbuf + h->n, 0, 8 * sizeof(double), h->stream));  // sequence numbers restart: no stale release word
  HIPCHK(hipStreamSynchronize(h->stream));
  h->trial_ready = false;
  h->last_solve_seq = 0;
  h->waited_seq = 0;
  h->auto_ready = true;
  if (const char* e = getenv("MCBA_SPECULATE")) h->speculate = atoi(e) != 0 && !h->sparse;
  return MCBA_OK;
}

static int auto_solve_impl(mcba_handle* h, unsigned long long seq, int decide, bool decided_by_syrk, bool fuse_next = false) {
  // frame-sharded ticks with one collective (the decision is taken here, after a speculative reduction that left a copy of the
  // pre-decision state behind): the back-substitution of the next trial step rides along as well
  if (decide && h && h->fuse_backsub && h->spec_copy_ready) fuse_next = true;
  if (!h || !h->auto_ready || seq == 0) return fail(MCBA_ERR_ARG, "mcba_lm_auto_solve: call mcba_lm_auto_config first; seq >= 1");
  if (h->have_bounds) return fail(MCBA_ERR_ARG, "box constraints are set (mcba_set_bounds): the device-resident loop does not project its trial points -- use the host-driven loop");
  if (!h->have_red) return fail(MCBA_ERR_ARG, "mcba_lm_auto_solve: no reduced system");
  HIPCHK(hipSetDevice(h->device));
  mcba::SolveArgs a;
  a.red = h->red; a.lms = h->red + h->nsys + 8; a.lms_in = decided_by_syrk ? post_state(h) : a.lms; a.work = h->swork; a.dc = h->dcbuf; a.x0 = h->x[0]; a.x1 = h->x[1];
  a.fixed = h->have_fixed ? h->fixed : nullptr;
  a.dscale = h->have_xscale ? h->dscale : nullptr;
  a.host_state = h->ring_dev + (size_t)(seq % kRing) * MCBA_LMS;
  a.flag = fuse_next ? h->dcbuf + h->n : nullptr;
  a.timeout_word = timeout_word(h);
  a.seq = (double)seq; a.gtol = h->gtol; a.lam_max = h->lam_max;
  h->last_solve_seq = seq;
  a.stage_tag = (double)(++h->solve_launches);
  a.n = h->n; a.npad = h->npad; a.use_lds = h->solve_lds; a.cw = h->cw;
  a.decide = decide ? 1 : 0; a.lam_min = h->lam_min; a.ftol = h->ftol; a.xtol = h->xtol; a.dec_floor = h->dec_floor;
  if (h->sparse) {   // the blocked multi-workgroup solve (mcba_sparse.hip); its decisions are taken before it (k_sum_trial / k_decide)
    if (decide) return fail(MCBA_ERR_ARG, "mcba_lm_auto_solve: the sparse-Schur handle takes the accept / reject decision before the solve (decide = 0)");
    h->trial_ready = false;
    return sparse_solve(h, a);
  }
  {
    Scope sc(h, K_SOLVE);
    if (fuse_next)  // + the back-substitution of the next tick's trial step, overlapped with the solve (polls bounded: ~0.5 s)
      mcba::launch_solve_backsub(h->stream, a, dev_sel(h, 0), h->rec2[0], h->rec2[1], h->fbuf, h->x[0], h->x[1], h->bpart, h->C, h->F, h->Fpad, decide ? post_state(h) : a.lms_in, h->fuse_max_polls, decide ? 1 : 0,
                                 timeout_word(h), h->ring_dev + (size_t)kRing * MCBA_LMS, h->strict_sync ? 1 : 0);
    else
      mcba::launch_solve_cam(h->stream, a);
  }
  h->trial_ready = fuse_next;
  return check_launch();
}

int mcba_lm_auto_solve(mcba_handle* h, unsigned long long seq, int decide) { return auto_solve_impl(h, seq, decide, false); }

// The release-word protocol between the solve and the back-substitution workgroups of k_solve_backsub (csrc/mcba_backsub.h): by default
// (round 6) the readers ACQUIRE the word with an agent-scope fence behind the poll -- the form the HIP memory model asks for.  on == 0 selects,
// at run time for this handle, the relaxed reader (agent-scope relaxed loads that bypass the per-XCD L2 + in-order issue): ~1.3 us per
// iteration faster, stress-tested, but a data race by the model.  A new handle starts from MCBA_STRICT_SYNC in the environment (unset = 1).
// Same results to the bit either way.
int mcba_set_strict_sync(mcba_handle* h, int on) {
  if (!h) return fail(MCBA_ERR_ARG, "NULL handle");
  h->strict_sync = on != 0;
  return MCBA_OK;
}
int mcba_get_strict_sync(const mcba_handle* h) { return h && h->strict_sync ? 1 : 0; }

int mcba_lm_set_decrease_floor(mcba_handle* h, double dec_floor) {
  if (!h || !(dec_floor >= 0.0) || dec_floor >= 1.0) return fail(MCBA_ERR_ARG, "mcba_lm_set_decrease_floor: 0 <= floor < 1 required (0 = 1/3)");
  h->dec_floor = dec_floor;
  return MCBA_OK;
}

// sum_here: k_sum_trial follows (frame-sharded ticks: the trial scalars are all-reduced); otherwise k_syrk sums and decides
static int auto_trial_impl(mcba_handle* h, int decide, bool sum_here) {
  if (!h || !h->auto_ready) return fail(MCBA_ERR_ARG, "mcba_lm_auto_trial: call mcba_lm_auto_config first");
  if (h->have_bounds) return fail(MCBA_ERR_ARG, "box constraints are set (mcba_set_bounds): the device-resident loop does not project its trial points -- use the host-driven loop");
  if (h->loss == mcba::LOSS_TABLE) return fail(MCBA_ERR_ARG, "a tabulated loss is set (mcba_set_loss_table): the device-resident loops cannot call the caller's function -- use the host-driven loop");
  if (!h->have_lin) return fail(MCBA_ERR_ARG, "mcba_lm_auto_trial: no linearisation");
  HIPCHK(hipSetDevice(h->device));
  int rc;
  const bool ready = h->trial_ready;  // (the previous tick's k_solve_backsub has already produced this trial step)
  h->trial_ready = false;
  if (!ready && (rc = backsub_launch(h, dev_sel(h, 0), 0, 1, 0, 1, nullptr))) return rc;
  if ((rc = gram_launch(h, dev_sel(h, 1), h->x[0], h->x[1], 0, 1))) return rc;
  if (!sum_here) return MCBA_OK;
  return trial_sum(h, dev_sel(h, 1), 0, 1, mcba::DecideArgs{decide ? 2 : 0, 0.0, 0.0, 0.0, h->lam_min, h->lam_max, h->red + h->nsys + 8, h->ftol, h->xtol, h->dec_floor});
}

// decide: 0 k_sum_trial follows (the trial scalars are all-reduced on their own), != 0 it also decides, -1 no k_sum_trial:
// the speculative reduction (mcba_lm_auto_reduce(h, 2, .)) sums the trial scalars itself
int mcba_lm_auto_trial(mcba_handle* h, int decide) { return auto_trial_impl(h, decide < 0 ? 0 : decide, decide >= 0); }

int mcba_lm_auto_reduce(mcba_handle* h, int decide, int rank_slot) {
  if (!h || !h->auto_ready || rank_slot < 0 || rank_slot > 11 || decide < 0 || decide > 2) return fail(MCBA_ERR_ARG, "mcba_lm_auto_reduce: bad argument");
  if (decide == 2 && h->sparse) return fail(MCBA_ERR_ARG, "mcba_lm_auto_reduce: the sparse-Schur handle has no speculative reduction (decide 0 or 1)");
  HIPCHK(hipSetDevice(h->device));
  if (decide == 1) {
    {
      Scope sc(h, K_DECIDE);
      mcba::launch_decide(h->stream, h->red + h->nsys, mcba::DecideArgs{2, 0.0, 0.0, 0.0, h->lam_min, h->lam_max, h->red + h->nsys + 8, h->ftol, h->xtol, h->dec_floor});
    }
    int rc = check_launch();
    if (rc) return rc;
  }
  return lm_reduce_chain(h, rank_slot, decide == 2);
}

int mcba_lm_auto_tick(mcba_handle* h, unsigned long long seq, int rank_slot) {
  if (!h) return fail(MCBA_ERR_ARG, "NULL handle");
  const bool coll = h->comm != nullptr;
  int rc;
  if (!coll && h->sparse) {  // sparse-Schur handle, one GPU: k_backsub -> k_gram -> k_sum_trial (+ decision) -> frame factors / pairs / assembly -> tail -> blocked solve
    if (rank_slot < 0 || rank_slot > 11) return fail(MCBA_ERR_ARG, "mcba_lm_auto_tick: bad rank slot");
    if ((rc = auto_trial_impl(h, 1, true))) return rc;
    if ((rc = lm_reduce_chain(h, rank_slot))) return rc;
    return auto_solve_impl(h, seq, 0, false);
  }
  if (!coll) {  // one GPU: [k_backsub ->] k_gram -> k_syrk (trial sums + decision + frame factors + SYRK) -> k_reduce_system -> k_solve_backsub
    if (rank_slot < 0 || rank_slot > 11) return fail(MCBA_ERR_ARG, "mcba_lm_auto_tick: bad rank slot");
    if ((rc = auto_trial_impl(h, 0, false))) return rc;
    if ((rc = lm_reduce_chain(h, rank_slot, false, true, seq))) return rc;
    return auto_solve_impl(h, seq, 0, true, h->fuse_backsub);
  }
  if (h->speculate) {  // ONE collective: speculative reduction, [system | trial scalars] all-reduced together, decision in k_solve_cam
    if ((rc = mcba_lm_auto_trial(h, -1))) return rc;
    if ((rc = mcba_lm_auto_reduce(h, 2, rank_slot))) return rc;
    if ((rc = mcba_comm_allreduce(h, 0, h->nsys + 8))) return rc;
    return mcba_lm_auto_solve(h, seq, 1);
  }
  if ((rc = mcba_lm_auto_trial(h, 0))) return rc;
  if ((rc = mcba_comm_allreduce(h, h->nsys, 8))) return rc;
  if ((rc = mcba_lm_auto_reduce(h, 1, rank_slot))) return rc;
  if ((rc = mcba_comm_allreduce(h, 0, h->nsys))) return rc;
  return mcba_lm_auto_solve(h, seq, 0);
}

int mcba_get_cam_step(mcba_handle* h, double* host) {
  if (!h || !host) return fail(MCBA_ERR_ARG, "mcba_get_cam_step: bad argument");
  HIPCHK(hipSetDevice(h->device));
  NEED_SOLVER(h);
  HIPCHK(hipMemcpyAsync(host, h->dcbuf, (size_t)h->n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return MCBA_OK;
}

int mcba_lm_auto_wait(mcba_handle* h, unsigned long long seq, double* state) {
  if (!h || !state || !h->auto_ready || seq == 0) return fail(MCBA_ERR_ARG, "mcba_lm_auto_wait: bad argument");
  volatile double* slot = h->ring + (size_t)(seq % kRing) * MCBA_LMS;
  const double want = (double)seq;
  auto t0 = std::chrono::steady_clock::now();
  bool synced = false;
  for (unsigned spin = 0;; ++spin) {
    if (slot[MCBA_LM_SEQ] == want) break;
    __builtin_ia32_pause();
    if ((spin & 0xFFF) == 0xFFF && !synced) {
      double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      if (el > 0.05) {  // not the fast path any more: block on the stream, then look once more
        HIPCHK(hipSetDevice(h->device));
        HIPCHK(hipStreamSynchronize(h->stream));
        synced = true;
        if (slot[MCBA_LM_SEQ] != want) return fail(MCBA_ERR_ARG, "mcba_lm_auto_wait: that tick was never enqueued (or the ring slot was overwritten)");
      }
    }
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  for (int i = 0; i < MCBA_LMS; ++i) state[i] = slot[i];
  if (seq > h->waited_seq) h->waited_seq = seq;
  if (h->fuse_backsub && const_cast<volatile double*>(h->ring)[(size_t)kRing * MCBA_LMS] != 0.0) {
    // a back-substitution workgroup of k_solve_backsub gave up waiting for the solve (mcba_backsub.h): the ticks already in
    // flight discard their stale trial points on the device; from here on the solve and the back-substitution are two launches
    h->fuse_backsub = false;
    h->trial_ready = false;
  }
  int sel = (int)state[3];
  if (sel == 0 || sel == 1) h->lin = sel;
  h->have_spec = false;
  return MCBA_OK;
}

// ---------------------------------------------------------------------------------------------------------
// The whole device-resident LM loop in ONE call (round 5): what solver.LevenbergMarquardt.start() + its iterate() loop + finalize() do
// through a dozen crossings and six host synchronisations before the first tick -- upload x0, linearise, reduce, read the cost back,
// write the state, configure, solve -- is enqueued here without a single wait: the start state is written ON THE DEVICE from the reduced
// system (k_lm_init), the first ticks are enqueued behind the first solve at once, and the host then only polls the ring.  Same ticks,
// same decisions, same order as the Python loop (the device decides; this loop only chooses how many ticks are in flight, by the same
// rule).  opt: 0 ftol 1 xtol 2 gtol 3 lam0 4 lam_min 5 lam_max 6 dec_floor 7 curvature floor 8 curvature switch (0 = fixed model)
// 9 max_nfev 10 max ticks (< 0: no limit) 11 ticks in flight (depth) 12 rank slot.  x0 NULL = start from what slot 0 holds.
// summary: 0 status (scipy's; 0 = a limit was reached) 1 rows recorded 2 rows the main loop consumed (the rest were retired by the
// final drain) -- fetch the rows with mcba_lm_history.
int mcba_lm_run(mcba_handle* h, const double* x0, const double* opt, const unsigned char* fixed, double* summary) {
  if (!h || !opt || !summary) return fail(MCBA_ERR_ARG, "mcba_lm_run: bad argument");
  if (!h->have_obs) return fail(MCBA_ERR_ARG, "mcba_lm_run: upload observations first");
  if (h->have_bounds) return fail(MCBA_ERR_ARG, "mcba_lm_run: box constraints are set (mcba_set_bounds) -- use the host-driven loop");
  if (h->loss == mcba::LOSS_TABLE) return fail(MCBA_ERR_ARG, "mcba_lm_run: a tabulated loss is set (mcba_set_loss_table) -- use the host-driven loop");
  const double lam0 = opt[3], lam_min = opt[4], lam_max = opt[5], cfl = opt[7], cfl_switch = opt[8];
  const int depth = std::max(1, std::min((int)opt[11], 12)), rank_slot = (int)opt[12];
  const double max_nfev = opt[9], max_ticks = opt[10];
  if (!(lam0 > 0.0) || !(lam_min > 0.0) || !(lam_max > lam_min) || !(cfl > 0.0) || cfl > 1.0 || rank_slot < 0 || rank_slot > 11 || !(opt[6] >= 0.0) || opt[6] >= 1.0)
    return fail(MCBA_ERR_ARG, "mcba_lm_run: bad option");
  HIPCHK(hipSetDevice(h->device));
  NEED_SOLVER(h);
  int rc;
  if (h->auto_ready) HIPCHK(hipStreamSynchronize(h->stream));  // no tick of an earlier run may still be posting into the ring
  if (x0) HIPCHK(hipMemcpyAsync(h->x[0], x0, ((size_t)12 * h->C + (size_t)6 * h->F) * sizeof(double), hipMemcpyHostToDevice, h->stream));  // (pageable: staged when the call returns)
  h->curv_floor = cfl;
  h->dec_floor = opt[6];
  h->lin = 0;   // parameter slot 0 and linearisation buffer 0 belong together (mcba_lm_set_state's convention)
  if ((rc = gram_launch(h, host_sel(0), h->x[0], h->x[0], 0, 0))) return rc;
  h->have_lin = true; h->have_spec = false;
  if ((rc = mcba_build_reduced(h, lam0, rank_slot))) return rc;
  if (h->comm && (rc = mcba_comm_allreduce(h, 0, h->nsys))) return rc;
  mcba::launch_lm_init(h->stream, h->red + (size_t)h->n * h->n + 3 * (size_t)h->n, h->red + h->nsys + 8, lam0, 0, cfl, cfl_switch, h->dcbuf + h->n);
  if ((rc = check_launch())) return rc;
  // mcba_lm_auto_config, without its two waits
  h->ftol = opt[0]; h->xtol = opt[1]; h->gtol = opt[2]; h->lam_min = lam_min; h->lam_max = lam_max;
  h->have_fixed = fixed != nullptr;
  if (fixed) HIPCHK(hipMemcpyAsync(h->fixed, fixed, (size_t)h->n, hipMemcpyHostToDevice, h->stream));
  memset(h->ring, 0, (size_t)kRing * MCBA_LMS * sizeof(double));
  h->trial_ready = false;
  h->last_solve_seq = 0;
  h->waited_seq = 0;
  h->auto_ready = true;
  if (const char* e = getenv("MCBA_SPECULATE")) h->speculate = atoi(e) != 0 && !h->sparse;
  // (with <= 9 cameras the first solve's launch already carries the back-substitution of the first trial step, like every later one)
  if ((rc = auto_solve_impl(h, 1, 0, false, h->fuse_backsub))) return rc;

  h->hist.clear();
  unsigned long long issued = 1, retired = 1;
  double nfev = 1.0, st[MCBA_LMS];
  auto top_up = [&]() -> int {
    while (issued - retired < (unsigned long long)depth) {
      const double inflight = (double)(issued - retired);
      if (nfev + inflight >= max_nfev) break;
      if (max_ticks >= 0.0 && (double)(issued - 1) >= max_ticks) break;
      ++issued;
      int r = mcba_lm_auto_tick(h, issued, rank_slot);
      if (r) return r;
    }
    return MCBA_OK;
  };
  if ((rc = top_up())) return rc;            // the first ticks go in behind the first solve: nobody waits for it on the way
  if ((rc = mcba_lm_auto_wait(h, 1, st))) return rc;
  h->hist.insert(h->hist.end(), st, st + MCBA_LMS);
  if (!std::isfinite(st[0])) return fail(MCBA_ERR_NONFINITE, "Residuals are not finite in the initial point.");
  const int status0 = (int)st[MCBA_LM_DONE];
  int status = -1;
  double steps = 0.0;
  for (;;) {
    if (nfev >= max_nfev || (max_ticks >= 0.0 && steps >= max_ticks)) { status = 0; break; }
    steps += 1.0;
    if (status0) { status = status0; break; }
    if ((rc = top_up())) return rc;
    if (issued == retired) { status = 0; break; }
    ++retired;
    if ((rc = mcba_lm_auto_wait(h, retired, st))) return rc;
    h->hist.insert(h->hist.end(), st, st + MCBA_LMS);
    if (st[MCBA_LM_REBUILD] == 0.0) nfev = 1.0 + st[MCBA_LM_NFEV];
    if (st[MCBA_LM_DONE] != 0.0) { status = (int)st[MCBA_LM_DONE]; break; }
  }
  const size_t n_main = h->hist.size() / MCBA_LMS;
  while (retired < issued) {   // stopped with ticks in flight: retire them (their accepted steps count unless the loop had terminated)
    ++retired;
    if ((rc = mcba_lm_auto_wait(h, retired, st))) return rc;
    h->hist.insert(h->hist.end(), st, st + MCBA_LMS);
  }
  summary[0] = (double)status;
  summary[1] = (double)(h->hist.size() / MCBA_LMS);
  summary[2] = (double)n_main;
  summary[3] = steps;
  return MCBA_OK;
}

int mcba_lm_history(mcba_handle* h, double* rows, size_t capacity_rows) {
  if (!h || !rows) return fail(MCBA_ERR_ARG, "mcba_lm_history: bad argument");
  const size_t n = h->hist.size() / MCBA_LMS;
  if (capacity_rows < n) return fail(MCBA_ERR_ARG, "mcba_lm_history: buffer too small (summary[1] of mcba_lm_run rows)");
  if (n) memcpy(rows, h->hist.data(), h->hist.size() * sizeof(double));
  return MCBA_OK;
}

// Solution and gradient of the current point in ONE device-to-host copy: out = [x (12C + 6F) | gradient (12C + 6F)] -- x of `slot`, the
// camera gradient of the reduced system in the reduce buffer (scattered to the parameter layout, zero where a parameter is held fixed by
// the camera block width or by mcba_lm_auto_config's / mcba_lm_run's flags), the frame gradients.  The reduced system must be that of
// the current point (after a terminated loop it is; solver.LevenbergMarquardt.finalize rebuilds it otherwise).
int mcba_lm_result(mcba_handle* h, int slot, double* x_out, double* grad_out, mcba_buffer** grad_dev) {
  if (!slot_ok(h, slot) || !x_out || (grad_out && grad_dev)) return fail(MCBA_ERR_ARG, "mcba_lm_result: bad argument");
  if (!h->have_red) return fail(MCBA_ERR_ARG, "mcba_lm_result: no reduced system");
  HIPCHK(hipSetDevice(h->device));
  const size_t nx = (size_t)12 * h->C + (size_t)6 * h->F;
  if (grad_out && grad_out != x_out + nx) return fail(MCBA_ERR_ARG, "mcba_lm_result: grad_out must directly follow x_out (x_out + 12C + 6F): both arrive in one copy");
  int rc;
  if (!h->outbuf && (rc = dalloc(h, &h->outbuf, 2 * nx, false))) return rc;
  mcba::launch_pack_result(h->stream, h->x[slot], h->red + (size_t)h->n * h->n + 2 * (size_t)h->n, h->fbuf, h->have_fixed ? h->fixed : nullptr, h->outbuf, h->C, h->F, h->cw);
  if ((rc = check_launch())) return rc;
  HIPCHK(hipMemcpyAsync(x_out, h->outbuf, (grad_out ? 2 : 1) * nx * sizeof(double), hipMemcpyDeviceToHost, h->stream));  // (grad_out, if given, must directly follow x_out: one copy)
  HIPCHK(hipStreamSynchronize(h->stream));
  if (grad_dev) {   // the gradient stays on the device as an object of its own (OptimizeResult.grad is rarely read: 0.48 MB of D2H at 6 x 10 000 x 54)
    *grad_dev = new mcba_buffer{h->outbuf + nx, nx, h->device, h->stream, h->outbuf, 2 * nx};
    for (size_t i = 0; i < h->bufs.size(); ++i)
      if (h->bufs[i].slot == reinterpret_cast<void**>(&h->outbuf)) { h->bufs.erase(h->bufs.begin() + i); break; }
    h->outbuf = nullptr;
  }
  return MCBA_OK;
}

// device-resident loop: how often a back-substitution workgroup of k_solve_backsub gave up waiting for the solve (a bounded
// poll, ~0.5 s) since mcba_lm_auto_config, and whether the fused launch is still in use (the first such event switches the
// handle to the two-launch k_solve_cam + k_backsub path for good)
int mcba_lm_fuse_status(mcba_handle* h, double* timeouts, int* fused) {
  if (!h || !h->have_solver) return fail(MCBA_ERR_ARG, "mcba_lm_fuse_status: bad argument");
  if (timeouts) *timeouts = const_cast<volatile double*>(h->ring)[(size_t)kRing * MCBA_LMS];
  if (fused) *fused = h->fuse_backsub ? 1 : 0;
  return MCBA_OK;
}

int mcba_get_frame_gradient(mcba_handle* h, double* host) {
  if (!h || !host) return fail(MCBA_ERR_ARG, "mcba_get_frame_gradient: bad argument");
  if (!h->have_red) return fail(MCBA_ERR_ARG, "mcba_get_frame_gradient: call mcba_build_reduced first");
  HIPCHK(hipMemcpy2DAsync(host, 6 * sizeof(double), h->fbuf + 27, MCBA_FB * sizeof(double), 6 * sizeof(double), h->F, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return MCBA_OK;
}

}  // extern "C"
