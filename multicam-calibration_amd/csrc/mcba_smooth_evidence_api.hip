// mcba_smooth_evidence_api.hip -- the stateless evidence calls of include/mcba.h (host arrays in, host arrays out, a device
// ordinal, no handle), in the idiom of mcba_smooth_api.hip: tracks run in chunks under the same device-memory budget (SmoothChunks of
// mcba_smooth_host.h).  Per chunk the detections are uploaded and prepared once; per candidate accel_std the chunk gets its 1 / a^2
// (SmoothChunks::set_accel: the walk itself is given no accel_std), the smoother's elimination and back-substitution, the kernels of
// mcba_smooth_evidence.hip and one small download (four doubles per running track).  The search of mcba_estimate_accel_std is evidence_search
// of mcba_smooth_evidence_math.h, decided on the host between candidates.  A pooled call couples its tracks: it is one chunk and is refused,
// before anything is allocated, when it does not fit the budget.
#include "mcba_smooth_host.h"
#include "mcba_smooth_evidence_math.h"

using namespace mcba_internal;

namespace {

// one call's chunks and what a candidate needs on the device
struct EvidenceChunks {
  SmoothChunks ch;
  size_t T = 0;
  int nblk = 0;
  size_t lanes = 0;
  double *d_x = nullptr, *d_d2 = nullptr, *d_dx = nullptr, *d_w2 = nullptr, *d_part = nullptr, *d_lane = nullptr, *d_res = nullptr;
  double ms_logdet = 0.0;
  mcba::SmData td{}, tdb{};   // the elimination's and the evaluation's view (w = the weights given), the back-substitution's (w = a plane to overwrite)
  std::vector<double> h_res;

  int setup(const char* who, size_t T_, size_t K, int segment, const double* points, const double* cov6, const double* weights) {
    T = T_;
    if (int rc = ch.setup(who, T, K, segment, points, cov6, nullptr, weights, mcba::evidence_chunk_doubles(T, 1, segment), 6)) return rc;
    const size_t TK = T * ch.Kc;
    nblk = mcba::smooth_eval_blocks(T);
    lanes = mcba::evidence_lanes(ch.lv, mcba::smooth_plan(T, segment, ch.Kc, ch.lv));
    StatelessCall& call = ch.call;
    if (int rc = call.scratch(&d_x, 3 * TK)) return rc;
    if (int rc = call.scratch(&d_d2, TK)) return rc;
    if (int rc = call.scratch(&d_dx, TK)) return rc;
    if (int rc = call.scratch(&d_w2, TK)) return rc;
    if (int rc = call.scratch(&d_part, (size_t)2 * nblk * ch.Kc)) return rc;
    if (int rc = call.scratch(&d_lane, lanes * ch.Kc)) return rc;
    if (int rc = call.scratch(&d_res, (size_t)mcba::EV_RES * ch.Kc)) return rc;
    return MCBA_OK;
  }

  int begin(int c) {
    HIPCHK(hipMemset(d_x, 0, 3 * T * ch.tracks_of(c) * sizeof(double)));   // (the step against it is written and never used)
    if (int rc = ch.begin(c)) return rc;
    for (int l = 1; l < ch.levels; ++l) ch.lv[l].x = ch.aux[l];
    td = ch.td;
    td.x = d_x; td.d2 = d_d2; td.dx = d_dx;
    tdb = td;
    tdb.w = d_w2;   // (the back-substitution writes the next IRLS weights: not into the plane the next candidate's matrix is built from)
    if (!ch.h_list.empty())
      if (int rc = ch.call.put(ch.d_list, ch.h_list.data(), ch.h_list.size())) return rc;
    return MCBA_OK;
  }

  // one candidate of the chunk begin() left: a (kc, positive at every track) -> out4 (kc, 4) = N, data, penalty, log det; NaN for a track
  // that does not run or whose pivot was refused at this candidate (refused[k] = 1)
  int evaluate(const double* a, double* out4, int* refused) {
    const int kc = ch.kc, nact = (int)ch.h_list.size();
    const double nan = __builtin_nan("");
    for (int i = 0; i < 4 * kc; ++i) out4[i] = nan;
    for (int k = 0; k < kc; ++k) refused[k] = 0;
    if (nact == 0) return MCBA_OK;
    StatelessCall& call = ch.call;
    if (int rc = ch.set_accel(a)) return rc;
    if (int rc = ch.open(true)) return rc;
    if (mcba::launch_smooth_reduce(nullptr, ch.lv, ch.levels, td, kc, ch.d_list, nact, ch.d_bad) != 0) return fail(MCBA_ERR_ARG, "smoother evidence: bad launch");
    if (mcba::launch_smooth_backsub(nullptr, ch.lv, ch.levels, tdb, kc, ch.d_list, nact) != 0) return fail(MCBA_ERR_ARG, "smoother evidence: bad launch");
    if (mcba::launch_smooth_evidence(nullptr, ch.lv, ch.levels, td, kc, ch.d_list, nact, ch.d_bad, d_part, d_lane, d_res, call.e1) != 0) return fail(MCBA_ERR_ARG, "smoother evidence: bad launch");
    if (int rc = ch.close_split(ms_logdet)) return rc;   // (the mark: launch_smooth_evidence records e1 ahead of the log-determinant)
    h_res.resize((size_t)mcba::EV_RES * nact);
    if (int rc = call.download(h_res.data(), d_res, (size_t)mcba::EV_RES * nact)) return rc;
    for (int kk = 0; kk < nact; ++kk) {
      const int k = ch.h_list[kk];
      if (h_res[(size_t)mcba::EV_RES * kk + 3] != 0.0) { refused[k] = 1; continue; }
      mcba::evidence_terms(h_res.data() + (size_t)mcba::EV_RES * kk, T, a[k], ch.h_ia2[k], out4 + 4 * k);
    }
    return MCBA_OK;
  }

  // n_eval: the evaluations of one track, as the entry counts them
  void info(double* info8, double* kernel_ms, int n_eval) const {
    ch.info(info8, kernel_ms, ch.Kc, ch.nchunks, n_eval, (double)mcba::evidence_chunk_doubles(T, ch.Kc, ch.segment) * sizeof(double), ms_logdet);
  }
};

}  // namespace

extern "C" {

int mcba_smooth_evidence(size_t n_frames, int n_tracks, const double* points, const double* cov6, const double* accel_std, const double* weights, int segment, int device, double* out4,
                         int* status, int* n_usable, double* info8, double* kernel_ms) {
  const char* who = "mcba_smooth_evidence";
  if (n_frames < 1 || n_frames > ((size_t)1 << 31) || n_tracks < 1 || !points || !cov6 || !accel_std || !out4 || !status || !n_usable || !info8)
    return fail(MCBA_ERR_ARG, "mcba_smooth_evidence: 1 .. 2^31 frames, at least one track, non-NULL arrays (but weights) required");
  const size_t T = n_frames, K = (size_t)n_tracks;
  if (int rc = smooth_check_common(who, "weights", T, n_tracks, accel_std, weights, segment)) return rc;
  if (int rc = stateless_device(device, who)) return rc;
  if (segment == 0) segment = mcba::SM_SEGMENT_DEFAULT;

  EvidenceChunks ev;
  if (int rc = ev.setup(who, T, K, segment, points, cov6, weights)) return rc;
  std::vector<double> o4;
  std::vector<int> refused;
  for (int c = 0; c < ev.ch.nchunks; ++c) {
    if (int rc = ev.begin(c)) return rc;
    const int kc = ev.ch.kc;
    o4.resize((size_t)4 * kc); refused.resize(kc);
    if (int rc = ev.evaluate(accel_std + ev.ch.k0, o4.data(), refused.data())) return rc;
    for (int k = 0; k < kc; ++k) {
      status[ev.ch.k0 + k] = ev.ch.h_nus[k] < 2 ? mcba::SM_TOO_FEW_FRAMES : refused[k] ? mcba::SM_PIVOT : mcba::SM_OK;
      n_usable[ev.ch.k0 + k] = ev.ch.h_nus[k];
      for (int e = 0; e < 4; ++e) out4[4 * (ev.ch.k0 + k) + e] = o4[4 * k + e];
    }
  }
  ev.info(info8, kernel_ms, 1);
  return MCBA_OK;
}

int mcba_estimate_accel_std(size_t n_frames, int n_tracks, const double* points, const double* cov6, double accel_lo, double accel_hi, int n_grid, double rtol, const double* weights,
                            const int* pool, int segment, int device, double* out_accel, double* out_log_std, int* out_edge, int* status, int* n_usable, double* grid, double* n_grid_out,
                            double* n_best, int* n_evaluations, double* info8, double* kernel_ms) {
  const char* who = "mcba_estimate_accel_std";
  if (n_frames < 1 || n_frames > ((size_t)1 << 31) || n_tracks < 1 || !points || !cov6 || !out_accel || !out_log_std || !out_edge || !status || !n_usable || !grid || !n_grid_out || !n_best ||
      !n_evaluations || !info8)
    return fail(MCBA_ERR_ARG, "mcba_estimate_accel_std: 1 .. 2^31 frames, at least one track, non-NULL arrays (but weights and pool) required");
  if (n_frames < 3) return fail(MCBA_ERR_ARG, "mcba_estimate_accel_std: at least 3 frames required (with 2 the evidence does not depend on accel_std)");
  const double range[2] = {accel_lo, accel_hi};
  if (!(accel_lo < accel_hi)) return fail(MCBA_ERR_ARG, "mcba_estimate_accel_std: accel_range must be 0 < lo < hi");
  if (n_grid < mcba::EV_GRID_MIN) return fail(MCBA_ERR_ARG, "mcba_estimate_accel_std: n_grid >= 3");
  if (!(rtol >= mcba::EV_RTOL_MIN) || !(rtol < 1.0)) return fail(MCBA_ERR_ARG, "mcba_estimate_accel_std: rtol must lie in [1e-6, 1)");
  const size_t T = n_frames, K = (size_t)n_tracks;
  if (int rc = smooth_check_common(who, "weights", T, 2, range, nullptr, segment)) return rc;   // (the range as two values of accel_std)
  if (int rc = smooth_check_weights(who, "weights", weights, T * K)) return rc;
  if (pool)
    for (size_t k = 0; k < K; ++k)
      if (pool[k] < 0 || (size_t)pool[k] >= K) return fail(MCBA_ERR_ARG, "mcba_estimate_accel_std: pool labels must lie in 0 .. n_tracks - 1");
  const int seg = segment == 0 ? mcba::SM_SEGMENT_DEFAULT : segment;
  if (pool && (double)mcba::evidence_chunk_doubles(T, n_tracks, seg) * sizeof(double) > smooth_budget_bytes())
    return fail(MCBA_ERR_ARG, "mcba_estimate_accel_std: the call does not fit the device-memory budget MCBA_SMOOTH_BUDGET_MB (a pool couples the tracks: it cannot run in chunks)");
  if (int rc = stateless_device(device, who)) return rc;
  segment = seg;

  const int G = n_grid;
  const double nan = __builtin_nan("");
  EvidenceChunks ev;
  if (int rc = ev.setup(who, T, K, segment, points, cov6, weights)) return rc;
  mcba::evidence_grid(accel_lo, accel_hi, G, grid);
  *n_evaluations = mcba::evidence_evaluations(accel_lo, accel_hi, G, rtol);
  std::vector<double> a_k, o4, ng, ah, ls, nb;
  std::vector<int> refused, unit, ed, an;
  for (int c = 0; c < ev.ch.nchunks; ++c) {
    if (int rc = ev.begin(c)) return rc;
    const int kc = ev.ch.kc, nt = (int)ev.ch.h_list.size();
    const size_t k0 = ev.ch.k0;
    for (int k = 0; k < kc; ++k) {
      status[k0 + k] = ev.ch.h_nus[k] < 2 ? mcba::SM_TOO_FEW_FRAMES : mcba::SM_OK;
      n_usable[k0 + k] = ev.ch.h_nus[k];
      out_accel[k0 + k] = out_log_std[k0 + k] = n_best[k0 + k] = nan;
      out_edge[k0 + k] = 0;
      for (int g = 0; g < G; ++g) n_grid_out[(size_t)g * K + k0 + k] = nan;
    }
    if (nt == 0) continue;
    a_k.assign(kc, 1.0); o4.resize((size_t)4 * kc); refused.resize(kc);
    unit.resize(nt); ng.resize((size_t)G * nt); ah.resize(nt); ls.resize(nt); nb.resize(nt); ed.resize(nt); an.resize(nt);
    for (int i = 0; i < nt; ++i) unit[i] = pool ? pool[ev.ch.h_list[i]] : i;   // (a pooled call is one chunk: k0 = 0)
    auto eval = [&](const double* a, double* n) -> int {
      for (int i = 0; i < nt; ++i) a_k[ev.ch.h_list[i]] = a[i];
      if (int rc = ev.evaluate(a_k.data(), o4.data(), refused.data())) return rc;
      for (int i = 0; i < nt; ++i) n[i] = o4[4 * ev.ch.h_list[i]];
      return 0;
    };
    if (int rc = mcba::evidence_search(nt, unit.data(), pool ? (int)K : nt, accel_lo, accel_hi, G, rtol, eval, grid, ng.data(), ah.data(), ls.data(), nb.data(), ed.data(), an.data()))
      return rc;
    for (int i = 0; i < nt; ++i) {
      const size_t k = k0 + ev.ch.h_list[i];
      if (an[i]) status[k] = mcba::SM_PIVOT;
      out_accel[k] = ah[i]; out_log_std[k] = ls[i]; out_edge[k] = ed[i]; n_best[k] = an[i] ? nan : nb[i];
      for (int g = 0; g < G; ++g) n_grid_out[(size_t)g * K + k] = ng[(size_t)g * nt + i];
    }
  }
  ev.info(info8, kernel_ms, *n_evaluations);
  return MCBA_OK;
}

}  // extern "C"
