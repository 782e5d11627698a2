// mcba_api.hip -- the C ABI of include/mcba.h: handle life cycle and buffer pool, launch geometry, upload, parameters, cost / residuals /
// Jacobian, the host-driven LM step and the launches of its chain, x_scale / bounds / frozen coordinates, detached buffers, profiling.
// The device-resident LM loops are in mcba_lm_api.hip, the frame pre-filter in mcba_prefilter_api.hip, calibrate() in mcba_calib_api.hip, the
// stateless geometry calls in mcba_geom_api.hip, RCCL in mcba_comm_api.hip; what they share is in mcba_handle.h.
#include <map>
#include <mutex>

#include "mcba_handle.h"

namespace mcba_internal {

thread_local std::string g_err;

// ---- buffer pool.  hipMalloc / hipFree / hipHostMalloc are synchronising driver calls of 50-400 us each, and a
// bundle_adjust() call creates and destroys three handles of ~25 buffers: 4 ms of its 16 ms at 6 x 10 000 x 54 was hipFree alone.
// Freed buffers are parked here (per device, keyed by their exact size -- repeated calls ask for the same sizes) and handed out
// again; MCBA_POOL_MB caps what is parked (default 2048 MiB of the 288 GB -- other allocators of the process, torch's or RCCL's, cannot
// see parked memory --; 0 switches the pool off; pinned host memory: 256 MiB), mcba_pool_trim() returns everything to the driver, and
// so does an allocation of this library that the driver answers with out-of-memory, before it asks once more.  Re-use is safe without
// events: every kernel and copy of this library is enqueued on the handle's stream, so a buffer that goes to a handle on the SAME stream
// is ordered behind whatever its previous owner still had in flight (round 5: mcba_destroy no longer waits for the stream -- a handle
// was closed while the next stage's kernels were still running, and the host stood still for them); a buffer that goes to another
// stream, or back to the driver, waits for the stream it was parked with first.
struct ParkedBuf {
  void* p;
  hipStream_t stream;  // work enqueued on this stream may still read / write the buffer (busy) ...
  bool busy;           // ... or nothing can (the owner synchronised before parking it)
};
struct BufferPool {
  std::mutex mu;
  std::multimap<std::pair<int, size_t>, ParkedBuf> dev;     // (device, bytes) -> pointer + who may still be using it
  std::multimap<std::pair<unsigned, size_t>, void*> host;  // (hipHostMalloc flags, bytes) -> pointer
  size_t parked = 0, parked_host = 0;
  const size_t host_cap = (size_t)256 << 20;  // pinned host memory parked at most (state rings and staging buffers: a few hundred KB each)
  size_t cap() {
    static size_t c = [] { const char* e = getenv("MCBA_POOL_MB"); return (size_t)(e ? atoll(e) : 2048) << 20; }();
    return c;
  }
};
static BufferPool g_pool;

static void pool_release_all();
hipError_t pool_malloc(void** p, size_t bytes, int device, hipStream_t stream, bool any_stream) {
  {
    ParkedBuf got{nullptr, nullptr, false};
    {
      std::lock_guard<std::mutex> lk(g_pool.mu);
      auto it = g_pool.dev.find({device, bytes});
      if (it != g_pool.dev.end()) { got = it->second; g_pool.dev.erase(it); g_pool.parked -= bytes; }
    }
    if (got.p) {
      // (any_stream: the caller cannot say which stream will touch the buffer)
      if (got.busy && (any_stream || got.stream != stream)) (void)hipStreamSynchronize(got.stream);
      *p = got.p;
      return hipSuccess;
    }
  }
  hipError_t e = hipMalloc(p, bytes);
  if (e == hipErrorOutOfMemory) {  // what the pool has parked is memory too: give it back to the driver and ask once more
    (void)hipGetLastError();
    pool_release_all();
    e = hipMalloc(p, bytes);
  }
  return e;
}
void pool_free(void* p, size_t bytes, int device, hipStream_t stream, bool busy) {
  if (!p) return;
  {
    std::lock_guard<std::mutex> lk(g_pool.mu);
    if (g_pool.parked + bytes <= g_pool.cap()) { g_pool.dev.insert({{device, bytes}, ParkedBuf{p, stream, busy}}); g_pool.parked += bytes; return; }
  }
  if (busy) (void)hipStreamSynchronize(stream);
  (void)hipFree(p);
}
hipError_t pool_host_malloc(void** p, size_t bytes, unsigned flags) {
  {
    std::lock_guard<std::mutex> lk(g_pool.mu);
    auto it = g_pool.host.find({flags, bytes});
    if (it != g_pool.host.end()) { *p = it->second; g_pool.host.erase(it); g_pool.parked_host -= bytes; return hipSuccess; }
  }
  return hipHostMalloc(p, bytes, flags);
}
void pool_host_free(void* p, size_t bytes, unsigned flags) {
  if (!p) return;
  std::lock_guard<std::mutex> lk(g_pool.mu);
  if (g_pool.cap() == 0 || g_pool.parked_host + bytes > g_pool.host_cap) { (void)hipHostFree(p); return; }
  g_pool.host.insert({{flags, bytes}, p});
  g_pool.parked_host += bytes;
}
static void pool_release_all() {
  std::lock_guard<std::mutex> lk(g_pool.mu);
  int cur = 0;
  (void)hipGetDevice(&cur);
  for (auto& kv : g_pool.dev) { (void)hipSetDevice(kv.first.first); if (kv.second.busy) (void)hipStreamSynchronize(kv.second.stream); (void)hipFree(kv.second.p); }
  for (auto& kv : g_pool.host) (void)hipHostFree(kv.second);
  g_pool.dev.clear();
  g_pool.host.clear();
  g_pool.parked = g_pool.parked_host = 0;
  (void)hipSetDevice(cur);
}

// MCBA_POISON (tests): buffers that are handed out WITHOUT a zero fill are filled with a byte pattern instead -- 1: 0xFF (every double a NaN,
// every byte mask "set"); 2: 0x3F (finite garbage: every double 4.8e-4, every 32-bit count 1 061 109 567 -- what recycled pool memory looks
// like; NaN is the benign value for several of these buffers, e.g. the errors the median skips: ADVICE r5).  0 / unset: no fill.
int poison_byte() {
  static const int b = [] { const char* e = getenv("MCBA_POISON"); const int v = e ? atoi(e) : 0; return v == 1 ? 0xFF : (v == 2 ? 0x3F : 0); }();
  return b;
}

}  // namespace mcba_internal

using namespace mcba_internal;

// The tile-pair tables of k_syrk / k_reduce_system (pair p of the NT x NT tile grid's upper triangle -> (i, j)) depend on NT alone:
// uploaded once per (device, NT) and process, shared by every handle and never freed (at most a few KB each) -- so the first solver
// call of a handle neither copies nor synchronises for them.
static int tile_tables(int device, int NT, int** ti, int** tj) {
  static std::mutex mu;
  static std::map<std::pair<int, int>, std::pair<int*, int*>> cache;
  std::lock_guard<std::mutex> lk(mu);
  auto it = cache.find({device, NT});
  if (it == cache.end()) {
    std::vector<int> ci, cj;
    for (int a = 0; a < NT; ++a) for (int b = a; b < NT; ++b) { ci.push_back(a); cj.push_back(b); }
    int *di = nullptr, *dj = nullptr;
    HIPCHK(hipMalloc(reinterpret_cast<void**>(&di), ci.size() * sizeof(int)));
    HIPCHK(hipMalloc(reinterpret_cast<void**>(&dj), cj.size() * sizeof(int)));
    HIPCHK(hipMemcpy(di, ci.data(), ci.size() * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dj, cj.data(), cj.size() * sizeof(int), hipMemcpyHostToDevice));
    it = cache.insert({{device, NT}, {di, dj}}).first;
  }
  *ti = it->second.first;
  *tj = it->second.second;
  return MCBA_OK;
}

// Launch geometry of the solver kernels, derived from the problem's shape, the device and the camera block width (h->cw): called by
// mcba_create and again by mcba_set_camera_block.
static int derive_geometry(mcba_handle* h) {
  const int C = h->C, F = h->F, N = h->N, device = h->device;
  const int ncu = h->ncu, slots = 4 * h->ncu;  // wavefront slots at one wavefront per SIMD: where k_gram's launch variants cut this shard into rounds
  h->n = h->cw * C;
  h->nsys = (size_t)h->n * h->n + 3 * h->n + 16;
  if (h->sparse) {
    // sparse-Schur handle: no k_syrk tile grid and no one-workgroup solve; the frame factors run one workgroup per 64 frames (fpart pairs)
    h->NT = h->NP = h->G = h->sq = h->sr = 0;
    h->FS = 0;
    h->ppw = 4;
  } else {
  // k_syrk geometry: (12C + 1) rows of [Y ; z^T] padded to NT tiles of 16, NP tile pairs (ti <= tj);
  // FS frames per LDS stage (a divisor of 64; <= 96 KiB so that two workgroups fit a CU when C is small)
  h->NT = (h->n + 1 + 15) / 16;
  h->NP = h->NT * (h->NT + 1) / 2;
  h->ppw = h->NP <= 64 ? 4 : 16;
  h->FS = 8;  // (measured at 6 x 10k: 8 frames per stage and up to 512 workgroups -- two per CU, one building Y while the
              //  other is in its MFMA phase -- 24.2 us; 16 frames / 256 workgroups 27.4 us)
  while (h->FS > 2 && (mcba::syrk_lds_bytes(C, h->FS, h->cw) > (size_t)h->lds_optin * 3 / 5 || (h->n + 1) * h->FS > 256 * mcba::syrk_items_per_thread())) h->FS /= 2;
  if ((h->n + 1) * h->FS > 256 * mcba::syrk_items_per_thread()) { return fail(MCBA_ERR_ARG, "too many cameras for k_syrk's per-thread item budget"); }
  if (mcba::syrk_lds_bytes(C, h->FS, h->cw) > (size_t)h->lds_optin) { return fail(MCBA_ERR_ARG, "too many cameras for the LDS staging of k_syrk"); }
  {
    int nstage = (F + h->FS - 1) / h->FS;
    // the 16-tile variant (> 13 cameras) runs ONE workgroup per CU and grid.y = ceil(NP / 64) of them share a set of frames:
    // one round of the 256 CUs, every workgroup as many stages as that allows -- 24 x 6250 x 200: 83 x 3 workgroups of 19 stages
    // 776 us per tick (33 MB of partial tiles) against 839 us for 391 x 3 of 4 stages (152 MB), 806 / 796 / 822 / 809 / 874 us
    // for G = 256 / 171 / 128 / 64 / 43
    int gmax = h->ppw == 4 ? std::min(512, 2 * ncu) : std::max(1, ncu / ((h->NP + 63) / 64));
    int g = std::min(nstage, gmax);
    // Two workgroups per CU (ppw == 4: <= 10 cameras): deal the stages out evenly over g workgroups -- measured at 6 x 10 000:
    // 1250 stages as 226 x 3 + 286 x 2 (no CU above five stages) 107.5 us per tick against 109.0 us for 417 x 3 (161 CUs with six).
    // One workgroup per CU (the 16-tile variant): every workgroup costs a prologue of its own, fewer and equal ones win
    // (24 x 6250 x 200: 873 us against 918 us).
    if (h->ppw == 4) {
      h->G = g;
      h->sq = nstage / g;
      h->sr = nstage % g;
    } else {
      h->sq = (nstage + g - 1) / g;
      h->sr = 0;
      h->G = (nstage + h->sq - 1) / h->sq;
    }
  }
  }
  h->nbblocks = h->Fpad / 64;
  // k_gram: which launches linearise this shard is a pure function of its shape (mcba_gram_plan.h); what the device and the
  // environment have to say about it is gathered here
  {
    static bool ps_ready[64] = {};  // the dynamic-LDS limit of the point split's instances is raised once per device
    static std::mutex ps_mu;        // (handles may be created from several threads: solver.InProcessShards)
    bool ps_ok = (size_t)h->lds_optin >= mcba::kGramPsplitLdsMax + 2048;
    {
      std::lock_guard<std::mutex> lk(ps_mu);
      if (ps_ok && !ps_ready[device & 63]) { ps_ok = mcba::gram_psplit_set_lds_limit() == 0; ps_ready[device & 63] = ps_ok; (void)hipGetLastError(); }
    }
    mcba::GramShape shape{C, h->nfb, N, slots, h->cw, ps_ok, -1, -1};
    // tuning knobs: 0 fused, 1 split roles, 2 fused + split-role tail, 3 fused + point-chunk tail, 4 point split, 5 fused + point-split tail
    if (const char* e = getenv("MCBA_GRAM_SPLIT")) shape.force_split = std::max(0, std::min(5, atoi(e)));
    if (const char* e = getenv("MCBA_GRAM_NPW")) shape.force_npw = atoi(e) == 2 ? 2 : 4;
    h->gram = mcba::gram_plan(shape);
    if (h->gram.refused) { return fail(MCBA_ERR_ARG, "MCBA_GRAM_SPLIT=4/5: this device cannot give k_gram_psplit its LDS"); }
  }
  // k_cost: split the board points so that ~4 waves per SIMD (1024 SIMDs) are in flight
  h->nch = std::max(1, std::min(std::min(8, N / 8), (4 * slots + C * h->nfb - 1) / (C * h->nfb)));
  h->nfblocks = h->G;  // (kept: k_syrk's workgroups factorise their own frames: one (max |g_f|, #failures) pair each)
  h->npad = 16 * h->NT;
  h->solve_lds = mcba::solve_fits_lds(h->npad, h->lds_optin);
  if (h->sparse) {
    h->nfblocks = h->nfb;
    h->npad = mcba::sp_npad(h->n);
    h->solve_lds = 0;
  }
  return MCBA_OK;
}

static int compose_dscale(mcba_handle* h) {
  // what the XS kernel instances read per parameter (csrc/mcba_kernels.hip: k_syrk's frame factor): > 0 the caller's fixed D = 1 / x_scale^2,
  // 0 Marquardt's diag(J^T J), < 0 frozen (frame coordinates only: frozen CAMERA parameters are flags of the camera system -- mcba_lm_auto_config,
  // or rows the host solve leaves out)
  const bool any_frozen = !h->frozen_host.empty();
  h->have_red = false;
  if (h->xs_host.empty() && !any_frozen) { h->have_xscale = false; return MCBA_OK; }
  std::vector<double> d(h->nx, 0.0);
  const size_t cnt = (size_t)12 * h->C + (size_t)6 * h->F, ncam = (size_t)12 * h->C;
  for (size_t i = 0; i < cnt; ++i) {
    d[i] = h->xs_host.empty() ? 0.0 : h->xs_host[i];
    if (any_frozen && i >= ncam && h->frozen_host[i]) d[i] = -1.0;
  }
  HIPCHK(hipMemcpyAsync(h->dscale, d.data(), h->nx * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  h->have_xscale = true;
  return MCBA_OK;
}

static int ensure_res(mcba_handle* h) {
  if (!h->res) return dalloc(h, &h->res, (size_t)2 * h->C * h->F * h->N, false);
  return MCBA_OK;
}


namespace mcba_internal {

// Solver buffers, allocated on first use (linearise / reduce / LM entry points): records, partial sums, reduce buffer, the host-
// mapped state ring.  A handle that only runs the pre-filter (api.select_frames over ALL frames of a long recording) never gets
// here, so its footprint is the observations alone.
int ensure_solver(mcba_handle* h) {
  if (h->have_solver) return MCBA_OK;
  const int C = h->C;
  int rc;
  // ONE device allocation for the whole set (round 5: sixteen pool look-ups and sixteen fill launches -- ~50 us of host time and as
  // much of the stream in front of the first linearisation -- became one of each), cut into 256-byte aligned pieces.  The pieces a
  // kernel overwrites completely before anything reads them (linearisation records, k_syrk's partial tiles, the point-chunk scratch:
  // 110 of the 116 MB at 6 x 10 000 x 54) sit behind the ones that start from zero and are not filled.
  if (!h->solver_arena) {
    struct Piece { double** p; size_t count; };
    size_t n_swork = h->solve_lds ? 16 : 2 * (size_t)h->npad * h->npad + 64 * (size_t)h->npad;  // two sets of 16 x 16 tiles of the lower triangle (mcba_solve.hip, right-looking variant)
    if (h->sparse) n_swork = (size_t)h->npad * h->npad;   // the blocked solve's matrix (mcba_sparse.hip)
    Piece zeroed[] = {{&h->gpart2[0], (size_t)C * h->nfb * MCBA_GP}, {&h->gpart2[1], (size_t)C * h->nfb * MCBA_GP}, {&h->fbuf, (size_t)h->Fpad * MCBA_FB}, {&h->fpart, (size_t)2 * h->nfblocks},
                      {&h->cpart, (size_t)2 * C * h->nfb * h->nch}, {&h->bpart, (size_t)3 * h->nbblocks}, {&h->red_own, h->nsys + 8 + 2 * MCBA_LMS},
                      {&h->dcbuf, (size_t)h->n + 8},  // + the word k_solve_backsub's solve releases, + the poll-timeout stamp
                      {&h->swork, n_swork}, {&h->dscale, h->nx}, {reinterpret_cast<double**>(&h->fixed), ((size_t)h->n + 7) / 8},
                      {&h->sp_damp, h->sparse ? (size_t)h->npad : 0}, {&h->sp_y, h->sparse ? (size_t)h->npad : 0}, {reinterpret_cast<double**>(&h->sp_ctl), h->sparse ? (size_t)1 : 0}};
    Piece plain[] = {{&h->rec2[0], (size_t)h->Fpad * C * MCBA_REC}, {&h->rec2[1], (size_t)h->Fpad * C * MCBA_REC},
                     {&h->spart, (size_t)h->G * h->NP * 256 + 64},
                     {&h->gchunk, h->gram.chunk_doubles()}};
    auto padded = [](size_t count) { return (std::max<size_t>(count, 1) * sizeof(double) + 255) / 256 * 256; };
    size_t zero_bytes = 0, total = 0;
    for (auto& pc : zeroed) if (pc.count) zero_bytes += padded(pc.count);   // (the sparse-Schur pieces have count 0 on a dense handle: no bytes)
    total = zero_bytes;
    for (auto& pc : plain) if (pc.count) total += padded(pc.count);
    if ((rc = dalloc(h, &h->solver_arena, total, false)) != MCBA_OK) return rc;
    HIPCHK(hipMemsetAsync(h->solver_arena, 0, zero_bytes, h->stream));
    if (poison_byte()) HIPCHK(hipMemsetAsync(h->solver_arena + zero_bytes, poison_byte(), total - zero_bytes, h->stream));
    size_t off = 0;
    for (auto& pc : zeroed) if (pc.count) { *pc.p = reinterpret_cast<double*>(h->solver_arena + off); off += padded(pc.count); }
    for (auto& pc : plain) if (pc.count) { *pc.p = reinterpret_cast<double*>(h->solver_arena + off); off += padded(pc.count); }
  }
  if (h->sparse) {
    h->sp_A = h->swork;
  } else if (mcba::solve_set_lds_limit(h->npad, h->solve_lds) != 0) return fail(MCBA_ERR_HIP, "cannot raise the dynamic LDS limit of k_solve_cam");
  h->fuse_backsub = h->solve_lds != 0;
  if (const char* e = getenv("MCBA_FUSE_BACKSUB")) h->fuse_backsub = h->fuse_backsub && atoi(e) != 0;  // tuning knob
  // (a part whose LDS limit cannot be raised keeps the two-launch k_solve_cam + k_backsub path instead of failing)
  if (h->fuse_backsub && mcba::solve_backsub_set_lds_limit(h->npad, h->cw) != 0) h->fuse_backsub = false;
  h->fuse_max_polls = 200000;
  if (const char* e = getenv("MCBA_FUSE_MAX_POLLS")) h->fuse_max_polls = std::max(0, atoi(e));  // test knob: 0 forces every poll to time out
  if (!h->ring) {
    h->ring_bytes = ((size_t)kRing * MCBA_LMS + 8) * sizeof(double);  // + the poll-timeout counter the GPU bumps
    h->ring_flags = hipHostMallocMapped | hipHostMallocCoherent;
    hipError_t e = pool_host_malloc(reinterpret_cast<void**>(&h->ring), h->ring_bytes, h->ring_flags);
    if (e != hipSuccess) { (void)hipGetLastError(); h->ring_flags = hipHostMallocDefault; e = pool_host_malloc(reinterpret_cast<void**>(&h->ring), h->ring_bytes, h->ring_flags); }
    if (e != hipSuccess) return fail(MCBA_ERR_HIP, "cannot allocate the host-mapped LM state ring");
    memset(h->ring, 0, h->ring_bytes);
    if (hipHostGetDevicePointer(reinterpret_cast<void**>(&h->ring_dev), h->ring, 0) != hipSuccess) return fail(MCBA_ERR_HIP, "hipHostGetDevicePointer failed for the LM state ring");
  }
  h->red = h->red_own;
  if (!h->sparse && (rc = tile_tables(h->device, h->NT, &h->tile_i, &h->tile_j)) != MCBA_OK) return rc;
  if (!h->pinned) {
    h->pinned_bytes = (h->nsys + 8 + MCBA_LMS + h->n) * sizeof(double);
    HIPCHK(pool_host_malloc(reinterpret_cast<void**>(&h->pinned), h->pinned_bytes, hipHostMallocDefault));
  }
  size_t lds = h->sparse ? 0 : mcba::syrk_lds_bytes(C, h->FS, h->cw);
  if (lds > 64 * 1024) {
    if (mcba::syrk_set_lds_limit(lds) != 0) return fail(MCBA_ERR_HIP, "cannot raise the dynamic LDS limit of k_syrk");
  }
  h->have_solver = true;
  // a numeric x_scale / a frozen set given before an mcba_trim are still the caller's: put them back into the new buffers
  if (!h->xs_host.empty() || !h->frozen_host.empty()) return compose_dscale(h);
  return MCBA_OK;
}
int upload_impl(mcba_handle* h, const double* uvs, const double* objpoints, bool sync) {
  size_t raw_count = (size_t)2 * h->C * h->F * h->N;
  // both layouts live in HBM: raw (C,F,N) for k_jacobian (lane = point), [C][N][Fpad] for k_gram / k_cost (lane = frame)
  hipError_t e = hipMemcpyAsync(h->obs_raw, uvs, raw_count * sizeof(double), hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess && !mcba::launch_store_small(h->stream, h->obj, objpoints, (size_t)3 * h->N))   // (boards of up to 160 points: through the kernel arguments)
    e = hipMemcpyAsync(h->obj, objpoints, (size_t)3 * h->N * sizeof(double), hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) {
    Scope sc(h, K_TRANSPOSE);
    mcba::launch_transpose_obs(h->stream, h->obs_raw, h->obs_t, h->C, h->F, h->N, h->Fpad);
  }
  if (e == hipSuccess) e = hipGetLastError();
  // (the sources are pageable host memory: the copies are staged / done when the calls return; callers that go on enqueueing need no wait)
  hipError_t e2 = sync ? hipStreamSynchronize(h->stream) : hipSuccess;
  if (e != hipSuccess || e2 != hipSuccess) { g_err = std::string("upload: ") + hipGetErrorString(e != hipSuccess ? e : e2); return MCBA_ERR_HIP; }
  if (!h->obj_host) h->obj_host = static_cast<double*>(malloc((size_t)3 * h->N * sizeof(double)));
  if (h->obj_host) memcpy(h->obj_host, objpoints, (size_t)3 * h->N * sizeof(double));
  h->planar = 1;
  for (int p = 0; p < h->N; ++p) if (objpoints[3 * p + 2] != 0.0) h->planar = 0;
  if (const char* e = getenv("MCBA_GRAM_FAST")) { if (atoi(e) == 0) h->planar = 0; }  // development knob: the general instance
  h->have_obs = true;
  h->have_lin = h->have_red = h->have_jac = false;
  h->sp_ready = false;
  return MCBA_OK;
}

// ---- the solver chain's launches, shared by the host-driven entry points here and the device-resident loops (mcba_lm_api.hip)
int gram_launch(mcba_handle* h, mcba::Sel sel, const double* xa, const double* xb, int la, int lb) {
  sel.cfl = h->curv_floor;   // (a linearisation's selector carries the curvature floor this handle linearises with: mcba_set_curvature_floor)
  { Scope sc(h, K_GRAM); mcba::launch_gram(h->stream, h->loss, h->f_scale, h->obs_t, h->obj, sel, xa, xb, h->rec2[la], h->rec2[lb], h->gpart2[la], h->gpart2[lb], h->C, h->N, h->Fpad, h->gram, h->planar, h->gchunk, h->loss_tab); }
  return check_launch();
}

int trial_sum(mcba_handle* h, mcba::Sel sel, int la, int lb, const mcba::DecideArgs& da) {
  { Scope sc(h, K_SUM_TRIAL); mcba::launch_sum_trial(h->stream, sel, h->gpart2[la] + (size_t)90 * h->nfb, h->gpart2[lb] + (size_t)90 * h->nfb, 1, h->nfb, (size_t)MCBA_GP * h->nfb, h->C * h->nfb, h->bpart, h->nbblocks, h->red + h->nsys, da); }
  return check_launch();
}

int backsub_launch(mcba_handle* h, mcba::Sel sel, int la, int lb, int xa, int xb, const double* delta_cam) {
  if (h->sparse && delta_cam) {  // (a camera step of more than 480 doubles does not fit the kernel arguments: it goes to the device buffer first)
    HIPCHK(hipMemcpyAsync(h->dcbuf, delta_cam, (size_t)h->n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    delta_cam = nullptr;
  }
  mcba::CamStep cs;
  if (delta_cam) memcpy(cs.v, delta_cam, h->n * sizeof(double));
  {
    Scope sc(h, K_BACKSUB);
    if (delta_cam) mcba::launch_backsub(h->stream, sel, h->rec2[la], h->rec2[lb], h->fbuf, cs, h->x[xa], h->x[xb], h->bpart, h->C, h->F, h->Fpad, h->cw);
    else mcba::launch_backsub_dev(h->stream, sel, h->rec2[la], h->rec2[lb], h->fbuf, h->dcbuf, h->x[xa], h->x[xb], h->bpart, h->C, h->F, h->Fpad, h->cw);
  }
  return check_launch();
}

int syrk_launch(mcba_handle* h, mcba::Sel sel, const mcba::SyrkFuse& fz) {
  if (h->sparse) {
    if (fz.decide) return fail(MCBA_ERR_ARG, "sparse-Schur handle: the decision is not fused into the Schur reduction");
    return sparse_build(h, sel);
  }
  { Scope sc(h, K_SYRK); mcba::launch_syrk(h->stream, sel, fz, h->rec2[0], h->rec2[1], h->fbuf, h->fpart, h->tile_i, h->tile_j, h->spart, h->C, h->F, h->Fpad, h->NT, h->NP, h->G, h->sq, h->sr, h->FS, h->ppw, h->have_xscale ? h->dscale : nullptr, h->cw); }
  return check_launch();
}

int reduce_launch(mcba_handle* h, mcba::Sel sel, int rank_slot, bool spec) {
  {
    Scope sc(h, K_REDUCE);
    // (sparse-Schur handle: NP = 0 -- S0 and rhs were assembled by k_sp_assemble; this launch is the tail: diag U, g_c, the scalars)
    mcba::launch_reduce_system(h->stream, sel, h->gpart2[0], h->gpart2[1], h->spart, h->fpart, h->tile_i, h->tile_j, h->red, h->C, h->nfb, h->G, h->NT, h->NP, h->nfblocks, rank_slot,
                               spec ? h->bpart : nullptr, h->nbblocks, spec ? post_state(h) : nullptr, h->cw, spec ? timeout_word(h) : nullptr, (double)h->last_solve_seq);
  }
  return check_launch();
}

}  // namespace mcba_internal

extern "C" {

int mcba_abi_version(void) { return 7; }  // 7 (round 6): calibrate() on the device (mcba_calib_*, mcba_pose_*, mcba_create_views); 6 (round 5): mcba_prefilter, mcba_lm_run / _history / _result -- whole stages of bundle_adjust() per crossing; additions only: every ABI-5 entry point is unchanged
const char* mcba_last_error(void) { return g_err.c_str(); }
const char* mcba_profile_names(void) { return kKernelNames; }

int mcba_device_count(int* count) {
  if (!count) return fail(MCBA_ERR_ARG, "count is NULL");
  hipError_t e = hipGetDeviceCount(count);
  if (e != hipSuccess) { *count = 0; g_err = hipGetErrorString(e); return MCBA_ERR_NODEVICE; }
  return MCBA_OK;
}

}  // extern "C"

namespace mcba_internal {
int create_impl(mcba_handle** out, int C, int F, int N, int device, bool sparse) {
  const char* who = sparse ? "mcba_create_sparse" : "mcba_create";
  if (!out || C < 1 || F < 1 || N < 1) { g_err = std::string(who) + ": need cameras >= 1, frames >= 1, points >= 1"; return MCBA_ERR_ARG; }
  if (!sparse && C > 40) {
    g_err = "mcba_create: " + std::to_string(C) + " cameras -- this build handles at most 40 per handle: the (12 C + 1)-row reduced camera system is factorised by ONE workgroup "
            "(k_solve_cam: tile tables, LDS and scratch are sized for 481 rows) and k_backsub takes the camera step through the kernel arguments (480 doubles); reduced_solver=\"host\" does not "
            "lift it (the Schur product's tile grid has the same bound).  The reference has no such limit (scipy's sparse LSMR); the sparse-Schur handle (mcba_create_sparse; ops.Problem(..., schur=\"sparse\"), bundle_adjust's default above 40 cameras) has none";
    return MCBA_ERR_ARG;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(MCBA_ERR_NODEVICE, "no HIP device visible");
  if (device < 0 || device >= ndev) return fail(MCBA_ERR_ARG, "device ordinal out of range");
  HIPCHK(hipSetDevice(device));
  mcba_handle* h = new mcba_handle();
  h->C = C; h->F = F; h->N = N; h->device = device;
  h->sparse = sparse;
  h->speculate = !sparse;   // (the sparse handle's frame-sharded ticks take two collectives: no speculative reduction)
  {  // the launch geometry below is derived from the device, not from MI355X constants (a part with fewer CUs or less LDS gets its own deal)
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) {
      if (prop.multiProcessorCount > 0) h->ncu = prop.multiProcessorCount;
      if (prop.sharedMemPerBlockOptin > 0) h->lds_optin = (int)std::min<size_t>(prop.sharedMemPerBlockOptin, 160 * 1024);
    }
  }
  if (const char* e = getenv("MCBA_STRICT_SYNC")) h->strict_sync = atoi(e) != 0;
  h->Fpad = (F + 63) / 64 * 64;
  h->nfb = h->Fpad / 64;
  h->nx = (size_t)12 * C + (size_t)6 * h->Fpad;
  {
    const int grc = derive_geometry(h);
    if (grc != MCBA_OK) { delete h; return grc; }
  }
  int rc;
#define DA(p, cnt, zero) if ((rc = dalloc(h, &h->p, (cnt), zero)) != MCBA_OK) { mcba_destroy(h); return rc; }
  // what every handle needs (a pre-filter handle needs nothing else): the two observation layouts, the board, the parameter slots
  DA(obs_t, (size_t)2 * C * N * h->Fpad, false);
  DA(obs_raw, (size_t)2 * C * F * N, false);
  {  // the two parameter slots and the board: one allocation, one fill (zero: the poses of the padding frames must be finite)
    const size_t nxp = (h->nx + 31) / 32 * 32;
    DA(core_arena, 2 * nxp + (size_t)3 * N, true);
    h->x[0] = h->core_arena; h->x[1] = h->core_arena + nxp; h->obj = h->core_arena + 2 * nxp;
  }
#undef DA
  // (no synchronisation: the zero fills above are ordered before everything else on this stream, and mcba_set_stream waits for the old stream when it changes it)
  *out = h;
  return MCBA_OK;
}
}  // namespace mcba_internal

extern "C" {

int mcba_create(mcba_handle** out, int C, int F, int N, int device) { return create_impl(out, C, F, N, device, false); }

// The sparse-Schur handle: any number of cameras.  Every entry point of the dense handle that bundle_adjust() reaches works on it; the Schur
// reduction runs over co-visible camera pairs (mcba_sparse.hip) and the reduced system is factorised by a sequence of multi-workgroup launches.
int mcba_create_sparse(mcba_handle** out, int C, int F, int N, int device) { return create_impl(out, C, F, N, device, true); }
int mcba_is_sparse(const mcba_handle* h) { return h && h->sparse ? 1 : 0; }

int mcba_destroy(mcba_handle* h) {
  if (!h) return MCBA_OK;
  (void)hipSetDevice(h->device);
  // Device buffers are parked as "busy on h->stream" and NOT waited for (a later owner on the same stream is ordered behind whatever is
  // still in flight; pool_malloc waits for anybody else).  What the GPU writes into HOST memory must be quiet, though: the state ring
  // (ticks that were enqueued but never waited for), profiling events, an RCCL communicator -- then the stream is waited for as before.
  const bool quiet = h->last_solve_seq == h->waited_seq && h->evs.empty() && !h->comm && !h->prof;
  if (!quiet) (void)hipStreamSynchronize(h->stream);
  if (h->comm && g_rccl.ok) { g_rccl.CommDestroy(h->comm); h->comm = nullptr; }
  for (auto& b : h->bufs) { pool_free(*b.slot, b.bytes, h->device, h->stream, quiet); *b.slot = nullptr; }
  free(h->obj_host);
  pool_host_free(h->pinned, h->pinned_bytes, hipHostMallocDefault);
  pool_host_free(h->ring, h->ring_bytes, h->ring_flags);
  pool_host_free(h->pf_host, h->pf_host_bytes, hipHostMallocDefault);
  for (auto& e : h->evs) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
  for (auto& e : h->pool) (void)hipEventDestroy(e);
  delete h;
  return MCBA_OK;
}

// Device memory a handle holds right now (bytes of its pooled buffers): what a caller that parks handles (api.py: the lazily attached
// result.jac) accounts for.
size_t mcba_device_bytes(const mcba_handle* h) {
  size_t tot = 0;
  if (h) for (auto& b : h->bufs) tot += b.bytes;
  return tot;
}

// Gives back (to the pool) every device buffer except what defines the problem: the observations in both layouts, the board, the two
// parameter slots (and a subset's index list).  Solver buffers (116 MB at 6 x 10 000 x 54), pre-filter scores, Jacobian / residual blocks
// go; the next call that needs them allocates them again.  For a handle that is kept only so that a Jacobian can be produced from it
// later: 0.26 GB -> 0.11 GB at that size.  Synchronises.
int mcba_trim(mcba_handle* h) {
  if (!h) return fail(MCBA_ERR_ARG, "NULL handle");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize(h->stream));
  // (the box of mcba_set_bounds stays as well: it is part of what defines the problem, and the steps after a trim must still be projected onto it)
  void** keep[] = {reinterpret_cast<void**>(&h->obs_t), reinterpret_cast<void**>(&h->obs_raw), reinterpret_cast<void**>(&h->core_arena), reinterpret_cast<void**>(&h->sub_frames),
                   reinterpret_cast<void**>(&h->blo), reinterpret_cast<void**>(&h->bhi)};
  std::vector<DevBuf> kept;
  for (auto& b : h->bufs) {
    bool k = false;
    for (void** s : keep) k = k || b.slot == s;
    if (k) { kept.push_back(b); continue; }
    pool_free(*b.slot, b.bytes, h->device);
    *b.slot = nullptr;
  }
  h->bufs.swap(kept);
  // the pieces of the solver arena
  h->rec2[0] = h->rec2[1] = h->gpart2[0] = h->gpart2[1] = h->fbuf = h->fpart = h->spart = h->cpart = h->bpart = h->red_own = h->red = h->dcbuf = h->swork = h->dscale = h->gchunk = nullptr;
  h->fixed = nullptr;
  sparse_forget(h);
  h->cal_out_cap = h->cal_rel_cap = h->cal_sel_cap = h->cal_views_cap = 0;
  h->have_cal_poses = false;
  h->have_solver = h->have_lin = h->have_red = h->have_spec = h->have_jac = h->auto_ready = h->have_xscale = h->have_fixed = h->trial_ready = false;
  return MCBA_OK;
}

// The observations as the handle holds them ((C,F,N,2), what was uploaded or gathered), back to the host: a caller that must let go of a
// parked handle keeps the VALUES the solve saw (api.py: a released result.jac re-creates its handle from them, not from the caller's
// array, which may have changed since).
int mcba_download_observations(mcba_handle* h, double* uvs) {
  if (!h || !uvs) return fail(MCBA_ERR_ARG, "mcba_download_observations: bad argument");
  if (!h->have_obs) return fail(MCBA_ERR_ARG, "mcba_download_observations: no observations");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipMemcpyAsync(uvs, h->obs_raw, (size_t)2 * h->C * h->F * h->N * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return MCBA_OK;
}

int mcba_pool_trim(void) {
  pool_release_all();
  return MCBA_OK;
}

int mcba_set_stream(mcba_handle* h, void* s) {
  if (!h) return fail(MCBA_ERR_ARG, "NULL handle");
  if (h->stream != reinterpret_cast<hipStream_t>(s)) HIPCHK(hipStreamSynchronize(h->stream));  // work (and zero fills) enqueued so far
  h->stream = reinterpret_cast<hipStream_t>(s);
  return MCBA_OK;
}

int mcba_synchronize(mcba_handle* h) {
  if (!h) return fail(MCBA_ERR_ARG, "NULL handle");
  HIPCHK(hipStreamSynchronize(h->stream));
  return MCBA_OK;
}

int mcba_upload_observations(mcba_handle* h, const double* uvs, const double* objpoints) {
  if (!h || !uvs || !objpoints) return fail(MCBA_ERR_ARG, "mcba_upload_observations: NULL argument");
  HIPCHK(hipSetDevice(h->device));
  return upload_impl(h, uvs, objpoints, true);
}

int mcba_set_loss(mcba_handle* h, int loss, double f_scale) {
  if (!h || loss < 0 || loss > 4 || !(f_scale > 0.0)) return fail(MCBA_ERR_ARG, "mcba_set_loss: loss in 0..4 and f_scale > 0 required");
  h->loss = loss; h->f_scale = f_scale;
  h->have_lin = h->have_red = false;
  return MCBA_OK;
}

// least_squares' CALLABLE `loss` (least_squares.py:160-227: rho(z) -> (rho, rho', rho''); the reference forwards it untouched,
// bundle_adjustment.py:301-313): the function is the caller's, so its values are -- tab3 = three (C,F,N,2) arrays in the order of the
// observations, evaluated by the caller at the residuals of the point it is about to linearise:
//   [0] this scalar's share of the cost, 0.5 f_scale^2 rho(z)      [1] rho'(z)      [2] scipy's J_scale^2 = max(rho' + 2 rho'' z, EPS)
// (entries of missing observations are ignored).  From this call on the handle's loss is MCBA_LOSS_TABLE: mcba_linearize builds the normal
// equations with these weights (k_gram_table), the trial cost of mcba_step is NOT evaluated with it (the caller evaluates its function
// on mcba_residuals of the trial point), mcba_jacobian_eval returns unscaled rows, and the device-resident loops refuse to run -- the host
// must call the function between a step and the next linearisation.  mcba_set_loss with one of the five names switches back.
int mcba_set_loss_table(mcba_handle* h, const double* tab3) {
  if (!h || !tab3) return fail(MCBA_ERR_ARG, "mcba_set_loss_table: NULL argument");
  if (!h->have_obs) return fail(MCBA_ERR_ARG, "mcba_set_loss_table: upload observations first");
  HIPCHK(hipSetDevice(h->device));
  int rc = ensure_res(h);
  if (rc) return rc;
  const size_t raw = (size_t)2 * h->C * h->F * h->N, plane = (size_t)2 * h->C * h->N * h->Fpad;
  if (!h->loss_tab && (rc = dalloc(h, &h->loss_tab, 3 * plane, false))) return rc;
  for (int k = 0; k < 3; ++k) {   // through the residual buffer as staging (the stream orders copy -> re-layout -> next copy)
    HIPCHK(hipMemcpyAsync(h->res, tab3 + k * raw, raw * sizeof(double), hipMemcpyHostToDevice, h->stream));
    mcba::launch_transpose_obs(h->stream, h->res, h->loss_tab + k * plane, h->C, h->F, h->N, h->Fpad);
  }
  if ((rc = check_launch())) return rc;
  HIPCHK(hipStreamSynchronize(h->stream));   // (tab3 is the caller's pageable memory)
  h->loss = mcba::LOSS_TABLE;
  h->f_scale = 1.0;   // (folded into the table by the caller)
  h->have_lin = h->have_red = false;
  return MCBA_OK;
}

// Camera block width: 12 (every camera parameter is a variable: the reference, bundle_adjustment.py:149-155) or 6 = the intrinsics
// (fx fy cx cy k1 k2) of EVERY camera are held fixed -- BASELINE configs[1]; SURVEY section 8c-8's wrapper around the reference's
// residuals().  With 6 the solver kernels run role A of the linearisation alone, the camera system is 6C x 6C (row i = parameter
// 6 + i % 6 of camera i / 6: rho, t), every camera-system vector of this ABI (reduced system, camera step, `fixed` flags of
// mcba_lm_auto_config) has 6 entries per camera; the parameter vector keeps the reference's layout.  Call it before the first
// solver entry point of the handle (the solver buffers' geometry follows from it).  Partially frozen cameras: keep 12 and pass flags.
int mcba_set_camera_block(mcba_handle* h, int width) {
  if (!h || (width != 6 && width != 12)) return fail(MCBA_ERR_ARG, "mcba_set_camera_block: width 6 or 12");
  if (width == h->cw) return MCBA_OK;
  // (any solver buffer, not just a complete set: a first attempt that ran out of memory part-way leaves buffers sized for the old width behind)
  if (h->have_solver || h->solver_arena) return fail(MCBA_ERR_ARG, "mcba_set_camera_block: call it before the first solver entry point of the handle");
  if (width == 6 && !h->sparse) {
    const int nt = (6 * h->C + 1 + 15) / 16;
    if (nt * (nt + 1) / 2 > 64) return fail(MCBA_ERR_ARG, "mcba_set_camera_block: more than 26 cameras -- hold the intrinsics with the flags of mcba_lm_auto_config instead");
  }
  const int old = h->cw;
  h->cw = width;
  HIPCHK(hipSetDevice(h->device));
  const int rc = derive_geometry(h);
  if (rc != MCBA_OK) { h->cw = old; (void)derive_geometry(h); return rc; }
  h->have_lin = h->have_red = h->have_spec = false;
  h->auto_ready = false;
  return MCBA_OK;
}
int mcba_get_camera_block(const mcba_handle* h) { return h ? h->cw : 0; }

// Curvature weight of the linearisations this handle launches from now on: w = max(rho' + 2 rho'' f^2, floor rho') (csrc/mcba_math.h).
// 1 (the default) = the IRLS weight rho': monotone, the model to be far from the optimum with; 0.1 = Triggs' second-order term with a
// safety floor: the model to finish with.  A kernel argument: takes effect with the next linearisation that is ENQUEUED (the caller's
// LM driver switches between ticks; solver.py), costs nothing, changes no buffer.
int mcba_set_curvature_floor(mcba_handle* h, double floor) {
  if (!h || !(floor > 0.0) || floor > 1.0) return fail(MCBA_ERR_ARG, "mcba_set_curvature_floor: 0 < floor <= 1");
  h->curv_floor = floor;
  return MCBA_OK;
}
double mcba_get_curvature_floor(const mcba_handle* h) { return h ? h->curv_floor : 0.0; }

int mcba_set_params(mcba_handle* h, int slot, const double* x) {
  if (!slot_ok(h, slot) || !x) return fail(MCBA_ERR_ARG, "mcba_set_params: bad handle/slot/pointer");
  HIPCHK(hipSetDevice(h->device));
  // pageable host memory: the async copy is staged by the runtime before it returns
  HIPCHK(hipMemcpyAsync(h->x[slot], x, ((size_t)12 * h->C + (size_t)6 * h->F) * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return MCBA_OK;
}

int mcba_get_params(mcba_handle* h, int slot, double* x) {
  if (!slot_ok(h, slot) || !x) return fail(MCBA_ERR_ARG, "mcba_get_params: bad handle/slot/pointer");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipMemcpyAsync(x, h->x[slot], ((size_t)12 * h->C + (size_t)6 * h->F) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return MCBA_OK;
}

int mcba_copy_params(mcba_handle* h, int dst, int src) {
  if (!slot_ok(h, dst) || !slot_ok(h, src)) return fail(MCBA_ERR_ARG, "mcba_copy_params: bad slot");
  if (dst == src) return MCBA_OK;
  HIPCHK(hipMemcpyAsync(h->x[dst], h->x[src], h->nx * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
  return MCBA_OK;
}

static int run_cost(mcba_handle* h, int slot, double* res_dev, const double* bpart, int nbp) {
  {
    Scope sc(h, K_COST);
    mcba::launch_cost(h->stream, h->loss, h->f_scale, h->obs_t, h->obj, h->x[slot], h->cpart, res_dev, h->C, h->F, h->N, h->Fpad, h->nch);
  }
  int rc = check_launch();
  if (rc) return rc;
  {
    Scope sc(h, K_SUM_TRIAL);
    mcba::launch_sum_trial(h->stream, host_sel(0), h->cpart, h->cpart, 2, h->C * h->nfb * h->nch, 0, h->C * h->nfb * h->nch, bpart, nbp, h->red + h->nsys, mcba::DecideArgs{0, 0.0, 0.0, 0.0, 0.0, 0.0, nullptr});
  }
  return check_launch();
}

static int fetch_trial(mcba_handle* h, double* host8) {
  HIPCHK(hipMemcpyAsync(h->pinned + h->nsys, h->red + h->nsys, 8 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  memcpy(host8, h->pinned + h->nsys, 8 * sizeof(double));
  return MCBA_OK;
}

int mcba_cost(mcba_handle* h, int slot, double* cost, double* n_residuals) {
  if (!slot_ok(h, slot) || !cost) return fail(MCBA_ERR_ARG, "mcba_cost: bad argument");
  if (!h->have_obs) return fail(MCBA_ERR_ARG, "mcba_cost: upload observations first");
  HIPCHK(hipSetDevice(h->device));
  NEED_SOLVER(h);
  int rc = run_cost(h, slot, nullptr, nullptr, 0);
  if (rc) return rc;
  double t[8];
  rc = fetch_trial(h, t);
  if (rc) return rc;
  *cost = t[0];
  if (n_residuals) *n_residuals = t[4];
  if (!isfinite(t[0])) return fail(MCBA_ERR_NONFINITE, "Residuals are not finite");
  return MCBA_OK;
}

int mcba_residuals(mcba_handle* h, int slot, double* res) {
  if (!slot_ok(h, slot) || !res) return fail(MCBA_ERR_ARG, "mcba_residuals: bad argument");
  if (!h->have_obs) return fail(MCBA_ERR_ARG, "mcba_residuals: upload observations first");
  HIPCHK(hipSetDevice(h->device));
  NEED_SOLVER(h);
  int rc = ensure_res(h);
  if (rc) return rc;
  rc = run_cost(h, slot, h->res, nullptr, 0);
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(res, h->res, (size_t)2 * h->C * h->F * h->N * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return MCBA_OK;
}

int mcba_jacobian_eval(mcba_handle* h, int slot, int robust_scaled) {
  if (!slot_ok(h, slot)) return fail(MCBA_ERR_ARG, "mcba_jacobian_eval: bad argument");
  if (!h->have_obs) return fail(MCBA_ERR_ARG, "mcba_jacobian_eval: upload observations first");
  HIPCHK(hipSetDevice(h->device));
  int rc = ensure_res(h);
  if (rc) return rc;
  if (!h->jac) {
    rc = dalloc(h, &h->jac, (size_t)36 * h->C * h->F * h->N, false);
    if (rc) return rc;
  }
  {
    Scope sc(h, K_JACOBIAN);
    mcba::launch_jacobian(h->stream, h->loss, h->f_scale, h->obs_raw, h->obj, h->x[slot], h->jac, h->res, h->C, h->F, h->N, h->Fpad, robust_scaled);
  }
  rc = check_launch();
  if (rc) return rc;
  h->have_jac = true;
  return MCBA_OK;
}

int mcba_jacobian_download(mcba_handle* h, double* jac, double* res) {
  if (!h) return fail(MCBA_ERR_ARG, "NULL handle");
  if (!h->have_jac) return fail(MCBA_ERR_ARG, "mcba_jacobian_download: call mcba_jacobian_eval first");
  size_t cnt = (size_t)h->C * h->F * h->N;
  if (jac) HIPCHK(hipMemcpyAsync(jac, h->jac, cnt * 36 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (res) HIPCHK(hipMemcpyAsync(res, h->res, cnt * 2 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return MCBA_OK;
}

int mcba_linearize(mcba_handle* h, int slot) {
  if (!slot_ok(h, slot)) return fail(MCBA_ERR_ARG, "mcba_linearize: bad argument");
  if (!h->have_obs) return fail(MCBA_ERR_ARG, "mcba_linearize: upload observations first");
  if (h->loss == mcba::LOSS_TABLE && !h->loss_tab) return fail(MCBA_ERR_ARG, "mcba_linearize: the loss table was released (mcba_trim): call mcba_set_loss_table again");
  HIPCHK(hipSetDevice(h->device));
  NEED_SOLVER(h);
  int rc = gram_launch(h, host_sel(0), h->x[slot], h->x[slot], h->lin, h->lin);
  if (rc) return rc;
  h->have_lin = true;
  h->have_red = false;
  h->have_spec = false;
  return MCBA_OK;
}

int mcba_build_reduced(mcba_handle* h, double lambda, int rank_slot) {
  if (!h || !(lambda >= 0.0) || rank_slot < 0 || rank_slot > 11) return fail(MCBA_ERR_ARG, "mcba_build_reduced: lambda >= 0 and rank_slot in 0..11 required");
  if (!h->have_lin) return fail(MCBA_ERR_ARG, "mcba_build_reduced: call mcba_linearize first");
  HIPCHK(hipSetDevice(h->device));
  int rc;
  if ((rc = syrk_launch(h, host_sel(h->lin, lambda), no_fuse()))) return rc;
  if ((rc = reduce_launch(h, host_sel(h->lin), rank_slot, false))) return rc;
  h->have_red = true;
  return MCBA_OK;
}

size_t mcba_reduced_size(const mcba_handle* h) { return h ? h->nsys + 8 + 2 * MCBA_LMS : 0; }

int mcba_bind_reduce_buffer(mcba_handle* h, double* p) {
  if (!h) return fail(MCBA_ERR_ARG, "NULL handle");
  HIPCHK(hipSetDevice(h->device));
  NEED_SOLVER(h);
  h->red = p ? p : h->red_own;
  h->have_red = false;
  return MCBA_OK;
}

int mcba_get_reduced(mcba_handle* h, double* host) {
  if (!h || !host) return fail(MCBA_ERR_ARG, "mcba_get_reduced: bad argument");
  if (!h->have_red) return fail(MCBA_ERR_ARG, "mcba_get_reduced: call mcba_build_reduced first");
  HIPCHK(hipMemcpyAsync(h->pinned, h->red, h->nsys * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  memcpy(host, h->pinned, h->nsys * sizeof(double));
  return MCBA_OK;
}

static int step_common(mcba_handle* h, const double* delta_cam, double lambda, int src, int dst) {
  // host-selected: 'current' operands are passed in position 0, the destination slot in position 1
  int rc = backsub_launch(h, host_sel(0, lambda), h->lin, h->lin, src, dst, delta_cam);
  if (rc || !h->have_bounds) return rc;
  mcba::launch_clip(h->stream, h->x[dst], h->blo, h->bhi, (size_t)12 * h->C + (size_t)6 * h->F);   // the trial point, projected onto the box
  return check_launch();
}

int mcba_step(mcba_handle* h, const double* delta_cam, double lambda, int src, int dst) {
  if (!slot_ok(h, src) || !slot_ok(h, dst) || src == dst || !delta_cam) return fail(MCBA_ERR_ARG, "mcba_step: bad argument (slots must differ)");
  if (!h->have_red) return fail(MCBA_ERR_ARG, "mcba_step: call mcba_build_reduced first");
  HIPCHK(hipSetDevice(h->device));
  int rc = step_common(h, delta_cam, lambda, src, dst);
  if (rc) return rc;
  h->have_spec = false;
  return run_cost(h, dst, nullptr, h->bpart, h->nbblocks);
}

int mcba_step_linearize(mcba_handle* h, const double* delta_cam, double lambda, int src, int dst) {
  if (!slot_ok(h, src) || !slot_ok(h, dst) || src == dst || !delta_cam) return fail(MCBA_ERR_ARG, "mcba_step_linearize: bad argument (slots must differ)");
  if (!h->have_red) return fail(MCBA_ERR_ARG, "mcba_step_linearize: call mcba_build_reduced first");
  if (h->loss == mcba::LOSS_TABLE) return fail(MCBA_ERR_ARG, "mcba_step_linearize: a tabulated loss is set -- step (mcba_step), evaluate the function at the trial residuals, mcba_set_loss_table, then mcba_linearize");
  HIPCHK(hipSetDevice(h->device));
  int rc = step_common(h, delta_cam, lambda, src, dst);
  if (rc) return rc;
  const int alt = 1 - h->lin;
  if ((rc = gram_launch(h, host_sel(0), h->x[dst], h->x[dst], alt, alt))) return rc;
  if ((rc = trial_sum(h, host_sel(0), alt, alt, mcba::DecideArgs{0, 0.0, 0.0, 0.0, 0.0, 0.0, nullptr}))) return rc;
  h->have_spec = true;
  return MCBA_OK;
}

int mcba_accept_linearization(mcba_handle* h) {
  if (!h) return fail(MCBA_ERR_ARG, "NULL handle");
  if (!h->have_spec) return fail(MCBA_ERR_ARG, "mcba_accept_linearization: no speculative linearisation (call mcba_step_linearize first)");
  h->lin = 1 - h->lin;
  h->have_spec = false;
  h->have_red = false;
  return MCBA_OK;
}

int mcba_get_trial(mcba_handle* h, double* host8) {
  if (!h || !host8) return fail(MCBA_ERR_ARG, "mcba_get_trial: bad argument");
  return fetch_trial(h, host8);
}

// Write the eight trial scalars back into the reduce buffer: with a tabulated loss (mcba_set_loss_table) the cost of this shard's trial point
// is the caller's function on its residuals -- a frame-sharded run fetches the scalars of mcba_step (mcba_get_trial), evaluates the function
// (mcba_residuals, which reuses the scalars' slots), and puts [its cost, the step's other scalars] here BEFORE the all-reduce.
int mcba_set_trial(mcba_handle* h, const double* host8) {
  if (!h || !host8 || !h->red) return fail(MCBA_ERR_ARG, "mcba_set_trial: bad argument, or no reduce buffer yet (call mcba_step first)");
  HIPCHK(hipSetDevice(h->device));
  memcpy(h->pinned + h->nsys, host8, 8 * sizeof(double));
  HIPCHK(hipMemcpyAsync(h->red + h->nsys, h->pinned + h->nsys, 8 * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return MCBA_OK;
}

int mcba_reduce_fetch(mcba_handle* h, double lambda, int rank_slot, double* host) {
  int rc = mcba_build_reduced(h, lambda, rank_slot);
  if (rc) return rc;
  return mcba_get_reduced(h, host);
}

int mcba_step_fetch(mcba_handle* h, const double* delta_cam, double lambda, int src, int dst, int linearize, double* host8) {
  int rc = linearize ? mcba_step_linearize(h, delta_cam, lambda, src, dst) : mcba_step(h, delta_cam, lambda, src, dst);
  if (rc) return rc;
  return mcba_get_trial(h, host8);
}

// ---------------------------------------------------------------------------------------------------------
// least_squares' numeric x_scale (the reference forwards **opt_kwargs verbatim: bundle_adjustment.py:301-313).  scipy's trust
// region lives in the variables x / x_scale; for Levenberg-Marquardt that is a FIXED damping matrix D = diag(1 / x_scale^2)
// in place of Marquardt's D = diag(J^T J) (= x_scale 'jac').  x_scale: 12C + 6F positive doubles in the layout of x, or NULL
// to return to 'jac'.
int mcba_set_x_scale(mcba_handle* h, const double* x_scale) {
  if (!h) return fail(MCBA_ERR_ARG, "NULL handle");
  HIPCHK(hipSetDevice(h->device));
  NEED_SOLVER(h);
  if (!x_scale) {
    if (h->xs_host.empty() && h->frozen_host.empty()) { h->have_red = false; h->have_xscale = false; return MCBA_OK; }   // (the usual call of every solve: nothing to upload)
    h->xs_host.clear();
    return compose_dscale(h);
  }
  const size_t cnt = (size_t)12 * h->C + (size_t)6 * h->F;
  std::vector<double> d(cnt);
  for (size_t i = 0; i < cnt; ++i) {
    if (!(x_scale[i] > 0.0) || !std::isfinite(x_scale[i])) return fail(MCBA_ERR_ARG, "`x_scale` must be 'jac' or array_like with positive numbers.");
    d[i] = 1.0 / (x_scale[i] * x_scale[i]);
  }
  h->xs_host.swap(d);
  return compose_dscale(h);
}

// Coordinates taken OUT of the system for the linear solves that follow (an active-set method's working set: solver.py, box constraints):
// mask = 12C + 6F bytes in the layout of x, non-zero = frozen, or NULL for none.  A frozen FRAME coordinate gets a step of exactly 0 and
// nothing couples to it (its row / column of V_f, its gradient entry, its column of every W block count as zero in k_syrk and k_backsub;
// the gradient mcba_get_frame_gradient reports stays the true one).  Camera entries of the mask are ignored here: freeze camera parameters
// with the flags of mcba_lm_auto_config, or leave their rows out of a host solve.  Takes effect with the next mcba_build_reduced.
int mcba_set_frozen(mcba_handle* h, const unsigned char* mask) {
  if (!h) return fail(MCBA_ERR_ARG, "NULL handle");
  HIPCHK(hipSetDevice(h->device));
  NEED_SOLVER(h);
  const size_t cnt = (size_t)12 * h->C + (size_t)6 * h->F, ncam = (size_t)12 * h->C;
  bool any = false;
  if (mask) for (size_t i = ncam; i < cnt; ++i) any = any || mask[i] != 0;
  if (!any) {
    if (h->frozen_host.empty()) return MCBA_OK;
    h->frozen_host.clear();
    return compose_dscale(h);
  }
  h->frozen_host.assign(mask, mask + cnt);
  return compose_dscale(h);
}

// Box constraints lo <= x <= hi (12C + 6F doubles each in the layout of x, -inf / +inf = none; both NULL: none at all): from now on the
// trial point of every mcba_step / mcba_step_linearize / mcba_step_fetch is PROJECTED onto the box before its cost is evaluated (k_clip).
// The working set is the caller's business (mcba_set_frozen + the camera rows it leaves out of the reduced solve): solver.py's bounded
// loop.  The device-resident loops (mcba_lm_iterate, mcba_lm_auto_*, mcba_lm_run) refuse to run while bounds are set.  Reference:
// bundle_adjustment.py:301-313 forwards `bounds` to scipy's least_squares (trf_bounds).
int mcba_set_bounds(mcba_handle* h, const double* lo, const double* hi) {
  if (!h || (lo == nullptr) != (hi == nullptr)) return fail(MCBA_ERR_ARG, "mcba_set_bounds: bad argument");
  HIPCHK(hipSetDevice(h->device));
  if (!lo) { h->have_bounds = false; return MCBA_OK; }
  const size_t cnt = (size_t)12 * h->C + (size_t)6 * h->F;
  for (size_t i = 0; i < cnt; ++i)
    if (!(lo[i] < hi[i])) return fail(MCBA_ERR_ARG, "Each lower bound must be strictly less than each upper bound.");
  int rc;
  if (!h->blo && (rc = dalloc(h, &h->blo, h->nx, false))) return rc;
  if (!h->bhi && (rc = dalloc(h, &h->bhi, h->nx, false))) return rc;
  std::vector<double> a(h->nx, -INFINITY), b(h->nx, INFINITY);
  memcpy(a.data(), lo, cnt * sizeof(double));
  memcpy(b.data(), hi, cnt * sizeof(double));
  HIPCHK(hipMemcpyAsync(h->blo, a.data(), h->nx * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(h->bhi, b.data(), h->nx * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  h->have_bounds = true;
  return MCBA_OK;
}

// ---------------------------------------------------------------------------------------------------------
// Residual vector left ON THE DEVICE and handed to the caller as an object of its own: api.bundle_adjust attaches it to the
// OptimizeResult and downloads it when (if) `result.fun` is first read -- 52 MB of D2H at 6 x 10 000 x 54 that most callers
// never look at (the reference materialises it: scipy trf.py:557-560).  The buffer outlives the handle.

int mcba_residuals_detach(mcba_handle* h, int slot, mcba_buffer** out) {
  if (!slot_ok(h, slot) || !out) return fail(MCBA_ERR_ARG, "mcba_residuals_detach: bad argument");
  if (!h->have_obs) return fail(MCBA_ERR_ARG, "mcba_residuals_detach: upload observations first");
  HIPCHK(hipSetDevice(h->device));
  NEED_SOLVER(h);
  int rc = ensure_res(h);
  if (rc) return rc;
  {  // (the residual vector alone: the cost sums of run_cost are not wanted here)
    Scope sc(h, K_COST);
    mcba::launch_cost(h->stream, h->loss, h->f_scale, h->obs_t, h->obj, h->x[slot], h->cpart, h->res, h->C, h->F, h->N, h->Fpad, h->nch, NAN);   // NaN where a scalar is missing: the vector is its own row mask
  }
  if ((rc = check_launch())) return rc;
  mcba_buffer* b = new mcba_buffer{h->res, (size_t)2 * h->C * h->F * h->N, h->device, h->stream, h->res, (size_t)2 * h->C * h->F * h->N};
  for (size_t i = 0; i < h->bufs.size(); ++i)
    if (h->bufs[i].slot == reinterpret_cast<void**>(&h->res)) { h->bufs.erase(h->bufs.begin() + i); break; }
  h->res = nullptr;
  h->have_jac = false;
  *out = b;
  return MCBA_OK;
}
size_t mcba_buffer_count(const mcba_buffer* b) { return b ? b->count : 0; }
int mcba_buffer_download(mcba_buffer* b, double* host) {
  if (!b || !host) return fail(MCBA_ERR_ARG, "mcba_buffer_download: bad argument");
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipMemcpyAsync(host, b->dev, b->count * sizeof(double), hipMemcpyDeviceToHost, b->stream));
  HIPCHK(hipStreamSynchronize(b->stream));
  return MCBA_OK;
}
int mcba_buffer_free(mcba_buffer* b) {
  if (!b) return MCBA_OK;
  (void)hipSetDevice(b->device);
  pool_free(b->base, b->base_count * sizeof(double), b->device, b->stream, true);   // (the kernel that fills it may still be running: parked as busy on its stream)
  delete b;
  return MCBA_OK;
}
// Measurement aid (bench.py): the FP64 vector rate this device sustains with one wavefront per SIMD on every compute unit issuing
// independent v_fma_f64 -- what k_gram's instruction stream can be priced against besides the datasheet peak.  ~0.3 ms of GPU time.
int mcba_fp64_issue_rate(int device, double* tflops) {
  if (!tflops) return fail(MCBA_ERR_ARG, "mcba_fp64_issue_rate: NULL");
  *tflops = 0.0;
  if (int rc = stateless_device(device)) return rc;
  hipDeviceProp_t prop;
  int ncu = 256;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) ncu = prop.multiProcessorCount;
  *tflops = mcba::measure_fp64_issue_rate(ncu);
  if (!(*tflops > 0.0)) return fail(MCBA_ERR_HIP, "mcba_fp64_issue_rate: the measurement kernel failed");
  return MCBA_OK;
}

int mcba_profile_enable(mcba_handle* h, int on) {
  if (!h) return fail(MCBA_ERR_ARG, "NULL handle");
  h->prof = on != 0;
  h->prof_mask = (on == 0 || on == 1) ? ~0u : ((unsigned)on >> 1);
  h->prof_stride = 1;
  h->prof_exact = false;
  return MCBA_OK;
}

// k_gram's launches (the fused kernel) are timed by events attached to the dispatch itself (hipExtLaunchKernelGGL): the kernel's own
// begin and end, what rocprofv3 reports -- an event pair recorded around a launch reads ~2.5 us more.  Reset by mcba_profile_enable.
int mcba_profile_exact(mcba_handle* h, int on) {
  if (!h) return fail(MCBA_ERR_ARG, "NULL handle");
  h->prof_exact = on != 0;
  return MCBA_OK;
}

int mcba_profile_stride(mcba_handle* h, int stride) {
  if (!h || stride < 1) return fail(MCBA_ERR_ARG, "mcba_profile_stride: stride >= 1 required");
  h->prof_stride = stride;
  return MCBA_OK;
}

// What a HIP-event bracket reads with NOTHING between its two records, on the handle's stream (mean of `pairs` back-to-back brackets, in
// microseconds): the part of a bracketed kernel's time that is the bracket's, not the kernel's.  bench.py subtracts it from the
// event-timed duration of the dominant kernel so that the figure agrees with rocprofv3's (50.4 us by events, 47.8 by rocprof).
int mcba_profile_bracket_overhead(mcba_handle* h, int pairs, double* us) {
  if (!h || !us || pairs < 1 || pairs > 4096) return fail(MCBA_ERR_ARG, "mcba_profile_bracket_overhead: bad argument");
  HIPCHK(hipSetDevice(h->device));
  std::vector<hipEvent_t> ev(2 * (size_t)pairs);
  for (auto& e : ev) HIPCHK(hipEventCreate(&e));
  HIPCHK(hipStreamSynchronize(h->stream));
  for (int i = 0; i < pairs; ++i) { HIPCHK(hipEventRecord(ev[2 * i], h->stream)); HIPCHK(hipEventRecord(ev[2 * i + 1], h->stream)); }
  HIPCHK(hipStreamSynchronize(h->stream));
  double tot = 0.0;
  for (int i = 0; i < pairs; ++i) { float ms = 0.f; HIPCHK(hipEventElapsedTime(&ms, ev[2 * i], ev[2 * i + 1])); tot += ms; }
  for (auto& e : ev) (void)hipEventDestroy(e);
  *us = 1e3 * tot / pairs;
  return MCBA_OK;
}

int mcba_profile_read(mcba_handle* h, double* ms_total, int* calls, int capacity, int* n_kernels) {
  if (!h || !ms_total || !calls || capacity < K_COUNT) return fail(MCBA_ERR_ARG, "mcba_profile_read: need capacity >= number of kernels");
  HIPCHK(hipStreamSynchronize(h->stream));
  for (int i = 0; i < K_COUNT; ++i) { ms_total[i] = 0.0; calls[i] = 0; }
  for (auto& e : h->evs) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, e.a, e.b) == hipSuccess) { ms_total[e.kid] += ms; calls[e.kid] += 1; }
    h->pool.push_back(e.a);
    h->pool.push_back(e.b);
  }
  h->evs.clear();
  if (n_kernels) *n_kernels = K_COUNT;
  return MCBA_OK;
}

}  // extern "C"
