// mcba_prefilter_api.hip -- bundle_adjust()'s frame pre-filter on the device (include/mcba.h): per-point reprojection errors, their exact
// medians and histograms, the selection and frame subsets without a second upload; also the reprojection diagnostics, which share the
// per-point errors and their medians.
#include "mcba_handle.h"

using namespace mcba_internal;

extern "C" {

// ---------------------------------------------------------------------------------------------------------
// bundle_adjust()'s frame pre-filter on the GPU (reference bundle_adjustment.py:265-285) and frame subsets without a second upload
static int ensure_diag(mcba_handle* h) {
  int rc;
  // (none of them is filled: k_frame_err / k_reproj_diag write every error and statistic, launch_select clears its states, the mask is
  //  written whole by whoever uses it)
  if (!h->err && (rc = dalloc(h, &h->err, (size_t)h->C * h->N * h->Fpad, false))) return rc;
  if (!h->dmean && (rc = dalloc(h, &h->dmean, std::max<size_t>((size_t)h->C * h->F, 8), false))) return rc;
  if (!h->dfull && (rc = dalloc(h, &h->dfull, (size_t)h->C * h->F, false))) return rc;
  if (!h->sel && (rc = dalloc(h, &h->sel, (size_t)2 * h->C, false))) return rc;
  if (!h->fmask && (rc = dalloc(h, &h->fmask, (size_t)h->Fpad, false))) return rc;
  return MCBA_OK;
}

// ---------------------------------------------------------------------------------------------------------
// bundle_adjust()'s pre-filter in ONE call and ONE host synchronisation (round 5): upload (observations, board, parameters of every
// frame), re-layout, k_frame_err, and the whole selection on the device (mcba_diag.hip: frames complete in two cameras, worst camera's
// mean error, 5 x nanmedian by a three-pass radix select, the comparison) -- the host reads 80 + F bytes.  The transfer is NOT cut
// into chunks with kernels in between: measured on the MI355X box (scripts/micro/h2d_pipeline.hip, profiles/round5/h2d_pipeline.txt)
// one hipMemcpyAsync of the 51.8 MB takes 0.92 ms (56 GB/s, the call blocks: pageable source), six chunks 1.10 ms, twelve 1.23 ms
// (~30 us per extra call), a pinned staging ring 1.93 ms -- while everything the GPU does behind the copy is ~60 us.
static int median_of_err(mcba_handle* h, size_t per_group, int groups, bool use_mask, double* median, double* count);
static int ensure_prefilter(mcba_handle* h) {
  int rc = ensure_diag(h);
  if (rc) return rc;
  if (!h->pf_state && (rc = dalloc(h, &h->pf_state, mcba::prefilter_state_bytes(), false))) return rc;
  if (!h->pf_status && (rc = dalloc(h, &h->pf_status, (size_t)h->Fpad, false))) return rc;
  if (!h->pf_worst && (rc = dalloc(h, &h->pf_worst, (size_t)h->Fpad, false))) return rc;
  if (!h->pf_packed && (rc = dalloc(h, &h->pf_packed, (size_t)h->Fpad + 128, false))) return rc;
  if (!h->pf_host) {
    h->pf_host_bytes = (size_t)h->Fpad + 128;
    HIPCHK(pool_host_malloc(reinterpret_cast<void**>(&h->pf_host), h->pf_host_bytes, hipHostMallocDefault));
  }
  return MCBA_OK;
}

int mcba_prefilter(mcba_handle* h, const double* uvs, const double* objpoints, const double* x, double outlier_threshold, unsigned char* status, double* info8) {
  if (!h || !x || !status || !info8 || (uvs == nullptr) != (objpoints == nullptr)) return fail(MCBA_ERR_ARG, "mcba_prefilter: bad argument");
  if (!uvs && !h->have_obs) return fail(MCBA_ERR_ARG, "mcba_prefilter: no observations (pass them, or upload them first)");
  HIPCHK(hipSetDevice(h->device));
  int rc = ensure_prefilter(h);
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(h->x[0], x, ((size_t)12 * h->C + (size_t)6 * h->F) * sizeof(double), hipMemcpyHostToDevice, h->stream));
  if (uvs && (rc = upload_impl(h, uvs, objpoints, false))) return rc;
  mcba::launch_frame_err(h->stream, h->obs_t, h->obj, h->x[0], h->err, h->dmean, h->dfull, h->C, h->F, h->N, h->Fpad, h->pf_state);
  mcba::launch_prefilter_select(h->stream, h->err, h->dmean, h->dfull, h->fmask, h->pf_status, h->pf_worst, h->pf_state, h->pf_packed, h->C, h->F, h->N, h->Fpad, outlier_threshold, true);
  if ((rc = check_launch())) return rc;
  const size_t nb = 64 + (size_t)h->F;
  auto fetch = [&]() -> int {
    HIPCHK(hipMemcpyAsync(h->pf_host, h->pf_packed, nb, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return MCBA_OK;
  };
  if ((rc = fetch())) return rc;
  double info[8];
  memcpy(info, h->pf_host, sizeof(info));
  const char* force = getenv("MCBA_PREFILTER_FALLBACK");   // test knob: take the eight-pass select whatever the candidate count
  if (outlier_threshold != outlier_threshold && (info[3] != 0.0 || (force && atoi(force) != 0))) {
    // more values share the median's 24 leading bits than the candidate list holds: the eight-pass radix select on the same mask
    double med = 0.0, cnt = 0.0;
    if ((rc = median_of_err(h, (size_t)h->C * h->N * h->Fpad, 1, true, &med, &cnt))) return rc;
    mcba::launch_prefilter_status(h->stream, h->pf_status, h->pf_worst, h->pf_state, h->pf_packed, h->F, 5.0 * med, 0);
    if ((rc = check_launch())) return rc;
    if ((rc = fetch())) return rc;
    memcpy(info, h->pf_host, sizeof(info));
    info[1] = med; info[2] = cnt; info[3] = 1.0;
  }
  memcpy(status, h->pf_host + 64, (size_t)h->F);
  {  // frames used / excluded / kept but incomplete in some camera (the counts of the printed line)
    double used = 0, excl = 0, inc = 0;
    for (int f = 0; f < h->F; ++f) { const unsigned char sf = status[f]; used += sf & 1; excl += (sf >> 1) & 1; inc += ((sf & 7) == 1) ? 1 : 0; }
    info[4] = used; info[5] = excl; info[6] = inc;
  }
  memcpy(info8, info, sizeof(info));
  return MCBA_OK;
}

// mcba_prefilter + what bundle_adjust does with its answer when no random draw stands in between (bundle_adjustment.py:292-296: the
// subsample is drawn from the caller's global numpy RNG only if n_frames <= the number of frames kept): the kept frames are gathered into a
// new handle right here, with the status bytes still warm -- the host round trip between "the selection is known" and "its gather is enqueued"
// was a Python function and a second crossing.  info8[7]: 0 nothing kept, 1 the caller must draw (no handle made), 2 every frame kept in
// order (solve on h itself), 3 *sub holds the kept frames (mcba_create_subset of them, in order).  n_frames < 0: no cap (None).
int mcba_prefilter_subset(mcba_handle* h, const double* uvs, const double* objpoints, const double* x, double outlier_threshold, int n_frames, unsigned char* status, double* info8,
                          mcba_handle** sub) {
  if (!sub) return fail(MCBA_ERR_ARG, "mcba_prefilter_subset: bad argument");
  *sub = nullptr;
  int rc = mcba_prefilter(h, uvs, objpoints, x, outlier_threshold, status, info8);
  if (rc) return rc;
  const int kept = (int)(info8[4] - info8[5]);
  if (kept == 0) { info8[7] = 0.0; return MCBA_OK; }
  if (n_frames >= 0 && n_frames <= kept) { info8[7] = 1.0; return MCBA_OK; }
  if (kept == h->F) { info8[7] = 2.0; return MCBA_OK; }
  std::vector<int> frames;
  frames.reserve((size_t)kept);
  for (int f = 0; f < h->F; ++f)
    if ((status[f] & 3) == 1) frames.push_back(f);
  if ((rc = mcba_create_subset(sub, h, frames.data(), (int)frames.size()))) return rc;
  info8[7] = 3.0;
  return MCBA_OK;
}

int mcba_frame_errors(mcba_handle* h, int slot, double* mean_cf, double* full_cf) {
  if (!slot_ok(h, slot) || !mean_cf || !full_cf) return fail(MCBA_ERR_ARG, "mcba_frame_errors: bad argument");
  if (!h->have_obs) return fail(MCBA_ERR_ARG, "mcba_frame_errors: upload observations first");
  HIPCHK(hipSetDevice(h->device));
  int rc = ensure_diag(h);
  if (rc) return rc;
  mcba::launch_frame_err(h->stream, h->obs_t, h->obj, h->x[slot], h->err, h->dmean, h->dfull, h->C, h->F, h->N, h->Fpad);
  if ((rc = check_launch())) return rc;
  const size_t cnt = (size_t)h->C * h->F * sizeof(double);
  HIPCHK(hipMemcpyAsync(mean_cf, h->dmean, cnt, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(full_cf, h->dfull, cnt, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return MCBA_OK;
}

// nan-median (exact order statistics) of `groups` equal slices of h->err restricted to the frames of h->fmask
static int median_of_err(mcba_handle* h, size_t per_group, int groups, bool use_mask, double* median, double* count) {
  std::vector<mcba::SelState> both(2 * (size_t)groups);  // state 2 g: rank (n - 1) / 2, state 2 g + 1: rank n / 2 -- found in the same eight passes
  mcba::launch_select(h->stream, h->err, use_mask ? h->fmask : nullptr, per_group, groups, h->Fpad, h->sel, 0);
  int rc = check_launch();
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(both.data(), h->sel, both.size() * sizeof(mcba::SelState), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  for (int g = 0; g < groups; ++g) {
    median[g] = mcba::sel_median(both[2 * g], both[2 * g + 1]);  // np.median / np.nanmedian
    if (count) count[g] = (double)both[2 * g].count;
  }
  return MCBA_OK;
}

int mcba_error_median(mcba_handle* h, const unsigned char* frame_mask, double* median, double* count) {
  if (!h || !median) return fail(MCBA_ERR_ARG, "mcba_error_median: bad argument");
  if (!h->err) return fail(MCBA_ERR_ARG, "mcba_error_median: call mcba_frame_errors first");
  HIPCHK(hipSetDevice(h->device));
  if (frame_mask) {
    HIPCHK(hipMemsetAsync(h->fmask, 0, (size_t)h->Fpad, h->stream));
    HIPCHK(hipMemcpyAsync(h->fmask, frame_mask, (size_t)h->F, hipMemcpyHostToDevice, h->stream));  // (pageable source: staged before the call returns)
  }
  return median_of_err(h, (size_t)h->C * h->N * h->Fpad, 1, frame_mask != nullptr, median, count);
}

// only_cam != nullptr (mcba_create_views): destination frame j keeps the detection of camera only_cam[j] alone
static int create_subset_impl(mcba_handle** out, mcba_handle* src, const int* frames, const int* only_cam, int n_frames) {
  if (!out || !src || !frames || n_frames < 1) return fail(MCBA_ERR_ARG, "mcba_create_subset: bad argument");
  if (!src->have_obs) return fail(MCBA_ERR_ARG, "mcba_create_subset: the source handle has no observations");
  for (int i = 0; i < n_frames; ++i)
    if (frames[i] < 0 || frames[i] >= src->F || (only_cam && (only_cam[i] < 0 || only_cam[i] >= src->C))) return fail(MCBA_ERR_ARG, "mcba_create_subset: frame / camera index out of range");
  int rc = create_impl(out, src->C, n_frames, src->N, src->device, src->sparse);   // (a subset is a handle of the same kind)
  if (rc) return rc;
  mcba_handle* h = *out;
  if (src->stream != h->stream) HIPCHK(hipStreamSynchronize(h->stream));  // mcba_create's zero fills ran on the creation stream
  h->stream = src->stream;
  h->loss = src->loss == mcba::LOSS_TABLE ? MCBA_LOSS_SOFT_L1 : src->loss;   // (a table belongs to its frames: the subset starts from the default)
  h->f_scale = src->f_scale;
  h->strict_sync = src->strict_sync;
  // (the index list lives and dies with the new handle: nothing to free here, so nothing to wait for)
  if ((rc = dalloc(h, &h->sub_frames, (size_t)n_frames * (only_cam ? 2 : 1), false)) != MCBA_OK) { mcba_destroy(h); *out = nullptr; return rc; }
  int* d_frames = h->sub_frames;
  hipError_t e = hipMemcpyAsync(d_frames, frames, (size_t)n_frames * sizeof(int), hipMemcpyHostToDevice, h->stream);  // (pageable source: staged before the call returns)
  if (e == hipSuccess && only_cam) e = hipMemcpyAsync(d_frames + n_frames, only_cam, (size_t)n_frames * sizeof(int), hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) {
    mcba::launch_gather_frames(h->stream, src->obs_raw, d_frames, h->obs_raw, h->C, src->F, h->F, h->N, only_cam ? d_frames + n_frames : nullptr);
    // ... and the parameters of the source's slot 0: the camera blocks + the poses of the chosen frames (what bundle_adjust starts from)
    mcba::launch_gather_params(h->stream, src->x[0], d_frames, h->x[0], h->C, h->F);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(h->obj, src->obj, (size_t)3 * h->N * sizeof(double), hipMemcpyDeviceToDevice, h->stream);
  if (e == hipSuccess) {
    Scope sc(h, K_TRANSPOSE);
    mcba::launch_transpose_obs(h->stream, h->obs_raw, h->obs_t, h->C, h->F, h->N, h->Fpad);
    e = hipGetLastError();
  }
  if (e != hipSuccess) {
    g_err = std::string("mcba_create_subset: ") + hipGetErrorString(e);
    mcba_destroy(h);
    *out = nullptr;
    return MCBA_ERR_HIP;
  }
  if (src->obj_host) {
    h->obj_host = static_cast<double*>(malloc((size_t)3 * h->N * sizeof(double)));
    if (h->obj_host) memcpy(h->obj_host, src->obj_host, (size_t)3 * h->N * sizeof(double));
    h->planar = src->planar;
  }
  h->have_obs = true;
  return MCBA_OK;
}

int mcba_create_subset(mcba_handle** out, mcba_handle* src, const int* frames, int n_frames) { return create_subset_impl(out, src, frames, nullptr, n_frames); }

// A handle of C cameras x n_views frames whose frame j holds the detection of view j = (camera, frame) of `src` in ITS camera alone (NaN in
// the others): the <= 100 sampled views of every camera side by side, so that ONE device-resident LM run refines every camera's intrinsics
// with its own views' poses (get_intrinsics, reference calibration.py:11-71) -- the normal equations are block-diagonal over the cameras.
int mcba_create_views(mcba_handle** out, mcba_handle* src, const int* views, int n_views) {
  if (!out || !src || !views || n_views < 1) return fail(MCBA_ERR_ARG, "mcba_create_views: bad argument");
  std::vector<int> frames((size_t)n_views), cams((size_t)n_views);
  for (int i = 0; i < n_views; ++i) { cams[i] = views[2 * i]; frames[i] = views[2 * i + 1]; }
  return create_subset_impl(out, src, frames.data(), cams.data(), n_views);
}

// ---------------------------------------------------------------------------------------------------------
// Reprojection diagnostics: the numeric core of plot_residuals (reference viz.py:166-186)
int mcba_reprojection_diagnostics(mcba_handle* h, int slot, const double* dist5, int undistort_iterations, double* median_error, double* reprojections, double* transformed) {
  if (!slot_ok(h, slot) || !median_error || undistort_iterations < 0) return fail(MCBA_ERR_ARG, "mcba_reprojection_diagnostics: bad argument");
  if (!h->have_obs || !h->obj_host) return fail(MCBA_ERR_ARG, "mcba_reprojection_diagnostics: upload observations first");
  HIPCHK(hipSetDevice(h->device));
  int rc = ensure_diag(h);
  if (rc) return rc;
  const size_t cnt = (size_t)2 * h->C * h->F * h->N;
  if (reprojections && !h->repro && (rc = dalloc(h, &h->repro, cnt))) return rc;
  if (transformed && !h->trans && (rc = dalloc(h, &h->trans, cnt))) return rc;
  if (!h->und && (rc = dalloc(h, &h->und, (size_t)2 * h->C * h->N * h->Fpad))) return rc;
  std::vector<double> d5((size_t)5 * h->C, 0.0), xc((size_t)12 * h->C);
  if (dist5) memcpy(d5.data(), dist5, d5.size() * sizeof(double));
  else {  // (k1, k2, 0, 0, 0) of the parameter vector
    HIPCHK(hipMemcpyAsync(xc.data(), h->x[slot], xc.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int c = 0; c < h->C; ++c) { d5[5 * c] = xc[12 * c + 4]; d5[5 * c + 1] = xc[12 * c + 5]; }
  }
  // Hartley normalisation of the board's XY: centroid and sqrt(2) / mean distance
  double bn[3] = {0.0, 0.0, 1.0};
  for (int p = 0; p < h->N; ++p) { bn[0] += h->obj_host[3 * p]; bn[1] += h->obj_host[3 * p + 1]; }
  bn[0] /= h->N; bn[1] /= h->N;
  double md = 0.0;
  for (int p = 0; p < h->N; ++p) md += hypot(h->obj_host[3 * p] - bn[0], h->obj_host[3 * p + 1] - bn[1]);
  bn[2] = md > 0.0 ? sqrt(2.0) * h->N / md : 1.0;
  double* d_bn = h->dmean;  // three doubles of scratch (the pre-filter's means are host-side by now)
  HIPCHK(hipMemcpyAsync(d_bn, bn, sizeof(bn), hipMemcpyHostToDevice, h->stream));
  mcba::launch_reproj_diag(h->stream, h->obs_t, h->obj, h->x[slot], d5.data(), d_bn, h->und, reprojections ? h->repro : nullptr, transformed ? h->trans : nullptr, h->err, h->C, h->F, h->N, h->Fpad,
                           undistort_iterations, 24);
  if ((rc = check_launch())) return rc;
  if ((rc = median_of_err(h, (size_t)h->N * h->Fpad, h->C, false, median_error, nullptr))) return rc;
  if (reprojections) HIPCHK(hipMemcpyAsync(reprojections, h->repro, cnt * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (transformed) HIPCHK(hipMemcpyAsync(transformed, h->trans, cnt * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return MCBA_OK;
}

// numpy.packbits(~numpy.isnan(uvs)) of the uploaded observations, taken from the device copy (k_seen_bits): 0.8 MB of D2H at
// 6 x 10 000 x 54 instead of 24 ms of numpy over the caller's 52 MB.
int mcba_seen_bits(mcba_handle* h, unsigned char* bits) {
  if (!h || !bits) return fail(MCBA_ERR_ARG, "mcba_seen_bits: bad argument");
  if (!h->have_obs) return fail(MCBA_ERR_ARG, "mcba_seen_bits: upload observations first");
  HIPCHK(hipSetDevice(h->device));
  const size_t count = (size_t)2 * h->C * h->F * h->N, words = (count + 63) / 64;
  unsigned long long* d = nullptr;
  HIPCHK(pool_malloc(reinterpret_cast<void**>(&d), words * 8, h->device, h->stream));
  mcba::launch_seen_bits(h->stream, h->obs_raw, count, d);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(bits, d, (count + 7) / 8, hipMemcpyDeviceToHost, h->stream);
  hipError_t e2 = hipStreamSynchronize(h->stream);
  pool_free(d, words * 8, h->device);
  if (e != hipSuccess || e2 != hipSuccess) { g_err = std::string("mcba_seen_bits: ") + hipGetErrorString(e != hipSuccess ? e : e2); return MCBA_ERR_HIP; }
  return MCBA_OK;
}

// ---------------------------------------------------------------------------------------------------------
// One pass of the radix select behind mcba_error_median, for callers that hold only a SHARD of the frames (frame-sharded
// bundle_adjust: every rank runs the pre-filter on its own slice): the 256-bin histogram of byte `pass` (0 = most significant)
// over this handle's per-point errors whose leading `pass` bytes equal `prefix`, restricted to frame_mask (F bytes, NULL = the mask
// of the previous call).  The caller sums the histograms over the ranks, picks the bin that holds the wanted rank and calls again
// with the longer prefix -- integer arithmetic only, so the order statistic is exact whatever the sharding.
int mcba_error_histogram(mcba_handle* h, const unsigned char* frame_mask, unsigned long long prefix, int pass, unsigned long long* hist256) {
  if (!h || !hist256 || pass < 0 || pass > 7) return fail(MCBA_ERR_ARG, "mcba_error_histogram: bad argument");
  if (!h->err) return fail(MCBA_ERR_ARG, "mcba_error_histogram: call mcba_frame_errors first");
  HIPCHK(hipSetDevice(h->device));
  if (frame_mask) {
    HIPCHK(hipMemsetAsync(h->fmask, 0, (size_t)h->Fpad, h->stream));
    HIPCHK(hipMemcpyAsync(h->fmask, frame_mask, (size_t)h->F, hipMemcpyHostToDevice, h->stream));
  }
  unsigned int hist[256];
  int rc = mcba::launch_select_hist(h->stream, h->err, h->fmask, (size_t)h->C * h->N * h->Fpad, h->Fpad, h->sel, prefix, pass, hist);
  if (rc) { g_err = "mcba_error_histogram: HIP error"; return MCBA_ERR_HIP; }
  for (int b = 0; b < 256; ++b) hist256[b] = hist[b];
  return MCBA_OK;
}

}  // extern "C"
