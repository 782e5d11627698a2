// mcba_calib_api.hip -- calibrate() on the device (include/mcba.h: the handle calls mcba_calib_*), the same pose-graph steps for a caller's own
// pose array (mcba_pose_*, stateless) and the single-camera normal equations (mcba_calib_normal_equations, stateless).
#include "mcba_handle.h"

using namespace mcba_internal;

// ---------------------------------------------------------------------------------------------------------
// calibrate() on the device (reference calibration.py:11-113 -- the two OpenCV calls per view -- and :116-277 -- the pose graph).
// The handle holds every detection (mcba_upload_observations); a call of calibrate() is: mcba_calib_complete -> [host: the reference's
// RNG draw] -> mcba_calib_homographies (sampled views) -> [host: Zhang's closed form, a 6-vector] -> mcba_calib_view_poses ->
// mcba_create_views + mcba_lm_run (all cameras' intrinsics in one run) -> mcba_calib_poses (every view, ONE launch; the poses stay on the
// device) -> [host: spanning tree] -> mcba_calib_pairwise -> [host: chain C - 1 transforms] -> mcba_calib_consensus.

// a scratch buffer of the handle that grows with the call
template <class T>
static int dgrow(mcba_handle* h, T** p, size_t* cap, size_t count) {
  if (*p && *cap >= count) return MCBA_OK;
  if (*p) {
    for (size_t i = 0; i < h->bufs.size(); ++i)
      if (h->bufs[i].slot == reinterpret_cast<void**>(p)) { pool_free(*p, h->bufs[i].bytes, h->device, h->stream, true); h->bufs.erase(h->bufs.begin() + i); break; }
    *p = nullptr;
  }
  *cap = 0;
  int rc = dalloc(h, p, count, false);
  if (rc == MCBA_OK) *cap = count;
  return rc;
}
// Hartley normalisation of the board's XY as calibration.py's closed-form start uses it: centroid, sqrt(2) / rms distance
static void board_normalisation(const double* obj, int N, double* bn) {
  bn[0] = bn[1] = 0.0; bn[2] = 1.0;
  for (int p = 0; p < N; ++p) { bn[0] += obj[3 * p]; bn[1] += obj[3 * p + 1]; }
  bn[0] /= N; bn[1] /= N;
  double ms = 0.0;
  for (int p = 0; p < N; ++p) ms += (obj[3 * p] - bn[0]) * (obj[3 * p] - bn[0]) + (obj[3 * p + 1] - bn[1]) * (obj[3 * p + 1] - bn[1]);
  if (ms > 0.0) bn[2] = sqrt(2.0) / sqrt(ms / N);
}
static int calib_ready(mcba_handle* h, const char* who) {
  if (!h) return fail(MCBA_ERR_ARG, "NULL handle");
  if (!h->have_obs || !h->obj_host) { g_err = std::string(who) + ": upload observations first"; return MCBA_ERR_ARG; }
  // calibrate()'s kernels hold at most 40 cameras (k_pose_chain's LDS tables, the per-view kernels' camera masks); only a sparse-Schur
  // handle can have more, and it serves bundle_adjust() alone
  if (h->C > 40) { g_err = std::string(who) + ": " + std::to_string(h->C) + " cameras -- calibrate() on the device handles at most 40 (the sparse-Schur handle serves bundle_adjust only)"; return MCBA_ERR_ARG; }
  for (int p = 0; p < h->N; ++p)
    if (h->obj_host[3 * p + 2] != 0.0) { g_err = std::string(who) + ": the closed-form start needs a planar calibration board (z = 0)"; return MCBA_ERR_ARG; }
  HIPCHK(hipSetDevice(h->device));
  return MCBA_OK;
}
static int upload_views(mcba_handle* h, const int* views, int n_views, const char* who) {
  for (int i = 0; i < n_views; ++i)
    if (views[2 * i] < 0 || views[2 * i] >= h->C || views[2 * i + 1] < 0 || views[2 * i + 1] >= h->F) { g_err = std::string(who) + ": view (camera, frame) out of range"; return MCBA_ERR_ARG; }
  int rc = dgrow(h, &h->cal_views, &h->cal_views_cap, (size_t)2 * n_views);
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(h->cal_views, views, (size_t)2 * n_views * sizeof(int), hipMemcpyHostToDevice, h->stream));
  return MCBA_OK;
}
static int upload_intr(mcba_handle* h, const double* intr9) {
  int rc;
  if (!h->cal_intr && (rc = dalloc(h, &h->cal_intr, (size_t)9 * h->C, false))) return rc;
  HIPCHK(hipMemcpyAsync(h->cal_intr, intr9, (size_t)9 * h->C * sizeof(double), hipMemcpyHostToDevice, h->stream));
  return MCBA_OK;
}
// medians of the pairwise transforms (calibration.py:143): rel [E][6][Fpad] -> out (E, 6), counts (E) = frames the pair shares
static int pairwise_medians(hipStream_t st, const double* rel, int n_edges, int Fpad, mcba::SelState* sel_dev, double* out, double* counts) {
  const int groups = 6 * n_edges;
  mcba::launch_select(st, rel, nullptr, (size_t)Fpad, groups, Fpad, sel_dev, 1);
  int rc = check_launch();
  if (rc) return rc;
  std::vector<mcba::SelState> sel((size_t)2 * groups);
  HIPCHK(hipMemcpyAsync(sel.data(), sel_dev, sel.size() * sizeof(mcba::SelState), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  for (int g = 0; g < groups; ++g) {
    out[g] = mcba::sel_median(sel[2 * g], sel[2 * g + 1]);   // no common frame: NaN
    if (counts && g % 6 == 0) counts[g / 6] = (double)sel[2 * g].count;
  }
  return MCBA_OK;
}
static size_t up256(size_t b) { return (b + 255) / 256 * 256; }

extern "C" {

// complete_cf (C, F) bytes: 1 = every scalar of the detection is present (what get_intrinsics samples from and estimate_pose solves: :55, :107)
int mcba_calib_complete(mcba_handle* h, unsigned char* complete_cf) {
  int rc = calib_ready(h, "mcba_calib_complete");
  if (rc) return rc;
  if (!complete_cf) return fail(MCBA_ERR_ARG, "mcba_calib_complete: NULL output");
  if (!h->cal_valid && (rc = dalloc(h, &h->cal_valid, (size_t)h->C * h->F, false))) return rc;
  mcba::launch_view_complete(h->stream, h->obs_t, h->cal_valid, h->C, h->F, h->N, h->Fpad);
  if ((rc = check_launch())) return rc;
  HIPCHK(hipMemcpyAsync(complete_cf, h->cal_valid, (size_t)h->C * h->F, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return MCBA_OK;
}

// Board-plane -> pixel homographies (H[2][2] = 1) of the listed (camera, frame) views: normalised DLT.  H_out n_views x 9; ok_out n_views bytes or NULL
int mcba_calib_homographies(mcba_handle* h, const int* views, int n_views, double* H_out, unsigned char* ok_out) {
  int rc = calib_ready(h, "mcba_calib_homographies");
  if (rc) return rc;
  if (!views || n_views < 1 || !H_out) return fail(MCBA_ERR_ARG, "mcba_calib_homographies: bad argument");
  if ((rc = upload_views(h, views, n_views, "mcba_calib_homographies"))) return rc;
  if ((rc = dgrow(h, &h->cal_out, &h->cal_out_cap, (size_t)10 * n_views + 8))) return rc;
  unsigned char* okd = reinterpret_cast<unsigned char*>(h->cal_out + (size_t)9 * n_views);
  double bn[3];
  board_normalisation(h->obj_host, h->N, bn);
  mcba::launch_pnp(h->stream, 0, h->obs_t, h->obj, nullptr, h->cal_views, n_views, bn, h->C, h->F, h->N, h->Fpad, 0, 0, h->cal_out, nullptr, okd, nullptr);
  if ((rc = check_launch())) return rc;
  HIPCHK(hipMemcpyAsync(H_out, h->cal_out, (size_t)9 * n_views * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (ok_out) HIPCHK(hipMemcpyAsync(ok_out, okd, (size_t)n_views, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return MCBA_OK;
}

// cv2.solvePnP's job (calibration.py:108) for the listed views: intr9 = C x (fx fy cx cy k1 k2 p1 p2 k3); poses_out n_views x 6 (NaN = none)
int mcba_calib_view_poses(mcba_handle* h, const int* views, int n_views, const double* intr9, int undistort_iterations, int max_evaluations, double* poses_out, unsigned char* ok_out) {
  int rc = calib_ready(h, "mcba_calib_view_poses");
  if (rc) return rc;
  if (!views || n_views < 1 || !intr9 || !poses_out || undistort_iterations < 0 || max_evaluations < 1) return fail(MCBA_ERR_ARG, "mcba_calib_view_poses: bad argument");
  if ((rc = upload_views(h, views, n_views, "mcba_calib_view_poses"))) return rc;
  if ((rc = upload_intr(h, intr9))) return rc;
  if ((rc = dgrow(h, &h->cal_out, &h->cal_out_cap, (size_t)10 * n_views + 8))) return rc;
  unsigned char* okd = reinterpret_cast<unsigned char*>(h->cal_out + (size_t)9 * n_views);
  double bn[3];
  board_normalisation(h->obj_host, h->N, bn);
  mcba::launch_pnp(h->stream, 1, h->obs_t, h->obj, h->cal_intr, h->cal_views, n_views, bn, h->C, h->F, h->N, h->Fpad, undistort_iterations, max_evaluations, h->cal_out, nullptr, okd, nullptr);
  if ((rc = check_launch())) return rc;
  HIPCHK(hipMemcpyAsync(poses_out, h->cal_out, (size_t)6 * n_views * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (ok_out) HIPCHK(hipMemcpyAsync(ok_out, okd, (size_t)n_views, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return MCBA_OK;
}

// The closed-form start of get_intrinsics for every camera at once, ONE crossing (what cv2.calibrateCamera does before it refines, calibration.py:68):
// homographies of the listed views -> Zhang's K per camera from its views (k_zhang; image_sizes = C x (width, height)) -> cv2.solvePnP's job
// for the same views with that K and no distortion.  k4_out C x (fx fy cx cy); closed_out (C bytes, optional) = 1 where the closed form was used
// (0: the fallback f = max(w, h), c = the image centre); poses_out n_views x 6 (NaN = none); ok_out (n_views bytes, optional).
int mcba_calib_start(mcba_handle* h, const int* views, int n_views, const double* image_sizes, int undistort_iterations, int max_evaluations, double* k4_out, unsigned char* closed_out,
                     double* poses_out, unsigned char* ok_out) {
  int rc = calib_ready(h, "mcba_calib_start");
  if (rc) return rc;
  if (!views || n_views < 1 || !image_sizes || !k4_out || !poses_out || undistort_iterations < 0 || max_evaluations < 1) return fail(MCBA_ERR_ARG, "mcba_calib_start: bad argument");
  for (int c = 0; c < h->C; ++c)
    if (!(image_sizes[2 * c] >= 1.0 && image_sizes[2 * c + 1] >= 1.0 && image_sizes[2 * c] < 1e9 && image_sizes[2 * c + 1] < 1e9)) return fail(MCBA_ERR_ARG, "mcba_calib_start: image sizes must be finite and >= 1");
  if ((rc = upload_views(h, views, n_views, "mcba_calib_start"))) return rc;
  if (!h->cal_intr && (rc = dalloc(h, &h->cal_intr, (size_t)9 * h->C, false))) return rc;
  const size_t tail = (size_t)10 * n_views + 8;   // [0, 9 n) homographies, then poses; [9 n, 10 n) the views' valid bytes; then sizes (2 C) and closed bytes (C)
  if ((rc = dgrow(h, &h->cal_out, &h->cal_out_cap, tail + (size_t)3 * h->C + 8))) return rc;
  unsigned char* okd = reinterpret_cast<unsigned char*>(h->cal_out + (size_t)9 * n_views);
  double* sizes_d = h->cal_out + tail;
  unsigned char* closed_d = reinterpret_cast<unsigned char*>(sizes_d + (size_t)2 * h->C);
  HIPCHK(hipMemcpyAsync(sizes_d, image_sizes, (size_t)2 * h->C * sizeof(double), hipMemcpyHostToDevice, h->stream));
  double bn[3];
  board_normalisation(h->obj_host, h->N, bn);
  mcba::launch_pnp(h->stream, 0, h->obs_t, h->obj, nullptr, h->cal_views, n_views, bn, h->C, h->F, h->N, h->Fpad, 0, 0, h->cal_out, nullptr, okd, nullptr);
  mcba::launch_zhang(h->stream, h->cal_out, okd, h->cal_views, n_views, sizes_d, h->C, h->cal_intr, closed_d);
  mcba::launch_pnp(h->stream, 1, h->obs_t, h->obj, h->cal_intr, h->cal_views, n_views, bn, h->C, h->F, h->N, h->Fpad, undistort_iterations, max_evaluations, h->cal_out, nullptr, okd, nullptr);
  if ((rc = check_launch())) return rc;
  std::vector<double> intr((size_t)9 * h->C);
  HIPCHK(hipMemcpyAsync(intr.data(), h->cal_intr, intr.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(poses_out, h->cal_out, (size_t)6 * n_views * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (ok_out) HIPCHK(hipMemcpyAsync(ok_out, okd, (size_t)n_views, hipMemcpyDeviceToHost, h->stream));
  if (closed_out) HIPCHK(hipMemcpyAsync(closed_out, closed_d, (size_t)h->C, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  for (int c = 0; c < h->C; ++c)
    for (int k = 0; k < 4; ++k) k4_out[4 * c + k] = intr[(size_t)9 * c + k];
  return MCBA_OK;
}

// estimate_pose (calibration.py:74-113) of EVERY camera in one launch: the board pose of every (camera, frame) with a complete detection.
// The poses stay on the device for mcba_calib_pairwise / mcba_calib_consensus; poses_out (C, F, 6) (NaN rows = no pose), ok_out (C, F) bytes
// and evals_out (C, F) bytes (LM evaluations a view took) are optional.
int mcba_calib_poses(mcba_handle* h, const double* intr9, int undistort_iterations, int max_evaluations, double* poses_out, unsigned char* ok_out, unsigned char* evals_out) {
  int rc = calib_ready(h, "mcba_calib_poses");
  if (rc) return rc;
  if (!intr9 || undistort_iterations < 0 || max_evaluations < 1) return fail(MCBA_ERR_ARG, "mcba_calib_poses: bad argument");
  if ((rc = upload_intr(h, intr9))) return rc;
  const size_t CF = (size_t)h->C * h->F;
  if (!h->cal_poses_t && (rc = dalloc(h, &h->cal_poses_t, (size_t)6 * h->C * h->Fpad, false))) return rc;
  if (!h->cal_valid && (rc = dalloc(h, &h->cal_valid, CF, false))) return rc;
  if (!h->cal_nit && (rc = dalloc(h, &h->cal_nit, CF, false))) return rc;
  if (poses_out && (rc = dgrow(h, &h->cal_out, &h->cal_out_cap, 6 * CF))) return rc;
  double bn[3];
  board_normalisation(h->obj_host, h->N, bn);
  mcba::launch_pnp(h->stream, 1, h->obs_t, h->obj, h->cal_intr, nullptr, 0, bn, h->C, h->F, h->N, h->Fpad, undistort_iterations, max_evaluations, poses_out ? h->cal_out : nullptr, h->cal_poses_t, h->cal_valid,
                   h->cal_nit);
  if ((rc = check_launch())) return rc;
  h->have_cal_poses = true;
  if (poses_out) HIPCHK(hipMemcpyAsync(poses_out, h->cal_out, 6 * CF * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (ok_out) HIPCHK(hipMemcpyAsync(ok_out, h->cal_valid, CF, hipMemcpyDeviceToHost, h->stream));
  if (evals_out) HIPCHK(hipMemcpyAsync(evals_out, h->cal_nit, CF, hipMemcpyDeviceToHost, h->stream));
  if (poses_out || ok_out || evals_out) HIPCHK(hipStreamSynchronize(h->stream));
  return MCBA_OK;
}

// estimate_pairwise_camera_transform (calibration.py:116-143) for a list of camera pairs (c1, c2) over the poses mcba_calib_poses left on
// the device: transforms_out (n_edges, 6) = component-wise median over the common frames of T2 T1^-1; counts_out (n_edges) or NULL
int mcba_calib_pairwise(mcba_handle* h, const int* edges, int n_edges, double* transforms_out, double* counts_out) {
  int rc = calib_ready(h, "mcba_calib_pairwise");
  if (rc) return rc;
  if (!edges || n_edges < 1 || !transforms_out) return fail(MCBA_ERR_ARG, "mcba_calib_pairwise: bad argument");
  if (!h->have_cal_poses) return fail(MCBA_ERR_ARG, "mcba_calib_pairwise: call mcba_calib_poses first");
  for (int i = 0; i < 2 * n_edges; ++i)
    if (edges[i] < 0 || edges[i] >= h->C) return fail(MCBA_ERR_ARG, "mcba_calib_pairwise: camera index out of range");
  if ((rc = dgrow(h, &h->cal_views, &h->cal_views_cap, (size_t)2 * n_edges))) return rc;
  if ((rc = dgrow(h, &h->cal_rel, &h->cal_rel_cap, (size_t)6 * n_edges * h->Fpad))) return rc;
  if ((rc = dgrow(h, &h->cal_sel, &h->cal_sel_cap, (size_t)12 * n_edges))) return rc;
  HIPCHK(hipMemcpyAsync(h->cal_views, edges, (size_t)2 * n_edges * sizeof(int), hipMemcpyHostToDevice, h->stream));
  mcba::launch_pose_pairs(h->stream, h->cal_poses_t, (size_t)6 * h->Fpad, 1, (size_t)h->Fpad, h->cal_views, n_edges, h->F, h->Fpad, h->cal_rel);
  if ((rc = check_launch())) return rc;
  return pairwise_medians(h->stream, h->cal_rel, n_edges, h->Fpad, h->cal_sel, transforms_out, counts_out);
}

// consensus_calib_poses (calibration.py:239-277): extrinsics (C, 6) world -> camera; poses_out (F, 6) = nan-median over the cameras of
// T_ext^-1 T_pose, NaN rows for frames no camera has a pose for
int mcba_calib_consensus(mcba_handle* h, const double* extrinsics, double* poses_out) {
  int rc = calib_ready(h, "mcba_calib_consensus");
  if (rc) return rc;
  if (!extrinsics || !poses_out) return fail(MCBA_ERR_ARG, "mcba_calib_consensus: bad argument");
  if (!h->have_cal_poses) return fail(MCBA_ERR_ARG, "mcba_calib_consensus: call mcba_calib_poses first");
  if (!h->cal_world && (rc = dalloc(h, &h->cal_world, (size_t)6 * h->C * h->Fpad, false))) return rc;
  if ((rc = dgrow(h, &h->cal_out, &h->cal_out_cap, (size_t)6 * h->F + (size_t)6 * h->C))) return rc;
  double* d_ext = h->cal_out + (size_t)6 * h->F;
  HIPCHK(hipMemcpyAsync(d_ext, extrinsics, (size_t)6 * h->C * sizeof(double), hipMemcpyHostToDevice, h->stream));
  mcba::launch_pose_consensus(h->stream, h->cal_poses_t, (size_t)6 * h->Fpad, 1, (size_t)h->Fpad, d_ext, h->C, h->F, h->Fpad, h->cal_world, h->cal_out);
  if ((rc = check_launch())) return rc;
  HIPCHK(hipMemcpyAsync(poses_out, h->cal_out, (size_t)6 * h->F * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return MCBA_OK;
}

// calibration.py:200-277 in ONE crossing on the poses mcba_calib_poses left on the device: the medians of the pairwise transforms of the spanning
// tree's edges (mcba_calib_pairwise's work), chained from `root` into the world -> camera extrinsics on the device (k_pose_chain; :226-235), and the
// consensus board poses with them (mcba_calib_consensus' work).  edges = n_edges x (c1, c2), ordered so that c1 is `root` or the c2 of an earlier
// edge, every camera reached exactly once (n_edges = C - 1; C = 1: none): the reference's tree, sorted by distance from the root.
// extrinsics_out (C, 6), the root's row exactly 0; poses_out (F, 6); transforms_out (n_edges, 6) and counts_out (n_edges) optional.
int mcba_calib_graph(mcba_handle* h, const int* edges, int n_edges, int root, double* extrinsics_out, double* poses_out, double* transforms_out, double* counts_out) {
  int rc = calib_ready(h, "mcba_calib_graph");
  if (rc) return rc;
  if (!extrinsics_out || !poses_out || n_edges < 0 || (n_edges > 0 && !edges) || root < 0 || root >= h->C) return fail(MCBA_ERR_ARG, "mcba_calib_graph: bad argument");
  if (!h->have_cal_poses) return fail(MCBA_ERR_ARG, "mcba_calib_graph: call mcba_calib_poses first");
  if (n_edges != h->C - 1) return fail(MCBA_ERR_ARG, "mcba_calib_graph: a spanning tree of C cameras has C - 1 edges");
  {
    std::vector<char> placed((size_t)h->C, 0);
    placed[(size_t)root] = 1;
    for (int e = 0; e < n_edges; ++e) {
      const int c1 = edges[2 * e], c2 = edges[2 * e + 1];
      if (c1 < 0 || c1 >= h->C || c2 < 0 || c2 >= h->C) return fail(MCBA_ERR_ARG, "mcba_calib_graph: camera index out of range");
      if (!placed[(size_t)c1] || placed[(size_t)c2]) return fail(MCBA_ERR_ARG, "mcba_calib_graph: edges must lead away from the root, every camera reached once");
      placed[(size_t)c2] = 1;
    }
  }
  const int E = n_edges;
  if (!h->cal_world && (rc = dalloc(h, &h->cal_world, (size_t)6 * h->C * h->Fpad, false))) return rc;
  if ((rc = dgrow(h, &h->cal_out, &h->cal_out_cap, (size_t)6 * h->F + (size_t)6 * h->C + (size_t)7 * E + 8))) return rc;
  double* d_ext = h->cal_out + (size_t)6 * h->F;
  double* d_tr = d_ext + (size_t)6 * h->C;
  double* d_cnt = d_tr + (size_t)6 * E;
  if (E > 0) {
    if ((rc = dgrow(h, &h->cal_views, &h->cal_views_cap, (size_t)2 * E))) return rc;
    if ((rc = dgrow(h, &h->cal_rel, &h->cal_rel_cap, (size_t)6 * E * h->Fpad))) return rc;
    if ((rc = dgrow(h, &h->cal_sel, &h->cal_sel_cap, (size_t)12 * E))) return rc;
    HIPCHK(hipMemcpyAsync(h->cal_views, edges, (size_t)2 * E * sizeof(int), hipMemcpyHostToDevice, h->stream));
    mcba::launch_pose_pairs(h->stream, h->cal_poses_t, (size_t)6 * h->Fpad, 1, (size_t)h->Fpad, h->cal_views, E, h->F, h->Fpad, h->cal_rel);
    mcba::launch_select(h->stream, h->cal_rel, nullptr, (size_t)h->Fpad, 6 * E, h->Fpad, h->cal_sel, 1);
  }
  mcba::launch_pose_chain(h->stream, h->cal_sel, h->cal_views, E, root, h->C, d_ext, d_tr, d_cnt);
  mcba::launch_pose_consensus(h->stream, h->cal_poses_t, (size_t)6 * h->Fpad, 1, (size_t)h->Fpad, d_ext, h->C, h->F, h->Fpad, h->cal_world, h->cal_out);
  if ((rc = check_launch())) return rc;
  HIPCHK(hipMemcpyAsync(extrinsics_out, d_ext, (size_t)6 * h->C * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(poses_out, h->cal_out, (size_t)6 * h->F * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (transforms_out && E > 0) HIPCHK(hipMemcpyAsync(transforms_out, d_tr, (size_t)6 * E * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (counts_out && E > 0) HIPCHK(hipMemcpyAsync(counts_out, d_cnt, (size_t)E * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return MCBA_OK;
}

// The same two pose-graph steps for a caller's own (C, F, 6) pose array (NaN rows = no detection): what the reference's public
// estimate_pairwise_camera_transform / consensus_calib_poses take.  Stateless; host arrays in, host arrays out.
int mcba_pose_pairwise(int n_cameras, int n_frames, const double* poses, const int* edges, int n_edges, int device, double* transforms_out, double* counts_out) {
  if (n_cameras < 1 || n_frames < 1 || !poses || !edges || n_edges < 1 || !transforms_out) return fail(MCBA_ERR_ARG, "mcba_pose_pairwise: bad argument");
  for (int i = 0; i < 2 * n_edges; ++i)
    if (edges[i] < 0 || edges[i] >= n_cameras) return fail(MCBA_ERR_ARG, "mcba_pose_pairwise: camera index out of range");
  int rc = stateless_device(device, "mcba_pose_pairwise");
  if (rc) return rc;
  const int Fpad = (n_frames + 63) / 64 * 64;
  const size_t b_pose = up256((size_t)6 * n_cameras * n_frames * sizeof(double)), b_edge = up256((size_t)2 * n_edges * sizeof(int)), b_rel = up256((size_t)6 * n_edges * Fpad * sizeof(double)),
               b_sel = up256((size_t)12 * n_edges * sizeof(mcba::SelState));
  StatelessCall call;
  unsigned char* t = nullptr;
  if ((rc = call.scratch(&t, b_pose + b_edge + b_rel + b_sel))) return rc;   // one slab: the two copies below fill its input slices (d_pose, d_edge)
  double* d_pose = reinterpret_cast<double*>(t);
  int* d_edge = reinterpret_cast<int*>(t + b_pose);
  double* d_rel = reinterpret_cast<double*>(t + b_pose + b_edge);
  mcba::SelState* d_sel = reinterpret_cast<mcba::SelState*>(t + b_pose + b_edge + b_rel);
  HIPCHK(hipMemcpyAsync(d_pose, poses, (size_t)6 * n_cameras * n_frames * sizeof(double), hipMemcpyHostToDevice, nullptr));
  HIPCHK(hipMemcpyAsync(d_edge, edges, (size_t)2 * n_edges * sizeof(int), hipMemcpyHostToDevice, nullptr));
  mcba::launch_pose_pairs(nullptr, d_pose, (size_t)6 * n_frames, 6, 1, d_edge, n_edges, n_frames, Fpad, d_rel);
  if ((rc = check_launch())) return rc;
  return pairwise_medians(nullptr, d_rel, n_edges, Fpad, d_sel, transforms_out, counts_out);
}

int mcba_pose_consensus(int n_cameras, int n_frames, const double* poses, const double* extrinsics, int device, double* poses_out) {
  if (n_cameras < 1 || n_cameras > 64 || n_frames < 1 || !poses || !extrinsics || !poses_out) return fail(MCBA_ERR_ARG, "mcba_pose_consensus: 1..64 cameras, non-NULL arrays required");
  int rc = stateless_device(device, "mcba_pose_consensus");
  if (rc) return rc;
  const int Fpad = (n_frames + 63) / 64 * 64;
  const size_t b_pose = up256((size_t)6 * n_cameras * n_frames * sizeof(double)), b_ext = up256((size_t)6 * n_cameras * sizeof(double)), b_world = up256((size_t)6 * n_cameras * Fpad * sizeof(double)),
               b_out = up256((size_t)6 * n_frames * sizeof(double));
  StatelessCall call;
  unsigned char* t = nullptr;
  if ((rc = call.scratch(&t, b_pose + b_ext + b_world + b_out))) return rc;   // one slab: the two copies below fill its input slices (d_pose, d_ext)
  double* d_pose = reinterpret_cast<double*>(t);
  double* d_ext = reinterpret_cast<double*>(t + b_pose);
  double* d_world = reinterpret_cast<double*>(t + b_pose + b_ext);
  double* d_out = reinterpret_cast<double*>(t + b_pose + b_ext + b_world);
  HIPCHK(hipMemcpyAsync(d_pose, poses, (size_t)6 * n_cameras * n_frames * sizeof(double), hipMemcpyHostToDevice, nullptr));
  HIPCHK(hipMemcpyAsync(d_ext, extrinsics, (size_t)6 * n_cameras * sizeof(double), hipMemcpyHostToDevice, nullptr));
  mcba::launch_pose_consensus(nullptr, d_pose, (size_t)6 * n_frames, 6, 1, d_ext, n_cameras, n_frames, Fpad, d_world, d_out);
  if ((rc = check_launch())) return rc;
  HIPCHK(hipMemcpyAsync(poses_out, d_out, (size_t)6 * n_frames * sizeof(double), hipMemcpyDeviceToHost, nullptr));
  HIPCHK(hipStreamSynchronize(nullptr));
  return MCBA_OK;
}

// ---------------------------------------------------------------------------------------------------------
// Single-camera calibration with OpenCV's five-coefficient model (reference calibration.py:11-71 -> cv2.calibrateCamera without
// CALIB_FIX_K3 / CALIB_ZERO_TANGENT_DIST; :74-113 -> cv2.solvePnP with such coefficients): stateless; per view the Gauss-Newton block of
// (fx fy cx cy k1 k2 p1 p2 k3 | w t), the gradient and the cost at the given parameters.  calibration.py drives the LM iteration.
int mcba_calib_normal_equations(int n_views, int n_points, const double* uvs, const double* objpoints, const double* intr9, const double* poses, int device, double* out) {
  if (n_views < 1 || n_points < 1 || !uvs || !objpoints || !intr9 || !poses || !out) return fail(MCBA_ERR_ARG, "mcba_calib_normal_equations: views >= 1, points >= 1, non-NULL arrays required");
  if (int rc = stateless_device(device)) return rc;
  const size_t nuv = (size_t)2 * n_views * n_points, nobj = (size_t)3 * n_points, npose = (size_t)6 * n_views, nout = (size_t)136 * n_views;
  const size_t total = nuv + nobj + 9 + npose + nout;
  StatelessCall call;
  double* d = nullptr;
  if (int rc = call.scratch(&d, total)) return rc;   // one slab: the four put() below fill its input slices, the kernel its last nout
  if (int rc = call.put(d, uvs, nuv)) return rc;
  if (int rc = call.put(d + nuv, objpoints, nobj)) return rc;
  if (int rc = call.put(d + nuv + nobj, intr9, 9)) return rc;
  if (int rc = call.put(d + nuv + nobj + 9, poses, npose)) return rc;
  mcba::launch_calib_views(nullptr, d, d + nuv, d + nuv + nobj, d + nuv + nobj + 9, n_views, n_points, d + nuv + nobj + 9 + npose);
  if (int rc = check_launch()) return rc;
  return call.download(out, d + nuv + nobj + 9 + npose, nout);
}

}  // extern "C"
