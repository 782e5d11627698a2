// mcba_traj_host.h -- the host side that the two fits of tracks on their detections share (mcba_traj_refine_api.hip, mcba_skeltraj_api.hip; host
// only): the reprojection planes of a chunk of tracks, how a chunk starts (load, count, which tracks run) and how every iteration and the
// returned point open (the pending steps applied, the linearisation).  The loops are the entry points' own: one decides per track, the other
// per call, and what they launch after the opening differs.
#pragma once
#include "mcba_smooth_host.h"
#include "mcba_traj_refine_math.h"

namespace mcba_internal {

struct TrackFit {
  SmoothChunks& ch;
  const char* family;   // what a refused launch is reported under
  int C;
  const double *uvs, *weights, *pixel_std, *start;   // (C, T, K, 2), (C, T, K) or NULL, (C), (T, K, 3)
  double f_scale;
  mcba::KpCam* d_cams = nullptr;
  double *d_det = nullptr, *d_sw = nullptr, *d_x = nullptr, *d_d = nullptr, *d_H = nullptr, *d_G = nullptr, *d_alpha = nullptr;
  int *d_run = nullptr, *d_nsg = nullptr, *d_nbs = nullptr;
  // what begin() left of the chunk ch.begin_shared(c) left: the planes for the kernels, the counts, the status every track starts with, the
  // tracks that run (ch.h_list; h_run: the same as flags, not uploaded)
  mcba::TrData rd{};
  std::vector<double> h_det, h_sw, h_x;
  std::vector<int> h_nus, h_nsg, h_nbs, h_stat, h_run;

  int bad_launch() const {
    g_err = std::string(family) + ": bad launch";
    return MCBA_ERR_ARG;
  }

  // after ch.setup_shared(): the camera table and the planes, sized for the widest chunk
  int setup(const double* cam12, const double* dist5) {
    StatelessCall& call = ch.call;
    const size_t Kc = (size_t)ch.Kc, TK = ch.T * Kc;
    if (int rc = upload_kp_cams(call, C, cam12, dist5, &d_cams)) return rc;
    if (int rc = call.scratch(&d_det, 2 * C * TK)) return rc;
    if (int rc = call.scratch(&d_sw, C * TK)) return rc;
    if (int rc = call.scratch(&d_x, 3 * TK)) return rc;
    if (int rc = call.scratch(&d_d, 3 * TK)) return rc;
    if (int rc = call.scratch(&d_H, 6 * TK)) return rc;
    if (int rc = call.scratch(&d_G, 3 * TK)) return rc;
    if (int rc = call.scratch(&d_alpha, Kc)) return rc;
    if (int rc = call.scratch(&d_run, Kc)) return rc;
    if (int rc = call.scratch(&d_nsg, Kc)) return rc;
    if (int rc = call.scratch(&d_nbs, Kc)) return rc;
    return MCBA_OK;
  }

  // after ch.begin_shared(c): the chunk's detections (C, T kc) pairs, sqrt(w) / pixel_std beside them and the start on the device; the count
  int begin() {
    StatelessCall& call = ch.call;
    const size_t T = ch.T, K = ch.K, k0 = ch.k0, kc = (size_t)ch.kc, tk = ch.tk;
    h_sw.resize(C * tk);
    mcba::kp_weight_box(weights, pixel_std, C, T, K, 0, T, k0, kc, h_sw.data());
    if (int rc = call.put(d_det, gather_tracks(uvs, C, T, K, k0, kc, 2, h_det), 2 * C * tk)) return rc;
    if (int rc = call.put(d_sw, h_sw.data(), C * tk)) return rc;
    if (int rc = call.put(d_x, gather_tracks(start, 1, T, K, k0, kc, 3, h_x), 3 * tk)) return rc;
    rd = mcba::TrData{T, d_det, d_sw, d_x, d_d, d_H, d_G, ch.d_ia2, f_scale * f_scale, 1.0 / (f_scale * f_scale)};
    if (int rc = ch.open()) return rc;
    if (mcba::launch_traj_count(nullptr, rd, C, ch.kc, ch.d_nus, d_nsg, d_nbs) != 0) return bad_launch();
    if (int rc = ch.close()) return rc;
    h_nus.resize(kc); h_nsg.resize(kc); h_nbs.resize(kc);
    if (int rc = call.download(h_nus.data(), ch.d_nus, kc)) return rc;
    if (int rc = call.download(h_nsg.data(), d_nsg, kc)) return rc;
    if (int rc = call.download(h_nbs.data(), d_nbs, kc)) return rc;
    h_stat.resize(kc); h_run.assign(kc, 0);
    ch.h_list.clear();
    for (int k = 0; k < ch.kc; ++k) {
      h_stat[k] = mcba::traj_start_status(h_nus[k], h_nbs[k] != 0);
      if (h_stat[k] == mcba::TR_OK) { ch.h_list.push_back(k); h_run[k] = 1; }
    }
    return MCBA_OK;
  }

  // the opening of every iteration and of the returned point: a bracket that starts with the accepted steps not yet applied (pending: there
  // are some; h_alpha per track, 0 = none) and the linearisation at the point, on the tracks d_run flags.  The caller goes on in the bracket
  // and closes it; split: with close_split()
  int open_linearised(int loss, bool pending, const std::vector<double>& h_alpha, bool split = false) {
    if (pending) if (int rc = ch.call.put(d_alpha, h_alpha.data(), (size_t)ch.kc)) return rc;
    if (int rc = ch.open(split)) return rc;
    if (pending && mcba::launch_traj_apply(nullptr, rd, ch.kc, d_alpha) != 0) return bad_launch();
    if (mcba::launch_traj_linearise(nullptr, loss, rd, d_cams, C, ch.kc, d_run) != 0) return bad_launch();
    return MCBA_OK;
  }
};

}  // namespace mcba_internal
