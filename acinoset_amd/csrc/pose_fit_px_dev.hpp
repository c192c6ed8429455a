// What the two pose fits from the detections share (pose_fit_px.hip: the cheetah; skel_pose_fit_px.hip: a link program): what
// their kernels read and write beyond PoseFitIo, the projection of a model point into a camera of the rig, and the checks of
// the C entries on the pixel parameters.
#pragma once
#include "pinhole.hpp"
#include "pose_fit_dev.hpp"

namespace acino {

// what the kernel reads and writes beyond PoseFitIo
struct PxArgs {
  const double *det, *cams;
  int n_cams;
  double thresh, fs2, ifs2, inv_sigma;
  uint16_t* ndet;
  double* weight;
};

// marker position X in camera cm: pixel, d(uv)/dX = J_pi R_c (JAC), and whether it is in front
template <bool JAC, class Rec>
__device__ __forceinline__ bool px_project(const Rec& cm, const double* X, double uv[2], double JR[2][3]) {
  const double xc = cm.R[0] * X[0] + cm.R[1] * X[1] + cm.R[2] * X[2] + cm.t[0];
  const double yc = cm.R[3] * X[0] + cm.R[4] * X[1] + cm.R[5] * X[2] + cm.t[1];
  const double zc = cm.R[6] * X[0] + cm.R[7] * X[1] + cm.R[8] * X[2] + cm.t[2];
  double J[2][3];
  mv_project(cm, xc, yc, zc, uv, J);
  if (JAC) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      JR[k][0] = J[k][0] * cm.R[0] + J[k][1] * cm.R[3] + J[k][2] * cm.R[6];
      JR[k][1] = J[k][0] * cm.R[1] + J[k][1] * cm.R[4] + J[k][2] * cm.R[7];
      JR[k][2] = J[k][0] * cm.R[2] + J[k][1] * cm.R[5] + J[k][2] * cm.R[8];
    }
  }
  return zc > 0.0;
}

// the checks of both pixel entries on the parameter block (prm is not NULL) and the camera count; ``fit`` receives the block of
// pf_check_params, ``count_text`` names the range of min_detections, 1 .. slots * n_cams
inline int px_check_params(const acino_pose_fit_px_params* prm, int64_t n_frames, int n_cams, int slots, const char* count_text,
                           acino_pose_fit_params& fit) {
  ACINO_REQUIRE(n_cams >= 1 && n_cams <= ACINO_MAX_CAMS, "n_cams must be 1..16");
  ACINO_REQUIRE(prm->camera_model == 0 || prm->camera_model == 1, "camera_model must be 0 (fisheye) or 1 (pinhole)");
  fit = {prm->max_iter, prm->min_detections, prm->lam0, prm->ftol, prm->xtol, prm->prior_sigma, 1.0};
  if (int rc = pf_check_params(&fit, n_frames, slots * n_cams, count_text)) return rc;
  ACINO_REQUIRE(prm->thresh == prm->thresh, "thresh must not be NaN");
  ACINO_REQUIRE(prm->f_scale > 0 && prm->f_scale < INFINITY, "f_scale must be > 0");
  ACINO_REQUIRE(prm->sigma_px > 0 && prm->sigma_px < INFINITY, "sigma_px must be > 0");
  return ACINO_OK;
}

inline void px_fill_args(PxArgs& b, const acino_pose_fit_px_params* prm, const double* d_det, const double* d_cams, int n_cams,
                         uint16_t* d_ndet, double* d_weight) {
  b.det = d_det, b.cams = d_cams, b.n_cams = n_cams, b.thresh = prm->thresh;
  b.fs2 = prm->f_scale * prm->f_scale, b.ifs2 = 1.0 / b.fs2, b.inv_sigma = 1.0 / prm->sigma_px;
  b.ndet = d_ndet, b.weight = d_weight;
}

}  // namespace acino
