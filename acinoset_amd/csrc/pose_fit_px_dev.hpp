// What the two pose fits from the detections share (pose_fit_px.hip: the cheetah; skel_pose_fit_px.hip: a link program): what
// their kernels read and write beyond PoseFitIo, the projection of a model point into a camera of the rig, the pixel
// measurement (px_valid, px_pair_cost, px_cost_finish, px_pair_rows, px_store_outputs: a model keeps where a position lives,
// its mask packing, camera grouping and Gram product) and the checks of the C entries on the pixel parameters.  The pieces
// keep the statement order the kernels had (the detection's address after the projection; profiles/pose_fit_shared/).
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

// a detection (x, y, likelihood) counts: likelihood above thresh, both pixel values finite
__device__ __forceinline__ bool px_valid(const double* d, double thresh) {
  return d[2] > thresh && m_finite(d[0]) && m_finite(d[1]);
}

// the two log terms of one valid pair: X in camera cm against detection e = c L + l of det; ``behind`` is set when z_c <= 0
template <class Rec>
__device__ __forceinline__ double px_pair_cost(const PxArgs& b, const Rec& cm, const double* X, const double* det, int e,
                                               bool& behind) {
  double uv[2];
  behind = !px_project<false>(cm, X, uv, nullptr) || behind;
  const double* d = det + e * 3;
  const double r0 = uv[0] - d[0], r1 = uv[1] - d[1];
  return 0.5 * b.fs2 * (log1p(r0 * r0 * b.ifs2) + log1p(r1 * r1 * b.ifs2));
}

// F from a lane's sum of pair terms: times 1 / sigma_px^2, the ridge of xv about m by lanes 3 .. P-1, the 64 partial sums by a
// butterfly whose additions pair the same operands in every lane (the same bits in every lane); +inf when a pair was behind
__device__ __forceinline__ double px_cost_finish(double part, const double* xv, const double* m, double kappa, int P, int lane,
                                                 const PxArgs& b, bool behind) {
  part *= b.inv_sigma * b.inv_sigma;
  if (lane >= 3 && lane < P) {
    const double e = xv[lane] - m[lane];
    part += 0.5 * kappa * e * e;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) part += __shfl_xor(part, off);
  return __any(behind) ? __builtin_huge_val() : part;
}

// the weighted rows of one valid pair, w = 1 / (1 + r^2 / f^2) per coordinate: jr = sqrt(w) / sigma_px * (J_pi R_c), u = ... * r
template <class Rec>
__device__ __forceinline__ void px_pair_rows(const PxArgs& b, const Rec& cm, const double* X, const double* det, int L, int c,
                                             int l, double jr[6], double u[2]) {
  double uv[2], JR[2][3];
  px_project<true>(cm, X, uv, JR);
  const double* d = det + (c * L + l) * 3;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const double r = uv[k] - d[k];
    const double sw = sqrt(rcp64(1.0 + r * r * b.ifs2)) * b.inv_sigma;
    jr[3 * k] = sw * JR[k][0];
    jr[3 * k + 1] = sw * JR[k][1];
    jr[3 * k + 2] = sw * JR[k][2];
    u[k] = sw * r;
  }
}

// frame n's count of valid detections and, over the L n_cams pairs, the weight every coordinate ended with at the positions
// pos(l) of the returned x - NaN when not live, exactly 0 for an invalid detection; valid(c, l) reads the model's mask
template <class Rec, class Valid, class Pos>
__device__ __forceinline__ void px_store_outputs(const PxArgs& b, const Rec* cams, const double* det, int L, int64_t n, int n_det,
                                                 bool live, int lane, Valid&& valid, Pos&& pos) {
  if (lane == 0 && b.ndet) b.ndet[n] = (uint16_t)n_det;
  if (!b.weight) return;
  const int pairs = L * b.n_cams;
  double* out = b.weight + n * pairs * 2;
  for (int t = lane; t < pairs; t += 64) {
    const int c = t / L, l = t - c * L;
    double w0 = live ? 0.0 : __builtin_nan(""), w1 = w0;
    if (live && valid(c, l)) {
      double uv[2];
      px_project<false>(cams[c], pos(l), uv, nullptr);
      const double* d = det + (c * L + l) * 3;
      const double r0 = uv[0] - d[0], r1 = uv[1] - d[1];
      w0 = rcp64(1.0 + r0 * r0 * b.ifs2);
      w1 = rcp64(1.0 + r1 * r1 * b.ifs2);
    }
    out[2 * t] = w0;
    out[2 * t + 1] = w1;
  }
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
