// An FTE iterate seen in image space (gfx950, fp64): per (frame, camera, marker) the predicted pixel, its 2 x 2 Laplace
// covariance J_pi cov_pos J_pi^T, the residual against the detection, the curvature weight the solve gave it, a gating
// distance and flags (acinoset_hip.h: acino_fte_reprojection).
//
// One workgroup handles FPB frames: phases A and B are the FK of k_fk (sin / cos, then the chain column-parallel into LDS -
// once per frame, not once per camera), phase C deals the workgroup's nf * C * 20 (frame, camera, marker) entries to its
// threads in output order, so every output array is written as one contiguous run per workgroup.  The projection and the
// loss are the assembly's own device functions (fisheye_nlp_uv / fisheye_nlp_jac, pinhole_project, redescending), applied
// in the assembly's order to the assembly's operands: uv, res and weight carry its bits.
// A streaming kernel: 24 B of detection + the marker's 72 B of cov_pos (shared by the C cameras through the cache) in, up
// to 113 B out per entry, a few hundred fp64 operations with one atan and two exp in between.
#include "fte_reproj.hpp"

#include "cheetah_fk.hpp"

namespace acino {

struct ReprojLds {
  static constexpr bool kHasOm = false;
  double sc[22][2];       // sin, cos of the active angles (index a-3)
  double pos[21][3];      // markers 0..19, head = 20
};

template <bool PINHOLE>
__global__ void __launch_bounds__(256)
k_fte_reproj(const FteConst* __restrict__ cst, const acino_fte_state* __restrict__ st, const double* __restrict__ det,
             const double* __restrict__ x0, const double* __restrict__ x1, const double* __restrict__ cov_pos,
             double* __restrict__ uv_out, double* __restrict__ cov_out, double* __restrict__ res_out,
             double* __restrict__ w_out, double* __restrict__ m2_out, uint8_t* __restrict__ flags_out) {
  __shared__ ReprojLds F[FPB];
  const int tid = threadIdx.x;
  const double* __restrict__ xh = st->cur ? x1 : x0;
  const FteConst& K = *cst;
  const int N = K.n_frames, C = K.n_cams;
  const int f0 = (int)blockIdx.x * FPB;
  const int nf = min(FPB, N - f0);
  // ---- A: sincos, head position
  for (int task = tid; task < nf * NP; task += blockDim.x) {
    int f = task / NP, a = task - f * NP;
    double xv = xh[(int64_t)(f0 + f + HALO) * NP + a];
    if (a < 3) {
      F[f].pos[20][a] = xv;
    } else {
      double s, c;
      sincos(xv, &s, &c);
      F[f].sc[a - 3][0] = s;
      F[f].sc[a - 3][1] = c;
    }
  }
  __syncthreads();
  // ---- B: chain, one thread per (frame, column)
  for (int task = tid; task < nf * 3; task += blockDim.x) fk_columns(F[task / 3], task % 3);
  __syncthreads();
  // ---- C: one (frame, camera, marker) per thread and turn
  const double nan = __builtin_nan("");
  const double Rm = 1.0 / K.inv_r, R2 = Rm * Rm;
  const int per_frame = C * NL;
  for (int task = tid; task < nf * per_frame; task += blockDim.x) {
    const int f = task / per_frame, rem = task - f * per_frame;
    const int ci = rem / NL, l = rem - ci * NL;
    const int n = f0 + f;
    const int64_t e = (int64_t)f0 * per_frame + task;          // = (n * C + ci) * 20 + l
    const double px = F[f].pos[l][0], py = F[f].pos[l][1], pz = F[f].pos[l][2];
    const double* d = det + e * 3;
    const double um = d[0], vm = d[1], lik = d[2];
    const bool finite = isfinite(um) && isfinite(vm);
    double w = (lik > K.dlc_thresh && finite) ? K.inv_r : 0.0;
    const auto& cam = cam_rec<PINHOLE>(K, ci);
    const double* Rc = cam.R;
    const double* tc = cam.t;
    double xc = Rc[0] * px + Rc[1] * py + Rc[2] * pz + tc[0];
    double yc = Rc[3] * px + Rc[4] * py + Rc[5] * pz + tc[1];
    double zc = Rc[6] * px + Rc[7] * py + Rc[8] * pz + tc[2];
    const bool behind = zc < 1e-6, sing = fabs(zc) < 1e-9;
    if (sing) w = 0.0;
    double u = nan, v = nan, ru = nan, rv = nan, hu = 0.0, hv = 0.0, m2 = nan, s00 = nan, s01 = nan, s11 = nan;
    if (!sing) {
      double jc[2][3];
      if constexpr (PINHOLE) {
        double uv[2];
        pinhole_project<true>(cam, xc, yc, zc, uv, jc);
        u = uv[0];
        v = uv[1];
      } else {
        FisheyeNlp fp;
        fisheye_nlp_uv(cam, xc, yc, zc, fp, u, v);
        fisheye_nlp_jac(cam, fp, jc[0], jc[1]);
      }
      if (finite) {
        ru = u - um;
        rv = v - vm;
      }
      if (w > 0) {
        double rho, drho;
        redescending<true>(K.loss, w * (u - um), rho, drho, hu);
        redescending<true>(K.loss, w * (v - vm), rho, drho, hv);
      }
      if (cov_pos) {
        double ju[3], jv[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          ju[j] = jc[0][0] * Rc[j] + jc[0][1] * Rc[3 + j] + jc[0][2] * Rc[6 + j];
          jv[j] = jc[1][0] * Rc[j] + jc[1][1] * Rc[3 + j] + jc[1][2] * Rc[6 + j];
        }
        const double* S = cov_pos + ((int64_t)n * NL + l) * 9;
        double tu[3], tv[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          tu[i] = S[3 * i] * ju[0] + S[3 * i + 1] * ju[1] + S[3 * i + 2] * ju[2];
          tv[i] = S[3 * i] * jv[0] + S[3 * i + 1] * jv[1] + S[3 * i + 2] * jv[2];
        }
        s00 = ju[0] * tu[0] + ju[1] * tu[1] + ju[2] * tu[2];
        s11 = jv[0] * tv[0] + jv[1] * tv[1] + jv[2] * tv[2];
        s01 = 0.5 * ((ju[0] * tv[0] + ju[1] * tv[1] + ju[2] * tv[2]) + (jv[0] * tu[0] + jv[1] * tu[1] + jv[2] * tu[2]));
        const double a00 = s00 + R2, a11 = s11 + R2;
        m2 = (a11 * ru * ru - 2.0 * s01 * ru * rv + a00 * rv * rv) / (a00 * a11 - s01 * s01);
      } else {
        m2 = (ru * ru + rv * rv) * (K.inv_r * K.inv_r);
      }
    }
    if (uv_out) {
      uv_out[2 * e] = u;
      uv_out[2 * e + 1] = v;
    }
    if (cov_out) {
      cov_out[4 * e] = s00;
      cov_out[4 * e + 1] = s01;
      cov_out[4 * e + 2] = s01;
      cov_out[4 * e + 3] = s11;
    }
    if (res_out) {
      res_out[2 * e] = ru;
      res_out[2 * e + 1] = rv;
    }
    if (w_out) {
      w_out[2 * e] = hu;
      w_out[2 * e + 1] = hv;
    }
    if (m2_out) m2_out[e] = m2;
    if (flags_out) flags_out[e] = (uint8_t)((w > 0 ? 1 : 0) | (behind ? 2 : 0) | (sing ? 4 : 0));
  }
}

int launch_fte_reproj(const PostIn& in, const double* d_cov_pos, double* d_uv, double* d_cov_uv, double* d_res,
                      double* d_weight, double* d_mahal2, uint8_t* d_flags, hipStream_t s) {
  const int nb = (in.h_c->n_frames + FPB - 1) / FPB;
  if (nb == 0) return ACINO_OK;
  const auto k = in.h_c->camera_model == CAMERA_PINHOLE ? k_fte_reproj<true> : k_fte_reproj<false>;
  hipLaunchKernelGGL(k, dim3(nb), dim3(256), 0, s, in.d_c, in.d_st, in.d_det, in.x[0], in.x[1], d_cov_pos, d_uv, d_cov_uv, d_res,
                     d_weight, d_mahal2, d_flags);
  ACINO_LAUNCH_CHECK();
  return ACINO_OK;
}

}  // namespace acino
