// Sensitivity of an FTE trajectory to the camera extrinsics (gfx950, fp64): S = d x_hat / d c = -A^-1 G, and the
// "consider" covariance S Sigma_c S^T it gives for a covariance Sigma_c of the extrinsics (acinoset_hip.h:
// acino_fte_calibration_sensitivity).  A, the pinned set and the node grid are those of fte_cov.hip.
//
//   k_fte_calib_rhs      one workgroup per frame: FK once into LDS with the rotation axes, J_l from omega_a x (p_l - pivot_a)
//                        (fte_cov_dev.hpp), per (camera, marker) the 3 x 6 block J_pi^T (w^2 h) J_c with the projection and the
//                        loss of the assembly (its device functions, its order, its operands), then
//                        -G_n[p, 6c + j] = -sum_l J_l[:, p] . block_cl[:, j] in a fixed order (no atomics), written as
//                        column 6c + j of the right-hand side [6C][N][25]; rows of pinned variables 0
//   launch_fte_solve_columns (fte_cov.hip)   A^-1 on the 6C columns: the sampler's sweep and factors, k_fte_sample_fwdsub,
//                        k_fte_sample_backsub<true>
//   k_fte_calib_combine  one workgroup per frame: S_n [25][6C] out, T = S_n Sigma_c, cov_x_cal = T S_n^T (Sigma_c is only PSD -
//                        a held camera has zero rows - and is never factored), J_l cov_x_cal J_l^T and its trace; the
//                        symmetric outputs are computed on one triangle and mirrored
//
// J_c = d uv / d (dw_c, dt_c) for R_c <- exp([dw]x) R_c, t_c <- t_c + dt: the camera-frame point moves by dw x (R_c p) + dt,
// so with j the camera-frame Jacobian row of a pixel component J_c = [ (R_c p) x j | j ].
// No workgroup waits for another; NaNs of a failed factorisation run through (the error word is launch_fte_cov_rates').
#include "fte_calib.hpp"

#include "fte_cov_dev.hpp"

namespace acino {

size_t calib_workspace_bytes(int64_t n_frames, int64_t clip_len, int n_cams) {
  return cov_workspace_bytes(n_frames, clip_len) + 2 * (size_t)(6 * n_cams) * (size_t)n_frames * NP * sizeof(double);
}

namespace {
constexpr int CJ = NL * 3 * NP;                            // J[(l * 3 + i) * NP + p]
constexpr int CF_DOUBLES = (sizeof(CovFrame) + 7) / 8;
size_t calib_rhs_lds(int C) { return (CF_DOUBLES + CJ + (size_t)C * NL * 18) * sizeof(double) + BS * sizeof(int); }
size_t calib_combine_lds(int C) {
  return (CF_DOUBLES + CJ + 2 * (size_t)NP * 6 * C + NP * NP + NL * 9) * sizeof(double) + BS * sizeof(int);
}

// FK of frame n into F (sin / cos, the chain column-parallel, the rotation axes), then J; ends with a barrier
__device__ __forceinline__ void calib_fk_jac(CovFrame& F, double* J, const double* xh, int64_t n, int tid) {
  if (tid < NP) {
    const double xv = xh[(n + HALO) * NP + tid];
    if (tid < 3) {
      F.pos[20][tid] = xv;
    } else {
      double s, c;
      sincos(xv, &s, &c);
      F.sc[tid - 3][0] = s;
      F.sc[tid - 3][1] = c;
    }
  }
  __syncthreads();
  if (tid < 3) fk_columns(F, tid);
  __syncthreads();
  for (int e = tid; e < CJ; e += 256) J[e] = rate_jac(F, e / (3 * NP), (e / NP) % 3, e % NP);
  __syncthreads();
}
}  // namespace

template <bool PINHOLE>
__global__ void __launch_bounds__(256)
k_fte_calib_rhs(const FteConst* __restrict__ cst, const acino_fte_state* __restrict__ st, const double* __restrict__ det,
                const double* x0, const double* x1, const double* g0, const double* g1, const double* H0, const double* H1,
                double* __restrict__ rhs) {
  extern __shared__ __attribute__((aligned(16))) double calib_smem[];
  CovFrame& F = *reinterpret_cast<CovFrame*>(calib_smem);
  double* J = calib_smem + CF_DOUBLES;
  double* Mb = J + CJ;                                     // [(c * NL + l) * 18 + i * 6 + j]
  const FteConst& K = *cst;
  const int N = K.n_frames, C = K.n_cams;
  int* code = reinterpret_cast<int*>(Mb + (size_t)C * NL * 18);
  const int tid = threadIdx.x;
  const int64_t n = blockIdx.x;
  const int cur = st->cur;
  const CovIn in{cur ? x1 : x0, cur ? g1 : g0, cur ? H1 : H0};
  cov_codes(code, in, K, n, 1, tid);                       // (rows 0 .. 24: this frame)
  calib_fk_jac(F, J, in.x, n, tid);
  for (int task = tid; task < C * NL; task += 256) {
    const int ci = task / NL, l = task - ci * NL;
    const double px = F.pos[l][0], py = F.pos[l][1], pz = F.pos[l][2];
    const double* d = det + ((n * C + ci) * NL + l) * 3;
    const double um = d[0], vm = d[1], lik = d[2];
    double w = (lik > K.dlc_thresh && isfinite(um) && isfinite(vm)) ? K.inv_r : 0.0;
    const auto& cam = cam_rec<PINHOLE>(K, ci);
    const double* Rc = cam.R;
    const double* tc = cam.t;
    const double xc = Rc[0] * px + Rc[1] * py + Rc[2] * pz + tc[0];
    const double yc = Rc[3] * px + Rc[4] * py + Rc[5] * pz + tc[1];
    const double zc = Rc[6] * px + Rc[7] * py + Rc[8] * pz + tc[2];
    if (fabs(zc) < 1e-9) w = 0.0;
    double* M = Mb + (size_t)task * 18;
    if (w == 0.0) {
#pragma unroll
      for (int e = 0; e < 18; ++e) M[e] = 0.0;
      continue;
    }
    double uv[2], jc[2][3];
    project_jac(cam, xc, yc, zc, uv, jc);
    const double u = uv[0], v = uv[1];
    double rho, drho, h_u = 0.0, h_v = 0.0;
    redescending<true>(K.loss, w * (u - um), rho, drho, h_u);
    redescending<true>(K.loss, w * (v - vm), rho, drho, h_v);
    const double hu = w * w * h_u, hv = w * w * h_v;
    double ju[3], jv[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      ju[j] = jc[0][0] * Rc[j] + jc[0][1] * Rc[3 + j] + jc[0][2] * Rc[6 + j];
      jv[j] = jc[1][0] * Rc[j] + jc[1][1] * Rc[3 + j] + jc[1][2] * Rc[6 + j];
    }
    const double q0 = Rc[0] * px + Rc[1] * py + Rc[2] * pz;             // R_c p
    const double q1 = Rc[3] * px + Rc[4] * py + Rc[5] * pz;
    const double q2 = Rc[6] * px + Rc[7] * py + Rc[8] * pz;
    const double cu[6] = {q1 * jc[0][2] - q2 * jc[0][1], q2 * jc[0][0] - q0 * jc[0][2], q0 * jc[0][1] - q1 * jc[0][0],
                          jc[0][0], jc[0][1], jc[0][2]};
    const double cv[6] = {q1 * jc[1][2] - q2 * jc[1][1], q2 * jc[1][0] - q0 * jc[1][2], q0 * jc[1][1] - q1 * jc[1][0],
                          jc[1][0], jc[1][1], jc[1][2]};
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 6; ++j) M[i * 6 + j] = hu * ju[i] * cu[j] + hv * jv[i] * cv[j];
  }
  __syncthreads();
  for (int task = tid; task < 6 * C * NP; task += 256) {
    const int col = task / NP, p = task - col * NP;
    const int ci = col / 6, j = col - 6 * ci;
    double acc = 0.0;
    if (code[p] == 0) {
      const double* M = Mb + (size_t)ci * NL * 18 + j;
      for (int l = 0; l < NL; ++l) {
        acc += J[(l * 3) * NP + p] * M[l * 18];
        acc += J[(l * 3 + 1) * NP + p] * M[l * 18 + 6];
        acc += J[(l * 3 + 2) * NP + p] * M[l * 18 + 12];
      }
      acc = -acc;
    }
    rhs[((size_t)col * N + n) * NP + p] = acc;
  }
}

__global__ void __launch_bounds__(256)
k_fte_calib_combine(const FteConst* __restrict__ cst, const acino_fte_state* __restrict__ st, const double* x0,
                    const double* x1, const double* __restrict__ sol, const double* __restrict__ sigma,
                    double* __restrict__ sens, double* __restrict__ cov_x, double* __restrict__ cov_pos,
                    double* __restrict__ std_pos) {
  extern __shared__ __attribute__((aligned(16))) double calib_smem[];
  const FteConst& K = *cst;
  const int N = K.n_frames, W = 6 * K.n_cams;
  CovFrame& F = *reinterpret_cast<CovFrame*>(calib_smem);
  double* J = calib_smem + CF_DOUBLES;
  double* Sm = J + CJ;                                     // S_n [25][W]
  double* Tm = Sm + NP * W;                                // S_n Sigma_c [25][W]
  double* Cx = Tm + NP * W;                                // cov_x_cal [25][25]
  double* Cp = Cx + NP * NP;                               // cov_pos_cal [20][9]
  const int tid = threadIdx.x;
  const int64_t n = blockIdx.x;
  for (int e = tid; e < NP * W; e += 256) {
    const int col = e / NP, p = e - col * NP;
    Sm[p * W + col] = sol[((size_t)col * N + n) * NP + p];
  }
  __syncthreads();
  if (sens)
    for (int e = tid; e < NP * W; e += 256) sens[n * (NP * W) + e] = Sm[e];
  if (!sigma) return;
  for (int e = tid; e < NP * W; e += 256) {
    const int p = e / W, j = e - p * W;
    double acc = 0.0;
    for (int i = 0; i < W; ++i) acc += Sm[p * W + i] * sigma[(size_t)i * W + j];
    Tm[e] = acc;
  }
  __syncthreads();
  for (int e = tid; e < NP * NP; e += 256) {
    const int p = e / NP, q = e - p * NP;
    if (p <= q) {
      double acc = 0.0;
      for (int j = 0; j < W; ++j) acc += Tm[p * W + j] * Sm[q * W + j];
      Cx[p * NP + q] = acc;
      Cx[q * NP + p] = acc;
    }
  }
  __syncthreads();
  if (cov_x)
    for (int e = tid; e < NP * NP; e += 256) cov_x[n * (NP * NP) + e] = Cx[e];
  if (!cov_pos && !std_pos) return;
  calib_fk_jac(F, J, st->cur ? x1 : x0, n, tid);
  if (tid < NL * 6) {                                      // the upper triangle of J_l cov_x_cal J_l^T, mirrored
    const int l = tid / 6, t = tid - 6 * l;
    const int i = t < 3 ? 0 : (t < 5 ? 1 : 2), i2 = t < 3 ? t : (t < 5 ? t - 2 : 2);
    const double* Ja = J + (l * 3 + i) * NP;
    const double* Jb = J + (l * 3 + i2) * NP;
    double acc = 0.0;
    for (int q = 0; q < NP; ++q) {
      double r = 0.0;
      for (int p = 0; p < NP; ++p) r += Ja[p] * Cx[p * NP + q];
      acc += r * Jb[q];
    }
    Cp[l * 9 + 3 * i + i2] = acc;
    Cp[l * 9 + 3 * i2 + i] = acc;
  }
  __syncthreads();
  if (cov_pos)
    for (int e = tid; e < NL * 9; e += 256) cov_pos[n * (NL * 9) + e] = Cp[e];
  if (std_pos && tid < NL) std_pos[n * NL + tid] = sqrt(fmax(Cp[tid * 9] + Cp[tid * 9 + 4] + Cp[tid * 9 + 8], 0.0));
}

int launch_fte_calib(const PostIn& in, void* d_ws, const double* d_cov_cams, double* d_sens, double* d_cov_x_cal,
                     double* d_cov_pos_cal, double* d_std_pos_cal, hipStream_t s) {
  const FteConst& h_c = *in.h_c;
  const int N = h_c.n_frames, C = h_c.n_cams;
  if (N == 0) return ACINO_OK;
  double* d_b = reinterpret_cast<double*>(reinterpret_cast<char*>(d_ws) + cov_workspace_bytes(N, h_c.clip_len));
  double* d_y = d_b + (size_t)(6 * C) * N * NP;
  const size_t lds_rhs = calib_rhs_lds(C), lds_comb = calib_combine_lds(C);
  const auto k_rhs = h_c.camera_model == CAMERA_PINHOLE ? k_fte_calib_rhs<true> : k_fte_calib_rhs<false>;
  ACINO_HIP_CHECK(set_dyn_lds(k_rhs, lds_rhs));
  hipLaunchKernelGGL(k_rhs, dim3(N), dim3(256), lds_rhs, s, in.d_c, in.d_st, in.d_det, in.x[0], in.x[1], in.g[0], in.g[1],
                     in.H[0], in.H[1], d_b);
  ACINO_LAUNCH_CHECK();
  if (int rc = launch_fte_solve_columns(in, d_ws, 6 * C, d_b, d_y, s)) return rc;
  ACINO_HIP_CHECK(set_dyn_lds(k_fte_calib_combine, lds_comb));
  hipLaunchKernelGGL(k_fte_calib_combine, dim3(N), dim3(256), lds_comb, s, in.d_c, in.d_st, in.x[0], in.x[1], d_b, d_cov_cams,
                     d_sens, d_cov_x_cal, d_cov_pos_cal, d_std_pos_cal);
  ACINO_LAUNCH_CHECK();
  return ACINO_OK;
}

}  // namespace acino
