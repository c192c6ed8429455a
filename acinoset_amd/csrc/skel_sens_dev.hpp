// What the sensitivities of a generic-skeleton FTE trajectory share on the device (skel_calib.hip: to the camera extrinsics;
// skel_links.hip: to the link lengths).  Both are S = -A^-1 G with another G, and the "consider" covariances S Sigma S^T and
// (...) Sigma (...)^T of a pose; the blocks below are what the right-hand-side kernels and the combines have in common.
// Workgroups of 256 threads; a frame n counts over all clips (n = b N + nl).  Every sum runs in the order written here.
// Not here: the kept row of a (camera, slot), the same lines in both right-hand-side kernels - as a shared function it compiles
// to other FMA pairings and S loses its last bits against the kernels that hold it inline (skel_calib.hip).
#pragma once
#include "skel_factor.hpp"

namespace acino {

// ---- a right-hand-side kernel, one workgroup per frame ------------------------------------------------------------------
// opv [n_ops][4][3] of frame n into LDS, the poses pos [n_pose][3] (coordinate by coordinate, in program order) and the pose
// Jacobians G [(l * 3 + i) * P + p] (skel_pose_jac_col).  Holds one workgroup barrier; the caller's barrier ends the stage.
__device__ __forceinline__ void skel_sens_frame(const SkelDev& D, int n, const double* __restrict__ x, const double* __restrict__ opv_all,
                                                double* opv, double* pos, double* G) {
  const int tid = threadIdx.x, P = D.n_act, NPOSE = D.n_pose, NOPS = D.n_ops;
  for (int e = tid; e < NOPS * 12; e += 256) opv[e] = opv_all[(size_t)n * NOPS * 12 + e];
  __syncthreads();
  if (tid < 3) {
    const double root = x[(size_t)n * P + tid];
    for (int s = 0; s < NPOSE; ++s) pos[s * 3 + tid] = root;
    for (int k = 0; k < NOPS; ++k) pos[D.op[k].child * 3 + tid] = pos[D.op[k].parent * 3 + tid] + opv[(k * 4) * 3 + tid];
  }
  for (int e = tid; e < NPOSE * P; e += 256) {
    const int l = e / P, p = e - l * P;
    double gc[3];
    skel_pose_jac_col(D, opv, l, p, gc);
    G[(l * 3) * P + p] = gc[0];
    G[(l * 3 + 1) * P + p] = gc[1];
    G[(l * 3 + 2) * P + p] = gc[2];
  }
}

// The end of a right-hand-side kernel: -G_n[p, col] = -sum_l G_l[:, p] . block(col, l, :) in slot order, 0 in the row of a
// pinned variable, as column col of rhs [B][cols][N][n_act].  block(col, l, i): coordinate i of the kernel's own block.
template <class F>
__device__ __forceinline__ void skel_sens_rhs_out(const SkelDev& D, int n, int cols, const double* G,
                                                  const unsigned char* __restrict__ fxm, double* __restrict__ rhs, F block) {
  const int P = D.n_act, N = D.n_frames, b = n / N, nl = n - b * N;
  for (int task = threadIdx.x; task < cols * P; task += 256) {
    const int col = task / P, p = task - col * P;
    double acc = 0.0;
    if (!fxm[(size_t)n * D.PT + p]) {
      for (int l = 0; l < D.n_pose; ++l) {
        acc += G[(l * 3) * P + p] * block(col, l, 0);
        acc += G[(l * 3 + 1) * P + p] * block(col, l, 1);
        acc += G[(l * 3 + 2) * P + p] * block(col, l, 2);
      }
      acc = -acc;
    }
    rhs[(((size_t)b * cols + col) * N + nl) * P + p] = acc;
  }
}

// ---- the links' groups (skel_links.hip: the sensitivity to the link lengths; skel_link_fit.hip: the joint fit's system) -------
constexpr int SKL_MAXK = 16;       // groups of links: MAX_LINK_GROUPS of build.py, LSC_MAXK of skel_link_scale.hip

struct SkelLinkGroups {            // by value to the kernels
  unsigned long long gm[SKL_MAXK]; // per group: its ops
  int32_t K, pad;
};

// D_l[i, g]: coordinate i of the sum of the rotated link vectors of group g's ops on slot l's path, in program order
__device__ __forceinline__ double skel_link_direct(const SkelDev& D, const SkelLinkGroups& grp, const double* __restrict__ opv, int l,
                                                   int i, int g) {
  const unsigned long long ops = D.pmask[l] & grp.gm[g];
  double acc = 0.0;
  for (int k = 0; k < D.n_ops; ++k)
    if ((ops >> k) & 1ull) acc += opv[k * 12 + i];
  return acc;
}

// ---- a combine kernel, one workgroup per frame ----------------------------------------------------------------------
// A singular clip: NaN in every output of frame n that is there (dpos [n_pose][3][cols]: the links' alone)
__device__ __forceinline__ void skel_sens_nan(const SkelDev& D, int n, int cols, double* __restrict__ sens, double* __restrict__ dpos,
                                              double* __restrict__ cov_x, double* __restrict__ cov_pos, double* __restrict__ std_pos) {
  const int tid = threadIdx.x, P = D.n_act, NPOSE = D.n_pose;
  const double nan = __builtin_nan("");
  for (int e = tid; e < P * cols; e += 256)
    if (sens) sens[(size_t)n * P * cols + e] = nan;
  for (int e = tid; e < NPOSE * 3 * cols; e += 256)
    if (dpos) dpos[(size_t)n * NPOSE * 3 * cols + e] = nan;
  for (int e = tid; e < P * P; e += 256)
    if (cov_x) cov_x[(size_t)n * P * P + e] = nan;
  for (int e = tid; e < NPOSE * 9; e += 256)
    if (cov_pos) cov_pos[(size_t)n * NPOSE * 9 + e] = nan;
  for (int e = tid; e < NPOSE; e += 256)
    if (std_pos) std_pos[(size_t)n * NPOSE + e] = nan;
}

// The states' share of frame n: S_n from the solution columns sol [B][cols][N][n_act] into Sm [P][ld] and out (sens, may be
// NULL); with `cov`, T = S_n Sigma into Tm [P][ld] (sigma [cols][cols], in memory or in LDS), cov_x = T S_n^T on one triangle
// and mirrored into Cx [P][P + 1] and out (cov_x, may be NULL).  Ends behind a workgroup barrier: Sm and, with `cov`, Cx stand.
__device__ __forceinline__ void skel_sens_states(const SkelDev& D, int n, int cols, int ld, const double* __restrict__ sol,
                                                 const double* sigma, bool cov, double* Sm, double* Tm, double* Cx,
                                                 double* __restrict__ sens, double* __restrict__ cov_x) {
  const int tid = threadIdx.x, P = D.n_act, N = D.n_frames, LDC = P + 1, b = n / N, nl = n - b * N;
  for (int e = tid; e < P * cols; e += 256) {
    const int col = e / P, p = e - col * P;
    Sm[p * ld + col] = sol[(((size_t)b * cols + col) * N + nl) * P + p];
  }
  __syncthreads();
  if (sens)
    for (int e = tid; e < P * cols; e += 256) sens[(size_t)n * P * cols + e] = Sm[(e / cols) * ld + e % cols];
  if (!cov) return;
  for (int e = tid; e < P * cols; e += 256) {
    const int p = e / cols, j = e - p * cols;
    double acc = 0.0;
    for (int i = 0; i < cols; ++i) acc += Sm[p * ld + i] * sigma[(size_t)i * cols + j];
    Tm[p * ld + j] = acc;
  }
  __syncthreads();
  for (int e = tid; e < P * P; e += 256) {
    const int p = e / P, q = e - p * P;
    if (p <= q) {
      double acc = 0.0;
      for (int j = 0; j < cols; ++j) acc += Tm[p * ld + j] * Sm[q * ld + j];
      Cx[p * LDC + q] = acc;
      Cx[q * LDC + p] = acc;
    }
  }
  __syncthreads();
  if (cov_x)
    for (int e = tid; e < P * P; e += 256) cov_x[(size_t)n * P * P + e] = Cx[(e / P) * LDC + e % P];
}

// Pose slot l's Jacobian G_l [3][P] into the wave's LDS (lane p: column p); true on a lane whose state is unobserved
// (unobs_b: the clip's mask [P], or NULL) and moves the slot.  The caller votes (__any) and hands Gw over.
__device__ __forceinline__ bool skel_sens_pose_jac(const SkelDev& D, const double* opv, int l, int lane,
                                                   const unsigned char* __restrict__ unobs_b, double* Gw) {
  const int P = D.n_act;
  if (lane >= P) return false;
  double gc[3];
  skel_pose_jac_col(D, opv, l, lane, gc);
  Gw[lane] = gc[0];
  Gw[P + lane] = gc[1];
  Gw[2 * P + lane] = gc[2];
  return unobs_b && unobs_b[lane] && (gc[0] != 0.0 || gc[1] != 0.0 || gc[2] != 0.0);
}

// The 3 x 3 covariance X Y^T of a pose slot from the wave's X, Y [3][len], which the wave has just written: six lanes on the upper
// triangle, mirrored into out9, then cov_pos_l [9] and std_pos_l = sqrt(trace) (either may be NULL); an undetermined slot gets
// NaN / +inf.  Ends with the wave barrier that lets the next slot overwrite the wave's LDS.
__device__ __forceinline__ void skel_sens_pos_out(int lane, int len, const double* X, const double* Y, double* out9, bool undet,
                                                  double* __restrict__ cov_pos_l, double* __restrict__ std_pos_l) {
  sk_wave_handover();
  if (lane < 6) {                                            // the upper triangle, mirrored
    const int i = lane < 3 ? 0 : (lane < 5 ? 1 : 2), j = lane < 3 ? lane : (lane < 5 ? lane - 2 : 2);
    double s = 0.0;
    for (int q = 0; q < len; ++q) s += X[i * len + q] * Y[j * len + q];
    out9[3 * i + j] = s;
    out9[3 * j + i] = s;
  }
  sk_wave_handover();
  if (lane < 9 && cov_pos_l) cov_pos_l[lane] = undet ? __builtin_nan("") : out9[lane];
  if (lane == 0 && std_pos_l) *std_pos_l = undet ? __builtin_inf() : sqrt(fmax(out9[0] + out9[4] + out9[8], 0.0));
  __builtin_amdgcn_wave_barrier();
}

}  // namespace acino
