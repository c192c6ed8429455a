// Error bars for the rates of the generic-skeleton FTE (gfx950, fp64): covariance of dx, ddx (the rule of the Python layer's
// _finite_diff_states) and of the pose velocities, per frame, from the blocks k_skel_selinv (skel_cov.hip) leaves in the band.
// With e the estimation error of a clip, Cov(e) = A^-1, every output is C S_win C^T for a window of at most three consecutive
// frames of the frame's OWN clip (local frame nl = n % N; a window never reaches into a neighbouring clip of the batch):
//   N >= 3, nl >= 2   window (nl-2, nl-1, nl): dx = (x_nl - x_nl-1) / h, ddx = (x_nl - 2 x_nl-1 + x_nl-2) / h^2
//   N >= 3, nl < 2    window (0, 1, 2): ddx as frame 2; dx_1 = (x_1 - x_0) / h, dx_0 = (-2 x_0 + 3 x_1 - x_2) / h
//   N = 2             ddx = 0, dx_1 = (x_1 - x_0) / h, dx_0 = 0;      N = 1: everything 0
//   v_nl,l = (G_l(x_m) e_m - G_l(x_m-1) e_m-1) / h with m = max(nl, 1): frame 0 repeats frame 1
// The blocks S_ab (a >= b, a - b <= 2) of A^-1 are band[b][a - b] after the recursion, S_aa symmetric; a variable pinned in
// frame a contributes nothing from frame a (row p of S_ab dropped if p is pinned in a, column q if q is pinned in b), which
// includes the clip's unobserved states when they are pinned.  The form differences nearly equal blocks; on the test inputs it
// stays within 1e-10 of the cancellation-free Y^T Y form built from the same factor (profiles/skel_cov_rates/route.txt), three
// orders below the disagreement of two factorisations of the same matrix, so no second sweep is run.
//   k_skel_cov_rates   one workgroup per frame, streaming: cov_dx / cov_ddx entry by entry from the six blocks in memory (L2: the
//                      blocks are 3 x 32 KB at most); then S_mm, S_m-1,m-1, S_m,m-1 into LDS and, one wave per pose slot,
//                      [G_m | -G_m-1] S [..]^T / h^2 as in k_skel_cov_pose.  No atomics, no MFMA (3 x P times P x P per slot).
#include <cstddef>

#include "skel_factor.hpp"

namespace acino {

__global__ void __launch_bounds__(256)
k_skel_cov_rates(const SkelDev* __restrict__ dev, const SkelClip* __restrict__ clip, const double* __restrict__ band,
                 const unsigned char* __restrict__ fxm, const double* __restrict__ opv_all, const unsigned char* __restrict__ unobs,
                 double h, double* __restrict__ cov_dx, double* __restrict__ cov_ddx, double* __restrict__ cov_vel,
                 double* __restrict__ std_vel) {
  const SkelDev& D = *dev;
  const int ng = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int P = D.n_act, PT = D.PT, N = D.n_frames, NPOSE = D.n_pose, NOPS = D.n_ops;
  const int b = ng / N, nl = ng - b * N;
  const size_t f0 = (size_t)b * N, BB = (size_t)PT * PT;
  const bool bad = clip[b].status != 0;
  if (bad || N == 1) {                                       // (uniform over the workgroup: before any barrier)
    const double v = bad ? __builtin_nan("") : 0.0;
    for (int e = tid; e < P * P; e += 256) {
      if (cov_dx) cov_dx[(size_t)ng * P * P + e] = v;
      if (cov_ddx) cov_ddx[(size_t)ng * P * P + e] = v;
    }
    for (int e = tid; e < NPOSE * 9; e += 256)
      if (cov_vel) cov_vel[(size_t)ng * NPOSE * 9 + e] = v;
    for (int e = tid; e < NPOSE; e += 256)
      if (std_vel) std_vel[(size_t)ng * NPOSE + e] = v;
    return;
  }
  // ---------------- dx, ddx: sum_a sum_b c_a c_b S_ab over the window (w0 .. w0 + K - 1), K = min(N, 3) ----------------
  if (cov_dx || cov_ddx) {
    const int K = N < 3 ? 2 : 3, w0 = nl >= 2 ? nl - 2 : 0;
    const double r = 1.0 / h;
    double c1[3] = {0.0, 0.0, 0.0}, c2[3] = {0.0, 0.0, 0.0};
    if (N >= 3) {
      c2[0] = r * r;
      c2[1] = -2.0 * r * r;
      c2[2] = r * r;
      if (nl >= 2) {
        c1[1] = -r;
        c1[2] = r;
      } else if (nl == 1) {
        c1[0] = -r;
        c1[1] = r;
      } else {
        c1[0] = -2.0 * r;
        c1[1] = 3.0 * r;
        c1[2] = -r;
      }
    } else if (nl == 1) {
      c1[0] = -r;
      c1[1] = r;
    }
    const double* Sw = band + (f0 + w0) * 4 * BB;            // band[w0 + b][a - b] = block (w0 + a, w0 + b)
    const unsigned char* fw = fxm + (f0 + w0) * PT;
    for (int e = tid; e < P * P; e += 256) {
      const int p = e / P, q = e % P;
      double s1 = 0.0, s2 = 0.0;
      for (int a = 0; a < K; ++a) {
        const bool ap = !fw[a * PT + p], aq = !fw[a * PT + q];
        const double d = (ap && aq) ? Sw[(size_t)a * 4 * BB + (size_t)max(p, q) * PT + min(p, q)] : 0.0;
        s1 += c1[a] * c1[a] * d;
        s2 += c2[a] * c2[a] * d;
        for (int bb = 0; bb < a; ++bb) {
          const bool bp = !fw[bb * PT + p], bq = !fw[bb * PT + q];
          const double* Sab = Sw + ((size_t)bb * 4 + (a - bb)) * BB;
          const double t = ((ap && bq) ? Sab[(size_t)p * PT + q] : 0.0) + ((bp && aq) ? Sab[(size_t)q * PT + p] : 0.0);
          s1 += c1[a] * c1[bb] * t;
          s2 += c2[a] * c2[bb] * t;
        }
      }
      if (cov_dx) cov_dx[(size_t)ng * P * P + e] = s1;
      if (cov_ddx) cov_ddx[(size_t)ng * P * P + e] = s2;
    }
  }
  if (!cov_vel && !std_vel) return;                          // (uniform)
  // ---------------- pose velocities: frames m = max(nl, 1) and m - 1 ----------------
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const int LDS = P + 1;
  double* Smm = reinterpret_cast<double*>(smem_raw);         // [P][P + 1] each
  double* Spp = Smm + P * LDS;
  double* Smp = Spp + P * LDS;                               // block (m, m - 1): row of frame m, column of frame m - 1
  __shared__ double opv[2][ACINO_SKEL_MAX_OPS * 12];
  __shared__ double G[4][6][SK_MAXP], T[4][6][SK_MAXP], out9[4][9];
  const size_t fm = f0 + (nl >= 1 ? nl : 1), fp = fm - 1;
  const unsigned char* fxm_m = fxm + fm * PT;
  const unsigned char* fxm_p = fxm + fp * PT;
  {
    const double* Bm = band + fm * 4 * BB;
    const double* Bp = band + fp * 4 * BB;
    for (int e = tid; e < P * P; e += 256) {
      const int p = e / P, q = e % P;
      const size_t lo = (size_t)max(p, q) * PT + min(p, q);
      Smm[p * LDS + q] = Bm[lo];
      Spp[p * LDS + q] = Bp[lo];
      Smp[p * LDS + q] = Bp[BB + (size_t)p * PT + q];
    }
    for (int e = tid; e < NOPS * 12; e += 256) {
      opv[0][e] = opv_all[fm * NOPS * 12 + e];
      opv[1][e] = opv_all[fp * NOPS * 12 + e];
    }
  }
  __syncthreads();
  const double ih2 = 1.0 / (h * h);
  for (int l0 = 0; l0 < NPOSE; l0 += 4) {
    const int l = l0 + wave;
    const bool on = l < NPOSE;
    bool dep = false;
    if (on && lane < P) {
      double gm[3] = {lane == 0 ? 1.0 : 0.0, lane == 1 ? 1.0 : 0.0, lane == 2 ? 1.0 : 0.0};
      double gp[3] = {gm[0], gm[1], gm[2]};
      const unsigned long long path = D.pmask[l];
      for (int k = 0; k < NOPS; ++k) {
        if (!((path >> k) & 1ull)) continue;
#pragma unroll
        for (int ax = 0; ax < 3; ++ax)
          if (D.amap[k][ax] == lane) {
            const double* dm = opv[0] + (k * 4 + 1 + ax) * 3;
            const double* dp = opv[1] + (k * 4 + 1 + ax) * 3;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
              gm[i] += dm[i];
              gp[i] += dp[i];
            }
          }
      }
      if (unobs)
        dep = unobs[(size_t)b * P + lane] &&
              (gm[0] != 0.0 || gm[1] != 0.0 || gm[2] != 0.0 || gp[0] != 0.0 || gp[1] != 0.0 || gp[2] != 0.0);
      const bool pm = fxm_m[lane] != 0, pp = fxm_p[lane] != 0;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        G[wave][i][lane] = pm ? 0.0 : gm[i];
        G[wave][3 + i][lane] = pp ? 0.0 : gp[i];
      }
    }
    const bool undet = __any(dep ? 1 : 0) != 0;              // (wave-wide: a wave is one pose slot)
    __syncthreads();
    if (on && lane < P) {                                    // T = [G_m | -G_m-1] S, column `lane` of either half
      double tm[3] = {0.0, 0.0, 0.0}, tp[3] = {0.0, 0.0, 0.0};
      for (int p = 0; p < P; ++p) {
        const double smm = Smm[p * LDS + lane], spp = Spp[p * LDS + lane], smp_t = Smp[lane * LDS + p], smp = Smp[p * LDS + lane];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          const double a = G[wave][i][p], c = G[wave][3 + i][p];
          tm[i] += a * smm - c * smp_t;
          tp[i] += a * smp - c * spp;
        }
      }
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        T[wave][i][lane] = tm[i];
        T[wave][3 + i][lane] = tp[i];
      }
    }
    __syncthreads();
    if (on && lane < 9) {
      const int i = lane / 3, j = lane % 3;
      double s = 0.0;
      for (int q = 0; q < P; ++q) s += T[wave][i][q] * G[wave][j][q] - T[wave][3 + i][q] * G[wave][3 + j][q];
      s *= ih2;
      out9[wave][lane] = s;
      if (cov_vel) cov_vel[((size_t)ng * NPOSE + l) * 9 + lane] = undet ? __builtin_nan("") : s;
    }
    __syncthreads();
    if (on && lane == 0 && std_vel)
      std_vel[(size_t)ng * NPOSE + l] = undet ? __builtin_inf() : sqrt(fmax(out9[wave][0] + out9[wave][4] + out9[wave][8], 0.0));
    __syncthreads();
  }
}

int skel_cov_launch_rates(size_t NT, int P, const SkelDev* d_dev, const SkelClip* d_clip, const double* d_band,
                          const unsigned char* d_fxm, const double* d_opv, const unsigned char* d_unobs, double h, double* d_cov_dx,
                          double* d_cov_ddx, double* d_cov_vel, double* d_std_vel, hipStream_t s) {
  static PerDeviceOnce attr;
  if (attr.first())
    ACINO_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_skel_cov_rates), hipFuncAttributeMaxDynamicSharedMemorySize,
                                        (int)skel_cov_rates_lds(SK_MAXP)));
  hipLaunchKernelGGL(k_skel_cov_rates, dim3((unsigned)NT), dim3(256), skel_cov_rates_lds(P), s, d_dev, d_clip, d_band, d_fxm, d_opv,
                     d_unobs, h, d_cov_dx, d_cov_ddx, d_cov_vel, d_std_vel);
  ACINO_LAUNCH_CHECK();
  return ACINO_OK;
}

}  // namespace acino
