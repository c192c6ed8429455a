// What the two link-scale kernels share (skel_link_scale.hip: from 3-D points; skel_link_scale_px.hip: from the detections of
// every camera): the most groups a call may name, the forward substitution of several right-hand sides on the
// register-resident factor (moved here from skel_link_scale.hip as it stood), the elimination of a frame's pose from the
// joint (pose, log-scale) system once A, B, C, g and c are in LDS, the per-frame stores, and the host launcher of the summing
// kernel, which is defined in skel_link_scale.hip beside k_link_scale_total (no device code is linked across files).
//
// lsc_eliminate and lsc_store hold the statements of k_skel_link_scale's tail.  That kernel keeps its own text: the pixel
// kernel is their only caller.
#pragma once
#include "pose_fit_skel.hpp"

namespace acino {

constexpr int LSC_MAXK = 16;

// v <- L^-1 v for NC right-hand sides at once, lane p holding entry p of each: the forward half of pf_solve
template <int N, int NC>
__device__ __forceinline__ void lsc_forward(const double (&r)[N], double dinv, double (&v)[NC], int lane) {
#pragma unroll
  for (int k = 0; k < N; ++k)
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const double zk = pf_readlane(v[c] * dinv, k);
      v[c] = lane == k ? zk : (lane > k ? v[c] - r[k] * zk : v[c]);
    }
}

// A in S.M (lower triangle), B in Bm (K columns of PT), C in Cm (LSC_MAXK x LSC_MAXK, mirrored), g in S.g, c in cv, F the
// frame's cost: A_FF = L L^T with lam = 0 (pinned rows the identity's), sens = -A_FF^-1 B_F into ``sens`` [P][K] when it is
// not NULL (pinned rows exactly 0), Y = L^-1 B_F in B's place and v = L^-1 g_F in g's, four columns at a time, then
// S = C - Y^T Y (lower triangle, mirrored: symmetric bit for bit) in Cm and r = c - Y^T v in cv, one entry per lane, summed
// over the states in state order.  False (the same in every lane) when there is no factor or a value is not finite.
template <int PT>
__device__ __forceinline__ bool lsc_eliminate(const Spf& S, const SkelDev& D, unsigned long long fixmask, double F, int K, double* Bm,
                                              double* Cm, double* cv, double* sens, int lane) {
  const int P = S.P;
  SkelCore<PT> core{S, D, lane};
  double r[PT], dinv;
  bool ok = core.factor(fixmask, 0.0, lane, r, dinv) && m_finite(F);
  if (lane < P) ok = ok && m_finite(S.x[lane]);
  ok = __all(ok);
  if (!ok) return false;
  const bool free_p = lane < P && !((fixmask >> lane) & 1);
  // the sensitivity first: it reads B, whose place Y takes below
  if (sens) {
#pragma unroll 1
    for (int g = 0; g < K; ++g) {
      const double b = free_p ? Bm[g * PT + lane] : 0.0;
      const double d = core.solve(r, dinv, -b, lane);
      if (lane < P) sens[lane * K + g] = free_p ? d : 0.0;
    }
  }
#pragma unroll 1
  for (int c0 = 0; c0 <= K; c0 += 4) {
    double v[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int g = c0 + c;
      v[c] = !free_p || g > K ? 0.0 : (g == K ? S.g[lane] : Bm[g * PT + lane]);
    }
    lsc_forward<PT, 4>(r, dinv, v, spf_here(lane));
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int g = c0 + c;
      if (lane < P && g <= K) (g == K ? S.g : Bm + g * PT)[lane] = v[c];
    }
  }
  __syncthreads();
  bool fin = true;
  for (int t = lane; t < K * (K + 1) / 2 + K; t += 64) {
    int i = 0, j = 0;
    const double* right = S.g;
    const bool tri = t < K * (K + 1) / 2;
    if (tri) {
      while ((i + 1) * (i + 2) / 2 <= t) ++i;
      j = t - i * (i + 1) / 2;
      right = Bm + j * PT;
    } else {
      i = t - K * (K + 1) / 2;
    }
    const double* left = Bm + i * PT;
    double sum = 0.0;
    for (int p = 0; p < P; ++p) sum += left[p] * right[p];
    if (tri) {                                    // (entry (i, j) is read by this lane alone, (j, i) above the diagonal by none)
      const double v = Cm[i * LSC_MAXK + j] - sum;
      fin = fin && m_finite(v);
      Cm[i * LSC_MAXK + j] = v;
      Cm[j * LSC_MAXK + i] = v;
    } else {
      const double v = cv[i] - sum;
      fin = fin && m_finite(v);
      cv[i] = v;
    }
  }
  ok = __all(fin);
  __syncthreads();
  return ok;
}

// what a frame leaves behind: S, r, F, used and the status (zeros and NaN in sens for a frame that did not enter)
struct LscOut {
  double *S, *r, *F, *sens;
  uint8_t *used, *frame_status;
};
__device__ __forceinline__ void lsc_store(const LscOut& o, int64_t n, int P, int K, bool live, int st_in, double F, const double* Cm,
                                          const double* cv, int lane) {
  for (int t = lane; t < K * K; t += 64) o.S[n * K * K + t] = live ? Cm[(t / K) * LSC_MAXK + t % K] : 0.0;
  if (lane < K) o.r[n * K + lane] = live ? cv[lane] : 0.0;
  if (!live && o.sens)
    for (int t = lane; t < P * K; t += 64) o.sens[n * P * K + t] = __builtin_nan("");
  if (lane == 0) {
    o.F[n] = live ? F : 0.0;
    o.used[n] = live ? 1 : 0;
    o.frame_status[n] = (uint8_t)(live || st_in >= 2 ? st_in : PF_NUMERIC);
  }
}

// [S | r | F | used] of the frames added up in frame order into d_total[K K + K + 2] (k_link_scale_total, skel_link_scale.hip)
int lsc_launch_total(const double* d_S, const double* d_r, const double* d_F, const uint8_t* d_used, int64_t n_frames, int K,
                     double* d_total, hipStream_t s);

}  // namespace acino
