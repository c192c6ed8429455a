// Extended Kalman filter + Rauch-Tung-Striebel smoother over the 25 cheetah pose parameters (gfx950, fp64).
//
// Reference: `ekf` in src/all_optimizations.py:569-865 - constant-acceleration model (75 states), measurement =
// fisheye projection of the 20 markers in every camera (up to 240 pixel coordinates per frame), Jacobian by forward
// differences with eps = 1e-3 (:631-646), 3-sigma gating (:815-819), K = P H^T inv(S) with S 240x240 (:822),
// P <- (I - K H) P (:829), smoother (:836-841).  The filter is sequential in frames, so ONE workgroup runs a whole
// sequence (grid = sequences) with the 75x75 covariance, the 240x25 Jacobian and every intermediate in LDS:
//   * FK of the 26 forward-difference variants column-parallel (78 threads); projections only of the (variant,
//     marker) pairs in which the marker moves with the perturbed parameter (about half; found once per launch by
//     probing the chain at a generic pose - the other forward differences are exactly 0 at every pose);
//   * H has 25 non-zero columns and R is diagonal, so with M = Hq^T R^-1 Hq, g = Hq^T R^-1 r (fp64 MFMA, g rides
//     along as a 26th column) the 240x240 inverse collapses to 25x25 algebra:
//       K r = P[:, :25] (I + M Pq)^-1 g,   P <- P - P[:, :25] (I + M Pq)^-1 M P[:25, :],   Pq = P[:25, :25],
//     evaluated through Pq = Lc Lc^T and the SPD matrix B = I + Lc^T M Lc (push-through identity) - identical
//     to the reference's formulas in exact arithmetic;  diag(S) for the gate is the row norms of Hq Lc, + R;
//   * every product is 16 x 16 fp64 MFMA tiles (tile_gemm); the two 25 x 25 Cholesky factorisations run in ONE wave's
//     registers (wave_chol32: the 16 x 16 register factorisation of dense80.hpp twice + MFMA glue), chol(Pq) in
//     wave 3 while waves 0-2 evaluate the 572 sines / cosines; triangular solves are products with U = L^-T.
// The smoother gains A_i = P_est[i] F^T inv(P_pred[i+1]) are independent across frames (one workgroup each, P_pred
// rebuilt from P_est, blocked Cholesky + two triangular products, pivoting fallback); only the 75x75 mat-vec
// recursion is sequential (one workgroup per sequence).  The reference never saves a covariance (:850-857), so this
// file computes none beyond P_est; the smoothed covariances P_s[i] = P_est[i] + A_i (P_s[i+1] - P_pred[i+1]) A_i^T and
// the marker error bars are an opt-in second pass over the workspace this file leaves behind (ekf_cov.hip), with the
// shared device code in ekf_dev.hpp.
#include "cheetah_fk.hpp"
#include "dense80.hpp"
#include "ekf_dev.hpp"
#include "pinhole.hpp"

namespace acino {

struct FkLite {
  static constexpr bool kHasOm = false;
  double sc[22][2];
  double pos[21][3];
};

__device__ __forceinline__ double ekf_readlane(double x, int lane) {
  long long b = __builtin_bit_cast(long long, x);
  int lo = __builtin_amdgcn_readlane((int)b, lane);
  int hi = __builtin_amdgcn_readlane((int)(b >> 32), lane);
  return __builtin_bit_cast(double, (long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
}

// Cholesky of the 25 x 25 SPD matrix A (LDS, leading dimension lda, lower triangle read) by ONE wave, blocked 16 + 9
// (the second tile padded with identity): the register-resident 16 x 16 factorisation of dense80.hpp twice, the panel
// L10 = A10 U00 and the Schur complement A11 - L10 L10^T on the matrix cores in between.  Lw (32 x 33) receives L
// (tiles (0,0), (1,0), (1,1)); Uw (32 x 33) the diagonal inverse factors U00 = L00^-T, U11 = L11^-T and, with WITH_U,
// the whole U = L^-T = [[U00, -U00 L10^T U11], [0, U11]] - a triangular solve then is a product with U^T.
// Everything a lane reads back was written by its own wave (LDS operations of one wave complete in order).  Forced inline: with
// two forward kernels calling it the compiler would otherwise make it a call.
constexpr int WLD = 33;
template <bool WITH_U>
__device__ __forceinline__ bool wave_chol32(const double* A, int lda, double* Lw, double* Uw, int lane) {
  const int li = lane & 15, lk = lane >> 4;
  d4 acc;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = lk + 4 * r;
    acc[r] = A[(i > li ? i : li) * lda + (i > li ? li : i)];
  }
  bool ok = chol16_inv_acc<WLD, true>(Uw, acc, lane, nullptr, Lw);
  double av[4], bv[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {                 // panel L10 = A10 U00
    av[s] = (16 + li < EP) ? A[(16 + li) * lda + 4 * s + lk] : 0.0;
    bv[s] = Uw[(4 * s + lk) * WLD + li];
  }
  d4 l10 = {0, 0, 0, 0};
#pragma unroll
  for (int s = 0; s < 4; ++s) l10 = __builtin_amdgcn_mfma_f64_16x16x4f64(av[s], bv[s], l10, 0, 0, 0);
#pragma unroll
  for (int r = 0; r < 4; ++r) Lw[(16 + lk + 4 * r) * WLD + li] = l10[r];
#pragma unroll
  for (int r = 0; r < 4; ++r) {                 // A11 (identity on the padding)
    const int i = 16 + lk + 4 * r, j = 16 + li;
    acc[r] = (i < EP && j < EP) ? A[(i > j ? i : j) * lda + (i > j ? j : i)] : (i == j ? 1.0 : 0.0);
  }
#pragma unroll
  for (int s = 0; s < 4; ++s) av[s] = Lw[(16 + li) * WLD + 4 * s + lk];
#pragma unroll
  for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-av[s], av[s], acc, 0, 0, 0);
  ok = chol16_inv_acc<WLD, true>(Uw + 16 * WLD + 16, acc, lane, nullptr, Lw + 16 * WLD + 16) && ok;
  if (WITH_U) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {               // Y = L10^T U11
      av[s] = Lw[(16 + 4 * s + lk) * WLD + li];
      bv[s] = Uw[(16 + 4 * s + lk) * WLD + 16 + li];
    }
    d4 y = {0, 0, 0, 0};
#pragma unroll
    for (int s = 0; s < 4; ++s) y = __builtin_amdgcn_mfma_f64_16x16x4f64(av[s], bv[s], y, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      Uw[(lk + 4 * r) * WLD + 16 + li] = y[r];
      Uw[(16 + lk + 4 * r) * WLD + li] = 0.0;
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {               // U01 = -U00 Y
      av[s] = Uw[li * WLD + 4 * s + lk];
      bv[s] = Uw[(4 * s + lk) * WLD + 16 + li];
    }
    d4 u01 = {0, 0, 0, 0};
#pragma unroll
    for (int s = 0; s < 4; ++s) u01 = __builtin_amdgcn_mfma_f64_16x16x4f64(-av[s], bv[s], u01, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 4; ++r) Uw[(lk + 4 * r) * WLD + 16 + li] = u01[r];
  }
  return ok;
}

__global__ void __launch_bounds__(256)
k_ekf_forward(EkfK K, const double* __restrict__ det_all, const double* __restrict__ cams,
              const double* __restrict__ states0_all, double* __restrict__ x_pred_all, double* __restrict__ x_est_all,
              double* __restrict__ P_est_all, int* __restrict__ outliers,
              int* __restrict__ numeric_err) {
#define ACINO_EKF_PINHOLE 0
#include "ekf_forward_body.inc"
#undef ACINO_EKF_PINHOLE
}

// The same filter on the OpenCV pinhole camera (cv2.projectPoints, pinhole.hpp): cams = n_cams records of 32 doubles.  A
// kernel name of its own, so that the fisheye kernel's name and code stay as they are; the smoother kernels below do not
// depend on the camera and serve both.
__global__ void __launch_bounds__(256)
k_ekf_forward_pinhole(EkfK K, const double* __restrict__ det_all, const double* __restrict__ cams,
                      const double* __restrict__ states0_all, double* __restrict__ x_pred_all, double* __restrict__ x_est_all,
                      double* __restrict__ P_est_all, int* __restrict__ outliers,
                      int* __restrict__ numeric_err) {
#define ACINO_EKF_PINHOLE 1
#include "ekf_forward_body.inc"
#undef ACINO_EKF_PINHOLE
}

// A_i = P_est[i] F^T inv(P_pred[i+1]) for i = 1 .. N-2 (one workgroup per (sequence, frame)), P_pred[i+1] = F P_est[i] F^T + Q
// rebuilt here;  A_i^T = inv(P_pred[i+1]) G, G = F P_est[i]^T.  P_pred is symmetric positive definite while the filter
// is healthy: blocked Cholesky with the inverse factor U = L^-T (dense80.hpp), then A_i = (U^T G)^T U^T - two
// triangular 80 x 80 products on the matrix cores.  If a pivot is not positive ((I - K H) P does not keep positive
// definiteness to round-off when a filter has lost its target), the workgroup falls back to Gauss-Jordan elimination
// with partial pivoting on [P_pred | G] - like the reference's np.linalg.inv (:840), no definiteness requirement.
__device__ void rts_build(double* Lp, double* G, const double* E, double sT, int tid) {
  const double a1 = sT, a2 = sT * sT / 2;
  for (int e = tid; e < EP * EP; e += 256) predict_cov_entry(E, LD, Lp, LD, e / EP, e % EP, sT);
  for (int e = tid; e < BS * BS; e += 256) {
    const int r = e / BS, c = e % BS;
    double g = 0.0;
    if (r < ES && c < ES) {     // G[r][c] = (F P_est^T)[r][c] = sum_k F[r][k] P_est[c][k]
      g = E[c * LD + r];
      if (r < 2 * EP) g += a1 * E[c * LD + r + EP];
      if (r < EP) g += a2 * E[c * LD + r + 2 * EP];
    } else {
      Lp[r * LD + c] = (r == c) ? 1.0 : 0.0;
    }
    G[r * LD + c] = g;
  }
}

__global__ void __launch_bounds__(256)
k_rts_gain(EkfK K, const double* __restrict__ P_est_all, double* __restrict__ A_all, int* __restrict__ numeric_err) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  double* Lp = sm;                 // [80][81] P_pred -> L / U
  double* G = Lp + MAT;            // [80][81] F P_est^T -> U^T G
  double* E = G + MAT;             // [80][81] P_est
  __shared__ int s_err, s_piv;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, lk = lane >> 4;
  const int N = K.n_frames, per = N - 2;
  const int seq = blockIdx.x / per, i = 1 + blockIdx.x % per;
  const double* Pe = P_est_all + ((size_t)seq * N + i) * ES * ES;
  double* At = A_all + ((size_t)seq * N + i) * ES * ES;     // stored TRANSPOSED: the recursion reads columns
  for (int e = tid; e < ES * ES; e += 256) E[(e / ES) * LD + e % ES] = Pe[e];
  if (tid == 0) s_err = 0;
  __syncthreads();
  rts_build(Lp, G, E, K.sT, tid);
  __syncthreads();
  if (!K.pivoting) chol80(Lp, tid, &s_err);
  if (!K.pivoting && !s_err) {
    d4 acc[7];
#pragma unroll
    for (int q = 0; q < 7; ++q) {          // T = U^T G : tile (ti, tj) = sum_{k <= ti} U(k, ti)^T G(k, tj)
      const int t = wave + 4 * q;
      acc[q] = d4{0, 0, 0, 0};
      if (t < 25) {
        const int ti = t / 5, tj = t % 5;
        for (int k = 0; k <= ti; ++k)
          acc[q] = mma_seq<4, false>(acc[q], Lp + (16 * k + lk) * LD + 16 * ti + li, 4 * LD, G + (16 * k + lk) * LD + 16 * tj + li,
                                     4 * LD);
      }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 7; ++q) {
      const int t = wave + 4 * q;
      if (t < 25) {
        const int ti = t / 5, tj = t % 5;
#pragma unroll
        for (int r = 0; r < 4; ++r) G[(16 * ti + lk + 4 * r) * LD + 16 * tj + li] = acc[q][r];
      }
    }
    __syncthreads();
    for (int t = wave; t < 25; t += 4) {   // A^T = U T : tile (ti, tj) = sum_{k >= ti} U(ti, k) T(k, tj)
      const int ti = t / 5, tj = t % 5;
      d4 a = {0, 0, 0, 0};
      for (int k = ti; k < 5; ++k)
        a = mma_seq<4, false>(a, Lp + (16 * ti + li) * LD + 16 * k + lk, 4, G + (16 * k + lk) * LD + 16 * tj + li, 4 * LD);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 16 * ti + lk + 4 * r, col = 16 * tj + li;
        if (row < ES && col < ES) At[row * ES + col] = a[r];
      }
    }
    return;
  }
  __syncthreads();
  rts_build(Lp, G, E, K.sT, tid);
  __syncthreads();
  for (int k = 0; k < ES; ++k) {
    if (tid < 64) {
      double best = -1.0;
      int bi = k;
      for (int r = k + lane; r < ES; r += 64) {
        const double v = fabs(Lp[r * LD + k]);
        if (v > best) {
          best = v;
          bi = r;
        }
      }
      for (int off = 32; off > 0; off >>= 1) {
        const double ob = __shfl_down(best, off, 64);
        const int oi = __shfl_down(bi, off, 64);
        if (ob > best || (ob == best && oi < bi)) {
          best = ob;
          bi = oi;
        }
      }
      if (lane == 0) {
        s_piv = bi;
        if (!(best > 0.0)) atomicCAS(numeric_err, 0, -(i + 1));
      }
    }
    __syncthreads();
    const int pr = s_piv;
    if (pr != k && tid < 2 * ES) {
      double* M2 = tid < ES ? Lp : G;
      const int c = tid % ES;
      const double t = M2[k * LD + c];
      M2[k * LD + c] = M2[pr * LD + c];
      M2[pr * LD + c] = t;
    }
    __syncthreads();
    const double d = Lp[k * LD + k];
    __syncthreads();
    const double inv = 1.0 / (d != 0.0 ? d : 1.0);
    if (tid < 2 * ES) {
      double* M2 = tid < ES ? Lp : G;
      M2[k * LD + tid % ES] *= inv;
    }
    __syncthreads();
    const int nc = (ES - k - 1) + ES;          // columns k+1.. of P_pred, all of G
    for (int e = tid; e < ES * nc; e += 256) {
      const int r = e / nc, cc = e % nc;
      if (r == k) continue;
      const double fct = Lp[r * LD + k];
      if (cc < ES - k - 1) Lp[r * LD + k + 1 + cc] -= fct * Lp[k * LD + k + 1 + cc];
      else G[r * LD + cc - (ES - k - 1)] -= fct * G[k * LD + cc - (ES - k - 1)];
    }
    __syncthreads();
  }
  for (int e = tid; e < ES * ES; e += 256) At[e] = G[(e / ES) * LD + e % ES];     // A^T = X
}

// smooth[i] = x_est[i] + A_i (smooth[i+1] - x_pred[i+1]), i = N-2 .. 1; frames 0 and N-1 keep the filtered state (:836-839).
// The recursion is a chain of 75 x 75 mat-vecs: one thread per row keeps its row of A_i in registers (the next
// frame's row is already in flight), the difference vector is double-buffered in LDS - ONE barrier per frame.
__global__ void __launch_bounds__(128)
k_rts_recurse(EkfK K, const double* __restrict__ x_pred_all, const double* __restrict__ x_est_all,
              const double* __restrict__ A_all, double* __restrict__ smooth_all) {
  __shared__ __attribute__((aligned(16))) double v[2][ES + 1];
  const int tid = threadIdx.x, N = K.n_frames, seq = blockIdx.x;
  const double* x_pred = x_pred_all + (size_t)seq * N * ES;
  const double* x_est = x_est_all + (size_t)seq * N * ES;
  const double* A = A_all + (size_t)seq * N * ES * ES;
  double* smooth = smooth_all + (size_t)seq * N * ES;
  const bool on = tid < ES;
  if (on) {
    smooth[tid] = x_est[tid];
    if (N > 1) smooth[(size_t)(N - 1) * ES + tid] = x_est[(size_t)(N - 1) * ES + tid];
  }
  if (N < 3) return;
  double a[ES], an[ES];
  double xe = 0.0, xp_next = 0.0;
  if (on) {
    v[0][tid] = x_est[(size_t)(N - 1) * ES + tid] - x_pred[(size_t)(N - 1) * ES + tid];
    xe = x_est[(size_t)(N - 2) * ES + tid];
    xp_next = x_pred[(size_t)(N - 2) * ES + tid];
#pragma unroll
    for (int c = 0; c < ES; ++c) a[c] = A[(size_t)(N - 2) * ES * ES + c * ES + tid];     // A is stored transposed
  }
  __syncthreads();
  int buf = 0;
  for (int i = N - 2; i >= 1; --i) {
    double xe_n = 0.0, xp_n = 0.0;
    if (on && i > 1) {                 // the next frame's operands: in flight during this frame's dot product
      xe_n = x_est[(size_t)(i - 1) * ES + tid];
      xp_n = x_pred[(size_t)(i - 1) * ES + tid];
#pragma unroll
      for (int c = 0; c < ES; ++c) an[c] = A[(size_t)(i - 1) * ES * ES + c * ES + tid];
    }
    if (on) {
      double s0 = 0.0, s1 = 0.0, s2 = 0.0;
#pragma unroll
      for (int c = 0; c < ES; c += 3) {
        s0 += a[c] * v[buf][c];
        s1 += a[c + 1] * v[buf][c + 1];
        s2 += a[c + 2] * v[buf][c + 2];
      }
      const double cur = xe + ((s0 + s1) + s2);
      smooth[(size_t)i * ES + tid] = cur;
      v[buf ^ 1][tid] = cur - xp_next;       // smooth[i] - x_pred[i]: the next frame's right-hand side
#pragma unroll
      for (int c = 0; c < ES; ++c) a[c] = an[c];
      xe = xe_n;
      xp_next = xp_n;
    }
    buf ^= 1;
    __syncthreads();
  }
}

constexpr size_t kRtsLds = 3 * MAT * sizeof(double);
constexpr size_t kEkfLds = (size_t)(PR * PLD + EROWS * HLD + 4 * EROWS + 80 + 32 + 32 + 2800 + 2 * 32 * 33) * sizeof(double) +
                           EKF_MAXC * sizeof(Cam) + (NL + 4) * 4 + (NL + EP * NL) * 2 + 8;
static_assert(sizeof(FkLite) * NVAR <= 6 * EP * SLD * sizeof(double), "FK frames must fit the scratch region");
static_assert((PR * VLD + 28 * PLD) <= EROWS * HLD, "V and Ptop alias the Jacobian storage");
static_assert(kEkfLds <= 160 * 1024, "EKF workgroup state must fit the 160 KB LDS");
// the pinhole twin: the same layout with the larger camera records (Pin, 32 doubles, in place of Cam, 24)
constexpr size_t kEkfLdsPinhole = kEkfLds - EKF_MAXC * sizeof(Cam) + EKF_MAXC * sizeof(Pin);
static_assert(kEkfLdsPinhole <= 160 * 1024, "pinhole EKF workgroup state must fit the 160 KB LDS");

}  // namespace acino

using namespace acino;

extern "C" {

size_t acino_sizeof_ekf_params(void) { return sizeof(acino_ekf_params); }

size_t acino_ekf_workspace_bytes(int64_t n_frames, int n_seq) {
  if (n_frames < 1 || n_seq < 1) return 0;
  const size_t N = (size_t)n_frames * n_seq;
  return 2 * a256(N * ES * ES * 8) + 2 * a256(N * ES * 8) + 1024;
}

static int ekf_run(const acino_ekf_params* prm, const double* d_det, const double* d_cams, const double* d_states0, void* d_ws,
                   size_t ws_bytes, double* d_est, double* d_smooth, int32_t* d_outliers, void* stream, bool pinhole) {
  ACINO_REQUIRE(prm, "params");
  ACINO_REQUIRE(prm->n_frames >= 1 && prm->n_seq >= 1, "n_frames, n_seq");
  ACINO_REQUIRE(prm->n_cams >= 1 && prm->n_cams <= EKF_MAXC, "n_cams in 1..6");
  ACINO_REQUIRE(prm->fps > 0 && prm->cam_width > 0, "fps, cam_width");
  ACINO_REQUIRE(d_det && d_cams && d_states0 && d_ws && d_est && d_smooth && d_outliers, "null buffer");
  ACINO_REQUIRE(((uintptr_t)d_ws & 255) == 0, "workspace must be 256-byte aligned");
  ACINO_REQUIRE(ws_bytes >= acino_ekf_workspace_bytes(prm->n_frames, prm->n_seq), "workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const size_t N = (size_t)prm->n_frames * prm->n_seq;
  char* w = (char*)d_ws;
  double* P_est = (double*)w;   w += a256(N * ES * ES * 8);
  double* A = (double*)w;       w += a256(N * ES * ES * 8);
  double* x_pred = (double*)w;  w += a256(N * ES * 8);
  int* nerr = (int*)w;
  EkfK K;
  K.n_frames = (int)prm->n_frames;
  K.n_cams = prm->n_cams;
  K.pivoting = prm->smoother_pivoting;
  K.sT = 1.0 / prm->fps;
  K.dlc_thresh = prm->dlc_thresh;
  K.max_pixel_err = prm->cam_width;
  K.eps = 1e-3;
  static PerDeviceOnce attr;
  if (attr.first()) {
    ACINO_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_ekf_forward),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)kEkfLds));
    ACINO_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_ekf_forward_pinhole),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)kEkfLdsPinhole));
    ACINO_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_rts_gain),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)kRtsLds));
  }
  ACINO_HIP_CHECK(hipMemsetAsync(d_outliers, 0, sizeof(int32_t) * prm->n_seq, s));
  ACINO_HIP_CHECK(hipMemsetAsync(nerr, 0, sizeof(int), s));
  if (pinhole)
    hipLaunchKernelGGL(k_ekf_forward_pinhole, dim3(prm->n_seq), dim3(256), kEkfLdsPinhole, s, K, d_det, d_cams, d_states0, x_pred,
                       d_est, P_est, d_outliers, nerr);
  else
    hipLaunchKernelGGL(k_ekf_forward, dim3(prm->n_seq), dim3(256), kEkfLds, s, K, d_det, d_cams, d_states0, x_pred, d_est,
                       P_est, d_outliers, nerr);
  ACINO_LAUNCH_CHECK();
  if (prm->n_frames >= 3) {
    hipLaunchKernelGGL(k_rts_gain, dim3((unsigned)(prm->n_seq * (prm->n_frames - 2))), dim3(256), kRtsLds, s, K, P_est, A, nerr);
    ACINO_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_rts_recurse, dim3(prm->n_seq), dim3(128), 0, s, K, x_pred, d_est, A, d_smooth);
  ACINO_LAUNCH_CHECK();
  int h_err = 0;
  ACINO_HIP_CHECK(hipMemcpyAsync(&h_err, nerr, sizeof(int), hipMemcpyDeviceToHost, s));
  ACINO_HIP_CHECK(hipStreamSynchronize(s));
  if (h_err) {
    if (h_err > 0)
      set_error("EKF: %s lost positive definiteness at frame %d", (h_err & 1) ? "the pose covariance" : "I + Lc^T M Lc",
                (h_err - 1) / 2);
    else
      set_error("EKF smoother: the predicted covariance of frame %d is singular", -h_err);
    return ACINO_ERR_NUMERIC;
  }
  return ACINO_OK;
}

int acino_ekf_run(const acino_ekf_params* prm, const double* d_det, const double* d_cams24, const double* d_states0,
                  void* d_ws, size_t ws_bytes, double* d_est, double* d_smooth, int32_t* d_outliers, void* stream) {
  return ekf_run(prm, d_det, d_cams24, d_states0, d_ws, ws_bytes, d_est, d_smooth, d_outliers, stream, false);
}

int acino_ekf_run_pinhole(const acino_ekf_params* prm, const double* d_det, const double* d_cams32, const double* d_states0,
                          void* d_ws, size_t ws_bytes, double* d_est, double* d_smooth, int32_t* d_outliers, void* stream) {
  return ekf_run(prm, d_det, d_cams32, d_states0, d_ws, ws_bytes, d_est, d_smooth, d_outliers, stream, true);
}

}  // extern "C"
