// Covariances of the EKF + RTS smoother (gfx950, fp64): the second half of Rauch-Tung-Striebel and the step from a
// 75 x 75 state covariance to metres per marker.  An opt-in second pass over what acino_ekf_run leaves in its workspace
// (include/acinoset_hip.h, EKF section): the filtered covariances P_est[i] and the smoother gains A_i, stored transposed.
//
//   P_s[i] = P_est[i] + A_i (P_s[i+1] - P_pred[i+1]) A_i^T,   i = N-2 .. 1,   P_pred[i+1] = F P_est[i] F^T + Q
//
// P_pred is rebuilt with predict_cov_entry, the arithmetic of the filter and of the gain kernel (ekf_dev.hpp); the forward
// kernel stores nothing new.  Frames 0 and N-1 carry P_est bit for bit: the reference's smoother returns the filtered
// state there (:836-839), so the filtered covariance is the one that belongs to the reported state.  The gate does not
// enter: a gated pair has its residual zeroed, K and (I - K H) P keep its rows of H.
//
// k_rts_cov_recurse: the chain is sequential in frames, so ONE workgroup runs a sequence with three 80 x 81 matrices in
// LDS (3 x 51 840 B = kRtsCovLds, what k_rts_gain opts in to; a fourth does not fit in 160 KB):
//   D   P_s[i+1]                  -> D - P_pred[i+1]   -> lower tiles of T A^T, mirrored -> P_s[i]
//   W   P_est[i] -> P_pred[i+1] in place               -> A_i^T (the workspace's layout, loaded as it lies)
//   T   A_i D
// Both products are 16 x 16 fp64 MFMA tiles (mma_seq).  Only the 15 lower-triangle tiles of the second product are
// computed and every entry is written to (r, c) and (c, r); of a diagonal tile the lower half is kept.  P_est is symmetric
// bit for bit, so P_s is.  The next frame's A_{i-1}^T and P_est[i-1] are requested before the products and land in
// registers while the matrix cores work; P_est[i] stays in the registers it arrived in until it is added at the end.
//
// k_ekf_marker_cov: one workgroup per (sequence, frame): FK frame with rotation axes at the reported pose, the analytic
// marker Jacobian J_l (axis x lever arm: rate_jac of fte_cov_dev.hpp, parameters mapped through c_ekf2act),
// cov_pos[l] = J_l P[:25, :25] J_l^T, std_pos[l] = sqrt(trace), std_state = sqrt(diag P).
#include "common.hpp"
#include "ekf_dev.hpp"
#include "fte_cov_dev.hpp"

namespace acino {

constexpr int CE = ES * ES;                    // 5625 doubles: a frame's covariance or gain in global memory
constexpr int CPT = (CE + 255) / 256;          // 22 of them per thread
constexpr size_t kRtsCovLds = 3 * MAT * sizeof(double);
static_assert(kRtsCovLds <= 160 * 1024, "three 80 x 81 matrices must fit the 160 KB LDS");

// The two halves of a 75 x 75 matrix's way from global memory into an 80 x 81 LDS buffer: request it into registers
// now, stage it when its turn comes (a frame is 45 000 B: not a multiple of 16, so single doubles).
__device__ __forceinline__ void cov_fetch(double (&v)[CPT], const double* __restrict__ src, int tid) {
#pragma unroll
  for (int k = 0; k < CPT; ++k) {
    const int e = tid + 256 * k;
    v[k] = e < CE ? src[e] : 0.0;
  }
}
__device__ __forceinline__ void cov_stage(double* dst, const double (&v)[CPT], int tid) {
#pragma unroll
  for (int k = 0; k < CPT; ++k) {
    const int e = tid + 256 * k;
    if (e < CE) dst[(e / ES) * LD + e % ES] = v[k];
  }
}

__global__ void __launch_bounds__(256)
k_rts_cov_recurse(EkfK K, const double* __restrict__ P_est_all, const double* __restrict__ A_all, double* __restrict__ P_s_all) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  double* D = sm;                  // [80][81]
  double* W = D + MAT;             // [80][81]
  double* T = W + MAT;             // [80][81]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, lk = lane >> 4;
  const int N = K.n_frames, seq = blockIdx.x;
  const double* Pe = P_est_all + (size_t)seq * N * CE;
  const double* At = A_all + (size_t)seq * N * CE;       // stored TRANSPOSED
  double* Ps = P_s_all + (size_t)seq * N * CE;
  for (int e = tid; e < CE; e += 256) {                  // the ends: the filtered covariance, bit for bit
    Ps[e] = Pe[e];
    if (N > 1) Ps[(size_t)(N - 1) * CE + e] = Pe[(size_t)(N - 1) * CE + e];
  }
  if (N < 3) return;
  double pe[CPT], at[CPT], pn[CPT];
  cov_fetch(pn, Pe + (size_t)(N - 1) * CE, tid);
  cov_fetch(pe, Pe + (size_t)(N - 2) * CE, tid);
  cov_fetch(at, At + (size_t)(N - 2) * CE, tid);
  for (int e = tid; e < 3 * MAT; e += 256) sm[e] = 0.0;  // the padding of all three stays 0 from here on
  __syncthreads();
  cov_stage(D, pn, tid);                                 // P_s[N-1]
  for (int i = N - 2; i >= 1; --i) {
    cov_stage(W, pe, tid);
    __syncthreads();
    for (int e = tid; e < EP * EP; e += 256) predict_cov_entry(W, LD, W, LD, e / EP, e % EP, K.sT);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < CPT; ++k) {                      // D = P_s[i+1] - P_pred[i+1]
      const int e = tid + 256 * k;
      if (e < CE) D[(e / ES) * LD + e % ES] -= W[(e / ES) * LD + e % ES];
    }
    __syncthreads();
    cov_stage(W, at, tid);                               // W = A_i^T : W[k][r] = A_i[r][k]
    if (i > 1) {                                         // the next frame's operands: in flight during the products
      cov_fetch(pn, Pe + (size_t)(i - 1) * CE, tid);
      cov_fetch(at, At + (size_t)(i - 1) * CE, tid);
    }
    __syncthreads();
    for (int t = wave; t < NT * NT; t += 4) {            // T = A_i D = W^T D
      const int ti = t / NT, tj = t % NT;
      d4 acc = {0, 0, 0, 0};
#pragma unroll
      for (int k = 0; k < NT; ++k)
        acc = mma_seq<4, false>(acc, W + (16 * k + lk) * LD + 16 * ti + li, 4 * LD, D + (16 * k + lk) * LD + 16 * tj + li, 4 * LD);
#pragma unroll
      for (int r = 0; r < 4; ++r) T[(16 * ti + lk + 4 * r) * LD + 16 * tj + li] = acc[r];
    }
    __syncthreads();
    for (int t = wave; t < NT * (NT + 1) / 2; t += 4) {  // lower tiles of T A_i^T = T W, mirrored into D
      const int ti = t >= 10 ? 4 : (t >= 6 ? 3 : (t >= 3 ? 2 : (t >= 1 ? 1 : 0))), tj = t - ti * (ti + 1) / 2;
      d4 acc = {0, 0, 0, 0};
#pragma unroll
      for (int k = 0; k < NT; ++k)
        acc = mma_seq<4, false>(acc, T + (16 * ti + li) * LD + 16 * k + lk, 4, W + (16 * k + lk) * LD + 16 * tj + li, 4 * LD);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 16 * ti + lk + 4 * r, col = 16 * tj + li;
        if (row >= col) {                                // always, off the diagonal tiles
          D[row * LD + col] = acc[r];
          D[col * LD + row] = acc[r];
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < CPT; ++k) {                      // P_s[i] = P_est[i] + T A_i^T : to global memory and into D
      const int e = tid + 256 * k;
      if (e < CE) {
        const double v = pe[k] + D[(e / ES) * LD + e % ES];
        D[(e / ES) * LD + e % ES] = v;
        Ps[(size_t)i * CE + e] = v;
      }
    }
#pragma unroll
    for (int k = 0; k < CPT; ++k) pe[k] = pn[k];
  }
}

__global__ void __launch_bounds__(128)
k_ekf_marker_cov(const double* __restrict__ states, const double* __restrict__ P_all, double* __restrict__ cov_pos,
                 double* __restrict__ std_pos, double* __restrict__ std_state) {
  __shared__ CovFrame F;
  __shared__ double S[EP][EP + 1];           // P[:25, :25]
  __shared__ double J[NL * 3][EP + 1];       // d FK_l,i / d pose parameter q (qb_list order)
  __shared__ double tr[NL * 3];
  const int tid = threadIdx.x;
  const size_t f = blockIdx.x;
  const double* x = states + f * ES;
  const double* P = P_all + f * CE;
  if (std_state && tid < ES) std_state[f * ES + tid] = sqrt(P[tid * ES + tid]);
  if (!cov_pos && !std_pos) return;
  for (int e = tid; e < EP * EP; e += 128) S[e / EP][e % EP] = P[(e / EP) * ES + e % EP];
  if (tid < EP) {
    const int a = c_ekf2act[tid];
    const double xv = x[tid];
    if (a < 3) {
      F.pos[20][a] = xv;
    } else {
      double s, c;
      sincos(xv, &s, &c);
      F.sc[a - 3][0] = s;
      F.sc[a - 3][1] = c;
    }
  }
  __syncthreads();
  if (tid < 3) fk_columns(F, tid);
  __syncthreads();
  for (int task = tid; task < NL * EP; task += 128) {
    const int l = task / EP, q = task % EP, p = c_ekf2act[q];
#pragma unroll
    for (int i = 0; i < 3; ++i) J[3 * l + i][q] = rate_jac(F, l, i, p);
  }
  __syncthreads();
  if (tid < NL * 3) {
    const int l = tid / 3, i = tid % 3;
    double o0 = 0.0, o1 = 0.0, o2 = 0.0;
    for (int q = 0; q < EP; ++q) {
      double t = 0.0;
      for (int p = 0; p < EP; ++p) t += J[tid][p] * S[p][q];
      o0 += t * J[3 * l][q];
      o1 += t * J[3 * l + 1][q];
      o2 += t * J[3 * l + 2][q];
    }
    if (cov_pos) {
      double* out = cov_pos + (f * NL + l) * 9 + 3 * i;
      out[0] = o0;
      out[1] = o1;
      out[2] = o2;
    }
    tr[tid] = i == 0 ? o0 : (i == 1 ? o1 : o2);
  }
  __syncthreads();
  if (std_pos && tid < NL) std_pos[f * NL + tid] = sqrt(fmax(tr[3 * tid] + tr[3 * tid + 1] + tr[3 * tid + 2], 0.0));
}

}  // namespace acino

using namespace acino;

extern "C" {

int acino_ekf_smoothed_covariance(const acino_ekf_params* prm, const void* d_ws, size_t ws_bytes, double* d_P_smooth, void* stream) {
  ACINO_REQUIRE(prm, "params");
  ACINO_REQUIRE(prm->n_frames >= 1 && prm->n_seq >= 1, "n_frames, n_seq");
  ACINO_REQUIRE(prm->n_frames <= INT32_MAX, "n_frames");
  ACINO_REQUIRE(prm->fps > 0, "fps");
  ACINO_REQUIRE(d_ws && d_P_smooth, "null buffer");
  ACINO_REQUIRE(((uintptr_t)d_ws & 255) == 0, "workspace must be 256-byte aligned");
  ACINO_REQUIRE(ws_bytes >= acino_ekf_workspace_bytes(prm->n_frames, prm->n_seq), "workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const size_t N = (size_t)prm->n_frames * prm->n_seq;
  const char* w = (const char*)d_ws;
  const double* P_est = (const double*)w;
  const double* A = (const double*)(w + a256(N * ES * ES * 8));
  EkfK K = {};
  K.n_frames = (int)prm->n_frames;
  K.sT = 1.0 / prm->fps;
  static PerDeviceOnce attr;
  if (attr.first())
    ACINO_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_rts_cov_recurse),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)kRtsCovLds));
  hipLaunchKernelGGL(k_rts_cov_recurse, dim3(prm->n_seq), dim3(256), kRtsCovLds, s, K, P_est, A, d_P_smooth);
  ACINO_LAUNCH_CHECK();
  return ACINO_OK;
}

int acino_ekf_marker_covariance(const acino_ekf_params* prm, const double* d_states, const double* d_P, double* d_cov_pos,
                                double* d_std_pos, double* d_std_state, void* stream) {
  ACINO_REQUIRE(prm, "params");
  ACINO_REQUIRE(prm->n_frames >= 1 && prm->n_seq >= 1, "n_frames, n_seq");
  ACINO_REQUIRE(prm->n_frames * (int64_t)prm->n_seq <= INT32_MAX, "n_seq * n_frames");
  ACINO_REQUIRE(d_states && d_P, "null buffer");
  ACINO_REQUIRE(d_cov_pos || d_std_pos || d_std_state, "no output requested");
  hipLaunchKernelGGL(k_ekf_marker_cov, dim3((unsigned)(prm->n_frames * prm->n_seq)), dim3(128), 0, (hipStream_t)stream, d_states,
                     d_P, d_cov_pos, d_std_pos, d_std_state);
  ACINO_LAUNCH_CHECK();
  return ACINO_OK;
}

}  // extern "C"
