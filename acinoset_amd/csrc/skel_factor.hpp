// What the uses of the skeleton FTE's Fisher matrix share (skel_cov.hip: the selected inverse; skel_sample.hip: joint
// posterior samples; skel_calib.hip: the sensitivity to the extrinsics; skel_links.hip: the sensitivity to the link lengths):
// the 16 x 16 tile product, the wave-level LDS hand-over, the banded block Cholesky A = L L^T as a device function template,
// the shape of the triangular solves on it, the workspace layout, the launches that build the band at an iterate and the one
// host pipeline of the two sensitivities (skel_sens_run; their device blocks are in skel_sens_dev.hpp).
#pragma once
#include <algorithm>
#include <cstddef>

#include "skel_host.hpp"

namespace acino {

constexpr double SK_PIV_REL = 1e-12;
// A state whose Fisher information, summed over the clip, is not above SK_UNOBS_REL times the largest such sum of the clip is
// UNOBSERVED (k_skel_observability): a Jacobian entry that is zero up to rounding is ~1e-16 relative, its square ~1e-32; the
// weakest genuinely observed state of the test inputs sits at 5e-5.
constexpr double SK_UNOBS_REL = ACINO_SKEL_UNOBS_REL;         // (acinoset_hip.h: part of the definition the ABI states)

// One 16 x 16 tile product on a wave: acc += sum_{k in [k0, k1)} a_at(k) b_at(k), where lane (li, lk) supplies
// a_at(k) = opA[row li][k] and b_at(k) = opB[k][col li]; acc[rr] is C[lk + 4 rr][li] (the MFMA layout of the solve).
template <class FA, class FB>
__device__ __forceinline__ d4 sk_tile_mac(d4 acc, int k0, int k1, int lk, FA a_at, FB b_at) {
  for (int k = k0; k < k1; k += 16) {
    double av[4], bv[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      av[s] = a_at(k + 4 * s + lk);
      bv[s] = b_at(k + 4 * s + lk);
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) acc = mfma(av[s], bv[s], acc);
  }
  return acc;
}

// What a wave's lanes have written to LDS is what its other lanes read next: no workgroup barrier, the wave alone
__device__ __forceinline__ void sk_wave_handover() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

constexpr int SKC_T = 512, SKC_W = SKC_T / 64;    // threads / waves of the one workgroup that factors a clip

// dynamic LDS of a kernel that calls skel_band_factor<PT>: the panel [4 PT][PT + 1]
inline size_t skel_factor_lds(int PT) { return sizeof(double) * (size_t)4 * PT * (PT + 1); }

// frame n's four blocks (n + j, n), j = 0..3, into the panel Pn[4 PT][PT + 1] (zeros past the clip's end); SKC_T threads
template <int PT>
__device__ __forceinline__ void skel_load_panel(double* __restrict__ Pn, const double* __restrict__ band, int n, int N) {
  constexpr int LDP = PT + 1, BB = PT * PT;
  for (int e = threadIdx.x; e < 4 * BB; e += SKC_T) {
    const int j = e / BB, rem = e % BB;
    Pn[(j * PT + rem / PT) * LDP + rem % PT] = (n + j < N) ? band[((size_t)n * 4 + j) * BB + rem] : 0.0;
  }
}

// The banded block Cholesky of one clip, left to right, by ONE workgroup of SKC_T threads (the factorisation of k_skel_solve
// without a right-hand side): panel in LDS, diagonal tiles by the register pivot chain, window update in memory, factored
// panels written back.  band[n][j] = block (n + j, n) of A in, of L out - except that every diagonal 16 x 16 tile of
// band[n][0] = L_nn is replaced by U_kk = L_kk^-T (upper triangular, exact zeros below).  diag0[n][PT]: the diagonal of A as
// built; a pivot that is not above SK_PIV_REL * A_pp sets *numeric_err.  Ends with a workgroup barrier.
template <int PT>
__device__ __forceinline__ void skel_band_factor(int N, double* __restrict__ band, const double* __restrict__ diag0,
                                                 int* numeric_err, double* __restrict__ Pn) {
  constexpr int LDP = PT + 1, NTP = PT / 16, RT = 4 * NTP, NT2 = NTP * NTP, BB = PT * PT;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, lk = lane >> 4;
  for (int n = 0; n < N; ++n) {
    skel_load_panel<PT>(Pn, band, n, N);
    __syncthreads();
#pragma unroll 1
    for (int kb = 0; kb < NTP; ++kb) {
      double* Tkk = Pn + (kb * 16) * LDP + kb * 16;
      if (wave == 0) {
        d4 acc;
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] = Tkk[(lk + 4 * r) * LDP + li];
        chol16_inv_acc<LDP>(Tkk, acc, lane, numeric_err);
      }
      __syncthreads();
      if (tid < 16) {                                          // pivot = 1 / U_pp^2 against the entry it was cancelled from
        const double u = Tkk[tid * LDP + tid];
        if (!(u * u * diag0[(size_t)n * PT + kb * 16 + tid] * SK_PIV_REL < 1.0)) atomicOr(numeric_err, 1);
      }
      for (int t = kb + 1 + wave; t < RT; t += SKC_W) {          // panel: tile(t, kb) <- tile(t, kb) U_kk
        double* At = Pn + (t * 16) * LDP + kb * 16;
        double av[4], bv[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          av[s] = At[li * LDP + 4 * s + lk];
          bv[s] = Tkk[(4 * s + lk) * LDP + li];
        }
        d4 acc = {0, 0, 0, 0};
#pragma unroll
        for (int s = 0; s < 4; ++s) acc = mfma(av[s], bv[s], acc);
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) At[(lk + 4 * rr) * LDP + li] = acc[rr];
      }
      __syncthreads();
      int q = 0;                                             // trailing tiles inside the panel
      for (int ct = kb + 1; ct < NTP; ++ct)
        for (int rt = ct; rt < RT; ++rt, ++q) {
          if (q % SKC_W != wave) continue;
          double* Cc = Pn + (rt * 16) * LDP + ct * 16;
          const double* Ar = Pn + (rt * 16) * LDP + kb * 16;
          const double* Ac = Pn + (ct * 16) * LDP + kb * 16;
          d4 a;
          double av[4], bv[4];
#pragma unroll
          for (int rr = 0; rr < 4; ++rr) a[rr] = Cc[(lk + 4 * rr) * LDP + li];
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            av[s] = Ar[li * LDP + 4 * s + lk];
            bv[s] = Ac[li * LDP + 4 * s + lk];
          }
#pragma unroll
          for (int s = 0; s < 4; ++s) a = mfma(-av[s], bv[s], a);
#pragma unroll
          for (int rr = 0; rr < 4; ++rr) Cc[(lk + 4 * rr) * LDP + li] = a[rr];
        }
      __syncthreads();
    }
    // ---- window update in memory: block (n + i, n + j) -= L_i L_j^T, stored at band[n + j][i - j]
    for (int t = wave; t < 6 * NT2; t += SKC_W) {
      const int blk = t / NT2, rem = t % NT2;
      const int i = blk < 1 ? 1 : (blk < 3 ? 2 : 3), j = blk < 1 ? 1 : (blk < 3 ? blk : blk - 2);
      const int rt = rem / NTP, ct = rem % NTP;
      if (n + i >= N) continue;
      double* Cg = band + ((size_t)(n + j) * 4 + (i - j)) * BB;
      d4 a;
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) a[rr] = Cg[(rt * 16 + lk + 4 * rr) * PT + ct * 16 + li];
      const double* Ar = Pn + (i * PT + rt * 16 + li) * LDP;
      const double* Ac = Pn + (j * PT + ct * 16 + li) * LDP;
      a = sk_tile_mac(a, 0, PT, lk, [&](int k) { return -Ar[k]; }, [&](int k) { return Ac[k]; });
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) Cg[(rt * 16 + lk + 4 * rr) * PT + ct * 16 + li] = a[rr];
    }
    // ---- the factored panel replaces the frame's blocks (read again by whoever walks back)
    for (int e = tid; e < 4 * BB; e += SKC_T) {
      const int j = e / BB, rem = e % BB;
      if (n + j < N || j == 0) band[((size_t)n * 4 + j) * BB + rem] = Pn[(j * PT + rem / PT) * LDP + rem % PT];
    }
    __syncthreads();
  }
}

// ---- the triangular solves on the factor, 64 right-hand-side columns per workgroup: k_skel_sample_back (skel_sample.hip,
//      L^-T) and k_skel_fwdsub (skel_calib.hip, L^-1) share the shape of a workgroup and the LDS layout of the blocks;
//      skel_links.hip launches both through their host launchers below
constexpr int SKS_W = 4, SKS_T = 64 * SKS_W, SKS_PANEL = 16 * SKS_W;

template <int PT>
struct SksShape {
  static constexpr bool ROT = PT % 32 == 0;        // L rows of 32 or 64 doubles: odd rows rotated by 16 columns
  static constexpr bool SROT = PT == 64;           // staging rows: padded by 2 doubles, or (no room at PT = 64) rotated by 2 li
  static constexpr int ST = SROT ? PT : PT + 2;
  static constexpr size_t lds = sizeof(double) * ((size_t)4 * PT * PT + (size_t)SKS_W * 16 * ST);
  // entry (k, m) of a block in LDS; m0 + li with m0 a multiple of 16 stays contiguous in li
  __device__ static __forceinline__ int at(int k, int m) { return k * PT + (ROT ? ((m + 16 * (k & 1)) & (PT - 1)) : m); }
  // entry (sample column c, state p) of a wave's staging tile
  __device__ static __forceinline__ int st(int c, int p) { return c * ST + (SROT ? ((p + 2 * c) & (PT - 1)) : p); }
};

// ---- host: the workspace both entries use, and the launches up to the band --------------------------------------------
struct SkelCovLayout {
  size_t dev, clip, H, g, hd, cost, opv, band, diag0, fxm, total;
  size_t dev0, unobs;              // with `observe` only (appended: the offsets above are the same either way)
};
// observe: room for what k_skel_observability needs - a second SkelDev (the prior switched off) and the mask [n_clips][P]
SkelCovLayout skel_cov_layout(size_t NT, int n_clips, int P, int PT, int n_ops, bool observe = false);
// Validates the link program, uploads it and the cameras (skel_upload: nothing on the host has to outlive the call), clears
// the clips' status words and launches k_skel_assemble<.., double> and k_skel_cov_build on stream s: on return the
// workspace holds band, fxm, diag0 and the link operators opv of every frame at d_x.
// observe (the layout must have been made with it): first the Fisher assembly with the prior off and k_skel_observability;
// the mask goes to the workspace and, if given, to d_unobserved[n_clips][P].  pin (needs observe): k_skel_cov_build pins the
// clip's unobserved states in every frame.  Without observe the launches and their arguments are what they were.
int skel_cov_launch_build(const acino_skel_fte_params* p, int n_clips, int camera_model, const acino_skel_op* h_ops,
                          const int32_t* h_active, const double* d_meas, const double* d_w, const double* d_cams,
                          const double* d_lo, const double* d_hi, const double* d_x, void* d_ws, const SkelCovLayout& lay,
                          hipStream_t s, bool observe = false, bool pin = false, uint8_t* d_unobserved = nullptr);
// The end of both entries: skel_read_status with the Fisher matrix's error text, and the clips' status words to h_status[n_clips]
// (may be NULL: then a singular clip fails the call whatever the batch).
int skel_cov_read_status(const SkelClip* d_clip, int n_clips, hipStream_t s, int32_t* h_status);
// k_skel_factor<PT> on stream s (skel_sample.hip), one workgroup per clip: band <- the factor, a failed pivot -> status 5.
int skel_launch_factor(int PT, int n_clips, const SkelDev* d_dev, SkelClip* d_clip, double* d_band, const double* d_diag0,
                       hipStream_t s);
// k_skel_fwdsub<PT> on stream s (skel_calib.hip): d_y[b][c] = L_b^-1 d_b[b][c] for the n_cols columns [n_clips][n_cols][N][n_act]
// (pinned and padding rows of d_b masked to 0 on the way in; a clip whose status is not 0 is left as it is).
int skel_launch_fwdsub(int PT, int n_clips, long long n_cols, const SkelDev* d_dev, const SkelClip* d_clip, const double* d_band,
                       const unsigned char* d_fxm, const double* d_b, double* d_y, hipStream_t s);
// k_skel_sample_back<PT> without the "+ x" on stream s: d_out[b][c] = L_b^-T d_y[b][c] for the n_cols columns
// [n_clips][n_cols][N][n_act] (the layout of the sampler's z, pinned rows masked to 0; NaN for a clip whose status is not 0).
int skel_launch_back_columns(int PT, int n_clips, long long n_cols, const SkelDev* d_dev, const SkelClip* d_clip,
                             const double* d_band, const unsigned char* d_fxm, const double* d_y, double* d_out, hipStream_t s);
// ---- host: the sensitivities S = -A^-1 G (skel_calib.hip, skel_links.hip): the covariance's workspace, then two column buffers
//      [n_clips][n_cols][N][n_act], the right-hand side (S in the end) and L^-1 of it
inline size_t skel_sens_column_bytes(const acino_skel_fte_params* p, int n_clips, int n_cols) {
  return skel_align256(sizeof(double) * (size_t)n_clips * n_cols * p->n_frames * p->n_active);
}
// what a ..._workspace_bytes query of theirs answers (0: outside the covariance's limits)
inline size_t skel_sens_workspace_bytes(const acino_skel_fte_params* p, int n_clips, int pin_unobserved, int n_cols) {
  const size_t cov = acino_skel_fte_covariance_pinned_workspace_bytes(p, n_clips, pin_unobserved);
  return cov == 0 ? 0 : cov + 2 * skel_sens_column_bytes(p, n_clips, n_cols);
}
struct SkelSens {                  // what the pipeline hands to an entry's two launches
  size_t NT;                       // frames of all clips: the grid of both
  hipStream_t s;
  const SkelDev* d_dev;
  const SkelClip* d_clip;
  const double* d_opv;
  const unsigned char *d_fxm, *d_unobs;      // d_unobs: the clips' masks when the unobserved states are pinned, else NULL
  double* d_cols;                  // the right-hand side -G out of rhs, S into combine
  const double* d_y;               // L^-1 of the right-hand side, for a combine that reduces over it (skel_link_fit.hip)
};
// An entry behind its own argument checks: the workspace check (query: the entry's ..._workspace_bytes; ws_cols: the columns
// its buffers are sized for), skel_cov_launch_build, rhs(SkelSens) -> factor -> L^-1 -> L^-T on n_cols columns -> combine(SkelSens),
// skel_cov_read_status.  rhs and combine each launch one kernel on stream s; kernels: the entry's three (both right-hand
// sides, the combine), which get the 160 KB dynamic-LDS attribute once per device (once: a static of the entry).
template <class Rhs, class Combine>
inline int skel_sens_run(const acino_skel_fte_params* p, int n_clips, int camera_model, const acino_skel_op* h_ops,
                         const int32_t* h_active, const double* d_meas, const double* d_w, const double* d_cams, const double* d_lo,
                         const double* d_hi, const double* d_x, int n_cols, int ws_cols, const char* query, int32_t* h_status,
                         void* d_ws, size_t ws_bytes, void* stream, int pin_unobserved, uint8_t* d_unobserved, PerDeviceOnce& once,
                         const void* const (&kernels)[3], Rhs rhs, Combine combine) {
  const int B = n_clips, P = p->n_active, PT = (P + 15) / 16 * 16;
  const size_t NT = (size_t)p->n_frames * B;
  const bool pin = pin_unobserved == 1, observe = pin || d_unobserved != nullptr;
  const SkelCovLayout lay = skel_cov_layout(NT, B, P, PT, p->n_ops, observe);
  const size_t col_bytes = skel_sens_column_bytes(p, B, ws_cols);
  int rc = skel_check_workspace(d_ws, ws_bytes, lay.total + 2 * col_bytes, query, ACINO_ERR_WORKSPACE);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  if ((rc = skel_cov_launch_build(p, B, camera_model, h_ops, h_active, d_meas, d_w, d_cams, d_lo, d_hi, d_x, d_ws, lay, s, observe, pin,
                                  d_unobserved)))
    return rc;
  char* base = (char*)d_ws;
  auto D = [&](size_t off) { return reinterpret_cast<double*>(base + off); };
  const SkelDev* d_dev = reinterpret_cast<const SkelDev*>(base + lay.dev);
  SkelClip* d_clip = reinterpret_cast<SkelClip*>(base + lay.clip);
  const unsigned char* d_fxm = reinterpret_cast<const unsigned char*>(base + lay.fxm);
  double *d_b = D(lay.total), *d_y = D(lay.total + col_bytes);      // -G, then S; L^-1 (-G)
  const SkelSens a = {NT, s, d_dev, d_clip, D(lay.opv), d_fxm, pin ? reinterpret_cast<const unsigned char*>(base + lay.unobs) : nullptr, d_b, d_y};
  if (once.first())
    for (const void* k : kernels) ACINO_HIP_CHECK(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  rhs(a);
  ACINO_LAUNCH_CHECK();
  if ((rc = skel_launch_factor(PT, B, d_dev, d_clip, D(lay.band), D(lay.diag0), s))) return rc;
  if ((rc = skel_launch_fwdsub(PT, B, n_cols, d_dev, d_clip, D(lay.band), d_fxm, d_b, d_y, s))) return rc;
  if ((rc = skel_launch_back_columns(PT, B, n_cols, d_dev, d_clip, D(lay.band), d_fxm, d_y, d_b, s))) return rc;
  combine(a);
  ACINO_LAUNCH_CHECK();
  return skel_cov_read_status(d_clip, B, s, h_status);
}
// dynamic LDS of k_skel_cov_rates (skel_cov_rates.hip): three blocks [P][P + 1]
inline size_t skel_cov_rates_lds(int P) { return sizeof(double) * (size_t)3 * P * (P + 1); }
// k_skel_cov_rates on stream s, one workgroup per frame, after k_skel_selinv has left the blocks of the inverse in d_band:
// covariance of dx, ddx ([NT][P][P]) and of the pose velocities ([NT][n_pose][3][3], [NT][n_pose]); any output may be NULL.
// d_unobs: NULL, or the clips' masks [n_clips][P] when the unobserved states are pinned.
int skel_cov_launch_rates(size_t NT, int P, const SkelDev* d_dev, const SkelClip* d_clip, const double* d_band,
                          const unsigned char* d_fxm, const double* d_opv, const unsigned char* d_unobs, double h, double* d_cov_dx,
                          double* d_cov_ddx, double* d_cov_vel, double* d_std_vel, hipStream_t s);

}  // namespace acino
