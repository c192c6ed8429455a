// Joint posterior samples of the generic-skeleton FTE trajectory (gfx950, fp64): with A the matrix of skel_cov.hip at the
// iterate x (Fisher blocks with w^2, 2 q D3^T D3, bound-active variables pinned by skel_fixed, unknowns frame-major, no
// Marquardt term) and A = L L^T its banded block Cholesky,
//     x_samples[b][s] = x[b] + delta,     delta = L_b^-T z[b][s],     z of a pinned variable counted as 0
// for the caller's z: Cov(delta) = A^-1 for standard-normal z, every cross-frame block included; delta is exactly 0 at pinned
// variables.  The map is deterministic (the library owns no random generator) and delta(s) depends on z(s) alone.  Samples
// are NOT clipped to the box: the Laplace posterior is a Gaussian, only the pinned variables are held.
//   k_skel_assemble<.., double>, k_skel_cov_build   skel_cov.hip's (skel_cov_launch_build).  With pin_unobserved the build
//                           step gets the clips' masks of k_skel_observability and pins those states in every frame: to the
//                           kernels below a clip-wide pin is a bound pin, delta is exactly 0 there whatever z holds.
//   k_skel_factor<PT>       one workgroup per clip: skel_band_factor<PT> (skel_factor.hpp, the forward half of k_skel_selinv).
//                           Afterwards band[n][j] = L_n+j,n, the diagonal 16 x 16 tiles of band[n][0] replaced by
//                           U_kk = L_kk^-T.  A pivot not above SK_PIV_REL * A_pp: status 5.
//   k_skel_sample_back<PT>  grid (sample panels, clips), the hot path.  A workgroup is SKS_W = 4 waves and owns a panel of
//                           SKS_PANEL = 64 samples, a wave 16 sample columns.  It walks n = N-1 .. 0; per frame the four blocks
//                           L_nn, L_n+1,n .. L_n+3,n go to LDS once for all four waves (the only two workgroup barriers of a
//                           frame), then every wave on its own columns:
//                               r = z_n - sum_{j=1..3} L_n+j,n^T delta_n+j
//                               delta_kb = U_kk (r_kb - sum_{t > kb} L(t, kb)^T delta_t),      kb = NTP-1 .. 0
//                           every product an fp64 16 x 16 x 4 MFMA.  The last three delta blocks of the panel stay in
//                           registers as MFMA accumulator tiles - which ARE the B operands of the next frames' products (lane
//                           (li, lk) holds rows lk + 4 s of column li, the k of step s) - so no delta is ever read back.
//                           The A operand of every product is a tile of L read DOWN its rows (A[m][k] = L[k][m]): lanes li
//                           run along a row of LDS; the diagonal tiles are stored transposed (U_kk^T) to read the same way,
//                           and where the row length is a multiple of 32 doubles the odd rows are rotated by 16 columns so
//                           that the two rows a half-wave reads fall into different banks.  z is read and x + delta written
//                           once each, rows of P contiguous doubles, through a per-wave staging tile [16][P] in LDS (z masked
//                           by the pin mask and the padding rows p >= P on the way in).
//                           LDS (SksShape<PT> of skel_factor.hpp, shared with k_skel_fwdsub of skel_calib.hip):
//                           4 PT^2 + SKS_W * 16 * ST doubles (ST = PT + 2, or PT with rotated rows at PT = 64):
//                           50 / 99 KB at PT = 32 / 48, and at PT = 64 the blocks' 128 KB + 32 KB = the whole 160 KB.
//   k_skel_sample_fk        one thread per (clip, sample, frame): the real forward kinematics of the sample (the link
//                           program on the sample's active states), not the linearisation.
// A singular clip (status 5) gets NaN in both outputs, written by the last two kernels; the other clips of the batch stand.
#include <cstddef>
#include <cstdint>
#include <limits>
#include <vector>

#include "skel_factor.hpp"

namespace acino {

template <int PT>
__global__ void __launch_bounds__(SKC_T)
k_skel_factor(const SkelDev* __restrict__ dev, SkelClip* __restrict__ clip, double* __restrict__ band_all,
              const double* __restrict__ diag0_all) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  SkelClip& cs = clip[blockIdx.x];
  const int N = dev->n_frames;
  const size_t fr0 = (size_t)blockIdx.x * N;
  skel_band_factor<PT>(N, band_all + fr0 * 4 * PT * PT, diag0_all + fr0 * PT, &cs.pivot_err,
                       reinterpret_cast<double*>(smem_raw));
  if (threadIdx.x == 0 && __hip_atomic_load(&cs.pivot_err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) cs.status = 5;
}

// ADDX: x + delta (the samples); false: delta alone (skel_launch_back_columns: x_all is not read)
template <int PT, bool ADDX>
__global__ void __launch_bounds__(SKS_T)
k_skel_sample_back(const SkelDev* __restrict__ dev, const SkelClip* __restrict__ clip, const double* __restrict__ band_all,
                   const unsigned char* __restrict__ fxm_all, const double* __restrict__ x_all, const double* __restrict__ z_all,
                   double* __restrict__ xs_all, long long S) {
  using Sh = SksShape<PT>;
  constexpr int NTP = PT / 16, BB = PT * PT;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, lk = lane >> 4;
  const int N = dev->n_frames, P = dev->n_act, b = blockIdx.y;
  const long long s0 = (long long)blockIdx.x * SKS_PANEL + wave * 16;      // this wave's first sample
  const size_t fr0 = (size_t)b * N;
  const double* const band = band_all + fr0 * 4 * BB;
  const unsigned char* const fxm = fxm_all + fr0 * PT;
  const double* const x = x_all + fr0 * P;
  const size_t row0 = ((size_t)b * (size_t)S + (size_t)s0) * N * P;        // (b, s0, 0, 0) of z and x_samples
  const size_t srow = (size_t)N * P;                                       // from one sample to the next
  if (clip[b].status != 0) {                                               // singular clip: NaN (uniform over the workgroup)
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (int c = 0; c < 16 && s0 + c < S; ++c)
      for (size_t e = lane; e < srow; e += 64) xs_all[row0 + c * srow + e] = nan;
    return;
  }
  double* const Lb = reinterpret_cast<double*>(smem_raw);                  // [4][PT][PT], Sh::at
  double* const stage = Lb + 4 * BB + wave * 16 * Sh::ST;                   // [16][ST], Sh::st: this wave's
  const bool busy = s0 < S;
  d4 d[3][NTP];                                                            // delta_n+1, delta_n+2, delta_n+3: tiles of 16 rows
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int t = 0; t < NTP; ++t) d[j][t] = d4{0, 0, 0, 0};
  for (int n = N - 1; n >= 0; --n) {
    __syncthreads();                                                       // the previous frame's blocks have been read
    for (int e = tid; e < 4 * BB; e += SKS_T) {
      const int j = e / BB, k = (e % BB) / PT, m = e % PT;
      if (n + j >= N) break;                                               // (e grows with j: nothing further to load)
      const double v = band[((size_t)n * 4 + j) * BB + k * PT + m];
      const bool diag = j == 0 && (k >> 4) == (m >> 4);                     // U_kk goes in transposed
      Lb[j * BB + (diag ? Sh::at((k & ~15) + (m & 15), (m & ~15) + (k & 15)) : Sh::at(k, m))] = v;
    }
    __syncthreads();
    if (!busy) continue;
    // ---- z_n of the wave's 16 samples -> staging (rows along p), masked; then r in the accumulator layout
    for (int e = lane; e < 16 * PT; e += 64) {
      const int c = e / PT, p = e % PT;
      double v = 0.0;
      if (s0 + c < S && p < P && !fxm[(size_t)n * PT + p]) v = z_all[row0 + c * srow + (size_t)n * P + p];
      stage[Sh::st(c, p)] = v;
    }
    sk_wave_handover();
    d4 r[NTP];
#pragma unroll
    for (int kb = 0; kb < NTP; ++kb)
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) r[kb][rr] = stage[Sh::st(li, kb * 16 + lk + 4 * rr)];
    // ---- r -= L_n+j,n^T delta_n+j
#pragma unroll
    for (int j = 1; j < 4; ++j) {
      if (n + j >= N) break;
      const double* Lj = Lb + j * BB;
#pragma unroll
      for (int kb = 0; kb < NTP; ++kb)
#pragma unroll
        for (int t = 0; t < NTP; ++t) {
          double av[4];
#pragma unroll
          for (int s = 0; s < 4; ++s) av[s] = Lj[Sh::at(t * 16 + 4 * s + lk, kb * 16 + li)];
#pragma unroll
          for (int s = 0; s < 4; ++s) r[kb] = mfma(-av[s], d[j - 1][t][s], r[kb]);
        }
    }
    // ---- delta_kb = U_kk (r_kb - sum_{t > kb} L(t, kb)^T delta_t), last tile first
    d4 dn[NTP];
#pragma unroll
    for (int kb = NTP - 1; kb >= 0; --kb) {
      d4 acc = r[kb];
#pragma unroll
      for (int t = kb + 1; t < NTP; ++t) {
        double av[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) av[s] = Lb[Sh::at(t * 16 + 4 * s + lk, kb * 16 + li)];
#pragma unroll
        for (int s = 0; s < 4; ++s) acc = mfma(-av[s], dn[t][s], acc);
      }
      double uv[4];
#pragma unroll
      for (int s = 0; s < 4; ++s) uv[s] = Lb[Sh::at(kb * 16 + 4 * s + lk, kb * 16 + li)];     // U_kk^T[k][li] = U_kk[li][k]
      d4 o = {0, 0, 0, 0};
#pragma unroll
      for (int s = 0; s < 4; ++s) o = mfma(uv[s], acc[s], o);
      dn[kb] = o;
    }
    // ---- x_n + delta -> x_samples through the staging tile
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int kb = 0; kb < NTP; ++kb)
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) stage[Sh::st(li, kb * 16 + lk + 4 * rr)] = dn[kb][rr];
    sk_wave_handover();
    for (int e = lane; e < 16 * PT; e += 64) {
      const int c = e / PT, p = e % PT;
      if (s0 + c < S && p < P) {
        if constexpr (ADDX) xs_all[row0 + c * srow + (size_t)n * P + p] = x[(size_t)n * P + p] + stage[Sh::st(c, p)];
        else xs_all[row0 + c * srow + (size_t)n * P + p] = stage[Sh::st(c, p)];
      }
    }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int t = 0; t < NTP; ++t) {
      d[2][t] = d[1][t];
      d[1][t] = d[0][t];
      d[0][t] = dn[t];
    }
  }
}

// poses of every sample: one thread per row (clip, sample, frame) of x_samples
__global__ void __launch_bounds__(256)
k_skel_sample_fk(const SkelDev* __restrict__ dev, const SkelClip* __restrict__ clip, const double* __restrict__ xs,
                 double* __restrict__ pos, long long S, long long n_rows) {
  const SkelDev& D = *dev;
  const long long row = (long long)blockIdx.x * 256 + threadIdx.x;
  if (row >= n_rows) return;
  double* out = pos + row * D.n_pose * 3;
  if (clip[row / (S * D.n_frames)].status != 0) {
    for (int e = 0; e < D.n_pose * 3; ++e) out[e] = std::numeric_limits<double>::quiet_NaN();
    return;
  }
  skel_pose_row(D, xs + row * D.n_act, out);
}

template <int PT>
static int skel_factor_launch(int B, const SkelDev* d_dev, SkelClip* d_clip, double* d_band, const double* d_diag0, hipStream_t s) {
  static PerDeviceOnce attr;
  if (attr.first())
    ACINO_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_skel_factor<PT>),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  static_assert(sizeof(double) * 4 * PT * (PT + 1) <= 160 * 1024, "LDS");
  hipLaunchKernelGGL(k_skel_factor<PT>, dim3(B), dim3(SKC_T), skel_factor_lds(PT), s, d_dev, d_clip, d_band, d_diag0);
  ACINO_LAUNCH_CHECK();
  return ACINO_OK;
}

template <int PT, bool ADDX>
static int skel_back_launch(int B, long long S, const SkelDev* d_dev, const SkelClip* d_clip, const double* d_band,
                            const unsigned char* d_fxm, const double* d_x, const double* d_z, double* d_xs, hipStream_t s) {
  static PerDeviceOnce attr;
  if (attr.first())
    ACINO_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_skel_sample_back<PT, ADDX>),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  static_assert(SksShape<PT>::lds <= 160 * 1024, "LDS");
  const long long panels = (S + SKS_PANEL - 1) / SKS_PANEL;
  hipLaunchKernelGGL((k_skel_sample_back<PT, ADDX>), dim3((unsigned)panels, (unsigned)B), dim3(SKS_T), SksShape<PT>::lds, s, d_dev,
                     d_clip, d_band, d_fxm, d_x, d_z, d_xs, S);
  ACINO_LAUNCH_CHECK();
  return ACINO_OK;
}

int skel_launch_factor(int PT, int n_clips, const SkelDev* d_dev, SkelClip* d_clip, double* d_band, const double* d_diag0,
                       hipStream_t s) {
  return skel_dispatch_pt(PT, [&](auto pt) { return skel_factor_launch<decltype(pt)::value>(n_clips, d_dev, d_clip, d_band, d_diag0, s); });
}

int skel_launch_back_columns(int PT, int n_clips, long long n_cols, const SkelDev* d_dev, const SkelClip* d_clip,
                             const double* d_band, const unsigned char* d_fxm, const double* d_y, double* d_out, hipStream_t s) {
  return skel_dispatch_pt(PT, [&](auto pt) {
    return skel_back_launch<decltype(pt)::value, false>(n_clips, n_cols, d_dev, d_clip, d_band, d_fxm, nullptr, d_y, d_out, s);
  });
}

static bool overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return pa < pb + nb && pb < pa + na;
}

}  // namespace acino

using namespace acino;

extern "C" {

size_t acino_skel_fte_sample_workspace_bytes(const acino_skel_fte_params* p, int n_clips, int64_t n_samples) {
  if (n_samples < 1) return 0;
  return acino_skel_fte_covariance_workspace_bytes(p, n_clips);             // (the samples live in the caller's arrays)
}

size_t acino_skel_fte_sample_pinned_workspace_bytes(const acino_skel_fte_params* p, int n_clips, int64_t n_samples,
                                                    int pin_unobserved) {
  if (n_samples < 1) return 0;
  return acino_skel_fte_covariance_pinned_workspace_bytes(p, n_clips, pin_unobserved);
}

int acino_skel_fte_sample_pinned(const acino_skel_fte_params* p, int n_clips, int camera_model, const acino_skel_op* h_ops,
                          const int32_t* h_active, const double* d_meas, const double* d_w, const double* d_cams,
                          const double* d_lo, const double* d_hi, const double* d_x, int64_t n_samples, const double* d_z,
                          double* d_x_samples, double* d_pos_samples, int32_t* h_status, void* d_ws, size_t ws_bytes,
                          void* stream, int pin_unobserved, uint8_t* d_unobserved) {
  int rc = skel_check_batch(p, n_clips, true, camera_model, h_ops && h_active && d_meas && d_w && d_cams && d_lo && d_hi && d_x && d_ws);
  if (rc) return rc;
  ACINO_REQUIRE(pin_unobserved == 0 || pin_unobserved == 1, "pin_unobserved: 0 or 1");
  ACINO_REQUIRE(n_samples >= 1, "n_samples >= 1");
  ACINO_REQUIRE(d_z && d_x_samples, "d_z and d_x_samples must not be NULL");
  const int N = p->n_frames, B = n_clips, P = p->n_active, PT = (P + 15) / 16 * 16;
  const size_t NT = (size_t)N * B;                           // frames of all clips
  ACINO_REQUIRE((uint64_t)n_samples <= (((uint64_t)1 << 31) - 1) * SKS_PANEL, "n_samples: too many sample panels for one launch");
  ACINO_REQUIRE((double)NT * (double)n_samples * (double)std::max(P, 3 * p->n_pose) < 9e18 / sizeof(double), "samples array too large");
  const size_t rows = NT * (size_t)n_samples, z_bytes = sizeof(double) * rows * P;
  ACINO_REQUIRE(!overlap(d_z, z_bytes, d_x_samples, z_bytes), "d_z overlaps d_x_samples");
  ACINO_REQUIRE(!d_pos_samples || !overlap(d_z, z_bytes, d_pos_samples, sizeof(double) * rows * p->n_pose * 3),
                "d_z overlaps d_pos_samples");
  const bool pin = pin_unobserved == 1, observe = pin || d_unobserved != nullptr;
  const SkelCovLayout lay = skel_cov_layout(NT, B, P, PT, p->n_ops, observe);
  if ((rc = skel_check_workspace(d_ws, ws_bytes, lay.total,
                                 observe ? "acino_skel_fte_sample_pinned_workspace_bytes" : "acino_skel_fte_sample_workspace_bytes",
                                 ACINO_ERR_WORKSPACE)))
    return rc;
  hipStream_t s = (hipStream_t)stream;
  if ((rc = skel_cov_launch_build(p, B, camera_model, h_ops, h_active, d_meas, d_w, d_cams, d_lo, d_hi, d_x, d_ws, lay, s, observe, pin,
                                  d_unobserved)))
    return rc;
  char* base = (char*)d_ws;
  auto D = [&](size_t off) { return reinterpret_cast<double*>(base + off); };
  SkelDev* d_dev = reinterpret_cast<SkelDev*>(base + lay.dev);
  SkelClip* d_clip = reinterpret_cast<SkelClip*>(base + lay.clip);
  unsigned char* d_fxm = reinterpret_cast<unsigned char*>(base + lay.fxm);
  if ((rc = skel_launch_factor(PT, B, d_dev, d_clip, D(lay.band), D(lay.diag0), s))) return rc;
  rc = skel_dispatch_pt(PT, [&](auto pt) {
    return skel_back_launch<decltype(pt)::value, true>(B, n_samples, d_dev, d_clip, D(lay.band), d_fxm, d_x, d_z, d_x_samples, s);
  });
  if (rc) return rc;
  if (d_pos_samples) {
    hipLaunchKernelGGL(k_skel_sample_fk, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, d_dev, d_clip, d_x_samples,
                       d_pos_samples, (long long)n_samples, (long long)rows);
    ACINO_LAUNCH_CHECK();
  }
  return skel_cov_read_status(d_clip, B, s, h_status);
}

int acino_skel_fte_sample(const acino_skel_fte_params* p, int n_clips, int camera_model, const acino_skel_op* h_ops,
                          const int32_t* h_active, const double* d_meas, const double* d_w, const double* d_cams,
                          const double* d_lo, const double* d_hi, const double* d_x, int64_t n_samples, const double* d_z,
                          double* d_x_samples, double* d_pos_samples, int32_t* h_status, void* d_ws, size_t ws_bytes,
                          void* stream) {
  return acino_skel_fte_sample_pinned(p, n_clips, camera_model, h_ops, h_active, d_meas, d_w, d_cams, d_lo, d_hi, d_x, n_samples,
                                      d_z, d_x_samples, d_pos_samples, h_status, d_ws, ws_bytes, stream, 0, nullptr);
}

}  // extern "C"
