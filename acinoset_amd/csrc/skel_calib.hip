// Sensitivity of a generic-skeleton FTE trajectory to the camera extrinsics (gfx950, fp64): S = -A^-1 G, and the "consider"
// covariance S Sigma S^T it gives for a covariance Sigma of the extrinsics (acinoset_hip.h:
// acino_skel_fte_calibration_sensitivity).  A, the bound pins, pin_unobserved and the status rules are those of skel_cov.hip;
// the factor A = L L^T is skel_sample.hip's k_skel_factor.  Camera parameters c = [dw_0, dt_0, ..., dw_C-1, dt_C-1],
// R_c <- exp([dw]x) R_c, t_c <- t_c + dt: the camera-frame point moves by dw x (R_c p) + dt, so with j the camera-frame
// Jacobian row of a pixel component J_c = [ (R_c p) x j | j ].  The weight of a kept row is the Fisher weight w^2 (the
// statement A makes), not the IRLS curvature.
//   k_skel_assemble<.., double>, k_skel_cov_build   skel_cov.hip's (skel_cov_launch_build): band, pin mask and the link
//                           operators opv of every frame, the unobserved states pinned when the caller asks
//   k_skel_calib_rhs<PINHOLE>  one workgroup per frame of every clip.  Poses from opv (the link program, in program order), the
//                           pose Jacobians G_l (skel_pose_jac_col, as k_skel_cov_pose) into LDS, per (camera, slot) the 3 x 6
//                           block J_pi^T w^2 J_c with the assembly's dropped rows (w = 0, non-finite measurement,
//                           |z_cam| < 1e-9), then -G_n[p, col] = -sum_l G_l[:, p] . block[:, col] in slot order, no atomics,
//                           as column `col` of the right-hand side [B][6C][N][n_act] (the layout of the sampler's z, columns
//                           in the place of samples); rows of pinned variables 0.
//                           LDS: (n_ops 12 + n_pose 3 + n_pose 3 n_act + n_cams n_pose 18) doubles, at most 123 KB.
//   k_skel_factor<PT>       skel_sample.hip's (skel_launch_factor)
//   k_skel_fwdsub<PT>       y = L^-1 b, grid (panels of SKS_PANEL = 64 columns, clips), SKS_W = 4 waves, 16 columns per wave:
//                           the mirror image of k_skel_sample_back.  It walks n = 0 .. N-1; per frame the four blocks L_nn,
//                           L_n,n-1 .. L_n,n-3 (band[n-j][j]) go to LDS once for all four waves, then every wave on its columns
//                               r = b_n - sum_{j=1..3} L_n,n-j y_n-j
//                               y_kb = U_kk^T (r_kb - sum_{t < kb} L(kb, t) y_t),      kb = 0 .. NTP-1
//                           every product an fp64 16 x 16 x 4 MFMA, the last three y blocks kept in accumulator registers as
//                           the B operands of the next frames.  The A operand of a product is now a tile of L read ALONG its
//                           rows (A[m][k] = L[m][k]), so the blocks go to LDS TRANSPOSED (entry (m, k) at SksShape::at(k, m))
//                           and the diagonal tiles U_kk as they are: every read is then the sampler's, lanes li along a row of
//                           LDS, with its rotation of the odd rows.  b is read and y written once each through the per-wave
//                           staging tile (b masked by the pin mask and the padding rows on the way in).
//                           LDS: SksShape<PT>::lds = 4 PT^2 + SKS_W * 16 * ST doubles: 50 / 99 KB at PT = 32 / 48 and the
//                           whole 160 KB at PT = 64.
//   k_skel_sample_back<PT, false>  skel_sample.hip's, without the "+ x" (skel_launch_back_columns): L^-T y
//   k_skel_calib_combine    one workgroup per frame: S_n [n_act][6C] out, T = S_n Sigma (Sigma is only PSD - a held camera has
//                           zero rows - and is multiplied, never factored), cov_x_cal = T S_n^T on one triangle and mirrored,
//                           then per pose slot (one wave each) G_l cov_x_cal G_l^T on its upper triangle, mirrored, and
//                           sqrt(trace); with pin_unobserved a slot that depends on an unobserved state gets +inf / NaN
//                           (k_skel_cov_pose's rule).  A singular clip: NaN in every output.
//                           LDS: (2 n_act 6C + n_act (n_act + 1) + n_ops 12 + 4 (6 n_act + 9)) doubles: 147 KB at n_act = 64
//                           with 16 cameras, so S_n and T both fit and Sigma is read from memory untiled.
// What the two kernels of this file share with those of skel_links.hip is in skel_sens_dev.hpp (the frame prologue and the tail
// of a right-hand-side kernel; the NaN fill, the states' share, a slot's G_l and the 3 x 3 tail of a combine), the host pipeline
// behind the entry's own checks in skel_factor.hpp (skel_sens_run).  The kept row of a (camera, slot) is written out in both
// right-hand-side kernels: moved into a shared function the compiler pairs its multiplies and adds into other FMAs, and
// the last bits of S change.
// n_cams <= ACINO_MAX_CAMS = 16 (96 columns).  No workgroup waits for another; vector stores only; the result of a clip is the
// same bits whatever else shares the call (every kernel's arithmetic on a clip reads that clip's data alone).
#include <cstddef>
#include <cstdint>

#include "skel_sens_dev.hpp"

namespace acino {

constexpr size_t skel_calib_rhs_doubles(size_t n_ops, size_t n_pose, size_t n_cams, size_t P) {
  return n_ops * 12 + n_pose * 3 + n_pose * 3 * P + n_cams * n_pose * 18;
}
constexpr size_t skel_calib_combine_doubles(size_t n_ops, size_t W, size_t P) {
  return 2 * P * W + P * (P + 1) + n_ops * 12 + 4 * (6 * P + 9);
}
// (the rhs kernel at the limits: n_cams n_pose <= SK_MAXROWS / 2 rows of (u, v), whatever the two factors are)
static_assert(sizeof(double) * (skel_calib_rhs_doubles(ACINO_SKEL_MAX_OPS, ACINO_SKEL_MAX_OPS + 1, 0, SK_MAXP) + (SK_MAXROWS / 2) * 18) <=
                      160 * 1024 &&
                  sizeof(double) * skel_calib_combine_doubles(ACINO_SKEL_MAX_OPS, 6 * ACINO_MAX_CAMS, SK_MAXP) <= 160 * 1024,
              "LDS of k_skel_calib_rhs / k_skel_calib_combine at the limits");

template <bool PINHOLE>
__global__ void __launch_bounds__(256)
k_skel_calib_rhs(const SkelDev* __restrict__ dev, const double* __restrict__ x, const double* __restrict__ meas,
                 const double* __restrict__ wgt, const double* __restrict__ opv_all, const unsigned char* __restrict__ fxm,
                 double* __restrict__ rhs) {
  extern __shared__ __attribute__((aligned(16))) double skc_smem[];
  const SkelDev& D = *dev;
  const int tid = threadIdx.x, n = blockIdx.x;
  const int P = D.n_act, C = D.n_cams, NPOSE = D.n_pose, NOPS = D.n_ops;
  double* opv = skc_smem;                                    // [n_ops][4][3]
  double* pos = opv + NOPS * 12;                             // [n_pose][3]
  double* G = pos + NPOSE * 3;                               // [(l * 3 + i) * P + p]
  double* Mb = G + (size_t)NPOSE * 3 * P;                    // [(c * n_pose + l) * 18 + i * 6 + j]
  skel_sens_frame(D, n, x, opv_all, opv, pos, G);
  __syncthreads();
  for (int task = tid; task < C * NPOSE; task += 256) {
    const int c = task / NPOSE, l = task - c * NPOSE;
    const double px = pos[l * 3], py = pos[l * 3 + 1], pz = pos[l * 3 + 2];
    const size_t e = ((size_t)n * C + c) * NPOSE + l;
    const double um = meas[2 * e], vm = meas[2 * e + 1];
    double w = wgt[e];
    if (!(m_finite(um) && m_finite(vm))) w = 0.0;
    const auto& cam = cam_rec<PINHOLE>(D, c);
    const double* Rc = cam.R;
    const double* tc = cam.t;
    const double q0 = Rc[0] * px + Rc[1] * py + Rc[2] * pz;              // R_c p
    const double q1 = Rc[3] * px + Rc[4] * py + Rc[5] * pz;
    const double q2 = Rc[6] * px + Rc[7] * py + Rc[8] * pz;
    const double xc = q0 + tc[0], yc = q1 + tc[1], zc = q2 + tc[2];
    if (fabs(zc) < 1e-9) w = 0.0;
    double* M = Mb + (size_t)task * 18;
    if (w == 0.0) {
#pragma unroll
      for (int k = 0; k < 18; ++k) M[k] = 0.0;
      continue;
    }
    double uv[2], jc[2][3];                                              // (the pixel itself is not used here)
    project_jac(cam, xc, yc, zc, uv, jc);
    double ju[3], jv[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      ju[j] = jc[0][0] * Rc[j] + jc[0][1] * Rc[3 + j] + jc[0][2] * Rc[6 + j];
      jv[j] = jc[1][0] * Rc[j] + jc[1][1] * Rc[3 + j] + jc[1][2] * Rc[6 + j];
    }
    const double cu[6] = {q1 * jc[0][2] - q2 * jc[0][1], q2 * jc[0][0] - q0 * jc[0][2], q0 * jc[0][1] - q1 * jc[0][0],
                          jc[0][0], jc[0][1], jc[0][2]};
    const double cv[6] = {q1 * jc[1][2] - q2 * jc[1][1], q2 * jc[1][0] - q0 * jc[1][2], q0 * jc[1][1] - q1 * jc[1][0],
                          jc[1][0], jc[1][1], jc[1][2]};
    const double w2 = w * w;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 6; ++j) M[i * 6 + j] = w2 * (ju[i] * cu[j] + jv[i] * cv[j]);
  }
  __syncthreads();
  skel_sens_rhs_out(D, n, 6 * C, G, fxm, rhs, [&](int col, int l, int i) {
    const int c = col / 6;
    return Mb[((size_t)c * NPOSE + l) * 18 + i * 6 + (col - 6 * c)];
  });
}

// y = L^-1 b on the factor of k_skel_factor<PT>: see the head of the file.  b_all, y_all: [n_clips][S][N][n_act]
template <int PT>
__global__ void __launch_bounds__(SKS_T)
k_skel_fwdsub(const SkelDev* __restrict__ dev, const SkelClip* __restrict__ clip, const double* __restrict__ band_all,
              const unsigned char* __restrict__ fxm_all, const double* __restrict__ b_all, double* __restrict__ y_all,
              long long S) {
  using Sh = SksShape<PT>;
  constexpr int NTP = PT / 16, BB = PT * PT;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, lk = lane >> 4;
  const int N = dev->n_frames, P = dev->n_act, b = blockIdx.y;
  if (clip[b].status != 0) return;                                         // singular clip (uniform): the combine writes NaN
  const long long s0 = (long long)blockIdx.x * SKS_PANEL + wave * 16;      // this wave's first column
  const size_t fr0 = (size_t)b * N;
  const double* const band = band_all + fr0 * 4 * BB;
  const unsigned char* const fxm = fxm_all + fr0 * PT;
  const size_t row0 = ((size_t)b * (size_t)S + (size_t)s0) * N * P;        // (b, s0, 0, 0) of b and y
  const size_t srow = (size_t)N * P;                                       // from one column to the next
  double* const Lb = reinterpret_cast<double*>(smem_raw);                  // [4][PT][PT], Sh::at, transposed
  double* const stage = Lb + 4 * BB + wave * 16 * Sh::ST;                   // [16][ST], Sh::st: this wave's
  const bool busy = s0 < S;
  d4 d[3][NTP];                                                            // y_n-1, y_n-2, y_n-3: tiles of 16 rows
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int t = 0; t < NTP; ++t) d[j][t] = d4{0, 0, 0, 0};
  for (int n = 0; n < N; ++n) {
    __syncthreads();                                                       // the previous frame's blocks have been read
    // 8 x 8 patches: a lane reads runs of 8 doubles and writes them down 8 rows of LDS
    for (int e = tid; e < 4 * BB; e += SKS_T) {
      const int j = e / BB, rem = e % BB, patch = rem >> 6, in = rem & 63;
      if (n - j < 0) break;                                                // (e grows with j: nothing further to load)
      const int m = (patch / (PT / 8)) * 8 + (in >> 3), k = (patch % (PT / 8)) * 8 + (in & 7);      // entry (m, k) of L_n,n-j
      const double v = band[((size_t)(n - j) * 4 + j) * BB + m * PT + k];
      const bool diag = j == 0 && (k >> 4) == (m >> 4);                     // U_kk stays as it is: its transpose is the operand
      Lb[j * BB + (diag ? Sh::at(m, k) : Sh::at(k, m))] = v;
    }
    __syncthreads();
    if (!busy) continue;
    // ---- b_n of the wave's 16 columns -> staging (rows along p), masked; then r in the accumulator layout
    for (int e = lane; e < 16 * PT; e += 64) {
      const int c = e / PT, p = e % PT;
      double v = 0.0;
      if (s0 + c < S && p < P && !fxm[(size_t)n * PT + p]) v = b_all[row0 + c * srow + (size_t)n * P + p];
      stage[Sh::st(c, p)] = v;
    }
    sk_wave_handover();
    d4 r[NTP];
#pragma unroll
    for (int kb = 0; kb < NTP; ++kb)
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) r[kb][rr] = stage[Sh::st(li, kb * 16 + lk + 4 * rr)];
    // ---- r -= L_n,n-j y_n-j
#pragma unroll
    for (int j = 1; j < 4; ++j) {
      if (n - j < 0) break;
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
    // ---- y_kb = U_kk^T (r_kb - sum_{t < kb} L(kb, t) y_t), first tile first
    d4 dn[NTP];
#pragma unroll
    for (int kb = 0; kb < NTP; ++kb) {
      d4 acc = r[kb];
#pragma unroll
      for (int t = 0; t < kb; ++t) {
        double av[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) av[s] = Lb[Sh::at(t * 16 + 4 * s + lk, kb * 16 + li)];
#pragma unroll
        for (int s = 0; s < 4; ++s) acc = mfma(-av[s], dn[t][s], acc);
      }
      double uv[4];
#pragma unroll
      for (int s = 0; s < 4; ++s) uv[s] = Lb[Sh::at(kb * 16 + 4 * s + lk, kb * 16 + li)];     // U_kk[k][li] = U_kk^T[li][k]
      d4 o = {0, 0, 0, 0};
#pragma unroll
      for (int s = 0; s < 4; ++s) o = mfma(uv[s], acc[s], o);
      dn[kb] = o;
    }
    // ---- y_n -> memory through the staging tile
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int kb = 0; kb < NTP; ++kb)
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) stage[Sh::st(li, kb * 16 + lk + 4 * rr)] = dn[kb][rr];
    sk_wave_handover();
    for (int e = lane; e < 16 * PT; e += 64) {
      const int c = e / PT, p = e % PT;
      if (s0 + c < S && p < P) y_all[row0 + c * srow + (size_t)n * P + p] = stage[Sh::st(c, p)];
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

// sol: [n_clips][W][N][n_act] (the columns of -A^-1 G); sigma: [W][W] or NULL; unobs: NULL, or the clips' masks [n_clips][P]
__global__ void __launch_bounds__(256)
k_skel_calib_combine(const SkelDev* __restrict__ dev, const SkelClip* __restrict__ clip, const double* __restrict__ sol,
                     const double* __restrict__ sigma, const double* __restrict__ opv_all, const unsigned char* __restrict__ unobs,
                     double* __restrict__ sens, double* __restrict__ cov_x, double* __restrict__ cov_pos,
                     double* __restrict__ std_pos) {
  extern __shared__ __attribute__((aligned(16))) double skc_smem[];
  const SkelDev& D = *dev;
  const int n = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int P = D.n_act, NPOSE = D.n_pose, NOPS = D.n_ops, W = 6 * D.n_cams, LDC = P + 1;
  const int b = n / D.n_frames;
  if (clip[b].status != 0) return skel_sens_nan(D, n, W, sens, nullptr, cov_x, cov_pos, std_pos);
  double* Sm = skc_smem;                                     // S_n [P][W]
  double* Tm = Sm + (size_t)P * W;                           // S_n Sigma [P][W]
  double* Cx = Tm + (size_t)P * W;                           // cov_x_cal [P][P + 1]
  double* opv = Cx + (size_t)P * LDC;                        // [n_ops][4][3]
  double* Gw = opv + NOPS * 12 + wave * (6 * P + 9);         // this wave's G_l [3][P], G_l cov_x_cal [3][P], out [9]
  double* Tw = Gw + 3 * P;
  double* out9 = Tw + 3 * P;
  skel_sens_states(D, n, W, W, sol, sigma, sigma != nullptr, Sm, Tm, Cx, sens, cov_x);
  if (!sigma || (!cov_pos && !std_pos)) return;
  for (int e = tid; e < NOPS * 12; e += 256) opv[e] = opv_all[(size_t)n * NOPS * 12 + e];
  __syncthreads();
  for (int l0 = 0; l0 < NPOSE; l0 += 4) {                   // a wave is one pose slot; no workgroup barrier inside
    const int l = l0 + wave;
    if (l >= NPOSE) break;
    const bool dep = skel_sens_pose_jac(D, opv, l, lane, unobs ? unobs + (size_t)b * P : nullptr, Gw);
    const bool undet = __any(dep ? 1 : 0) != 0;
    sk_wave_handover();
    if (lane < P) {
      double t0 = 0.0, t1 = 0.0, t2 = 0.0;
      for (int q = 0; q < P; ++q) {
        const double c = Cx[q * LDC + lane];
        t0 += Gw[q] * c;
        t1 += Gw[P + q] * c;
        t2 += Gw[2 * P + q] * c;
      }
      Tw[lane] = t0;
      Tw[P + lane] = t1;
      Tw[2 * P + lane] = t2;
    }
    skel_sens_pos_out(lane, P, Tw, Gw, out9, undet, cov_pos ? cov_pos + ((size_t)n * NPOSE + l) * 9 : nullptr,
                      std_pos ? std_pos + (size_t)n * NPOSE + l : nullptr);
  }
}

template <int PT>
static int skel_fwdsub_launch(int B, long long S, const SkelDev* d_dev, const SkelClip* d_clip, const double* d_band,
                              const unsigned char* d_fxm, const double* d_b, double* d_y, hipStream_t s) {
  static PerDeviceOnce attr;
  if (attr.first())
    ACINO_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_skel_fwdsub<PT>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                        160 * 1024));
  static_assert(SksShape<PT>::lds <= 160 * 1024, "LDS");
  const long long panels = (S + SKS_PANEL - 1) / SKS_PANEL;
  hipLaunchKernelGGL(k_skel_fwdsub<PT>, dim3((unsigned)panels, (unsigned)B), dim3(SKS_T), SksShape<PT>::lds, s, d_dev, d_clip, d_band,
                     d_fxm, d_b, d_y, S);
  ACINO_LAUNCH_CHECK();
  return ACINO_OK;
}

int skel_launch_fwdsub(int PT, int n_clips, long long n_cols, const SkelDev* d_dev, const SkelClip* d_clip, const double* d_band,
                       const unsigned char* d_fxm, const double* d_b, double* d_y, hipStream_t s) {
  return skel_dispatch_pt(PT, [&](auto pt) {
    return skel_fwdsub_launch<decltype(pt)::value>(n_clips, n_cols, d_dev, d_clip, d_band, d_fxm, d_b, d_y, s);
  });
}

}  // namespace acino

using namespace acino;

extern "C" {

size_t acino_skel_fte_calibration_workspace_bytes(const acino_skel_fte_params* p, int n_clips, int pin_unobserved) {
  const size_t cov = acino_skel_fte_covariance_pinned_workspace_bytes(p, n_clips, pin_unobserved);
  if (cov == 0 || p->n_cams < 1 || p->n_cams > ACINO_MAX_CAMS) return 0;
  return skel_sens_workspace_bytes(p, n_clips, pin_unobserved, 6 * p->n_cams);
}

int acino_skel_fte_calibration_sensitivity(const acino_skel_fte_params* p, int n_clips, int camera_model, const acino_skel_op* h_ops,
                                           const int32_t* h_active, const double* d_meas, const double* d_w, const double* d_cams,
                                           const double* d_lo, const double* d_hi, const double* d_x, const double* d_cov_cams,
                                           double* d_sens, double* d_cov_x_cal, double* d_cov_pos_cal, double* d_std_pos_cal,
                                           int32_t* h_status, void* d_ws, size_t ws_bytes, void* stream, int pin_unobserved,
                                           uint8_t* d_unobserved) {
  int rc = skel_check_batch(p, n_clips, true, camera_model, h_ops && h_active && d_meas && d_w && d_cams && d_lo && d_hi && d_x && d_ws);
  if (rc) return rc;
  // (the cross term G carries the Fisher weights w^2 of the L1 model; its counterpart under the redescending loss is not built)
  ACINO_REQUIRE(p->loss == ACINO_SKEL_LOSS_L1, "the calibration sensitivity is defined for the L1 loss only (loss = redescending)");
  ACINO_REQUIRE(pin_unobserved == 0 || pin_unobserved == 1, "pin_unobserved: 0 or 1");
  ACINO_REQUIRE(d_sens || d_cov_x_cal || d_cov_pos_cal || d_std_pos_cal,
                "at least one of d_sens, d_cov_x_cal, d_cov_pos_cal, d_std_pos_cal");
  ACINO_REQUIRE(d_cov_cams || !(d_cov_x_cal || d_cov_pos_cal || d_std_pos_cal), "a cov / std output needs d_cov_cams");
  ACINO_REQUIRE(p->n_cams <= ACINO_MAX_CAMS, "n_cams <= 16 (96 columns)");
  const int P = p->n_active, W = 6 * p->n_cams;
  static PerDeviceOnce attr;
  const void* const kernels[3] = {(const void*)k_skel_calib_rhs<false>, (const void*)k_skel_calib_rhs<true>, (const void*)k_skel_calib_combine};
  return skel_sens_run(
      p, n_clips, camera_model, h_ops, h_active, d_meas, d_w, d_cams, d_lo, d_hi, d_x, W, W, "acino_skel_fte_calibration_workspace_bytes",
      h_status, d_ws, ws_bytes, stream, pin_unobserved, d_unobserved, attr, kernels,
      [&](const SkelSens& a) {
        hipLaunchKernelGGL(skel_camera_kernel(camera_model, k_skel_calib_rhs<false>, k_skel_calib_rhs<true>), dim3((unsigned)a.NT), dim3(256),
                           sizeof(double) * skel_calib_rhs_doubles(p->n_ops, p->n_pose, p->n_cams, P), a.s, a.d_dev, d_x, d_meas, d_w,
                           a.d_opv, a.d_fxm, a.d_cols);
      },
      [&](const SkelSens& a) {
        hipLaunchKernelGGL(k_skel_calib_combine, dim3((unsigned)a.NT), dim3(256), sizeof(double) * skel_calib_combine_doubles(p->n_ops, W, P),
                           a.s, a.d_dev, a.d_clip, a.d_cols, d_cov_cams, a.d_opv, a.d_unobs, d_sens, d_cov_x_cal, d_cov_pos_cal,
                           d_std_pos_cal);
      });
}

}  // extern "C"
