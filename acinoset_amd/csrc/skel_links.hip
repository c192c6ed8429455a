// Sensitivity of a generic-skeleton FTE trajectory to the link lengths (gfx950, fp64): S = -A^-1 G, the poses' total derivative
// T_l = G_l S_n + D_l and the "consider" covariances S Sigma S^T, T_l Sigma T_l^T they give for a covariance Sigma of the links'
// log-scales (acinoset_hip.h: acino_skel_fte_link_sensitivity).  theta_g is the log-scale of group g of the link program's ops
// (build.link_groups; K <= SKL_MAXK = 16 groups, -1: an op whose offset stays fixed), theta = 0 the model's current offsets:
//   pos_l(x, theta) = root + sum_{k on l's path} exp(theta_g(k)) M_k(x) off_k
//   D_l[:, g] = d pos_l / d theta_g = sum_{k in pmask[l], g(k) = g} opv[k][0]      (the rotated link vectors, in program order)
//   G_n[p, g] = sum_c sum_l G_l[:, p] . (w^2 J_pi^T J_pi) D_l[:, g]               (Fisher weights w^2, the statement A makes)
// A, the bound pins, pin_unobserved and the status rules are those of skel_cov.hip and skel_calib.hip; the smoothness prior does
// not depend on theta.  A pose moves through the states AND directly: leaving D_l out of T_l is the obvious mistake.
//   k_skel_assemble<.., double>, k_skel_cov_build   skel_cov.hip's (skel_cov_launch_build): band, pin mask, opv of every frame
//   k_skel_links_rhs<PINHOLE>  one workgroup per frame of every clip, as k_skel_calib_rhs: poses from opv (program order), G_l
//                           (skel_pose_jac_col) and D_l into LDS, per slot Mw_l = sum_c w^2 (ju ju^T + jv jv^T) in camera order
//                           with the assembly's dropped rows (w = 0, non-finite measurement, |z_cam| < 1e-9), V_l,g = Mw_l D_l[:, g]
//                           in the place of D_l, then -G_n[p, g] = -sum_l G_l[:, p] . V_l,g in slot order, no atomics, as column g
//                           of the right-hand side [B][K][N][n_act]; rows of pinned variables 0.
//                           Known slack, left because the kernel is 0.17 ms of a 9 ms call (78 clips of 100 frames): the Mw_l
//                           stage is one thread per pose slot, so at most 65 of the 256 threads work in it (a thread per
//                           (camera, slot) with a sum in camera order would fill more), and skel_link_direct scans all n_ops
//                           for every (l, i, g) where per-group op lists would not.
//                           LDS: (n_ops 12 + n_pose 3 + n_pose 3 n_act + n_pose 3 K + n_pose 9) doubles, at most 134 KB.
//   k_skel_factor<PT>, k_skel_fwdsub<PT>, k_skel_sample_back<PT, false>   the solves of skel_calib.hip, through their host launchers
//                           (skel_launch_factor, skel_launch_fwdsub, skel_launch_back_columns); K <= 16 columns are one ragged
//                           panel with one wave busy.
//   k_skel_links_combine    one workgroup per frame: S_n [n_act][K] out, T = S_n Sigma (Sigma is only PSD - a held group has zero
//                           rows - and is multiplied, never factored), cov_x_links = T S_n^T on one triangle and mirrored; then per
//                           pose slot (one wave each) G_l and D_l, T_l = G_l S_n + D_l [3][K] out, T_l Sigma, T_l Sigma T_l^T on its
//                           upper triangle, mirrored, and sqrt(trace).  With pin_unobserved a slot that depends on an unobserved
//                           state gets +inf / NaN (k_skel_cov_pose's rule); so does a slot whose path holds an op of a group the
//                           caller marks `unknown`.  A singular clip: NaN in every output.
//                           The products are K <= 16 wide (3 x K per slot, n_act x K per frame): fractions of one 16 x 16 x 4 MFMA
//                           tile, so they are plain fp64 FMAs from LDS; the rows of S_n and T are padded to an odd length (K | 1)
//                           so that lanes walking down a column fall on different banks.
//                           LDS: (2 n_act (K | 1) + n_act (n_act + 1) + K^2 + n_ops 12 + 4 (3 n_act + 6 K + 9)) doubles, 67 KB at
//                           the limits.
// The blocks both kernels share with skel_calib.hip's are in skel_sens_dev.hpp, the host pipeline behind the entry's own checks is
// skel_factor.hpp's skel_sens_run; the kept row of a (camera, slot) stays written out here, as there (skel_calib.hip says why).
// No workgroup waits for another; vector stores only; the result of a clip is the same bits whatever else shares the call (every
// kernel's arithmetic on a clip reads that clip's data alone).
#include <cstddef>
#include <cstdint>

#include "skel_sens_dev.hpp"

namespace acino {

constexpr size_t skel_links_rhs_doubles(size_t n_ops, size_t n_pose, size_t P, size_t K) {
  return n_ops * 12 + n_pose * 3 + n_pose * 3 * P + n_pose * 3 * K + n_pose * 9;
}
constexpr size_t skel_links_combine_doubles(size_t n_ops, size_t P, size_t K) {
  return 2 * P * (K | 1) + P * (P + 1) + K * K + n_ops * 12 + 4 * (3 * P + 6 * K + 9);
}
static_assert(sizeof(double) * skel_links_rhs_doubles(ACINO_SKEL_MAX_OPS, ACINO_SKEL_MAX_OPS + 1, SK_MAXP, SKL_MAXK) <= 160 * 1024 &&
                  sizeof(double) * skel_links_combine_doubles(ACINO_SKEL_MAX_OPS, SK_MAXP, SKL_MAXK) <= 160 * 1024,
              "LDS of k_skel_links_rhs / k_skel_links_combine at the limits");

template <bool PINHOLE>
__global__ void __launch_bounds__(256)
k_skel_links_rhs(const SkelDev* __restrict__ dev, const SkelLinkGroups grp, const double* __restrict__ x, const double* __restrict__ meas,
                 const double* __restrict__ wgt, const double* __restrict__ opv_all, const unsigned char* __restrict__ fxm,
                 double* __restrict__ rhs) {
  extern __shared__ __attribute__((aligned(16))) double skl_smem[];
  const SkelDev& D = *dev;
  const int tid = threadIdx.x, n = blockIdx.x;
  const int P = D.n_act, C = D.n_cams, NPOSE = D.n_pose, NOPS = D.n_ops, K = grp.K;
  double* opv = skl_smem;                                    // [n_ops][4][3]
  double* pos = opv + NOPS * 12;                             // [n_pose][3]
  double* G = pos + NPOSE * 3;                               // [(l * 3 + i) * P + p]
  double* V = G + (size_t)NPOSE * 3 * P;                     // [(l * 3 + i) * K + g]: D_l, then Mw_l D_l
  double* Mw = V + (size_t)NPOSE * 3 * K;                    // [l * 9 + i * 3 + j]
  skel_sens_frame(D, n, x, opv_all, opv, pos, G);
  for (int e = tid; e < NPOSE * 3 * K; e += 256) {
    const int li = e / K, g = e - li * K;
    V[e] = skel_link_direct(D, grp, opv, li / 3, li % 3, g);
  }
  __syncthreads();
  for (int l = tid; l < NPOSE; l += 256) {                   // Mw_l: the cameras in their order
    const double px = pos[l * 3], py = pos[l * 3 + 1], pz = pos[l * 3 + 2];
    double m[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int c = 0; c < C; ++c) {
      const size_t e = ((size_t)n * C + c) * NPOSE + l;
      const double um = meas[2 * e], vm = meas[2 * e + 1];
      double w = wgt[e];
      if (!(m_finite(um) && m_finite(vm))) w = 0.0;
      const auto& cam = cam_rec<PINHOLE>(D, c);
      const double* Rc = cam.R;
      const double* tc = cam.t;
      const double xc = Rc[0] * px + Rc[1] * py + Rc[2] * pz + tc[0];
      const double yc = Rc[3] * px + Rc[4] * py + Rc[5] * pz + tc[1];
      const double zc = Rc[6] * px + Rc[7] * py + Rc[8] * pz + tc[2];
      if (fabs(zc) < 1e-9) w = 0.0;
      if (w == 0.0) continue;
      double uv[2], jc[2][3];                                              // (the pixel itself is not used here)
      project_jac(cam, xc, yc, zc, uv, jc);
      double ju[3], jv[3];
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        ju[j] = jc[0][0] * Rc[j] + jc[0][1] * Rc[3 + j] + jc[0][2] * Rc[6 + j];
        jv[j] = jc[1][0] * Rc[j] + jc[1][1] * Rc[3 + j] + jc[1][2] * Rc[6 + j];
      }
      const double w2 = w * w;
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) m[i * 3 + j] += w2 * (ju[i] * ju[j] + jv[i] * jv[j]);
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) Mw[l * 9 + k] = m[k];
  }
  __syncthreads();
  for (int e = tid; e < NPOSE * K; e += 256) {               // V_l,g = Mw_l D_l[:, g], in place: a thread owns its (l, g)
    const int l = e / K, g = e - l * K;
    const double d0 = V[(l * 3) * K + g], d1 = V[(l * 3 + 1) * K + g], d2 = V[(l * 3 + 2) * K + g];
    const double* M = Mw + l * 9;
    V[(l * 3) * K + g] = M[0] * d0 + M[1] * d1 + M[2] * d2;
    V[(l * 3 + 1) * K + g] = M[3] * d0 + M[4] * d1 + M[5] * d2;
    V[(l * 3 + 2) * K + g] = M[6] * d0 + M[7] * d1 + M[8] * d2;
  }
  __syncthreads();
  skel_sens_rhs_out(D, n, K, G, fxm, rhs, [&](int g, int l, int i) { return V[(l * 3 + i) * K + g]; });
}

// sol: [n_clips][K][N][n_act] (the columns of -A^-1 G); sigma: [K][K] or NULL; unknown: [K] or NULL; unobs: NULL, or the clips'
// masks [n_clips][P]
__global__ void __launch_bounds__(256)
k_skel_links_combine(const SkelDev* __restrict__ dev, const SkelClip* __restrict__ clip, const SkelLinkGroups grp,
                     const double* __restrict__ sol, const double* __restrict__ sigma, const unsigned char* __restrict__ unknown,
                     const double* __restrict__ opv_all, const unsigned char* __restrict__ unobs, double* __restrict__ sens,
                     double* __restrict__ dpos, double* __restrict__ cov_x, double* __restrict__ cov_pos, double* __restrict__ std_pos) {
  extern __shared__ __attribute__((aligned(16))) double skl_smem[];
  const SkelDev& D = *dev;
  const int n = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int P = D.n_act, NPOSE = D.n_pose, NOPS = D.n_ops, K = grp.K, LDK = K | 1, LDC = P + 1;
  const int b = n / D.n_frames;
  if (clip[b].status != 0) return skel_sens_nan(D, n, K, sens, dpos, cov_x, cov_pos, std_pos);
  double* Sm = skl_smem;                                     // S_n [P][LDK]
  double* Tm = Sm + (size_t)P * LDK;                         // S_n Sigma [P][LDK]
  double* Cx = Tm + (size_t)P * LDK;                         // cov_x_links [P][P + 1]
  double* Sg = Cx + (size_t)P * LDC;                         // Sigma [K][K]
  double* opv = Sg + K * K;                                  // [n_ops][4][3]
  double* Gw = opv + NOPS * 12 + wave * (3 * P + 6 * K + 9); // this wave's G_l [3][P], T_l [3][K], T_l Sigma [3][K], out [9]
  double* Tl = Gw + 3 * P;
  double* Ts = Tl + 3 * K;
  double* out9 = Ts + 3 * K;
  if (sigma)
    for (int e = tid; e < K * K; e += 256) Sg[e] = sigma[e];
  skel_sens_states(D, n, K, LDK, sol, Sg, sigma && cov_x, Sm, Tm, Cx, sens, cov_x);
  if (!dpos && !cov_pos && !std_pos) return;
  const bool want_cov = sigma && (cov_pos || std_pos);
  for (int e = tid; e < NOPS * 12; e += 256) opv[e] = opv_all[(size_t)n * NOPS * 12 + e];
  __syncthreads();
  for (int l0 = 0; l0 < NPOSE; l0 += 4) {                   // a wave is one pose slot; no workgroup barrier inside
    const int l = l0 + wave;
    if (l >= NPOSE) break;
    bool dep = skel_sens_pose_jac(D, opv, l, lane, unobs ? unobs + (size_t)b * P : nullptr, Gw);
    if (unknown && lane < K) dep = dep || (unknown[lane] && (D.pmask[l] & grp.gm[lane]) != 0ull);
    const bool undet = __any(dep ? 1 : 0) != 0;
    sk_wave_handover();
    if (lane < 3 * K) {                                      // T_l = G_l S_n + D_l: the states' share in state order, then the direct term
      const int i = lane / K, g = lane - i * K;
      double acc = 0.0;
      for (int p = 0; p < P; ++p) acc += Gw[i * P + p] * Sm[p * LDK + g];
      acc += skel_link_direct(D, grp, opv, l, i, g);
      Tl[lane] = acc;
      if (dpos) dpos[((size_t)n * NPOSE + l) * 3 * K + lane] = acc;
    }
    if (!want_cov) {
      __builtin_amdgcn_wave_barrier();
      continue;
    }
    sk_wave_handover();
    if (lane < 3 * K) {
      const int i = lane / K, j = lane - i * K;
      double acc = 0.0;
      for (int g = 0; g < K; ++g) acc += Tl[i * K + g] * Sg[g * K + j];
      Ts[lane] = acc;
    }
    skel_sens_pos_out(lane, K, Ts, Tl, out9, undet, cov_pos ? cov_pos + ((size_t)n * NPOSE + l) * 9 : nullptr,
                      std_pos ? std_pos + (size_t)n * NPOSE + l : nullptr);
  }
}

}  // namespace acino

using namespace acino;

extern "C" {

size_t acino_skel_fte_link_workspace_bytes(const acino_skel_fte_params* p, int n_clips, int pin_unobserved) {
  return skel_sens_workspace_bytes(p, n_clips, pin_unobserved, SKL_MAXK);
}

int acino_skel_fte_link_sensitivity(const acino_skel_fte_params* p, int n_clips, int camera_model, const acino_skel_op* h_ops,
                                    const int32_t* h_active, const double* d_meas, const double* d_w, const double* d_cams,
                                    const double* d_lo, const double* d_hi, const double* d_x, const int32_t* h_group, int n_groups,
                                    const double* d_cov_links, const uint8_t* d_unknown, double* d_sens, double* d_dpos,
                                    double* d_cov_x, double* d_cov_pos, double* d_std_pos, int32_t* h_status, void* d_ws,
                                    size_t ws_bytes, void* stream, int pin_unobserved, uint8_t* d_unobserved) {
  int rc = skel_check_batch(p, n_clips, true, camera_model, h_ops && h_active && d_meas && d_w && d_cams && d_lo && d_hi && d_x && d_ws);
  if (rc) return rc;
  // (the cross term G carries the Fisher weights w^2 of the L1 model; its counterpart under the redescending loss is not built)
  ACINO_REQUIRE(p->loss == ACINO_SKEL_LOSS_L1, "the link sensitivity is defined for the L1 loss only (loss = redescending)");
  ACINO_REQUIRE(pin_unobserved == 0 || pin_unobserved == 1, "pin_unobserved: 0 or 1");
  ACINO_REQUIRE(d_sens || d_dpos || d_cov_x || d_cov_pos || d_std_pos,
                "at least one of d_sens, d_dpos, d_cov_x, d_cov_pos, d_std_pos");
  ACINO_REQUIRE(d_cov_links || !(d_cov_x || d_cov_pos || d_std_pos), "a cov / std output needs d_cov_links");
  ACINO_REQUIRE(n_groups >= 1 && n_groups <= SKL_MAXK, "n_groups must be 1..16");
  ACINO_REQUIRE(h_group != nullptr || p->n_ops == 0, "null buffer (h_group)");
  SkelLinkGroups grp;
  memset(&grp, 0, sizeof(grp));
  grp.K = n_groups;
  for (int k = 0; k < p->n_ops; ++k) {
    ACINO_REQUIRE(h_group[k] >= -1 && h_group[k] < n_groups, "h_group: every op's group must be -1 (fixed) or 0..n_groups-1");
    if (h_group[k] >= 0) grp.gm[h_group[k]] |= 1ull << k;
  }
  const int P = p->n_active, K = n_groups;
  static PerDeviceOnce attr;
  const void* const kernels[3] = {(const void*)k_skel_links_rhs<false>, (const void*)k_skel_links_rhs<true>, (const void*)k_skel_links_combine};
  // (the column buffers are sized for SKL_MAXK groups whatever K is: the query does not know K)
  return skel_sens_run(
      p, n_clips, camera_model, h_ops, h_active, d_meas, d_w, d_cams, d_lo, d_hi, d_x, K, SKL_MAXK, "acino_skel_fte_link_workspace_bytes",
      h_status, d_ws, ws_bytes, stream, pin_unobserved, d_unobserved, attr, kernels,
      [&](const SkelSens& a) {
        hipLaunchKernelGGL(skel_camera_kernel(camera_model, k_skel_links_rhs<false>, k_skel_links_rhs<true>), dim3((unsigned)a.NT), dim3(256),
                           sizeof(double) * skel_links_rhs_doubles(p->n_ops, p->n_pose, P, K), a.s, a.d_dev, grp, d_x, d_meas, d_w, a.d_opv,
                           a.d_fxm, a.d_cols);
      },
      [&](const SkelSens& a) {
        hipLaunchKernelGGL(k_skel_links_combine, dim3((unsigned)a.NT), dim3(256), sizeof(double) * skel_links_combine_doubles(p->n_ops, P, K),
                           a.s, a.d_dev, a.d_clip, grp, a.d_cols, d_cov_links, d_unknown, a.d_opv, a.d_unobs, d_sens, d_dpos, d_cov_x,
                           d_cov_pos, d_std_pos);
      });
}

}  // extern "C"
