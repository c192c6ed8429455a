// The reduced system of a JOINT fit of a generic-skeleton FTE trajectory and the log-scales theta of its links (gfx950, fp64;
// acinoset_hip.h: acino_skel_fte_link_fit_system).  With A the matrix of skel_cov.hip, G the cross term of skel_links.hip and
//   C = sum w^2 J_theta^T J_theta,   c = dF/dtheta = sum w sign(e) J_theta,   g_x = the solver's gradient of F in the states
// (J_theta = J_pi D_l, the kept rows and weights those of the assembly and of k_skel_links_rhs), the joint quadratic model at
// (x, theta = 0) has the information [[A, G], [G^T, C]] and the gradient (g_x, c).  Eliminating the trajectory leaves
//   S = C - G^T A^-1 G = C - Y^T Y,   r = c - G^T A^-1 g_x = c - Y^T y,      Y = L^-1 G,  y = L^-1 g_x,  A = L L^T
// per clip; clips that share theta add their S and r (the caller's sum).  The right-hand side carries K + 1 columns, [-G | -g_x]:
// the solved columns are the link sensitivity -A^-1 G (the bits of acino_skel_fte_link_sensitivity: a column's solve reads
// that column alone) and the Fisher-scoring step -A^-1 g_x of the trajectory.
//   k_skel_assemble<.., double>, k_skel_cov_build   skel_cov.hip's (skel_cov_launch_build): band, pin mask, opv, and the solver's
//                           own g and per-frame cost at x, which this entry reads from the workspace
//   k_skel_link_fit_rhs<PINHOLE>   one workgroup per frame: k_skel_links_rhs's stages (skel_sens_frame, D_l by skel_link_direct,
//                           Mw_l in camera order, V_l = Mw_l D_l) with D_l kept beside V_l and, in a camera loop of its
//                           own on the workgroup's upper half (the Mw_l loop stays k_skel_links_rhs's: see there),
//                           gl_l = sum_c w (sign(eu) ju + sign(ev) jv), e = w (uv - meas): the assembly's gu = w sign(eu).  Then
//                           -G_n as columns 0..K-1 (the statements of skel_sens_rhs_out, in a buffer of K + 1 columns) and
//                           -g_x,n as column K, rows of pinned variables 0;  C_n[g, h] = sum_l D_l[:, g] . V_l[:, h] in slot order on
//                           one triangle, mirrored;  c_n[g] = sum_l gl_l . D_l[:, g] in slot order.  No atomics.
//                           LDS: skel_links_rhs_doubles + n_pose 3 (K + 1) doubles, 163.7 KB at the limits.
//   k_skel_factor<PT>, k_skel_fwdsub<PT>, k_skel_sample_back<PT, false>   skel_sens_run's, on K + 1 <= 17 columns
//   k_skel_link_fit_reduce  one workgroup of four waves per clip.  The Gram products Y^T [Y | y] over the depth N n_act are
//                           16 x 16 tiles of v_mfma_f64_16x16x4f64: lane (li, lk) loads Y[k][li] once and feeds it as BOTH
//                           operands (tile 1, Y^T Y) and beside y[k] (tile 2, every column Y^T y).  The depth, frame-major and
//                           padded with zeros to a multiple of 16, is cut into four contiguous runs, one per wave; the four
//                           partial tiles meet in LDS and are added in wave order.  Thread (g <= h) adds C_n over the frames in
//                           frame order, subtracts and writes both (g, h) and (h, g); c_n and the cost likewise.  The order
//                           depends on N, n_act and K alone.  With sens / newton it also transposes the solved columns out.
// A group on no weighted slot's path has D_l[:, g] = 0 on every weighted slot and V_l = gl_l = 0 on the others: exact zeros in C_n,
// c_n, its column of G, of Y and so of S and r.  No workgroup waits for another; vector stores only; a clip's bits do not depend on
// what else shares the call.
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "skel_sens_dev.hpp"

namespace acino {

constexpr int SKLF_COLS = SKL_MAXK + 1;      // [-G | -g_x]

constexpr size_t skel_link_fit_rhs_doubles(size_t n_ops, size_t n_pose, size_t P, size_t K) {
  return n_ops * 12 + n_pose * 3 + n_pose * 3 * P + 2 * n_pose * 3 * K + n_pose * 9 + n_pose * 3;
}
static_assert(sizeof(double) * skel_link_fit_rhs_doubles(ACINO_SKEL_MAX_OPS, ACINO_SKEL_MAX_OPS + 1, SK_MAXP, SKL_MAXK) <= 160 * 1024,
              "LDS of k_skel_link_fit_rhs at the limits");

// rhs: [n_clips][K + 1][N][n_act]; Cn: [NT][K][K]; cn: [NT][K]; g: the solver's gradient [NT][n_act]
template <bool PINHOLE>
__global__ void __launch_bounds__(256)
k_skel_link_fit_rhs(const SkelDev* __restrict__ dev, const SkelLinkGroups grp, const double* __restrict__ x,
                    const double* __restrict__ meas, const double* __restrict__ wgt, const double* __restrict__ opv_all,
                    const unsigned char* __restrict__ fxm, const double* __restrict__ g, double* __restrict__ rhs,
                    double* __restrict__ Cn, double* __restrict__ cn) {
  extern __shared__ __attribute__((aligned(16))) double sklf_smem[];
  const SkelDev& D = *dev;
  const int tid = threadIdx.x, n = blockIdx.x;
  const int P = D.n_act, C = D.n_cams, NPOSE = D.n_pose, NOPS = D.n_ops, K = grp.K;
  double* opv = sklf_smem;                                   // [n_ops][4][3]
  double* pos = opv + NOPS * 12;                             // [n_pose][3]
  double* G = pos + NPOSE * 3;                               // [(l * 3 + i) * P + p]
  double* V = G + (size_t)NPOSE * 3 * P;                     // [(l * 3 + i) * K + g]: Mw_l D_l
  double* Dl = V + (size_t)NPOSE * 3 * K;                    // [(l * 3 + i) * K + g]: D_l
  double* Mw = Dl + (size_t)NPOSE * 3 * K;                   // [l * 9 + i * 3 + j]
  double* gl = Mw + (size_t)NPOSE * 9;                       // [l * 3 + i]: d F_n / d pos_l
  skel_sens_frame(D, n, x, opv_all, opv, pos, G);
  for (int e = tid; e < NPOSE * 3 * K; e += 256) {
    const int li = e / K, gg = e - li * K;
    Dl[e] = skel_link_direct(D, grp, opv, li / 3, li % 3, gg);
  }
  __syncthreads();
  for (int l = tid; l < NPOSE; l += 256) {                   // Mw_l: the cameras in their order (k_skel_links_rhs's loop, as it stands)
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
  // gl_l = sum_c w (sign(eu) ju + sign(ev) jv), on the upper half of the workgroup.  A loop of its own: with the pixel in use in the
  // loop above, the pinhole projection's Jacobian compiles to other FMA pairings and -G loses the bits of k_skel_links_rhs.
  for (int l = tid - 128; l >= 0 && l < NPOSE; l += 128) {
    const double px = pos[l * 3], py = pos[l * 3 + 1], pz = pos[l * 3 + 2];
    double gs[3] = {0, 0, 0};
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
      double uv[2], jc[2][3];
      project_jac(cam, xc, yc, zc, uv, jc);
      const double eu = w * (uv[0] - um), ev = w * (uv[1] - vm);
      const double gu = w * (eu > 0 ? 1.0 : (eu < 0 ? -1.0 : 0.0)), gv = w * (ev > 0 ? 1.0 : (ev < 0 ? -1.0 : 0.0));
#pragma unroll
      for (int j = 0; j < 3; ++j)
        gs[j] += gu * (jc[0][0] * Rc[j] + jc[0][1] * Rc[3 + j] + jc[0][2] * Rc[6 + j]) +
                 gv * (jc[1][0] * Rc[j] + jc[1][1] * Rc[3 + j] + jc[1][2] * Rc[6 + j]);
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) gl[l * 3 + i] = gs[i];
  }
  __syncthreads();
  for (int e = tid; e < NPOSE * K; e += 256) {               // V_l,g = Mw_l D_l[:, g]: a thread owns its (l, g)
    const int l = e / K, gg = e - l * K;
    const double d0 = Dl[(l * 3) * K + gg], d1 = Dl[(l * 3 + 1) * K + gg], d2 = Dl[(l * 3 + 2) * K + gg];
    const double* M = Mw + l * 9;
    V[(l * 3) * K + gg] = M[0] * d0 + M[1] * d1 + M[2] * d2;
    V[(l * 3 + 1) * K + gg] = M[3] * d0 + M[4] * d1 + M[5] * d2;
    V[(l * 3 + 2) * K + gg] = M[6] * d0 + M[7] * d1 + M[8] * d2;
  }
  __syncthreads();
  // ---- [-G_n | -g_x,n] as K + 1 columns: skel_sens_rhs_out's statements for the first K, the solver's gradient for the last
  const int N = D.n_frames, b = n / N, nl = n - b * N;
  for (int task = tid; task < (K + 1) * P; task += 256) {
    const int col = task / P, p = task - col * P;
    double acc = 0.0;
    if (!fxm[(size_t)n * D.PT + p]) {
      if (col < K) {
        for (int l = 0; l < NPOSE; ++l) {
          acc += G[(l * 3) * P + p] * V[(l * 3) * K + col];
          acc += G[(l * 3 + 1) * P + p] * V[(l * 3 + 1) * K + col];
          acc += G[(l * 3 + 2) * P + p] * V[(l * 3 + 2) * K + col];
        }
      } else {
        acc = g[(size_t)n * P + p];
      }
      acc = -acc;
    }
    rhs[(((size_t)b * (K + 1) + col) * N + nl) * P + p] = acc;
  }
  // ---- the frame's partials of C and c, slots in their order
  for (int e = tid; e < K * K; e += 256) {
    const int gg = e / K, hh = e - gg * K;
    if (gg > hh) continue;
    double acc = 0.0;
    for (int li = 0; li < NPOSE * 3; ++li) acc += Dl[li * K + gg] * V[li * K + hh];
    Cn[(size_t)n * K * K + gg * K + hh] = acc;
    Cn[(size_t)n * K * K + hh * K + gg] = acc;
  }
  for (int gg = tid; gg < K; gg += 256) {
    double acc = 0.0;
    for (int li = 0; li < NPOSE * 3; ++li) acc += gl[li] * Dl[li * K + gg];
    cn[(size_t)n * K + gg] = acc;
  }
}

// y, sol: [n_clips][K + 1][N][n_act] (L^-1 and A^-1 of the right-hand side); Cn, cn, cost_part: the frames' partials;
// S, C: [n_clips][K][K]; r, c: [n_clips][K]; cost: [n_clips]; sens [n_clips][N][n_act][K] and newton [n_clips][N][n_act] may be NULL
__global__ void __launch_bounds__(256)
k_skel_link_fit_reduce(const SkelDev* __restrict__ dev, const SkelClip* __restrict__ clip, int K, const double* __restrict__ y,
                       const double* __restrict__ sol, const double* __restrict__ Cn, const double* __restrict__ cn,
                       const double* __restrict__ cost_part, double* __restrict__ S, double* __restrict__ r, double* __restrict__ C,
                       double* __restrict__ c, double* __restrict__ cost, double* __restrict__ sens, double* __restrict__ newton) {
  extern __shared__ __attribute__((aligned(16))) double sklf_smem[];
  double (*part)[2][256] = reinterpret_cast<double (*)[2][256]>(sklf_smem);      // [wave][tile][16 x 16]
  const SkelDev& D = *dev;
  const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, lk = lane >> 4;
  const int N = D.n_frames, P = D.n_act;
  const size_t M = (size_t)N * P;
  if (clip[b].status != 0) {                                 // a singular clip: NaN in everything
    const double nan = __builtin_nan("");
    for (int e = tid; e < K * K; e += 256) S[(size_t)b * K * K + e] = C[(size_t)b * K * K + e] = nan;
    for (int e = tid; e < K; e += 256) r[(size_t)b * K + e] = c[(size_t)b * K + e] = nan;
    if (tid == 0) cost[b] = nan;
    if (sens)
      for (size_t e = tid; e < M * K; e += 256) sens[(size_t)b * M * K + e] = nan;
    if (newton)
      for (size_t e = tid; e < M; e += 256) newton[(size_t)b * M + e] = nan;
    return;
  }
  const double* Yb = y + (size_t)b * (K + 1) * M;
  const size_t chunks = (M + 15) / 16, per_wave = (chunks + 3) / 4;
  const size_t k0 = (size_t)wave * per_wave * 16, k1 = (k0 + per_wave * 16 < chunks * 16) ? k0 + per_wave * 16 : chunks * 16;
  d4 a1 = {0, 0, 0, 0}, a2 = {0, 0, 0, 0};
  for (size_t k = k0; k < k1; k += 16) {
    double yv[4], gv[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const size_t kk = k + 4 * s + lk;
      yv[s] = (li < K && kk < M) ? Yb[(size_t)li * M + kk] : 0.0;
      gv[s] = kk < M ? Yb[(size_t)K * M + kk] : 0.0;
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      a1 = mfma(yv[s], yv[s], a1);
      a2 = mfma(yv[s], gv[s], a2);
    }
  }
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    part[wave][0][(lk + 4 * rr) * 16 + li] = a1[rr];
    part[wave][1][(lk + 4 * rr) * 16 + li] = a2[rr];
  }
  __syncthreads();
  const double* Cb = Cn + (size_t)b * N * K * K;
  const double* cb = cn + (size_t)b * N * K;
  for (int e = tid; e < K * K; e += 256) {
    const int gg = e / K, hh = e - gg * K;
    if (gg > hh) continue;
    const int t = gg * 16 + hh;
    const double yty = ((part[0][0][t] + part[1][0][t]) + part[2][0][t]) + part[3][0][t];
    double acc = 0.0;
    for (int n = 0; n < N; ++n) acc += Cb[(size_t)n * K * K + gg * K + hh];
    C[(size_t)b * K * K + gg * K + hh] = acc;
    C[(size_t)b * K * K + hh * K + gg] = acc;
    S[(size_t)b * K * K + gg * K + hh] = acc - yty;
    S[(size_t)b * K * K + hh * K + gg] = acc - yty;
  }
  for (int gg = tid; gg < K; gg += 256) {
    const int t = gg * 16;                                   // (every column of tile 2 holds Y^T y: column 0)
    const double ytg = ((part[0][1][t] + part[1][1][t]) + part[2][1][t]) + part[3][1][t];
    double acc = 0.0;
    for (int n = 0; n < N; ++n) acc += cb[(size_t)n * K + gg];
    c[(size_t)b * K + gg] = acc;
    r[(size_t)b * K + gg] = acc - ytg;
  }
  if (tid == 255) {
    double acc = 0.0;
    for (int n = 0; n < N; ++n) acc += cost_part[(size_t)b * N + n];
    cost[b] = acc;
  }
  const double* Xb = sol + (size_t)b * (K + 1) * M;
  if (sens)
    for (size_t e = tid; e < M * K; e += 256) {
      const size_t np = e / K, gg = e - np * K;
      sens[(size_t)b * M * K + e] = Xb[gg * M + np];
    }
  if (newton)
    for (size_t e = tid; e < M; e += 256) newton[(size_t)b * M + e] = Xb[(size_t)K * M + e];
}

// the frames' partials behind the two column buffers: C_n [NT][16][16] and c_n [NT][16] (sized for SKL_MAXK whatever K is)
static size_t sklf_partial_bytes(size_t NT) {
  return skel_align256(sizeof(double) * NT * SKL_MAXK * SKL_MAXK) + skel_align256(sizeof(double) * NT * SKL_MAXK);
}

}  // namespace acino

using namespace acino;

extern "C" {

size_t acino_skel_fte_link_fit_workspace_bytes(const acino_skel_fte_params* p, int n_clips, int pin_unobserved) {
  const size_t sens = skel_sens_workspace_bytes(p, n_clips, pin_unobserved, SKLF_COLS);
  return sens == 0 ? 0 : sens + sklf_partial_bytes((size_t)p->n_frames * n_clips);
}

int acino_skel_fte_link_fit_system(const acino_skel_fte_params* p, int n_clips, int camera_model, const acino_skel_op* h_ops,
                                   const int32_t* h_active, const double* d_meas, const double* d_w, const double* d_cams,
                                   const double* d_lo, const double* d_hi, const double* d_x, const int32_t* h_group, int n_groups,
                                   double* d_S, double* d_r, double* d_C, double* d_c, double* d_cost, double* d_sens,
                                   double* d_newton, int32_t* h_status, void* d_ws, size_t ws_bytes, void* stream, int pin_unobserved,
                                   uint8_t* d_unobserved) {
  int rc = skel_check_batch(p, n_clips, true, camera_model, h_ops && h_active && d_meas && d_w && d_cams && d_lo && d_hi && d_x && d_ws);
  if (rc) return rc;
  // (C, G and the Fisher weights w^2 are those of the L1 model; their counterparts under the redescending loss are not built)
  ACINO_REQUIRE(p->loss == ACINO_SKEL_LOSS_L1, "the link sensitivity is defined for the L1 loss only (loss = redescending)");
  ACINO_REQUIRE(pin_unobserved == 0 || pin_unobserved == 1, "pin_unobserved: 0 or 1");
  ACINO_REQUIRE(d_S && d_r && d_C && d_c && d_cost, "null buffer (d_S, d_r, d_C, d_c and d_cost are all required)");
  ACINO_REQUIRE(n_groups >= 1 && n_groups <= SKL_MAXK, "n_groups must be 1..16");
  ACINO_REQUIRE(h_group != nullptr || p->n_ops == 0, "null buffer (h_group)");
  SkelLinkGroups grp;
  memset(&grp, 0, sizeof(grp));
  grp.K = n_groups;
  for (int k = 0; k < p->n_ops; ++k) {
    ACINO_REQUIRE(h_group[k] >= -1 && h_group[k] < n_groups, "h_group: every op's group must be -1 (fixed) or 0..n_groups-1");
    if (h_group[k] >= 0) grp.gm[h_group[k]] |= 1ull << k;
  }
  const int B = n_clips, P = p->n_active, PT = (P + 15) / 16 * 16, K = n_groups;
  const size_t NT = (size_t)p->n_frames * B;
  // the layout skel_sens_run makes of the same arguments: the solver's g and per-frame cost, and where the column buffers end
  const SkelCovLayout lay = skel_cov_layout(NT, B, P, PT, p->n_ops, pin_unobserved == 1 || d_unobserved != nullptr);
  const size_t partials = lay.total + 2 * skel_sens_column_bytes(p, B, SKLF_COLS);
  if ((rc = skel_check_workspace(d_ws, ws_bytes, partials + sklf_partial_bytes(NT), "acino_skel_fte_link_fit_workspace_bytes",
                                 ACINO_ERR_WORKSPACE)))
    return rc;
  char* base = (char*)d_ws;
  const double* d_g = reinterpret_cast<const double*>(base + lay.g);
  const double* d_cost_part = reinterpret_cast<const double*>(base + lay.cost);
  double* d_Cn = reinterpret_cast<double*>(base + partials);
  double* d_cn = reinterpret_cast<double*>(base + partials + skel_align256(sizeof(double) * NT * SKL_MAXK * SKL_MAXK));
  static PerDeviceOnce attr;
  const void* const kernels[3] = {(const void*)k_skel_link_fit_rhs<false>, (const void*)k_skel_link_fit_rhs<true>,
                                  (const void*)k_skel_link_fit_reduce};
  return skel_sens_run(
      p, n_clips, camera_model, h_ops, h_active, d_meas, d_w, d_cams, d_lo, d_hi, d_x, K + 1, SKLF_COLS,
      "acino_skel_fte_link_fit_workspace_bytes", h_status, d_ws, ws_bytes, stream, pin_unobserved, d_unobserved, attr, kernels,
      [&](const SkelSens& a) {
        hipLaunchKernelGGL(skel_camera_kernel(camera_model, k_skel_link_fit_rhs<false>, k_skel_link_fit_rhs<true>), dim3((unsigned)a.NT),
                           dim3(256), sizeof(double) * skel_link_fit_rhs_doubles(p->n_ops, p->n_pose, P, K), a.s, a.d_dev, grp, d_x, d_meas,
                           d_w, a.d_opv, a.d_fxm, d_g, a.d_cols, d_Cn, d_cn);
      },
      [&](const SkelSens& a) {
        hipLaunchKernelGGL(k_skel_link_fit_reduce, dim3((unsigned)B), dim3(256), sizeof(double) * 4 * 2 * 256, a.s, a.d_dev, a.d_clip, K, a.d_y, a.d_cols, d_Cn, d_cn,
                           d_cost_part, d_S, d_r, d_C, d_c, d_cost, d_sens, d_newton);
      });
}

}  // extern "C"
