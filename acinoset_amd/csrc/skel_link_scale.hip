// Link lengths of a skeleton from the pose fits of a clip (gfx950, fp64): acino_skel_link_scale.
//
// One log-scale theta_g per group of links, off_k -> exp(theta_g(k)) off_k.  A pose is root + sum_{k on path} M_k(x) off_k, linear
// in the offsets, so d pose_l / d theta_g at the current scales is the sum of M_k off_k over the ops of group g on l's path: the
// first three entries of S.opv, which spf_frame has filled, no division.  Without the smoothness prior the frames are
// independent given the scales and the joint Gauss-Newton matrix of all poses and scales is an arrow: every frame eliminates
// its own pose and leaves a K x K matrix and a K-vector to sum,
//   S_n = C - Y^T Y,  r_n = c - Y^T v,   Y = L^-1 B_F,  v = L^-1 g_F,  A_FF = L L^T  (lam = 0; pinned rows the identity's)
//   A = Jw^T Jw + kappa, B = Jw^T Js, C = Js^T Js, g = Jw^T u + kappa (x - m), c = Js^T u
// at the pose x and with the active set the pose fit returned.  A model on top of pose_fit_skel.hpp, as skel_pose_fit.hip is:
// the carved LDS (Spf), spf_frame, spf_jacobian<false>, spf_gram, SkelCore<PT>::factor / solve, pf_whiten.  That file's kernels
// are not touched.  What the fit shares with its pixel form (skel_link_scale_px.hip) is link_scale_dev.hpp's: the arguments, the
// layout around the measurement's regions, the group masks, the load of x, m and pinned, the scale directions, the Gram store,
// the elimination, the stores and the host path.  Here: the 3-D measurement - the whitening prologue, the cost, one Gram pass,
// g and c in slot order - and k_link_scale_total.
//
// One 64-lane wave per frame, PT = 16, 32, 48, 64, a grid-stride loop over the frames.  The K columns of Js follow the P columns
// of Jw in ONE array of P + K columns (leading dimension ldj), so that one Gram product of PT / 16 + 1 tile rows on the fp64
// matrix cores gives A, B and C together: result rows below P are A's (into S.M, lower triangle), rows P .. P + K - 1 hold B in
// the columns below P and C's lower triangle beyond (mirrored: symmetric bit for bit).  A column of zeros - a group no entering
// slot hangs on - gives exact zeros throughout.  The factor stays in registers (row i in lane i); Y and v come from its
// forward substitution, four columns at a time; Y^T Y and Y^T v are summed over the states in state order, one entry per lane.
// k_link_scale_total then adds the frames up in frame order, one entry per lane: no atomics, the same bits on every call.
#include "link_scale_dev.hpp"

namespace acino {

struct LinkScaleArgs {
  LscArgs c;
  const double *points, *cov;
  double inv_sigma_iso;
};

// lsc_layout_around the 3-D measurement's regions, with ent
struct Lsc3Layout {
  LscLayout l;
  int y, U, u;
};
__host__ __device__ inline Lsc3Layout lsc_layout(int P, int PT, int n_pose, int n_ops, int K) {
  Lsc3Layout L;
  L.l = lsc_layout_around(P, PT, n_pose, n_ops, K, true, [&](SpfTake& t) {
    L.y = t(3 * n_pose);
    L.U = t(6 * n_pose);
    L.u = t(3 * n_pose);
  });
  return L;
}

// F(S.x) of the poses S.pos: the whitened residuals into S.u, the sum in the order of the pose fit (the same value in every lane)
__device__ __forceinline__ double lsc_cost(const Spf& S, double kappa, int lane) {
  for (int l = lane; l < S.n_pose; l += 64) {
    const double r0 = S.pos[3 * l] - S.y[3 * l], r1 = S.pos[3 * l + 1] - S.y[3 * l + 1], r2 = S.pos[3 * l + 2] - S.y[3 * l + 2];
    const double* U = S.U + 6 * l;
    const double u0 = U[0] * r0, u1 = U[1] * r0 + U[2] * r1, u2 = U[3] * r0 + U[4] * r1 + U[5] * r2;
    S.u[3 * l] = u0;
    S.u[3 * l + 1] = u1;
    S.u[3 * l + 2] = u2;
    S.red[l] = 0.5 * (u0 * u0 + u1 * u1 + u2 * u2);
  }
  if (lane >= 3 && lane < S.P) {
    const double e = S.x[lane] - S.m[lane];
    S.red[S.n_pose + lane - 3] = 0.5 * kappa * e * e;
  }
  __syncthreads();
  double f = 0.0;
  for (int k = 0; k < S.n_pose + S.P - 3; ++k) f += S.red[k];
  __syncthreads();
  return f;
}

template <int PT>
__global__ void __launch_bounds__(64) k_skel_link_scale(LinkScaleArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const LscArgs& b = a.c;
  const SkelDev& D = *b.dev;
  const int lane = threadIdx.x;
  const int P = D.n_act, NPOSE = D.n_pose, NOPS = D.n_ops, R3 = 3 * NPOSE, K = b.K;
  const Lsc3Layout lay = lsc_layout(P, PT, NPOSE, NOPS, K);
  double* base = reinterpret_cast<double*>(smem_raw);
  Spf S = spf_carve(base, lay.l.s, [&](Spf& S) { S.y = base + lay.y, S.U = base + lay.U, S.u = base + lay.u; });
  S.ent = reinterpret_cast<int*>(base + lay.l.ent);
  const LscLds W = lsc_carve(base, lay.l);

  // ---- once per workgroup: the masks of pose_fit_skel.hpp, the ops of every group, the padding rows of Jw and Js
  spf_masks(S, D, P, NPOSE, NOPS, lane);
  lsc_group_masks(W.gm, b.grp, NOPS, lane);
  for (int e = lane; e < (P + K) * (4 * S.ks - R3); e += 64)
    S.Jw[(e / (4 * S.ks - R3)) * S.ldj + R3 + e % (4 * S.ks - R3)] = 0.0;

  for (int64_t n = blockIdx.x; n < b.n_frames; n += gridDim.x) {
    __syncthreads();                              // the previous frame is done with S (and the tables are complete)
    const int st_in = b.status[n];
    bool live = st_in < 2;
    double F = 0.0;
    if (live) {
      // ---- the slots that enter and their whitening factors: the prologue of k_skel_pose_fit
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int l = lane + 64 * h;
        if (l < NPOSE) {
          double y[3], U[6];
          const bool enter =
              pf_whiten(a.points + (n * NPOSE + l) * 3, a.cov ? a.cov + (n * NPOSE + l) * 9 : nullptr, a.inv_sigma_iso, y, U);
#pragma unroll
          for (int k = 0; k < 3; ++k) S.y[3 * l + k] = enter ? y[k] : 0.0;
#pragma unroll
          for (int k = 0; k < 6; ++k) S.U[6 * l + k] = U[k];
          S.ent[l] = enter ? 1 : 0;
        }
      }
      const unsigned long long fixmask = lsc_load_frame(S, b, n, lane);
      __syncthreads();

      // ---- FK, residuals and F at x; Jw, Js; A, B, C in one Gram product; g and c
      spf_frame(S, D, S.x, lane);
      F = lsc_cost(S, b.kappa, lane);
      spf_jacobian<false>(S, lane);
      lsc_scale_jacobian<false>(S, W.gm, K, 0, 0, lane);
      spf_gram<PT + 16>(S.Jw, S.ldj, S.ks, P + K, lane, lsc_gram_store<PT>(S, K, W));
      __syncthreads();
      if (lane >= 3 && lane < P) S.M[lane * (PT + 1) + lane] += b.kappa;
      // column t = lane, lane + 64 of [Jw Js] (P + K may exceed 64) against u over the entering slots, in slot order
      for (int t = lane; t < P + K; t += 64) {
        double sum = 0.0;
        const double* col = S.Jw + t * S.ldj;
        for (int l = 0; l < NPOSE; ++l)
          if (S.ent[l]) sum += col[3 * l] * S.u[3 * l] + col[3 * l + 1] * S.u[3 * l + 1] + col[3 * l + 2] * S.u[3 * l + 2];
        if (t < P) {
          if (t >= 3) sum += b.kappa * (S.x[t] - S.m[t]);
          S.g[t] = sum;
        } else {
          W.cv[t - P] = sum;
        }
      }
      __syncthreads();

      // ---- the pose eliminated: S_n, r_n, sens_n
      live = lsc_eliminate<PT>(S, D, fixmask, F, K, W.Bm, W.Cm, W.cv, b.out.sens ? b.out.sens + n * P * K : nullptr, lane);
    }
    lsc_store(b.out, n, P, K, live, st_in, F, W.Cm, W.cv, lane);
  }
}

// the frames added up in frame order, one entry of [S | r | F | used] per lane
__global__ void __launch_bounds__(320) k_link_scale_total(const double* __restrict__ S, const double* __restrict__ r,
                                                          const double* __restrict__ F, const uint8_t* __restrict__ used,
                                                          int64_t n_frames, int K, double* __restrict__ total) {
  const int t = threadIdx.x, KK = K * K;
  if (t >= KK + K + 2) return;
  double sum = 0.0;
  for (int64_t n = 0; n < n_frames; ++n)
    sum += t < KK ? S[n * KK + t] : (t < KK + K ? r[n * K + t - KK] : (t == KK + K ? F[n] : (double)used[n]));
  total[t] = sum;
}

int lsc_launch_total(const double* d_S, const double* d_r, const double* d_F, const uint8_t* d_used, int64_t n_frames, int K,
                     double* d_total, hipStream_t s) {
  hipLaunchKernelGGL(k_link_scale_total, dim3(1), dim3(320), 0, s, d_S, d_r, d_F, d_used, n_frames, K, d_total);
  ACINO_LAUNCH_CHECK();
  return ACINO_OK;
}

}  // namespace acino

using namespace acino;

extern "C" {

size_t acino_skel_link_scale_workspace_bytes(const acino_skel_fte_params* p) { return spf_workspace_bytes(p); }

int acino_skel_link_scale(const acino_skel_fte_params* p, const acino_skel_op* h_ops, const int32_t* h_active,
                          const int32_t* h_group, int n_groups, double prior_sigma, double sigma_iso, const double* d_points,
                          const double* d_cov, const double* d_x, const double* d_m, const uint8_t* d_pinned,
                          const uint8_t* d_status, int64_t n_frames, double* d_S, double* d_r, double* d_F, uint8_t* d_used,
                          uint8_t* d_frame_status, double* d_sens, double* d_total, void* d_ws, size_t ws_bytes, void* stream) {
  SkelDev h;
  auto check_fit = [&]() -> int {
    ACINO_REQUIRE(n_frames >= 0, "n_frames");
    ACINO_REQUIRE(n_groups >= 1 && n_groups <= LSC_MAXK, "n_groups must be 1..16");
    ACINO_REQUIRE(prior_sigma > 0 && prior_sigma < INFINITY, "prior_sigma must be > 0");
    ACINO_REQUIRE(sigma_iso > 0 && sigma_iso < INFINITY, "sigma_iso must be > 0");
    return lsc_check_groups(p, h_group, n_groups);
  };
  if (int rc = spf_program(p, h_ops, h_active, h, check_fit)) return rc;
  const size_t lds = sizeof(double) * (size_t)lsc_layout(h.n_act, h.PT, h.n_pose, h.n_ops, n_groups).l.total;
  ACINO_REQUIRE(lds <= SPF_LDS_MAX, "n_active x n_pose does not fit the pose fit's 160 KB of LDS");
  if (n_frames == 0) return ACINO_OK;
  ACINO_REQUIRE(d_points && d_x && d_m && d_pinned && d_status && d_S && d_r && d_F && d_used && d_frame_status && d_ws,
                "null buffer (d_points, d_x, d_m, d_pinned, d_status, d_S, d_r, d_F, d_used, d_frame_status, d_ws)");
  hipStream_t s = (hipStream_t)stream;
  LinkScaleArgs a;
  if (int rc = spf_upload(h, p, d_ws, ws_bytes, "acino_skel_link_scale_workspace_bytes", s, a.c.dev)) return rc;
  lsc_fill_args(a.c, h, h_group, n_groups, prior_sigma, d_x, d_m, d_pinned, d_status, n_frames, d_S, d_r, d_F, d_used,
                d_frame_status, d_sens);
  a.points = d_points, a.cov = d_cov, a.inv_sigma_iso = 1.0 / sigma_iso;
  return lsc_finish(h.PT, a.c, d_total, s, [&](auto pt) -> int {
    static PerDeviceOnce attr;                    // (per PT: one per instantiation of this body)
    return spf_launch(k_skel_link_scale<decltype(pt)::value>, attr, n_frames, lds, s, a);
  });
}

}  // extern "C"
