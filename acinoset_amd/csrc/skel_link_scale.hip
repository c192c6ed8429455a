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
// are not touched; the three pieces it keeps to itself (layout, cost, g) have their counterparts here, with the K columns.
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
  const SkelDev* dev;
  const double *points, *cov, *x, *m;
  const uint8_t *pinned, *status;
  int64_t n_frames;
  double *S, *r, *F, *sens;
  uint8_t *used, *frame_status;
  double kappa, inv_sigma_iso;
  int K;
  int8_t grp[ACINO_SKEL_MAX_OPS];  // per op: its group, -1: fixed
};

// offsets into the dynamic LDS, in units of 8 bytes: SpfLayout with Jw widened by the K columns of Js, the 3-D measurement's
// regions and B (K columns of PT; Y takes its place), C, c and the op mask of every group
struct LscLayout {
  SpfLayout s;
  int y, U, u, B, C, c, gm, ent, total;
};
__host__ __device__ inline LscLayout lsc_layout(int P, int PT, int n_pose, int n_ops, int K) {
  LscLayout L;
  SpfTake take;
  SpfLayout& s = L.s;
  s.P = P, s.n_pose = n_pose, s.n_ops = n_ops;
  s.ldj = 4 * (((3 * n_pose > P ? 3 * n_pose : P) + 3) / 4) + 1;
  s.ldm = PT + 1;
  s.Jw = take((P + K) * s.ldj);
  s.M = take(PT * s.ldm);
  L.y = take(3 * n_pose);
  L.U = take(6 * n_pose);
  L.u = take(3 * n_pose);
  L.B = take(LSC_MAXK * PT);
  L.C = take(LSC_MAXK * LSC_MAXK);
  L.c = take(LSC_MAXK);
  s.pos = take(3 * n_pose);
  s.opv = take(12 * (n_ops > 0 ? n_ops : 1));
  s.vec = take(6 * SK_MAXP);
  s.red = take(3 * SK_MAXP);
  s.pm = take(n_pose);
  s.opm = take(SK_MAXP);
  s.cm = take(2 * SK_MAXP);
  s.axs = take(SK_MAXP / 2);
  L.gm = take(LSC_MAXK);
  L.ent = take((n_pose + 1) / 2);
  L.total = take.o;
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

// Js = U * (sum of M_k off_k over the ops of group g on the slot's path) as the columns P .. P + K - 1 of S.Jw, zero where the
// slot does not enter or no op of the group lies on its path
__device__ __forceinline__ void lsc_scale_jacobian(const Spf& S, const unsigned long long* gm, int K, int lane) {
  lane = spf_here(lane);
  const int T = K * S.n_pose;
  for (int t = lane; t < T; t += 64) {
    const int g = t / S.n_pose, l = t - g * S.n_pose;
    double w0 = 0.0, w1 = 0.0, w2 = 0.0;
    unsigned long long mk = gm[g] & S.pm[l];
    if (mk && S.ent[l]) {
      double j0 = 0.0, j1 = 0.0, j2 = 0.0;
      while (mk) {
        const int k = __ffsll((long long)mk) - 1;
        mk &= mk - 1;
        const double* dv = S.opv + k * 12;
        j0 += dv[0];
        j1 += dv[1];
        j2 += dv[2];
      }
      const double* U = S.U + 6 * l;
      w0 = U[0] * j0;
      w1 = U[1] * j0 + U[2] * j1;
      w2 = U[3] * j0 + U[4] * j1 + U[5] * j2;
    }
    double* o = S.Jw + (S.P + g) * S.ldj + 3 * l;
    o[0] = w0;
    o[1] = w1;
    o[2] = w2;
  }
  __syncthreads();
}

template <int PT>
__global__ void __launch_bounds__(64) k_skel_link_scale(LinkScaleArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const SkelDev& D = *a.dev;
  const int lane = threadIdx.x;
  const int P = D.n_act, NPOSE = D.n_pose, NOPS = D.n_ops, R3 = 3 * NPOSE, K = a.K;
  const LscLayout lay = lsc_layout(P, PT, NPOSE, NOPS, K);
  double* base = reinterpret_cast<double*>(smem_raw);
  Spf S = spf_carve(base, lay.s, [&](Spf& S) { S.y = base + lay.y, S.U = base + lay.U, S.u = base + lay.u; });
  S.ent = reinterpret_cast<int*>(base + lay.ent);
  double *Bm = base + lay.B, *Cm = base + lay.C, *cv = base + lay.c;
  unsigned long long* gm = reinterpret_cast<unsigned long long*>(base + lay.gm);
  const double NaN = __builtin_nan("");

  // ---- once per workgroup: the masks of pose_fit_skel.hpp, the ops of every group, the padding rows of Jw and Js
  spf_masks(S, D, P, NPOSE, NOPS, lane);
  if (lane < LSC_MAXK) {
    unsigned long long om = 0;
    for (int k = 0; k < NOPS; ++k)
      if (a.grp[k] == lane) om |= 1ull << k;
    gm[lane] = om;
  }
  for (int e = lane; e < (P + K) * (4 * S.ks - R3); e += 64)
    S.Jw[(e / (4 * S.ks - R3)) * S.ldj + R3 + e % (4 * S.ks - R3)] = 0.0;

  for (int64_t n = blockIdx.x; n < a.n_frames; n += gridDim.x) {
    __syncthreads();                              // the previous frame is done with S (and the tables are complete)
    const int st_in = a.status[n];
    bool live = st_in < 2;
    unsigned long long fixmask = 0;
    double F = 0.0;
    if (live) {
      // ---- the slots that enter and their whitening factors: the prologue of k_skel_pose_fit
      unsigned long long em0 = 0, em1 = 0;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int l = lane + 64 * h;
        bool enter = false;
        if (l < NPOSE) {
          double y[3], U[6];
          enter = pf_whiten(a.points + (n * NPOSE + l) * 3, a.cov ? a.cov + (n * NPOSE + l) * 9 : nullptr, a.inv_sigma_iso, y, U);
#pragma unroll
          for (int k = 0; k < 3; ++k) S.y[3 * l + k] = enter ? y[k] : 0.0;
#pragma unroll
          for (int k = 0; k < 6; ++k) S.U[6 * l + k] = U[k];
          S.ent[l] = enter ? 1 : 0;
        }
        (h ? em1 : em0) = __ballot(enter);
      }
      bool pin = false;
      if (lane < P) {
        S.x[lane] = a.x[n * P + lane];
        S.m[lane] = lane >= 3 ? a.m[n * P + lane] : 0.0;
        pin = a.pinned[n * P + lane] != 0;
      }
      fixmask = __ballot(pin);
      __syncthreads();

      // ---- FK, residuals and F at x; Jw, Js; A, B, C in one Gram product; g and c
      spf_frame(S, D, S.x, lane);
      F = lsc_cost(S, a.kappa, lane);
      spf_jacobian<false>(S, lane);
      lsc_scale_jacobian(S, gm, K, lane);
      spf_gram<PT + 16>(S.Jw, S.ldj, S.ks, P + K, lane, [&](int row, int col, double v) {
        if (row < P) {
          S.M[row * (PT + 1) + col] = v;
        } else if (row < P + K) {
          const int g = row - P;
          if (col < P) {
            Bm[g * PT + col] = v;
          } else {
            Cm[g * LSC_MAXK + col - P] = v;
            Cm[(col - P) * LSC_MAXK + g] = v;
          }
        }
      });
      __syncthreads();
      if (lane >= 3 && lane < P) S.M[lane * (PT + 1) + lane] += a.kappa;
      if (lane < P + K) {                         // column ``lane`` of [Jw Js] against u over the entering slots, in slot order
        double sum = 0.0;
        const double* col = S.Jw + lane * S.ldj;
        for (int l = 0; l < NPOSE; ++l)
          if (S.ent[l]) sum += col[3 * l] * S.u[3 * l] + col[3 * l + 1] * S.u[3 * l + 1] + col[3 * l + 2] * S.u[3 * l + 2];
        if (lane < P) {
          if (lane >= 3) sum += a.kappa * (S.x[lane] - S.m[lane]);
          S.g[lane] = sum;
        } else {
          cv[lane - P] = sum;
        }
      }
      __syncthreads();

      // ---- A_FF = L L^T, the factor in registers
      SkelCore<PT> core{S, D, lane};
      double r[PT], dinv;
      bool ok = core.factor(fixmask, 0.0, lane, r, dinv) && m_finite(F);
      if (lane < P) ok = ok && m_finite(S.x[lane]);
      ok = __all(ok);
      if (ok) {
        const bool free_p = lane < P && !((fixmask >> lane) & 1);
        // the sensitivity first: it reads B, whose place Y takes below
        if (a.sens) {
#pragma unroll 1
          for (int g = 0; g < K; ++g) {
            const double b = free_p ? Bm[g * PT + lane] : 0.0;
            const double d = core.solve(r, dinv, -b, lane);
            if (lane < P) a.sens[(n * P + lane) * K + g] = free_p ? d : 0.0;
          }
        }
        // Y = L^-1 B_F and v = L^-1 g_F, four columns at a time (column K: g)
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
        // S = C - Y^T Y (lower triangle, mirrored), r = c - Y^T v: one entry per lane, summed over the states in state order
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
          if (tri) {                              // (entry (i, j) is read by this lane alone, (j, i) above the diagonal by none)
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
      }
      live = ok;
    }
    for (int t = lane; t < K * K; t += 64) a.S[n * K * K + t] = live ? Cm[(t / K) * LSC_MAXK + t % K] : 0.0;
    if (lane < K) a.r[n * K + lane] = live ? cv[lane] : 0.0;
    if (!live && a.sens)
      for (int t = lane; t < P * K; t += 64) a.sens[n * P * K + t] = NaN;
    if (lane == 0) {
      a.F[n] = live ? F : 0.0;
      a.used[n] = live ? 1 : 0;
      a.frame_status[n] = (uint8_t)(live || st_in >= 2 ? st_in : PF_NUMERIC);
    }
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
    ACINO_REQUIRE(h_group != nullptr, "null buffer (h_group)");
    for (int k = 0; k < p->n_ops; ++k)
      ACINO_REQUIRE(h_group[k] >= -1 && h_group[k] < n_groups, "h_group: every op's group must be -1 (fixed) or 0..n_groups-1");
    return ACINO_OK;
  };
  if (int rc = spf_program(p, h_ops, h_active, h, check_fit)) return rc;
  const size_t lds = sizeof(double) * (size_t)lsc_layout(h.n_act, h.PT, h.n_pose, h.n_ops, n_groups).total;
  ACINO_REQUIRE(lds <= SPF_LDS_MAX, "n_active x n_pose does not fit the pose fit's 160 KB of LDS");
  if (n_frames == 0) return ACINO_OK;
  ACINO_REQUIRE(d_points && d_x && d_m && d_pinned && d_status && d_S && d_r && d_F && d_used && d_frame_status && d_ws,
                "null buffer (d_points, d_x, d_m, d_pinned, d_status, d_S, d_r, d_F, d_used, d_frame_status, d_ws)");
  hipStream_t s = (hipStream_t)stream;
  LinkScaleArgs a;
  if (int rc = spf_upload(h, p, d_ws, ws_bytes, "acino_skel_link_scale_workspace_bytes", s, a.dev)) return rc;
  a.points = d_points, a.cov = d_cov, a.x = d_x, a.m = d_m, a.pinned = d_pinned, a.status = d_status, a.n_frames = n_frames;
  a.S = d_S, a.r = d_r, a.F = d_F, a.sens = d_sens, a.used = d_used, a.frame_status = d_frame_status;
  a.kappa = 1.0 / (prior_sigma * prior_sigma), a.inv_sigma_iso = 1.0 / sigma_iso, a.K = n_groups;
  for (int k = 0; k < ACINO_SKEL_MAX_OPS; ++k) a.grp[k] = (int8_t)(k < h.n_ops ? h_group[k] : -1);
  if (int rc = skel_dispatch_pt(h.PT, [&](auto pt) -> int {
        static PerDeviceOnce attr;                // (per PT: one per instantiation of this body)
        return spf_launch(k_skel_link_scale<decltype(pt)::value>, attr, n_frames, lds, s, a);
      }))
    return rc;
  if (d_total) return lsc_launch_total(d_S, d_r, d_F, d_used, n_frames, n_groups, d_total, s);
  return ACINO_OK;
}

}  // extern "C"
