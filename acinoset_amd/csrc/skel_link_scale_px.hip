// Link lengths of a skeleton from the pixel pose fits of a clip (gfx950, fp64): acino_skel_link_scale_px, the form of
// skel_link_scale.hip whose measurement is the detections of every camera instead of triangulated points.
//
// One log-scale theta_g per group of links, off_k -> exp(theta_g(k)) off_k.  The objective is the sum over the frames of
// acino_skel_pose_fit_px's: the per-coordinate Cauchy loss on every valid detection, 1 / sigma_px^2, the ridge about m.  Per frame,
// at the pose x, the active set and the status that fit returned, with the IRLS weights w = 1 / (1 + r^2 / f^2) at x:
//   Jc  = sqrt(w) / sigma_px (J_pi R_c) G_l     P columns: the rows SkelPxFit::linearise builds
//   Jsc = sqrt(w) / sigma_px (J_pi R_c) d_gl    K columns: d_gl = sum of M_k off_k over the ops of group g on slot l's path
//   A = sum_c Jc^T Jc + kappa, B = sum_c Jc^T Jsc, C = sum_c Jsc^T Jsc, g = sum_c Jc^T u + kappa (x - m), c = sum_c Jsc^T u
//   S_n = C - Y^T Y,  r_n = c - Y^T v,   Y = L^-1 B_F,  v = L^-1 g_F,  A_FF = L L^T  (lam = 0; pinned rows the identity's)
// g and c carry w r, the exact gradient of the Cauchy cost; S_n is the IRLS Gauss-Newton curvature.  A model on top of
// pose_fit_skel.hpp and pose_fit_px_dev.hpp, as skel_pose_fit_px.hip is.  What the fit shares with its 3-D form is
// link_scale_dev.hpp's: the arguments, the layout around the measurement's regions, the group masks, the load of x, m and pinned,
// the scale directions, the Gram store, the elimination, the stores and the host path.  The kernels of skel_pose_fit.hip and
// skel_pose_fit_px.hip are not touched.
//
// One 64-lane wave per frame, PT = 16, 32, 48, 64, both camera models, a grid-stride loop over the frames, no atomics, nothing
// waits on another workgroup.
//   raw        spf_frame at x; spf_jacobian<true> leaves G as the P columns of S.Jw; the K raw directions d_gl follow as the
//              columns P .. P + K - 1 (exact zeros for a group with no op on the slot's path and for a slot no camera detects).
//   cameras    in the order and the groups of SkelPxFit::linearise: a group of cameras projects over the lanes and leaves
//              sqrt(w) / sigma_px (J_pi R_c) (2 x 3) and u = sqrt(w) r / sigma_px per (camera, slot); then camera by camera the
//              2 n_pose rows of [Jc Jsc] for all P + K columns, and the k-steps of ONE Gram product of PT / 16 + 1 tile rows
//              (spf_gram_passes<PT + 16>) carried across the cameras.  A camera without a valid detection is skipped.  The store
//              is lsc_gram_store: rows below P are A's, rows P .. P + K - 1 hold B below column P and C's lower triangle beyond,
//              mirrored.  The full 2 n_pose C x (P + K) Jacobian is never in LDS.
//   g, c       column t = lane, lane + 64 (P + K may exceed 64: P = 51 with K = 16) against u, in (camera, row) order.
//   tail       the cost by px_pair_cost / px_cost_finish (the value the pose fit reports), lsc_eliminate, lsc_store.
//
// Dynamic LDS from lsp_layout(P, PT, n_pose, n_ops, n_cams, K, camera model); Jc has the odd leading dimension of spx_layout.
#include "link_scale_dev.hpp"
#include "pose_fit_px_dev.hpp"

namespace acino {

struct LinkScalePxArgs {
  PxArgs px;
  LscArgs c;
};

// lsc_layout_around the pixel measurement's regions (as spx_layout; Jc has P + K columns), without ent
struct LspLayout {
  LscLayout l;
  int ldc, group;
  int Jc, cams, det, vm, jr, ur;
};
__host__ __device__ inline LspLayout lsp_layout(int P, int PT, int n_pose, int n_ops, int n_cams, int K, bool pinhole) {
  LspLayout L;
  L.ldc = 4 * ((2 * n_pose + 3) / 4) + 1;
  L.group = n_pose >= 64 ? 1 : 64 / n_pose;
  if (L.group > n_cams) L.group = n_cams;
  L.l = lsc_layout_around(P, PT, n_pose, n_ops, K, false, [&](SpfTake& t) {
    L.Jc = t((P + K) * L.ldc);
    L.cams = t(n_cams * (pinhole ? ACINO_PINHOLE_STRIDE : ACINO_CAM_STRIDE));
    L.det = t(n_cams * n_pose * 3);
    L.vm = t(2 * n_cams);
    L.jr = t(L.group * n_pose * 6);
    L.ur = t(L.group * 2 * n_pose);
  });
  return L;
}

template <int PT, bool PINHOLE>
__global__ void __launch_bounds__(64) k_skel_link_scale_px(LinkScalePxArgs a) {
  constexpr int STRIDE = PINHOLE ? ACINO_PINHOLE_STRIDE : ACINO_CAM_STRIDE;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const LscArgs& q = a.c;
  const SkelDev& D = *q.dev;
  const PxArgs& b = a.px;
  const int lane = threadIdx.x;
  const int P = D.n_act, NPOSE = D.n_pose, NOPS = D.n_ops, C = b.n_cams, K = q.K, R2 = 2 * NPOSE;
  const LspLayout lay = lsp_layout(P, PT, NPOSE, NOPS, C, K, PINHOLE);
  double* base = reinterpret_cast<double*>(smem_raw);
  const Spf S = spf_carve(base, lay.l.s, [](Spf&) {});
  double *Jc = base + lay.Jc, *det = base + lay.det, *jr = base + lay.jr, *ur = base + lay.ur;
  const LscLds W = lsc_carve(base, lay.l);
  unsigned long long* vm = reinterpret_cast<unsigned long long*>(base + lay.vm);
  double* const recs = base + lay.cams;
  const CamRec<PINHOLE>* cams = reinterpret_cast<const CamRec<PINHOLE>*>(recs);
  const int ldc = lay.ldc, ks2 = (R2 + 3) / 4, group = lay.group;
  auto valid = [&](int c, int l) -> bool { return (vm[2 * c + (l >> 6)] >> (l & 63)) & 1ull; };
  auto moves = [&](int p, int l) -> bool { return (S.cm[2 * p + (l >> 6)] >> (l & 63)) & 1ull; };

  // ---- once per workgroup: the masks of pose_fit_skel.hpp, the ops of every group, the camera records, Jc's padding rows
  spf_masks(S, D, P, NPOSE, NOPS, lane);
  lsc_group_masks(W.gm, q.grp, NOPS, lane);
  for (int e = lane; e < C * STRIDE; e += 64) recs[e] = b.cams[e];
  for (int e = lane; e < (P + K) * ldc; e += 64) Jc[e] = 0.0;
  const int frame_doubles = C * NPOSE * 3;

  for (int64_t n = blockIdx.x; n < q.n_frames; n += gridDim.x) {
    __syncthreads();                              // the previous frame is done with the LDS (and the tables are complete)
    const int st_in = q.status[n];
    bool live = st_in < 2;
    double F = 0.0;
    if (live) {
      const double* src = b.det + n * frame_doubles;
      for (int e = lane; e < frame_doubles; e += 64) det[e] = src[e];
      __syncthreads();
      // ---- the valid detections, camera by camera, 64 slots at a time; any0, any1: the slots some camera detects
      unsigned long long any0 = 0, any1 = 0;
      for (int c = 0; c < C; ++c)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int l = lane + 64 * h;
          bool ok = false;
          if (l < NPOSE) ok = px_valid(det + (c * NPOSE + l) * 3, b.thresh);
          const unsigned long long m = __ballot(ok);
          if (lane == 0) vm[2 * c + h] = m;
          (h ? any1 : any0) |= m;
        }
      const unsigned long long fixmask = lsc_load_frame(S, q, n, lane);
      __syncthreads();

      // ---- FK and F at x: SkelPxFit::eval
      spf_frame(S, D, S.x, lane);
      {
        const int pairs = NPOSE * C;
        double part = 0.0;
        bool behind = false;
        for (int t = lane; t < pairs; t += 64) {
          const int c = t / NPOSE, l = t - c * NPOSE;
          if (!valid(c, l)) continue;
          part += px_pair_cost(b, cams[c], S.pos + 3 * l, det, t, behind);
        }
        F = px_cost_finish(part, S.x, S.m, q.kappa, P, lane, b, behind);
      }

      // ---- the raw directions: G, then d_gl as the columns P .. P + K - 1 of S.Jw
      spf_jacobian<true>(S, lane);
      lsc_scale_jacobian<true>(S, W.gm, K, any0, any1, lane);

      // ---- A, B, C in one Gram product carried across the cameras; g and c beside it
      {
        const int here = spf_here(lane);
        double gs0 = 0.0, gs1 = 0.0;              // column here and column here + 64 of [Jc Jsc] against u
        int c = -1, c0 = -group;                  // the camera whose rows are in Jc; the first camera of the group in jr, ur
        const double* urc = ur;
        // the next camera with a valid detection into Jc (false: there is none), a barrier behind it
        auto advance = [&]() -> bool {
          for (++c; c < C; ++c) {
            if (c >= c0 + group) {
              // ---- a group of cameras over the lanes: pair (cc, l) projects slot l in camera c0 + cc
              c0 += group;
              for (int t = here; t < group * NPOSE; t += 64) {
                const int cc = t / NPOSE, l = t - cc * NPOSE, cg = c0 + cc;
                double q[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, u[2] = {0.0, 0.0};
                if (cg < C && valid(cg, l)) px_pair_rows(b, cams[cg], S.pos + 3 * l, det, NPOSE, cg, l, q, u);
#pragma unroll
                for (int k = 0; k < 6; ++k) jr[t * 6 + k] = q[k];
                ur[cc * R2 + 2 * l] = u[0];
                ur[cc * R2 + 2 * l + 1] = u[1];
              }
              __syncthreads();
            }
            if ((vm[2 * c] | vm[2 * c + 1]) == 0ull) continue;      // (the same in every lane)
            // ---- the camera's 2 n_pose rows of [Jc Jsc]: its 2 x 3 block times the column's 3-vector
            const double* jrc = jr + (c - c0) * NPOSE * 6;
            urc = ur + (c - c0) * R2;
            for (int t = here; t < (P + K) * NPOSE; t += 64) {
              const int p = t / NPOSE, l = t - p * NPOSE;
              double v0 = 0.0, v1 = 0.0;
              if ((p >= P || moves(p, l)) && valid(c, l)) {
                const double *w = S.Jw + p * S.ldj + 3 * l, *q = jrc + 6 * l;
                v0 = q[0] * w[0] + q[1] * w[1] + q[2] * w[2];
                v1 = q[3] * w[0] + q[4] * w[1] + q[5] * w[2];
              }
              Jc[p * ldc + 2 * l] = v0;
              Jc[p * ldc + 2 * l + 1] = v1;
            }
            __syncthreads();
            return true;
          }
          return false;
        };
        bool more = advance();
        spf_gram_passes<PT + 16>(Jc, ldc, more ? ks2 : 0, P + K, lane,
                                 [&]() -> bool {
                                   if (!more) return false;
                                   for (int t = here; t < P + K; t += 64) {
                                     const double* col = Jc + t * ldc;
                                     double sum = t < 64 ? gs0 : gs1;
                                     for (int e = 0; e < R2; ++e) sum += col[e] * urc[e];
                                     (t < 64 ? gs0 : gs1) = sum;
                                   }
                                   __syncthreads();  // (Jc is free for the next camera, jr and ur after the last of the group)
                                   more = advance();
                                   return more;
                                 },
                                 lsc_gram_store<PT>(S, K, W));
        for (int t = here; t < P + K; t += 64) {
          const double sum = t < 64 ? gs0 : gs1;
          if (t < P)
            S.g[t] = sum;
          else
            W.cv[t - P] = sum;
        }
        __syncthreads();
        if (here >= 3 && here < P) {
          S.M[here * (PT + 1) + here] += q.kappa;
          S.g[here] += q.kappa * (S.x[here] - S.m[here]);
        }
        __syncthreads();
      }

      // ---- the pose eliminated: S_n, r_n, sens_n
      live = lsc_eliminate<PT>(S, D, fixmask, F, K, W.Bm, W.Cm, W.cv, q.out.sens ? q.out.sens + n * P * K : nullptr, lane);
    }
    lsc_store(q.out, n, P, K, live, st_in, F, W.Cm, W.cv, lane);
  }
}

}  // namespace acino

using namespace acino;

extern "C" {

size_t acino_skel_link_scale_px_workspace_bytes(const acino_skel_fte_params* p) { return spf_workspace_bytes(p); }

int acino_skel_link_scale_px(const acino_pose_fit_px_params* prm, const acino_skel_fte_params* p, const acino_skel_op* h_ops,
                             const int32_t* h_active, const int32_t* h_group, int n_groups, const double* d_det, int64_t n_frames,
                             int n_cams, const double* d_cams, const double* d_x, const double* d_m, const uint8_t* d_pinned,
                             const uint8_t* d_status, double* d_S, double* d_r, double* d_F, uint8_t* d_used,
                             uint8_t* d_frame_status, double* d_sens, double* d_total, void* d_ws, size_t ws_bytes, void* stream) {
  ACINO_REQUIRE(prm != nullptr, "prm");
  acino_pose_fit_params fit;
  SkelDev h;
  auto check_fit = [&]() -> int {
    if (int rc = px_check_params(prm, n_frames, n_cams, p->n_pose, "min_detections must be 1..n_pose n_cams", fit)) return rc;
    ACINO_REQUIRE(n_groups >= 1 && n_groups <= LSC_MAXK, "n_groups must be 1..16");
    return lsc_check_groups(p, h_group, n_groups);
  };
  if (int rc = spf_program(p, h_ops, h_active, h, check_fit)) return rc;
  const bool pinhole = prm->camera_model == 1;
  const size_t lds = sizeof(double) * (size_t)lsp_layout(h.n_act, h.PT, h.n_pose, h.n_ops, n_cams, n_groups, pinhole).l.total;
  ACINO_REQUIRE(lds <= SPF_LDS_MAX, "n_active x n_pose x n_cams does not fit the pixel pose fit's 160 KB of LDS");
  if (n_frames == 0) return ACINO_OK;
  ACINO_REQUIRE(d_det && d_cams && d_x && d_m && d_pinned && d_status && d_S && d_r && d_F && d_used && d_frame_status && d_ws,
                "null buffer (d_det, d_cams, d_x, d_m, d_pinned, d_status, d_S, d_r, d_F, d_used, d_frame_status, d_ws)");
  hipStream_t s = (hipStream_t)stream;
  LinkScalePxArgs a;
  if (int rc = spf_upload(h, p, d_ws, ws_bytes, "acino_skel_link_scale_px_workspace_bytes", s, a.c.dev)) return rc;
  px_fill_args(a.px, prm, d_det, d_cams, n_cams, nullptr, nullptr);
  lsc_fill_args(a.c, h, h_group, n_groups, prm->prior_sigma, d_x, d_m, d_pinned, d_status, n_frames, d_S, d_r, d_F, d_used,
                d_frame_status, d_sens);
  return lsc_finish(h.PT, a.c, d_total, s, [&](auto pt) -> int {
    constexpr int T = decltype(pt)::value;
    static PerDeviceOnce attr_pinhole, attr_fisheye;          // (per PT: one pair per instantiation of this body)
    return pinhole ? spf_launch(k_skel_link_scale_px<T, true>, attr_pinhole, n_frames, lds, s, a)
                   : spf_launch(k_skel_link_scale_px<T, false>, attr_fisheye, n_frames, lds, s, a);
  });
}

}  // extern "C"
