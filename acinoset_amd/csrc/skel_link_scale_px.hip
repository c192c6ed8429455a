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
// pose_fit_skel.hpp and pose_fit_px_dev.hpp, as skel_pose_fit_px.hip is; the elimination, the stores and the summing launch are
// link_scale_dev.hpp's.  The kernels of skel_pose_fit.hip, skel_pose_fit_px.hip and skel_link_scale.hip are not touched.
//
// One 64-lane wave per frame, PT = 16, 32, 48, 64, both camera models, a grid-stride loop over the frames, no atomics, nothing
// waits on another workgroup.
//   raw        spf_frame at x; spf_jacobian<true> leaves G as the P columns of S.Jw; the K raw directions d_gl follow as the
//              columns P .. P + K - 1 (exact zeros for a group with no op on the slot's path and for a slot no camera detects).
//   cameras    in the order and the groups of SkelPxFit::linearise: a group of cameras projects over the lanes and leaves
//              sqrt(w) / sigma_px (J_pi R_c) (2 x 3) and u = sqrt(w) r / sigma_px per (camera, slot); then camera by camera the
//              2 n_pose rows of [Jc Jsc] for all P + K columns, and the k-steps of ONE Gram product of PT / 16 + 1 tile rows
//              (spf_gram_passes<PT + 16>) carried across the cameras.  A camera without a valid detection is skipped.  The store
//              splits the result as the 3-D kernel does: rows below P are A's, rows P .. P + K - 1 hold B below column P and C's
//              lower triangle beyond, mirrored.  The full 2 n_pose C x (P + K) Jacobian is never in LDS.
//   g, c       column t = lane, lane + 64 (P + K may exceed 64: P = 51 with K = 16) against u, in (camera, row) order.
//   tail       the cost by px_pair_cost / px_cost_finish (the value the pose fit reports), lsc_eliminate, lsc_store.
//
// Dynamic LDS from lsp_layout(P, PT, n_pose, n_ops, n_cams, K, camera model); Jc has the odd leading dimension of spx_layout.
#include "link_scale_dev.hpp"
#include "pose_fit_px_dev.hpp"

namespace acino {

struct LinkScalePxArgs {
  PxArgs px;
  const SkelDev* dev;
  const double *x, *m;
  const uint8_t *pinned, *status;
  int64_t n_frames;
  LscOut out;
  double kappa;
  int K;
  int8_t grp[ACINO_SKEL_MAX_OPS];  // per op: its group, -1: fixed
};

// offsets into the dynamic LDS, in units of 8 bytes: Jw widened by the K raw scale directions, the pixel measurement's regions
// (as spx_layout; Jc has P + K columns), B (K columns of PT; Y takes its place), C, c and the op mask of every group
struct LspLayout {
  SpfLayout s;
  int ldc, group;
  int Jc, cams, det, vm, jr, ur, B, C, c, gm, total;
};
__host__ __device__ inline LspLayout lsp_layout(int P, int PT, int n_pose, int n_ops, int n_cams, int K, bool pinhole) {
  LspLayout L;
  SpfTake take;
  SpfLayout& s = L.s;
  s.P = P, s.n_pose = n_pose, s.n_ops = n_ops;
  s.ldj = 4 * (((3 * n_pose > P ? 3 * n_pose : P) + 3) / 4) + 1;
  s.ldm = PT + 1;
  s.Jw = take((P + K) * s.ldj);
  s.M = take(PT * s.ldm);
  L.ldc = 4 * ((2 * n_pose + 3) / 4) + 1;
  L.group = n_pose >= 64 ? 1 : 64 / n_pose;
  if (L.group > n_cams) L.group = n_cams;
  L.Jc = take((P + K) * L.ldc);
  L.cams = take(n_cams * (pinhole ? ACINO_PINHOLE_STRIDE : ACINO_CAM_STRIDE));
  L.det = take(n_cams * n_pose * 3);
  L.vm = take(2 * n_cams);
  L.jr = take(L.group * n_pose * 6);
  L.ur = take(L.group * 2 * n_pose);
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
  L.total = take.o;
  return L;
}

template <int PT, bool PINHOLE>
__global__ void __launch_bounds__(64) k_skel_link_scale_px(LinkScalePxArgs a) {
  constexpr int STRIDE = PINHOLE ? ACINO_PINHOLE_STRIDE : ACINO_CAM_STRIDE;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const SkelDev& D = *a.dev;
  const PxArgs& b = a.px;
  const int lane = threadIdx.x;
  const int P = D.n_act, NPOSE = D.n_pose, NOPS = D.n_ops, C = b.n_cams, K = a.K, R2 = 2 * NPOSE;
  const LspLayout lay = lsp_layout(P, PT, NPOSE, NOPS, C, K, PINHOLE);
  double* base = reinterpret_cast<double*>(smem_raw);
  const Spf S = spf_carve(base, lay.s, [](Spf&) {});
  double *Jc = base + lay.Jc, *det = base + lay.det, *jr = base + lay.jr, *ur = base + lay.ur;
  double *Bm = base + lay.B, *Cm = base + lay.C, *cv = base + lay.c;
  unsigned long long* vm = reinterpret_cast<unsigned long long*>(base + lay.vm);
  unsigned long long* gm = reinterpret_cast<unsigned long long*>(base + lay.gm);
  double* const recs = base + lay.cams;
  const CamRec<PINHOLE>* cams = reinterpret_cast<const CamRec<PINHOLE>*>(recs);
  const int ldc = lay.ldc, ks2 = (R2 + 3) / 4, group = lay.group;
  auto valid = [&](int c, int l) -> bool { return (vm[2 * c + (l >> 6)] >> (l & 63)) & 1ull; };
  auto moves = [&](int p, int l) -> bool { return (S.cm[2 * p + (l >> 6)] >> (l & 63)) & 1ull; };

  // ---- once per workgroup: the masks of pose_fit_skel.hpp, the ops of every group, the camera records, Jc's padding rows
  spf_masks(S, D, P, NPOSE, NOPS, lane);
  if (lane < LSC_MAXK) {
    unsigned long long om = 0;
    for (int k = 0; k < NOPS; ++k)
      if (a.grp[k] == lane) om |= 1ull << k;
    gm[lane] = om;
  }
  for (int e = lane; e < C * STRIDE; e += 64) recs[e] = b.cams[e];
  for (int e = lane; e < (P + K) * ldc; e += 64) Jc[e] = 0.0;
  const int frame_doubles = C * NPOSE * 3;

  for (int64_t n = blockIdx.x; n < a.n_frames; n += gridDim.x) {
    __syncthreads();                              // the previous frame is done with the LDS (and the tables are complete)
    const int st_in = a.status[n];
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
      bool pin = false;
      if (lane < P) {
        S.x[lane] = a.x[n * P + lane];
        S.m[lane] = lane >= 3 ? a.m[n * P + lane] : 0.0;
        pin = a.pinned[n * P + lane] != 0;
      }
      const unsigned long long fixmask = __ballot(pin);
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
        F = px_cost_finish(part, S.x, S.m, a.kappa, P, lane, b, behind);
      }

      // ---- the raw directions: G, then d_gl as the columns P .. P + K - 1 of S.Jw
      spf_jacobian<true>(S, lane);
      {
        const int here = spf_here(lane);
        for (int t = here; t < K * NPOSE; t += 64) {
          const int g = t / NPOSE, l = t - g * NPOSE;
          double j0 = 0.0, j1 = 0.0, j2 = 0.0;
          unsigned long long mk = gm[g] & S.pm[l];
          if (!(((l < 64 ? any0 : any1) >> (l & 63)) & 1ull)) mk = 0;
          while (mk) {
            const int k = __ffsll((long long)mk) - 1;
            mk &= mk - 1;
            const double* dv = S.opv + k * 12;
            j0 += dv[0];
            j1 += dv[1];
            j2 += dv[2];
          }
          double* o = S.Jw + (P + g) * S.ldj + 3 * l;
          o[0] = j0;
          o[1] = j1;
          o[2] = j2;
        }
        __syncthreads();
      }

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
                                 [&](int row, int col, double v) {
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
        for (int t = here; t < P + K; t += 64) {
          const double sum = t < 64 ? gs0 : gs1;
          if (t < P)
            S.g[t] = sum;
          else
            cv[t - P] = sum;
        }
        __syncthreads();
        if (here >= 3 && here < P) {
          S.M[here * (PT + 1) + here] += a.kappa;
          S.g[here] += a.kappa * (S.x[here] - S.m[here]);
        }
        __syncthreads();
      }

      // ---- the pose eliminated: S_n, r_n, sens_n
      live = lsc_eliminate<PT>(S, D, fixmask, F, K, Bm, Cm, cv, a.out.sens ? a.out.sens + n * P * K : nullptr, lane);
    }
    lsc_store(a.out, n, P, K, live, st_in, F, Cm, cv, lane);
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
    ACINO_REQUIRE(h_group != nullptr, "null buffer (h_group)");
    for (int k = 0; k < p->n_ops; ++k)
      ACINO_REQUIRE(h_group[k] >= -1 && h_group[k] < n_groups, "h_group: every op's group must be -1 (fixed) or 0..n_groups-1");
    return ACINO_OK;
  };
  if (int rc = spf_program(p, h_ops, h_active, h, check_fit)) return rc;
  const bool pinhole = prm->camera_model == 1;
  const size_t lds = sizeof(double) * (size_t)lsp_layout(h.n_act, h.PT, h.n_pose, h.n_ops, n_cams, n_groups, pinhole).total;
  ACINO_REQUIRE(lds <= SPF_LDS_MAX, "n_active x n_pose x n_cams does not fit the pixel pose fit's 160 KB of LDS");
  if (n_frames == 0) return ACINO_OK;
  ACINO_REQUIRE(d_det && d_cams && d_x && d_m && d_pinned && d_status && d_S && d_r && d_F && d_used && d_frame_status && d_ws,
                "null buffer (d_det, d_cams, d_x, d_m, d_pinned, d_status, d_S, d_r, d_F, d_used, d_frame_status, d_ws)");
  hipStream_t s = (hipStream_t)stream;
  LinkScalePxArgs a;
  if (int rc = spf_upload(h, p, d_ws, ws_bytes, "acino_skel_link_scale_px_workspace_bytes", s, a.dev)) return rc;
  px_fill_args(a.px, prm, d_det, d_cams, n_cams, nullptr, nullptr);
  a.x = d_x, a.m = d_m, a.pinned = d_pinned, a.status = d_status, a.n_frames = n_frames;
  a.out.S = d_S, a.out.r = d_r, a.out.F = d_F, a.out.sens = d_sens, a.out.used = d_used, a.out.frame_status = d_frame_status;
  a.kappa = 1.0 / (prm->prior_sigma * prm->prior_sigma), a.K = n_groups;
  for (int k = 0; k < ACINO_SKEL_MAX_OPS; ++k) a.grp[k] = (int8_t)(k < h.n_ops ? h_group[k] : -1);
  if (int rc = skel_dispatch_pt(h.PT, [&](auto pt) -> int {
        constexpr int T = decltype(pt)::value;
        static PerDeviceOnce attr_pinhole, attr_fisheye;      // (per PT: one pair per instantiation of this body)
        return pinhole ? spf_launch(k_skel_link_scale_px<T, true>, attr_pinhole, n_frames, lds, s, a)
                       : spf_launch(k_skel_link_scale_px<T, false>, attr_fisheye, n_frames, lds, s, a);
      }))
    return rc;
  if (d_total) return lsc_launch_total(d_S, d_r, d_F, d_used, n_frames, n_groups, d_total, s);
  return ACINO_OK;
}

}  // extern "C"
