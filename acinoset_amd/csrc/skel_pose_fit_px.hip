// Per-frame pose fit of a generic skeleton from the detections of every camera (gfx950, fp64): acino_skel_pose_fit_px, the
// analogue of pose_fit_px.hip for a link program and the fourth model of pf_fit_frame<N> (pose_fit_dev.hpp).
//
// Per frame the minimiser, over the P = n_active states x inside the frame's box lo <= x <= hi, of
//   F(x) = 1/sigma_px^2 sum_{(c,l) valid} sum_{k in (u,v)} 1/2 f^2 log1p(r_k^2 / f^2) + 1/2 sum_{p >= 3} (x_p - m_p)^2 / prior_sigma^2
// with r = pi_c(FK_l(x)) - det[n, c, l, :2]: FK the link program of SkelDev, pi_c the calibration-level projection mv_project
// (pinhole.hpp: fisheye with skew, or pinhole), a detection valid when its likelihood is above thresh and both pixel values
// finite, F = +inf when a valid detection's slot has z_c <= 0, m the start clipped to the box.  Gradient and matrix carry the
// IRLS weight w = 1 / (1 + r_k^2 / f^2), J = (J_pi R_c) G_l; the same A serves step, predicted reduction, active set and
// outputs.  The model is SkelPxFit<PT, PINHOLE>: SkelCore<PT> of pose_fit_skel.hpp (link operators, poses, raw Jacobian, Gram
// product, factor, solve, cov_x: what skel_pose_fit.hip's SkelFit runs) plus the pixel measurement of pose_fit_px_dev.hpp
// (what pose_fit_px.hip's CheetahPxFit runs); the layout's head and tail, the carving and the host path are pose_fit_skel.hpp's.
//
// One 64-lane wave per frame, one launch, a grid-stride loop over the frames, no atomics, nothing waits on another workgroup.
//   eval       FK, then the n_cams n_pose (camera, slot) pairs over the lanes, pair t = lane + 64 k: project, add the two log
//              terms; the ridge terms by lanes 3 .. P-1; the 64 partial sums by a butterfly of lane exchanges whose additions
//              pair the same operands in every lane: every lane holds the same bits, the same from run to run.
//   linearise  the raw G once (spf_jacobian<true>, P columns of 3 n_pose rows in S.Jw).  Then the cameras in groups of
//              max(1, 64 / n_pose): pair (camera of the group, slot) per lane projects its slot and leaves sqrt(w) / sigma_px *
//              (J_pi R_c) (2 x 3) and sqrt(w) / sigma_px * r.  Then camera by camera: the P n_pose (state, slot) entries of
//              Jc = that block times G_l over the lanes - 2 n_pose rows padded to a multiple of 4, exact zeros for an invalid
//              detection and outside a column's slots -, and ceil(2 n_pose / 4) k-steps into the PT/16 (PT/16 + 1) / 2
//              accumulator tiles of spf_gram_passes on the fp64 matrix cores, carried across the cameras.  A camera without a valid
//              detection is skipped.  The full 2 n_pose C x P Jacobian is never in LDS.
//   g          in (camera, row) order either way.  Where P < PT the weighted residuals ride as column P of Jc and row P of
//              the product is Jc^T (sqrt(w) r / sigma_px): g without its ridge comes out of the tiles that give A.  Where
//              P = PT (no spare row), or when the caller's block sets bit 0 of ``reserved`` (the switch of the measurement in
//              NOTES_perf.md), lane p sums its column of Jc against the residuals camera by camera.
//   outputs    the count of valid detections (uint16) and the weights at the returned x, stored by the model (outputs_at_x).
//
// Dynamic LDS, sized from (P, PT, n_pose, n_ops, n_cams, camera model) by spx_layout: G as P columns of ldj, Jc as P + 1 columns
// of ldc = 4 ceil(2 n_pose / 4) + 1 (both odd: columns on unlike banks), the PT x (PT + 1) array of A and the factor, the
// camera records (once per launch), the frame's detections, the validity mask as two 64-bit words per camera (n_pose may
// exceed 64), a group's 2 x 3 blocks and residuals, the [3 n_pose][3] products of the outputs.  The shipped human skeleton
// (P = 36, n_pose = 15) with 2 cameras takes 55 088 bytes; a shape beyond 160 KB is refused before any device call.
#include "pose_fit_px_dev.hpp"
#include "pose_fit_skel.hpp"

namespace acino {

struct SkelPxArgs {
  PoseFitIo io;
  PxArgs px;
  const SkelDev* dev;
  const double *lo, *hi;
  int loop_g;                      // g by the per-state loop even where P < PT
};

// offsets into the dynamic LDS, in units of 8 bytes: SpfLayout with the pixel measurement's regions
struct SpxLayout {
  SpfLayout s;
  int ldc, group;                  // leading dimension of Jc (odd); cameras projected in one pass
  int Jc, cams, det, vm, jr, ur, cp, total;
};
__host__ __device__ inline SpxLayout spx_layout(int P, int PT, int n_pose, int n_ops, int n_cams, bool pinhole) {
  SpxLayout L;
  SpfTake take;
  L.s = spf_layout(P, PT, n_pose, n_ops, take, [&](SpfTake& t) {
    L.ldc = 4 * ((2 * n_pose + 3) / 4) + 1;
    L.group = n_pose >= 64 ? 1 : 64 / n_pose;
    if (L.group > n_cams) L.group = n_cams;
    L.Jc = t((P + 1) * L.ldc);     // (column P: the weighted residuals)
    L.cams = t(n_cams * (pinhole ? ACINO_PINHOLE_STRIDE : ACINO_CAM_STRIDE));
    L.det = t(n_cams * n_pose * 3);
    L.vm = t(2 * n_cams);
    L.jr = t(L.group * n_pose * 6);
    L.ur = t(L.group * 2 * n_pose);
    L.cp = t(9 * n_pose);
  });
  L.total = take.o;
  return L;
}

struct Spx {                       // the carved LDS of the pixel measurement
  double *Jc, *det, *jr, *ur, *cp;
  unsigned long long* vm;          // per camera: the slots with a valid detection [2]
  int ldc, ks2, group;
};

template <int PT, bool PINHOLE>
struct SkelPxFit : SkelCore<PT> {
  typedef SkelCore<PT> Core;
  using Core::D;
  using Core::lane;
  using Core::S;
  const Spx& X;
  const PxArgs& b;
  const CamRec<PINHOLE>* const cams;
  const double kappa;
  const int64_t n;
  const int n_det;
  const bool gcol;                 // g from row P of the Gram product

  __device__ __forceinline__ SkelPxFit(const Spf& S_, const SkelDev& D_, int lane_, const Spx& X_, const PxArgs& b_,
                                       const CamRec<PINHOLE>* cams_, double kappa_, int64_t n_, int n_det_, bool gcol_)
      : Core{S_, D_, lane_}, X(X_), b(b_), cams(cams_), kappa(kappa_), n(n_), n_det(n_det_), gcol(gcol_) {}

  __device__ __forceinline__ double* cp() const { return X.cp; }
  __device__ __forceinline__ bool valid(int c, int l) const { return (X.vm[2 * c + (l >> 6)] >> (l & 63)) & 1ull; }

  // F(xv): the link operators and poses of xv, the pairs over the lanes, the same sum in every lane
  __device__ __forceinline__ double eval(const double* xv, bool) {
    spf_frame(S, D, xv, lane);
    const int L = S.n_pose, pairs = L * b.n_cams;
    double part = 0.0;
    bool behind = false;
    for (int t = lane; t < pairs; t += 64) {
      const int c = t / L, l = t - c * L;
      if (!valid(c, l)) continue;
      part += px_pair_cost(b, cams[c], S.pos + 3 * l, X.det, t, behind);
    }
    return px_cost_finish(part, xv, S.m, kappa, S.P, lane, b, behind);
  }

  // G, then A and g at S.x camera by camera (S.opv and S.pos are S.x's: the last eval was the accepted trial's or the start's)
  __device__ __forceinline__ void linearise() {
    spf_jacobian<true>(S, lane);
    const int here = spf_here(lane);
    const int P = S.P, L = S.n_pose, C = b.n_cams, R2 = 2 * L;
    double gsum = 0.0;
    int c = -1, c0 = -X.group;                    // the camera whose rows are in Jc; the first camera of the group in jr, ur
    const double* urc = X.ur;
    // the next camera with a valid detection into Jc (false: there is none), a barrier behind it
    auto advance = [&]() -> bool {
      for (++c; c < C; ++c) {
        if (c >= c0 + X.group) {
          // ---- a group of cameras over the lanes: pair (cc, l) projects slot l in camera c0 + cc
          c0 += X.group;
          for (int t = here; t < X.group * L; t += 64) {
            const int cc = t / L, l = t - cc * L, cg = c0 + cc;
            double jr[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, u[2] = {0.0, 0.0};
            // The twin of px_pair_rows (pose_fit_px_dev.hpp), kept here as text, as the weight loop of outputs_at_x is the twin
            // of px_store_outputs: called as those functions the statements reach this kernel in another order, two
            // instantiations took other AGPR counts and <48, false> measured 0.2 to 0.8 % slower (NOTES_perf.md).
            if (cg < C && valid(cg, l)) {
              double uv[2], JR[2][3];
              px_project<true>(cams[cg], S.pos + 3 * l, uv, JR);
              const double* d = X.det + (cg * L + l) * 3;
#pragma unroll
              for (int k = 0; k < 2; ++k) {
                const double r = uv[k] - d[k];
                const double sw = sqrt(rcp64(1.0 + r * r * b.ifs2)) * b.inv_sigma;
                jr[3 * k] = sw * JR[k][0];
                jr[3 * k + 1] = sw * JR[k][1];
                jr[3 * k + 2] = sw * JR[k][2];
                u[k] = sw * r;
              }
            }
#pragma unroll
            for (int k = 0; k < 6; ++k) X.jr[t * 6 + k] = jr[k];
            X.ur[cc * R2 + 2 * l] = u[0];
            X.ur[cc * R2 + 2 * l + 1] = u[1];
          }
          __syncthreads();
        }
        if ((X.vm[2 * c] | X.vm[2 * c + 1]) == 0ull) continue;      // (the same in every lane)
        // ---- the camera's 2 n_pose rows of Jc, the residuals beside them
        const double* jrc = X.jr + (c - c0) * L * 6;
        urc = X.ur + (c - c0) * R2;
        for (int t = here; t < P * L; t += 64) {
          const int p = t / L, l = t - p * L;
          double v0 = 0.0, v1 = 0.0;
          if (this->moves(p, l) && valid(c, l)) {
            const double *a = S.Jw + p * S.ldj + 3 * l, *q = jrc + 6 * l;
            v0 = q[0] * a[0] + q[1] * a[1] + q[2] * a[2];
            v1 = q[3] * a[0] + q[4] * a[1] + q[5] * a[2];
          }
          X.Jc[p * X.ldc + 2 * l] = v0;
          X.Jc[p * X.ldc + 2 * l + 1] = v1;
        }
        if (gcol)
          for (int t = here; t < R2; t += 64) X.Jc[P * X.ldc + t] = urc[t];
        __syncthreads();
        return true;
      }
      return false;
    };
    bool more = advance();
    spf_gram_passes<PT>(X.Jc, X.ldc, more ? X.ks2 : 0, gcol ? P + 1 : P, lane,
                        [&]() -> bool {
                          if (!more) return false;
                          if (!gcol && here < P) {
                            const double* col = X.Jc + here * X.ldc;
                            for (int t = 0; t < R2; ++t) gsum += col[t] * urc[t];
                          }
                          __syncthreads();        // (Jc is free for the next camera, jr and ur after the last of the group)
                          more = advance();
                          return more;
                        },
                        [&](int row, int col, double v) {
                          S.M[row * (PT + 1) + col] = row < P ? v : 0.0;      // (the rows beyond P are zeros, as the 3-D fit stores them)
                          if (gcol && row == P && col < P) S.g[col] = v;      // row P: Jc^T (sqrt(w) r / sigma_px)
                        });
    if (!gcol && here < P) S.g[here] = gsum;
    __syncthreads();
    if (here >= 3 && here < P) {
      S.M[here * (PT + 1) + here] += kappa;
      S.g[here] += kappa * (S.x[here] - S.m[here]);
    }
    __syncthreads();
  }
  __device__ __forceinline__ void accepted() {}

  // the count of valid detections and, at the returned x, the poses and the weight every coordinate ended with
  __device__ __forceinline__ void outputs_at_x(bool live) {
    if (live) spf_frame(S, D, S.x, lane);          // (S.opv and S.pos hold the last trial's, which may have been refused)
    if (lane == 0 && b.ndet) b.ndet[n] = (uint16_t)n_det;
    if (!b.weight) return;
    const int L = S.n_pose, pairs = L * b.n_cams;
    double* out = b.weight + n * pairs * 2;
    for (int t = lane; t < pairs; t += 64) {
      const int c = t / L, l = t - c * L;
      double w0 = live ? 0.0 : __builtin_nan(""), w1 = w0;
      if (live && valid(c, l)) {
        double uv[2];
        px_project<false>(cams[c], S.pos + 3 * l, uv, nullptr);
        const double* d = X.det + (c * L + l) * 3;
        const double r0 = uv[0] - d[0], r1 = uv[1] - d[1];
        w0 = rcp64(1.0 + r0 * r0 * b.ifs2);
        w1 = rcp64(1.0 + r1 * r1 * b.ifs2);
      }
      out[2 * t] = w0;
      out[2 * t + 1] = w1;
    }
  }
};

template <int PT, bool PINHOLE>
__global__ void __launch_bounds__(64) k_skel_pose_fit_px(SkelPxArgs a) {
  constexpr int STRIDE = PINHOLE ? ACINO_PINHOLE_STRIDE : ACINO_CAM_STRIDE;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const SkelDev& D = *a.dev;
  const PxArgs& b = a.px;
  const int lane = threadIdx.x;
  const int P = D.n_act, NPOSE = D.n_pose, NOPS = D.n_ops, C = b.n_cams;
  const SpxLayout lay = spx_layout(P, PT, NPOSE, NOPS, C, PINHOLE);
  double* base = reinterpret_cast<double*>(smem_raw);
  const Spf S = spf_carve(base, lay.s, [](Spf&) {});
  Spx X;
  X.Jc = base + lay.Jc, X.det = base + lay.det, X.jr = base + lay.jr, X.ur = base + lay.ur, X.cp = base + lay.cp;
  X.vm = reinterpret_cast<unsigned long long*>(base + lay.vm);
  X.ldc = lay.ldc, X.ks2 = (2 * NPOSE + 3) / 4, X.group = lay.group;
  double* const recs = base + lay.cams;

  // ---- once per workgroup: the op and slot masks of every state, the camera records, the padding rows of Jc
  spf_masks(S, D, P, NPOSE, NOPS, lane);
  for (int e = lane; e < C * STRIDE; e += 64) recs[e] = b.cams[e];
  for (int e = lane; e < (P + 1) * lay.ldc; e += 64) X.Jc[e] = 0.0;
  const bool gcol = P < PT && !a.loop_g;
  const int frame_doubles = C * NPOSE * 3;

  for (int64_t n = blockIdx.x; n < a.io.n_frames; n += gridDim.x) {
    const PoseFitIo& io = a.io;
    __syncthreads();                              // the previous frame is done with S and X (and the tables are complete)
    const double* src = b.det + n * frame_doubles;
    for (int e = lane; e < frame_doubles; e += 64) X.det[e] = src[e];
    __syncthreads();
    // ---- the valid detections, camera by camera, 64 slots at a time
    int n_det = 0;
    for (int c = 0; c < C; ++c)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int l = lane + 64 * h;
        bool ok = false;
        if (l < NPOSE) {
          const double* d = X.det + (c * NPOSE + l) * 3;
          ok = px_valid(d, b.thresh);
        }
        const unsigned long long vm = __ballot(ok);
        if (lane == 0) X.vm[2 * c + h] = vm;
        n_det += __popcll(vm);
      }
    // ---- the caller's start, clipped to the frame's box: the first iterate and the centre of the ridge
    if (lane < P) {
      const double lo = a.lo[n * P + lane], hi = a.hi[n * P + lane];
      const double v = pf_clip(io.x0[n * P + lane], lo, hi);
      S.lo[lane] = lo;
      S.hi[lane] = hi;
      S.m[lane] = v;
      S.x[lane] = v;
    }
    __syncthreads();
    SkelPxFit<PT, PINHOLE> m(S, D, lane, X, b, reinterpret_cast<const CamRec<PINHOLE>*>(recs), io.kappa, n, n_det, gcol);
    pf_fit_frame<PT>(m, io, n, lane, n_det);
  }
}

}  // namespace acino

using namespace acino;

extern "C" {

size_t acino_skel_pose_fit_px_workspace_bytes(const acino_skel_fte_params* p) { return spf_workspace_bytes(p); }

int acino_skel_pose_fit_px(const acino_pose_fit_px_params* prm, const acino_skel_fte_params* p, const acino_skel_op* h_ops,
                           const int32_t* h_active, const double* d_det, int64_t n_frames, int n_cams, const double* d_cams,
                           const double* d_x0, const double* d_lo, const double* d_hi, double* d_x, double* d_cost,
                           uint16_t* d_ndet, uint8_t* d_status, uint8_t* d_iters, uint8_t* d_pinned, double* d_cov_x, double* d_pos,
                           double* d_cov_pos, double* d_std_pos, double* d_weight, void* d_ws, size_t ws_bytes, void* stream) {
  ACINO_REQUIRE(prm != nullptr, "prm");
  acino_pose_fit_params fit;
  SkelDev h;
  auto check_fit = [&] {
    return px_check_params(prm, n_frames, n_cams, p->n_pose, "min_detections must be 1..n_pose n_cams", fit);
  };
  if (int rc = spf_program(p, h_ops, h_active, h, check_fit)) return rc;
  const bool pinhole = prm->camera_model == 1;
  const size_t lds = sizeof(double) * (size_t)spx_layout(h.n_act, h.PT, h.n_pose, h.n_ops, n_cams, pinhole).total;
  ACINO_REQUIRE(lds <= SPF_LDS_MAX, "n_active x n_pose x n_cams does not fit the pixel pose fit's 160 KB of LDS");
  if (n_frames == 0) return ACINO_OK;
  ACINO_REQUIRE(d_det && d_cams && d_x0 && d_lo && d_hi && d_x && d_status && d_ws,
                "null buffer (d_det, d_cams, d_x0, d_lo, d_hi, d_x, d_status, d_ws)");
  hipStream_t s = (hipStream_t)stream;
  SkelPxArgs a;
  if (int rc = spf_upload(h, p, d_ws, ws_bytes, "acino_skel_pose_fit_px_workspace_bytes", s, a.dev)) return rc;
  a.lo = d_lo, a.hi = d_hi, a.loop_g = prm->reserved & 1;
  pf_fill_io(a.io, &fit, nullptr, nullptr, d_x0, n_frames, d_x, d_cost, nullptr, d_status, d_iters, d_pinned, d_cov_x, d_pos,
             d_cov_pos, d_std_pos);
  px_fill_args(a.px, prm, d_det, d_cams, n_cams, d_ndet, d_weight);
  return skel_dispatch_pt(h.PT, [&](auto pt) -> int {
    constexpr int T = decltype(pt)::value;
    static PerDeviceOnce attr_pinhole, attr_fisheye;      // (per PT: one pair per instantiation of this body)
    return pinhole ? spf_launch(k_skel_pose_fit_px<T, true>, attr_pinhole, n_frames, lds, s, a)
                   : spf_launch(k_skel_pose_fit_px<T, false>, attr_fisheye, n_frames, lds, s, a);
  });
}

}  // extern "C"
