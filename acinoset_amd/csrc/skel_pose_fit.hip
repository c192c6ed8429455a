// Per-frame pose fit of a generic skeleton from 3-D points with a covariance each (gfx950, fp64): acino_skel_pose_fit, the
// analogue of pose_fit.hip for a link program.
//
// Per frame the minimiser, over the P = n_active states x inside the frame's box lo <= x <= hi, of
//   F(x) = 1/2 sum_{l enters} (FK_l(x) - y_l)^T W_l (FK_l(x) - y_l) + 1/2 sum_{p >= 3} (x_p - m_p)^2 / prior_sigma^2
// with FK the link program of SkelDev, W_l = S_l^-1 (or I / sigma_iso^2) and m the start clipped to the box, by the projected
// Levenberg-Marquardt that pose_fit.hip runs too: one definition, pf_fit_frame<PT> of pose_fit_dev.hpp (active set,
// damped step on the free states, Nielsen's rule, the stops, the status codes, the stores and cov_pos), instantiated here with
// the model SkelFit<PT>: SkelCore<PT> of pose_fit_skel.hpp (FK and Jacobian of the link program, the Gram product, where the
// factor is stored, cov_x - what skel_pose_fit_px.hip's model shares) plus the 3-D measurement and the LDS layout of this file.
//
// One 64-lane wave per frame, one wave per workgroup, a grid-stride loop over the frames, no atomics: every barrier is
// wave-wide and nothing waits on another workgroup.  The kernel is a template on PT = 16, 32, 48, 64 (P rounded up to 16):
// row i of the Cholesky factor lives in the registers of lane i and the pivot column passes between lanes by v_readlane, which
// needs a compile-time bound; rows P .. PT-1 are identity rows.  A = Jw^T Jw runs on the fp64 matrix cores (dense80.hpp's
// wrapper): PT/16 (PT/16 + 1) / 2 lower tiles over ceil(3 n_pose / 4) k-steps, Jw = U G whitened per slot.
//
// The link operators (M off and its three derivatives per op: the assembly's arithmetic, skel_assemble.hpp) are evaluated one
// op per lane; a pose is the sum of the operators on its path in program order, which is what the program's own sequence
// pos[child] = pos[parent] + M off adds, term for term.  Column p of G_l is the sum of the derivative operators of the ops on
// l's path that hang on state p (skel_pose_jac_col's sum, from per-state op masks built once per workgroup instead of a scan of
// the program per entry); it is evaluated only where that set is not empty, and g is summed over those slots in slot order.
//
// Dynamic LDS, sized from (P, n_pose, n_ops) by spf3_layout (spf_layout of pose_fit_skel.hpp around y, U, u, rest; that header
// also carves Spf and holds the entry's host path): Jw as P columns of 4 ceil(3 n_pose / 4) + 1, ONE PT x (PT + 1)
// array that holds A in its lower triangle and the factor's strict lower triangle transposed above it (the factor's diagonal
// stays in registers), one set of link operators and poses (the trial's; the returned point's are evaluated again for the
// outputs), the points and whitening factors.  cov_x = X^T X with X = L^-1: the factor is inverted in its own registers
// (with a second register set for the columns of the inverse, PT = 64 spilled to scratch) and the product runs on the matrix
// cores as A's does.  The shipped human skeleton (P = 36, n_pose = 15) takes 42 KB, the largest
// shape the limits allow (P = 64, n_pose = 65) 157 KB; a shape beyond 160 KB is refused.
#include "pose_fit_skel.hpp"

namespace acino {

struct SkelPoseFitArgs {
  PoseFitIo io;
  const SkelDev* dev;
  const double *lo, *hi;
};

// offsets into the dynamic LDS, in units of 8 bytes: SpfLayout with the 3-D measurement's regions
struct Spf3Layout {
  SpfLayout s;
  int y, U, u, rest, ent, total;
};
__host__ __device__ inline Spf3Layout spf3_layout(int P, int PT, int n_pose, int n_ops) {
  Spf3Layout L;
  SpfTake take;
  L.s = spf_layout(P, PT, n_pose, n_ops, take, [&](SpfTake& t) {
    L.y = t(3 * n_pose);           // y | U | u are consecutive: the outputs' [3 n_pose][3] products take their place
    L.U = t(6 * n_pose);
    L.u = t(3 * n_pose);
    L.rest = t(3 * n_pose);
  });
  L.ent = take((n_pose + 1) / 2);
  L.total = take.o;
  return L;
}

// F(xv) of the poses S.pos: the whitened residuals into S.u, the sum in a fixed order (the same value in every lane)
__device__ __forceinline__ double spf_cost(const Spf& S, const double* xv, double kappa, int lane) {
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
    const double e = xv[lane] - S.m[lane];
    S.red[S.n_pose + lane - 3] = 0.5 * kappa * e * e;
  }
  __syncthreads();
  double f = 0.0;
  for (int k = 0; k < S.n_pose + S.P - 3; ++k) f += S.red[k];
  __syncthreads();
  return f;
}

// A = Jw^T Jw + diag(kappa) into the lower triangle of S.M (spf_gram over the 3 n_pose rows of Jw).  A column of zeros (a
// state no entering slot moves) gives exact zeros.  g = Jw^T u + kappa (x - m) at S.x over the entering slots of the column,
// in slot order, one state per lane.
template <int PT>
__device__ __forceinline__ void spf_normal(const Spf& S, double kappa, unsigned long long em0, unsigned long long em1, int lane) {
  spf_gram<PT>(S.Jw, S.ldj, S.ks, S.P, lane, [&](int row, int col, double v) {
    S.M[row * (PT + 1) + col] = v;
  });
  __syncthreads();
  if (lane >= 3 && lane < S.P) S.M[lane * (PT + 1) + lane] += kappa;
  if (lane < S.P) {
    double sum = 0.0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      unsigned long long mk = S.cm[2 * lane + h] & (h ? em1 : em0);
      while (mk) {
        const int l = 64 * h + __ffsll((long long)mk) - 1;
        mk &= mk - 1;
        const double *a = S.Jw + lane * S.ldj + 3 * l, *b = S.u + 3 * l;
        sum += a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
      }
    }
    if (lane >= 3) sum += kappa * (S.x[lane] - S.m[lane]);
    S.g[lane] = sum;
  }
  __syncthreads();
}

// a link program seen as 3-D points: SkelCore of pose_fit_skel.hpp plus the measurement - the whitened residuals and their
// sum, Jw = U G and the Gram product over the entering slots
template <int PT>
struct SkelFit : SkelCore<PT> {
  typedef SkelCore<PT> Core;
  using Core::D;
  using Core::lane;
  using Core::S;
  const double kappa;
  const unsigned long long em0, em1;

  __device__ __forceinline__ SkelFit(const Spf& S_, const SkelDev& D_, double kappa_, int lane_, unsigned long long em0_,
                                     unsigned long long em1_)
      : Core{S_, D_, lane_}, kappa(kappa_), em0(em0_), em1(em1_) {}

  __device__ __forceinline__ double* cp() const { return S.y; }             // (y, U, u are not read by then)

  __device__ __forceinline__ double eval(const double* xv, bool) {
    spf_frame(S, D, xv, lane);
    return spf_cost(S, xv, kappa, lane);
  }
  __device__ __forceinline__ void linearise() {
    spf_jacobian<false>(S, lane);
    spf_normal<PT>(S, kappa, em0, em1, lane);
  }
  __device__ __forceinline__ void accepted() {}
  __device__ __forceinline__ void outputs_at_x(bool live) {
    if (live) spf_frame(S, D, S.x, lane);          // (S.opv and S.pos hold the last trial's, which may have been refused)
  }
};

template <int PT>
__global__ void __launch_bounds__(64) k_skel_pose_fit(SkelPoseFitArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const SkelDev& D = *a.dev;
  const int lane = threadIdx.x;
  const int P = D.n_act, NPOSE = D.n_pose, NOPS = D.n_ops, R3 = 3 * NPOSE;
  const Spf3Layout lay = spf3_layout(P, PT, NPOSE, NOPS);
  double* base = reinterpret_cast<double*>(smem_raw);
  Spf S = spf_carve(base, lay.s, [&](Spf& S) {
    S.y = base + lay.y, S.U = base + lay.U, S.u = base + lay.u, S.rest = base + lay.rest;
  });
  S.ent = reinterpret_cast<int*>(base + lay.ent);

  // ---- once per workgroup: the op and slot masks of every state, the rest pose.  The masks are the twin of spf_masks
  //      (pose_fit_skel.hpp), kept here as text: called as that function the same statements come out in another register
  //      order and this kernel measured 0.08 to 0.19 ms slower on the 6 240 frames of the shipped video (NOTES_perf.md).
  for (int l = lane; l < NPOSE; l += 64) S.pm[l] = D.pmask[l];
  {
    unsigned long long om = 0;
    int ax = 0;
    if (lane < P)
      for (int k = 0; k < NOPS; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c)
          if (D.amap[k][c] == lane) om |= 1ull << k, ax = c;
    S.opm[lane] = om;
    S.axs[lane] = ax;
    S.x[lane] = 0.0;
  }
  __syncthreads();
  {
    unsigned long long c0 = 0, c1 = 0;
    if (lane < P)
      for (int l = 0; l < NPOSE; ++l)
        if (lane < 3 || (S.opm[lane] & S.pm[l])) (l < 64 ? c0 : c1) |= 1ull << (l & 63);
    S.cm[2 * lane] = c0;
    S.cm[2 * lane + 1] = c1;
  }
  spf_frame(S, D, S.x, lane);
  for (int t = lane; t < R3; t += 64) S.rest[t] = S.pos[t];

  for (int64_t n = blockIdx.x; n < a.io.n_frames; n += gridDim.x) {
    const PoseFitIo& io = a.io;
    __syncthreads();                              // the previous frame is done with S (and the tables are complete)
    for (int e = lane; e < P * (4 * S.ks - R3); e += 64)      // the padding rows of Jw (cov_x's product has used them)
      S.Jw[(e / (4 * S.ks - R3)) * S.ldj + R3 + e % (4 * S.ks - R3)] = 0.0;
    // ---- the slots that enter, their whitening factors (k_pose_fit holds the twin of this prologue)
    unsigned long long em0 = 0, em1 = 0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int l = lane + 64 * h;
      bool enter = false;
      if (l < NPOSE) {
        double y[3], U[6];
        enter = pf_whiten(io.points + (n * NPOSE + l) * 3, io.cov ? io.cov + (n * NPOSE + l) * 9 : nullptr, io.inv_sigma_iso, y, U);
#pragma unroll
        for (int k = 0; k < 3; ++k) S.y[3 * l + k] = enter ? y[k] : 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) S.U[6 * l + k] = U[k];
        S.ent[l] = enter ? 1 : 0;
      }
      (h ? em1 : em0) = __ballot(enter);
    }
    const int n_enter = __popcll(em0) + __popcll(em1);
    __syncthreads();
    // ---- the start: the caller's, or every angle 0 and the root at the mean of y_l - rest_l over the entering slots, in
    //      slot order; clipped to the box, and the centre of the ridge
    if (lane < P) {
      const double lo = a.lo[n * P + lane], hi = a.hi[n * P + lane];
      double v = 0.0;
      if (io.x0) {
        v = io.x0[n * P + lane];
      } else if (lane < 3 && n_enter > 0) {
        double sum = 0.0;
        for (int l = 0; l < NPOSE; ++l)
          if (S.ent[l]) sum += S.y[3 * l + lane] - S.rest[3 * l + lane];
        v = sum / (double)n_enter;
      }
      v = pf_clip(v, lo, hi);
      S.lo[lane] = lo;
      S.hi[lane] = hi;
      S.m[lane] = v;
      S.x[lane] = v;
    }
    __syncthreads();
    SkelFit<PT> m{S, D, io.kappa, lane, em0, em1};
    pf_fit_frame<PT>(m, io, n, lane, n_enter);
  }
}

}  // namespace acino

using namespace acino;

extern "C" {

size_t acino_skel_pose_fit_workspace_bytes(const acino_skel_fte_params* p) { return spf_workspace_bytes(p); }

int acino_skel_pose_fit(const acino_pose_fit_params* prm, const acino_skel_fte_params* p, const acino_skel_op* h_ops,
                        const int32_t* h_active, const double* d_points, const double* d_cov, const double* d_x0,
                        const double* d_lo, const double* d_hi, int64_t n_frames, double* d_x, double* d_cost,
                        uint8_t* d_nmarkers, uint8_t* d_status, uint8_t* d_iters, uint8_t* d_pinned, double* d_cov_x,
                        double* d_pos, double* d_cov_pos, double* d_std_pos, void* d_ws, size_t ws_bytes, void* stream) {
  ACINO_REQUIRE(prm != nullptr, "prm");
  SkelDev h;
  auto check_fit = [&] { return pf_check_params(prm, n_frames, p->n_pose, "min_markers must be 1..n_pose"); };
  if (int rc = spf_program(p, h_ops, h_active, h, check_fit)) return rc;
  const size_t lds = sizeof(double) * (size_t)spf3_layout(h.n_act, h.PT, h.n_pose, h.n_ops).total;
  ACINO_REQUIRE(lds <= SPF_LDS_MAX, "n_active x n_pose does not fit the pose fit's 160 KB of LDS");
  if (n_frames == 0) return ACINO_OK;
  ACINO_REQUIRE(d_points && d_lo && d_hi && d_x && d_status && d_ws, "null buffer (d_points, d_lo, d_hi, d_x, d_status, d_ws)");
  hipStream_t s = (hipStream_t)stream;
  SkelPoseFitArgs a;
  if (int rc = spf_upload(h, p, d_ws, ws_bytes, "acino_skel_pose_fit_workspace_bytes", s, a.dev)) return rc;
  a.lo = d_lo, a.hi = d_hi;
  pf_fill_io(a.io, prm, d_points, d_cov, d_x0, n_frames, d_x, d_cost, d_nmarkers, d_status, d_iters, d_pinned, d_cov_x, d_pos,
             d_cov_pos, d_std_pos);
  return skel_dispatch_pt(h.PT, [&](auto pt) -> int {
    static PerDeviceOnce attr;                  // (per PT: one per instantiation of this body)
    return spf_launch(k_skel_pose_fit<decltype(pt)::value>, attr, n_frames, lds, s, a);
  });
}

}  // extern "C"
