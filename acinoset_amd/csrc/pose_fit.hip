// Per-frame cheetah pose fit from 3-D marker points with a covariance each (gfx950, fp64): acino_cheetah_pose_fit.
//
// Per frame the minimiser, over the 25 active states x inside the box of the FTE, of
//   F(x) = 1/2 sum_{l enters} (FK_l(x) - y_l)^T W_l (FK_l(x) - y_l) + 1/2 sum_{p = 3..24} (x_p - m_p)^2 / prior_sigma^2
// with W_l = S_l^-1 (or I / sigma_iso^2) and m the start clipped to the box: a projected Levenberg-Marquardt with the
// controller of the FTE solve (active set "at a bound, gradient pushing outward, |g_p| > 1e-14 A_pp"; (A + lam diag A) d = -g
// on the free states; Nielsen's damping), run per frame.  At the returned x: the cost, the active set, cov_x = A_free^-1 (no
// Marquardt term, pinned rows and columns exactly 0), the marker positions and cov_pos = J cov_x J^T.
//
// Frames stop after unlike numbers of trials, so a frame is one 64-lane wave and a workgroup is one wave: every barrier
// below is wave-wide and every loop bound is the same in all lanes of it.  One launch, a grid-stride loop over the frames, no
// atomics.  The FK frame with its rotation axes and the marker Jacobian are the posterior kernels' (cheetah_fk.hpp:
// fk_columns; fte_cov_dev.hpp: CovFrame, rate_pivot, rate_cross, cov_marker_grp).  In LDS per frame (about 28 KB): two FK
// frames (the iterate's and the trial's), the whitened Jacobian Jw = U J (W = U^T U, U = D^-1/2 L^-1 of S = L D L^T) as 25
// columns of 60, A [25][26] and the rows of its Cholesky factor [25][26].  A column of J is non-zero only for the markers
// that hang on its angle (c_ancmask): those entries are the only ones evaluated, and g is summed over them in marker order.
// A = Jw^T Jw runs on the fp64 matrix cores (three 16 x 16 tiles, dense80.hpp's wrapper): measured at 10 000 frames, A and g
// took 22.4 k ticks per trial with A on the VALU (325 entries over 64 lanes, summed over the markers two columns share) and
// 9.5 k with the tiles.  The factorisation keeps row i of L in the registers of lane i and passes the pivot column between
// lanes by v_readlane (no LDS traffic inside its 25 steps: the LDS form, a read-modify-write per entry, made the kernel twice
// as long); the inverse for cov_x is 25 right-hand sides, one per lane, on the same registers.  The frame after its prologue -
// controller, factor steps, substitutions, epilogue - is pf_fit_frame<25> of pose_fit_dev.hpp, which skel_pose_fit.hip
// instantiates too; this file is its model CheetahFit: the whitened residuals, Jw = U J and the three-tile Gram product on top of
// CheetahCore (pose_fit_cheetah.hpp: FK frames, marker Jacobian, factor, cov_x), which pose_fit_px.hip's model shares.
#include "pose_fit_cheetah.hpp"

namespace acino {

using PoseFitArgs = PoseFitIo;

struct PoseFitLds {
  CovFrame F[2];
  double Jw[NP][PF_ROWS + 1];  // (+ 1: columns on unlike LDS banks) column p of U J (of J itself for the outputs), zero outside the column's markers
  double A[NP][PF_LD];         // J^T W J + diag(kappa); the inverse of the free block for the outputs
  double L[NP][PF_LD];         // rows of the Cholesky factor (pf_factor)
  double y[PF_ROWS];           // the points (0 where the marker does not enter)
  double U[NL][6];             // u00 u10 u11 u20 u21 u22 of the lower-triangular U (0 where the marker does not enter)
  double u[PF_ROWS];           // U (FK - y) of the last evaluation
  double x[NP], xt[NP], m[NP], g[NP];
  double red[64];
  unsigned colmask[NP];        // the markers that move with state p
};

// F(xv) of the frame F holds: the whitened residuals into S.u, the sum in a fixed order (the same value in every lane)
__device__ __forceinline__ double pf_cost(PoseFitLds& S, const CovFrame& F, const double* xv, double kappa, int lane) {
  double part = 0.0;
  if (lane < NL) {
    const double r0 = F.pos[lane][0] - S.y[3 * lane], r1 = F.pos[lane][1] - S.y[3 * lane + 1],
                 r2 = F.pos[lane][2] - S.y[3 * lane + 2];
    const double* U = S.U[lane];
    const double u0 = U[0] * r0, u1 = U[1] * r0 + U[2] * r1, u2 = U[3] * r0 + U[4] * r1 + U[5] * r2;
    S.u[3 * lane] = u0;
    S.u[3 * lane + 1] = u1;
    S.u[3 * lane + 2] = u2;
    part = 0.5 * (u0 * u0 + u1 * u1 + u2 * u2);
  } else if (lane < NL + NP - 3) {
    const int p = lane - NL + 3;
    const double e = xv[p] - S.m[p];
    part = 0.5 * kappa * e * e;
  }
  S.red[lane] = part;
  __syncthreads();
  double f = 0.0;
  for (int k = 0; k < NL + NP - 3; ++k) f += S.red[k];
  __syncthreads();
  return f;
}

// A = Jw^T Jw + diag(kappa) on the fp64 matrix cores - the three lower 16 x 16 tiles of the 25 x 25 padded to 32, 15 k-steps
// of four rows each, through the wrapper of dense80.hpp: lane (i, k) = (lane & 15, lane >> 4) feeds Jw[i][4 s + k] and
// Jw[16 + i][4 s + k] and holds result[4 r + k][i] in register r.  A column of zeros (a state no entering marker moves)
// gives exact zeros.  g = Jw^T u + kappa (x - m) at S.x over the markers of the column, in marker order, one state per lane.
__device__ __forceinline__ void pf_normal(PoseFitLds& S, unsigned emask, double kappa, int lane) {
  const int i = lane & 15, k = lane >> 4;
  const bool upper = 16 + i < NP;
  const double *plo = &S.Jw[i][k], *phi = &S.Jw[upper ? 16 + i : 0][k];
  double lo[PF_ROWS / 4], hi[PF_ROWS / 4];
#pragma unroll
  for (int s = 0; s < PF_ROWS / 4; ++s) {
    lo[s] = plo[4 * s];
    const double h = phi[4 * s];
    hi[s] = upper ? h : 0.0;
  }
  d4 a00 = {0.0, 0.0, 0.0, 0.0}, a10 = a00, a11 = a00;
#pragma unroll
  for (int s = 0; s < PF_ROWS / 4; ++s) {
    a00 = mfma(lo[s], lo[s], a00);
    a10 = mfma(hi[s], lo[s], a10);
    a11 = mfma(hi[s], hi[s], a11);
  }
  pf_store_tiles(S, a00, a10, a11, kappa, lane);
  if (lane < NP) {
    unsigned mk = S.colmask[lane] & emask;
    double acc = 0.0;
    while (mk) {
      const int l = __ffs((int)mk) - 1;
      mk &= mk - 1;
      const double *a = &S.Jw[lane][3 * l], *b = &S.u[3 * l];
      acc += a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
    }
    if (lane >= 3) acc += kappa * (S.x[lane] - S.m[lane]);
    S.g[lane] = acc;
  }
  __syncthreads();
}

// the cheetah fitted to 3-D points as a model of pf_fit_frame (pose_fit_dev.hpp): CheetahCore (pose_fit_cheetah.hpp) plus the
// whitened residuals, Jw = U J and the three-tile Gram product
struct CheetahFit : CheetahCore<PoseFitLds> {
  const double kappa;
  const unsigned emask;

  __device__ __forceinline__ CheetahFit(PoseFitLds& S_, const int (&piv_)[PF_TASKS], double kappa_, int lane_, unsigned emask_)
      : CheetahCore<PoseFitLds>(S_, piv_, lane_), kappa(kappa_), emask(emask_) {}

  __device__ __forceinline__ double eval(const double* xv, bool trial) {
    CovFrame& T = S.F[trial ? cur ^ 1 : cur];
    pf_frame(T, xv, lane);
    return pf_cost(S, T, xv, kappa, lane);
  }
  __device__ __forceinline__ void linearise() {
    pf_jacobian<false>(S, S.F[cur], emask, piv, lane);
    pf_normal(S, emask, kappa, lane);
  }
  __device__ __forceinline__ void accepted() { cur ^= 1; }
  __device__ __forceinline__ void outputs_at_x(bool) {}                     // (F[cur] is the returned point's)
};

__global__ void __launch_bounds__(64) k_pose_fit(PoseFitArgs a) {
  __shared__ PoseFitLds S;
  const int lane = threadIdx.x;
  if (lane < NP) {                                // (pf_colmask of pose_fit_cheetah.hpp is the twin of these lines: called from
    unsigned mk = 0xFFFFFu;                       //  here it reorders this kernel's instructions, and the kernel keeps its code)
    if (lane >= 3) {
      mk = 0;
      for (int l = 0; l < NL; ++l)
        if ((c_ancmask[cov_marker_grp(l)] >> c_state_grp[lane]) & 1) mk |= 1u << l;
    }
    S.colmask[lane] = mk;
  }
  int piv[PF_TASKS];
  pf_tasks(lane, piv);
  for (int64_t n = blockIdx.x; n < a.n_frames; n += gridDim.x) {
    __syncthreads();                              // the previous frame is done with S (and colmask is complete)
    // ---- the markers that enter, their whitening factors (k_skel_pose_fit holds the twin of this prologue)
    bool enter = false;
    if (lane < NL) {
      double y[3], U[6];
      enter = pf_whiten(a.points + (n * NL + lane) * 3, a.cov ? a.cov + (n * NL + lane) * 9 : nullptr, a.inv_sigma_iso, y, U);
      S.y[3 * lane] = enter ? y[0] : 0.0;
      S.y[3 * lane + 1] = enter ? y[1] : 0.0;
      S.y[3 * lane + 2] = enter ? y[2] : 0.0;
#pragma unroll
      for (int k = 0; k < 6; ++k) S.U[lane][k] = U[k];
    }
    const unsigned emask = (unsigned)(__ballot(enter) & 0xFFFFFull);
    const int n_enter = __popc(emask);
    __syncthreads();
    // ---- the start: the caller's, or the head from the entering markers among 0, 1, 2 (else from all) and psi_0 from
    //      marker 2 - marker 3; clipped to the box, and the centre of the ridge
    if (lane < NP) {
      double v = 0.0;
      if (a.x0) {
        v = a.x0[n * NP + lane];
      } else if (lane < 3 && n_enter > 0) {
        const unsigned hm = (emask & 7u) ? (emask & 7u) : emask;
        double sum = 0.0;
        for (int l = 0; l < NL; ++l)
          if ((hm >> l) & 1u) sum += S.y[3 * l + lane];
        v = sum / (double)__popc(hm);
      } else if (lane == 20 && (emask & 12u) == 12u) {
        v = atan2(S.y[3 * 2 + 1] - S.y[3 * 3 + 1], S.y[3 * 2] - S.y[3 * 3]);
      }
      v = pf_clip(v, c_pf_lo[lane], c_pf_hi[lane]);
      S.m[lane] = v;
      S.x[lane] = v;
    }
    __syncthreads();
    CheetahFit m(S, piv, a.kappa, lane, emask);
    pf_fit_frame<NP>(m, a, n, lane, n_enter);
  }
}

}  // namespace acino

using namespace acino;

extern "C" {

size_t acino_sizeof_pose_fit_params(void) { return sizeof(acino_pose_fit_params); }

int acino_cheetah_pose_fit(const acino_pose_fit_params* prm, const double* d_points, const double* d_cov, const double* d_x0,
                           int64_t n_frames, double* d_x, double* d_cost, uint8_t* d_nmarkers, uint8_t* d_status,
                           uint8_t* d_iters, uint8_t* d_pinned, double* d_cov_x, double* d_pos, double* d_cov_pos,
                           double* d_std_pos, void* stream) {
  ACINO_REQUIRE(prm != nullptr, "prm");
  if (int rc = pf_check_params(prm, n_frames, ACINO_N_MARKERS, "min_markers must be 1..20")) return rc;
  if (n_frames == 0) return ACINO_OK;
  ACINO_REQUIRE(d_points && d_x && d_status, "null buffer (d_points, d_x, d_status)");
  PoseFitArgs a;
  pf_fill_io(a, prm, d_points, d_cov, d_x0, n_frames, d_x, d_cost, d_nmarkers, d_status, d_iters, d_pinned, d_cov_x, d_pos, d_cov_pos,
             d_std_pos);
  const int grid = grid_for(n_frames, 1);       // one frame per workgroup pass, grid-stride beyond the cap
  hipLaunchKernelGGL(k_pose_fit, dim3(grid), dim3(64), 0, (hipStream_t)stream, a);
  ACINO_LAUNCH_CHECK();
  return ACINO_OK;
}

}  // extern "C"
