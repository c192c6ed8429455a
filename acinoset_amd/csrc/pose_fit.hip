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
// as long); the inverse for cov_x is 25 right-hand sides, one per lane, on the same registers.
#include "fte_cov_dev.hpp"
#include "pose_fit_dev.hpp"

namespace acino {

constexpr int PF_ROWS = 3 * NL;      // 60 rows of J
constexpr int PF_LD = NP + 1;        // leading dimension of A and of its factor
constexpr int PF_PAIRS = NP * (NP + 1) / 2;

// the box of the 25 active states (all_optimizations.py:403-483; acinoset_amd.fte.bounds45()[ACTIVE])
#define PF_INF __builtin_huge_val()
static __device__ const double c_pf_lo[NP] = {
    -PF_INF,      -PF_INF,      -PF_INF,      -M_PI / 6,    -M_PI / 6,    -M_PI / 6,   -M_PI / 6, -M_PI / 6, -M_PI / 6,
    -M_PI / 6,    -M_PI / 1.5,  -M_PI / 1.5,  -M_PI / 2,    -M_PI,        -M_PI / 2,   -M_PI,     -M_PI / 2, 0.0,
    -M_PI / 2,    0.0,          -PF_INF,      -M_PI / 6,    -M_PI / 6,    -M_PI / 1.5, -M_PI / 1.5};
static __device__ const double c_pf_hi[NP] = {
    PF_INF,       PF_INF,       PF_INF,       M_PI / 6,     M_PI / 6,     M_PI / 6,    M_PI / 6,  M_PI / 6,  M_PI / 6,
    M_PI / 6,     M_PI / 1.5,   M_PI / 1.5,   M_PI / 2,     0.0,          M_PI / 2,    0.0,       M_PI / 2,  M_PI,
    M_PI / 2,     M_PI,         PF_INF,       M_PI / 6,     M_PI / 6,     M_PI / 1.5,  M_PI / 1.5};
#undef PF_INF

struct PoseFitArgs {
  const double *points, *cov, *x0;
  int64_t n_frames;
  double *x, *cost;
  uint8_t *nmarkers, *status, *iters, *pinned;
  double *cov_x, *pos, *cov_pos, *std_pos;
  int max_iter, min_markers;
  double lam0, ftol, xtol, kappa, inv_sigma_iso;
};

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

// np.clip: a NaN stays a NaN
__device__ __forceinline__ double pf_clip(double v, int p) { return v != v ? v : fmin(fmax(v, c_pf_lo[p]), c_pf_hi[p]); }

// sin / cos and the head position of ``xv``, then the three columns of the chain
__device__ __forceinline__ void pf_frame(CovFrame& F, const double* xv, int lane) {
  if (lane < NP) {
    if (lane < 3) {
      F.pos[20][lane] = xv[lane];
    } else {
      double s, c;
      sincos(xv[lane], &s, &c);
      F.sc[lane - 3][0] = s;
      F.sc[lane - 3][1] = c;
    }
  }
  __syncthreads();
  if (lane < 3) fk_columns(F, lane);
  __syncthreads();
}

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

constexpr int PF_TASKS = (NP * NL + 63) / 64;      // (state, marker) entries of J per lane: entry t = lane + 64 k

// what lane ``lane`` needs for its entries of J, once per launch: the pivot of (p, l) = (t / 20, t % 20) - rate_pivot -, -1
// where the marker does not hang on the angle, -2 for a column of the head position (the identity)
__device__ __forceinline__ void pf_tasks(int lane, int (&piv)[PF_TASKS]) {
#pragma unroll
  for (int k = 0; k < PF_TASKS; ++k) {
    const int t = lane + 64 * k, p = t / NL, l = t - p * NL;
    piv[k] = t >= NP * NL ? -1 : (p < 3 ? -2 : rate_pivot(l, p));
  }
}

// Jw = U J (RAW: J, every marker) of the frame F, zero outside the markers of a column
template <bool RAW>
__device__ __forceinline__ void pf_jacobian(PoseFitLds& S, const CovFrame& F, unsigned emask, const int (&piv)[PF_TASKS],
                                            int lane) {
#pragma unroll
  for (int k = 0; k < PF_TASKS; ++k) {
    const int t = lane + 64 * k, p = t / NL, l = t - p * NL;
    if (t >= NP * NL) break;
    double w0 = 0.0, w1 = 0.0, w2 = 0.0;
    if (piv[k] != -1 && (RAW || ((emask >> l) & 1u))) {
      double j[3] = {p == 0 ? 1.0 : 0.0, p == 1 ? 1.0 : 0.0, p == 2 ? 1.0 : 0.0};
      if (piv[k] >= 0) rate_cross(F, l, p, piv[k], j);
      if (RAW) {
        w0 = j[0], w1 = j[1], w2 = j[2];
      } else {
        const double* U = S.U[l];
        w0 = U[0] * j[0];
        w1 = U[1] * j[0] + U[2] * j[1];
        w2 = U[3] * j[0] + U[4] * j[1] + U[5] * j[2];
      }
    }
    S.Jw[p][3 * l] = w0;
    S.Jw[p][3 * l + 1] = w1;
    S.Jw[p][3 * l + 2] = w2;
  }
  __syncthreads();
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
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int m = 4 * r + k;
    if (m >= i) {                                 // the lower triangle of the diagonal tiles, mirrored
      const double v = a00[r] + (m == i && m >= 3 ? kappa : 0.0);
      S.A[m][i] = v;
      S.A[i][m] = v;
      if (16 + m < NP) {
        const double w = a11[r] + (m == i ? kappa : 0.0);
        S.A[16 + m][16 + i] = w;
        S.A[16 + i][16 + m] = w;
      }
    }
    if (16 + m < NP) {
      S.A[16 + m][i] = a10[r];
      S.A[i][16 + m] = a10[r];
    }
  }
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

// the active set at S.x, one bit per state: at a bound with the gradient pushing outward (oracle active_set, cov_codes)
__device__ __forceinline__ unsigned pf_active_set(const PoseFitLds& S, int lane) {
  bool fixed = false;
  if (lane < NP) {
    const double xv = S.x[lane], gv = S.g[lane], gtol = GRAD_ZERO_REL * S.A[lane][lane];
    fixed = (xv <= c_pf_lo[lane] && gv > gtol) || (xv >= c_pf_hi[lane] && gv < -gtol);
  }
  return (unsigned)__ballot(fixed);
}

// Cholesky factor of A + lam diag(A) on the free states (identity rows for the pinned ones), row i in the registers of lane
// i: r[j] = L[i][j] for j < i, dinv = 1 / L[i][i]; the rows are stored to S.L as well, for the products with L^T.  No LDS
// traffic and no barrier inside the 25 steps: the pivot column passes between lanes by v_readlane.  False on a pivot that is
// not above zero (the same value in every lane).
__device__ __forceinline__ bool pf_factor(PoseFitLds& S, unsigned fixmask, double lam, int lane, double (&r)[NP],
                                          double& dinv) {
  const int i = lane < NP ? lane : NP - 1;        // (the lanes beyond the matrix shadow its last row; nothing reads them)
  const bool fi = (fixmask >> i) & 1u;
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    double v = S.A[i][j];
    if (fi || ((fixmask >> j) & 1u))
      v = i == j ? 1.0 : 0.0;
    else if (i == j)
      v += lam * fmax(v, DIAG_FLOOR);
    r[j] = v;
  }
  bool ok = true;
  dinv = 0.0;
#pragma unroll
  for (int k = 0; k < NP; ++k) {
    const double dk = pf_readlane(r[k], k);
    ok = ok && dk > 0.0 && m_finite(dk);
    double ik = __builtin_amdgcn_rsq(dk);         // 1 / sqrt(dk): the hardware estimate and two Newton steps
#pragma unroll
    for (int nr = 0; nr < 2; ++nr) ik = fma(0.5 * ik, fma(-dk * ik, ik, 1.0), ik);
    const double lik = r[k] * ik;                 // L[i][k] in the lanes i > k
    r[k] = lik;
    if (lane == k) dinv = ik;
#pragma unroll
    for (int j = k + 1; j < NP; ++j) r[j] -= lik * pf_readlane(lik, j);
  }
  __syncthreads();                                // (the readers of the previous factor are done)
  if (lane < NP) {
#pragma unroll
    for (int j = 0; j < NP; ++j) S.L[lane][j] = r[j];
  }
  __syncthreads();
  return ok;
}

// d = (L L^T)^-1 b, lane p holding entry p: forward substitution on the rows in registers, back substitution on the rows
// of S.L read as columns of L^T, the finished entry passed on by v_readlane
__device__ __forceinline__ double pf_solve(const PoseFitLds& S, const double (&r)[NP], double dinv, double v, int lane) {
#pragma unroll
  for (int k = 0; k < NP; ++k) {
    const double zk = pf_readlane(v * dinv, k);
    v = lane == k ? zk : (lane > k ? v - r[k] * zk : v);
  }
  const int col = lane < NP ? lane : 0;
#pragma unroll
  for (int k = NP - 1; k >= 0; --k) {
    const double xk = pf_readlane(v * dinv, k);
    v = lane == k ? xk : (lane < k ? v - S.L[k][col] * xk : v);
  }
  return v;
}

// column ``lane`` of (L L^T)^-1 into z, every lane a right-hand side of its own: the entries of L come by v_readlane
__device__ __forceinline__ void pf_inverse_column(const double (&r)[NP], double dinv, int lane, double (&z)[NP]) {
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    double acc = i == lane ? 1.0 : 0.0;
#pragma unroll
    for (int k = 0; k < i; ++k) acc -= pf_readlane(r[k], i) * z[k];
    z[i] = acc * pf_readlane(dinv, i);
  }
#pragma unroll
  for (int i = NP - 1; i >= 0; --i) {
    double acc = z[i];
#pragma unroll
    for (int k = i + 1; k < NP; ++k) acc -= pf_readlane(r[i], k) * z[k];
    z[i] = acc * pf_readlane(dinv, i);
  }
}

__global__ void __launch_bounds__(64) k_pose_fit(PoseFitArgs a) {
  __shared__ PoseFitLds S;
  const int lane = threadIdx.x;
  const double NaN = __builtin_nan("");
  if (lane < NP) {
    unsigned mk = 0xFFFFFu;
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
    // ---- the markers that enter, their whitening factors
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
      v = pf_clip(v, lane);
      S.m[lane] = v;
      S.x[lane] = v;
    }
    __syncthreads();

    int st = PF_MAX_ITER, it = 0, cur = 0;
    double F = NaN;
    if (n_enter < a.min_markers) {
      st = PF_FEW_MARKERS;
    } else {
      pf_frame(S.F[0], S.x, lane);
      F = pf_cost(S, S.F[0], S.x, a.kappa, lane);
      pf_jacobian<false>(S, S.F[0], emask, piv, lane);
      pf_normal(S, emask, a.kappa, lane);
      double lam = a.lam0, nu = 2.0;
      if (!m_finite(F)) st = PF_NUMERIC;
#pragma unroll 1
      while (st == PF_MAX_ITER && it < a.max_iter) {
        ++it;
        const unsigned fixmask = pf_active_set(S, lane);
        double r[NP], dinv;
        if (!pf_factor(S, fixmask, lam, lane, r, dinv)) {
          st = PF_NUMERIC;
          break;
        }
        const bool free_p = lane < NP && !((fixmask >> lane) & 1u);
        const double pg = free_p ? S.g[lane] : 0.0;
        const double d = pf_solve(S, r, dinv, -pg, lane);
        double term = 0.0, mv = 0.0;
        if (lane < NP) {
          const double xo = S.x[lane], xn = pf_clip(xo + d, lane);
          S.xt[lane] = xn;
          term = d * (lam * fmax(S.A[lane][lane], DIAG_FLOOR) * d - pg);
          mv = fabs(xn - xo);
        }
        if (lane < NP) {
          S.red[lane] = term;
          S.red[32 + lane] = mv;
        }
        __syncthreads();
        double pred = 0.0, step = 0.0;
        for (int k = 0; k < NP; ++k) {
          pred += S.red[k];
          step = fmax(step, S.red[32 + k]);
        }
        pred *= 0.5;
        __syncthreads();
        CovFrame& T = S.F[cur ^ 1];
        pf_frame(T, S.xt, lane);
        const double Ft = pf_cost(S, T, S.xt, a.kappa, lane);
        if (Ft < F) {
          const double dF = F - Ft, gain = pred > 0.0 ? dF / pred : -1.0;
          cur ^= 1;
          F = Ft;
          if (lane < NP) S.x[lane] = S.xt[lane];
          __syncthreads();
          pf_jacobian<false>(S, S.F[cur], emask, piv, lane);
          pf_normal(S, emask, a.kappa, lane);
          const double t = 2.0 * gain - 1.0;
          lam *= fmax(1.0 / 3.0, 1.0 - t * t * t);
          nu = 2.0;
          if (dF <= a.ftol * fabs(F) || step <= a.xtol) st = PF_CONVERGED;
        } else {
          lam *= nu;
          nu *= 2.0;
          if (lam > 1e16) break;
        }
      }
    }

    // ---- the outputs at the returned x: the active set, A_free^-1, positions and J cov_x J^T
    const bool want_cov = a.cov_x || a.cov_pos || a.std_pos;
    bool live = st == PF_CONVERGED || st == PF_MAX_ITER;
    unsigned fixmask = 0;
    if (live) {
      fixmask = pf_active_set(S, lane);
      double r[NP], dinv;
      bool ok = pf_factor(S, fixmask, 0.0, lane, r, dinv) && m_finite(F);
      if (lane < NP) ok = ok && m_finite(S.x[lane]);
      ok = __all(ok);
      if (ok && want_cov) {
        // column c of the inverse by lane c, into row c of S.A (A itself is not read again); then symmetric bit for bit,
        // pinned rows and columns exactly 0
        double z[NP];
        pf_inverse_column(r, dinv, lane, z);
        if (lane < NP) {
#pragma unroll
          for (int i = 0; i < NP; ++i) {
            S.A[lane][i] = z[i];
            ok = ok && m_finite(z[i]);
          }
        }
        ok = __all(ok);
        __syncthreads();
        for (int t = lane; t < PF_PAIRS; t += 64) {
          int p = (int)((sqrtf(8.0f * (float)t + 1.0f) - 1.0f) * 0.5f);
          if (p * (p + 1) / 2 > t) --p;
          if ((p + 1) * (p + 2) / 2 <= t) ++p;
          const int q = t - p * (p + 1) / 2;
          const double v = (((fixmask >> p) | (fixmask >> q)) & 1u) ? 0.0 : 0.5 * (S.A[p][q] + S.A[q][p]);
          S.A[p][q] = v;
          S.A[q][p] = v;
        }
      }
      if (!ok) {
        st = PF_NUMERIC;
        live = false;
      }
      __syncthreads();
    }

    if (lane == 0) {
      a.status[n] = (uint8_t)st;
      if (a.nmarkers) a.nmarkers[n] = (uint8_t)n_enter;
      if (a.iters) a.iters[n] = (uint8_t)it;
      if (a.cost) a.cost[n] = live ? F : NaN;
    }
    if (lane < NP) {
      a.x[n * NP + lane] = live ? S.x[lane] : NaN;
      if (a.pinned) a.pinned[n * NP + lane] = (uint8_t)(live ? (fixmask >> lane) & 1u : 0);
    }
    if (a.pos && lane < PF_ROWS) a.pos[n * PF_ROWS + lane] = live ? S.F[cur].pos[lane / 3][lane % 3] : NaN;
    if (a.cov_x)
      for (int t = lane; t < NP * NP; t += 64) a.cov_x[n * NP * NP + t] = live ? S.A[t / NP][t % NP] : NaN;
    if (a.cov_pos || a.std_pos) {
      double* CP = &S.L[0][0];                     // [60][3]; the factor is not read again
      if (live) {
        pf_jacobian<true>(S, S.F[cur], emask, piv, lane);
        if (lane < PF_ROWS) {
          const int l = lane / 3;
          double t[NP];
#pragma unroll
          for (int q = 0; q < NP; ++q) t[q] = 0.0;
          for (int p = 0; p < NP; ++p) {
            if (!((S.colmask[p] >> l) & 1u)) continue;
            const double jp = S.Jw[p][lane];
#pragma unroll
            for (int q = 0; q < NP; ++q) t[q] += jp * S.A[p][q];
          }
#pragma unroll
          for (int j = 0; j < 3; ++j) {
            double acc = 0.0;
#pragma unroll
            for (int q = 0; q < NP; ++q) acc += t[q] * S.Jw[q][3 * l + j];
            CP[lane * 3 + j] = acc;
          }
        }
        __syncthreads();
      }
      if (lane < PF_ROWS) {
        const int l = lane / 3, i = lane - 3 * l;
        if (a.cov_pos)
#pragma unroll
          for (int j = 0; j < 3; ++j)
            a.cov_pos[(n * NL + l) * 9 + i * 3 + j] = live ? 0.5 * (CP[lane * 3 + j] + CP[(3 * l + j) * 3 + i]) : NaN;
        if (a.std_pos && i == 0)
          a.std_pos[n * NL + l] = live ? sqrt((CP[(3 * l) * 3] + CP[(3 * l + 1) * 3 + 1]) + CP[(3 * l + 2) * 3 + 2]) : NaN;
      }
    }
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
  ACINO_REQUIRE(n_frames >= 0, "n_frames");
  ACINO_REQUIRE(prm->max_iter >= 1 && prm->max_iter <= 255, "max_iter must be 1..255 (the iteration count is one byte)");
  ACINO_REQUIRE(prm->min_markers >= 1 && prm->min_markers <= ACINO_N_MARKERS, "min_markers must be 1..20");
  ACINO_REQUIRE(prm->lam0 > 0 && prm->lam0 < INFINITY, "lam0 must be > 0");
  ACINO_REQUIRE(prm->ftol > 0 && prm->ftol < INFINITY, "ftol must be > 0");
  ACINO_REQUIRE(prm->xtol > 0 && prm->xtol < INFINITY, "xtol must be > 0");
  ACINO_REQUIRE(prm->prior_sigma > 0 && prm->prior_sigma < INFINITY, "prior_sigma must be > 0");
  ACINO_REQUIRE(prm->sigma_iso > 0 && prm->sigma_iso < INFINITY, "sigma_iso must be > 0");
  if (n_frames == 0) return ACINO_OK;
  ACINO_REQUIRE(d_points && d_x && d_status, "null buffer (d_points, d_x, d_status)");
  PoseFitArgs a;
  a.points = d_points, a.cov = d_cov, a.x0 = d_x0, a.n_frames = n_frames, a.x = d_x, a.cost = d_cost;
  a.nmarkers = d_nmarkers, a.status = d_status, a.iters = d_iters, a.pinned = d_pinned;
  a.cov_x = d_cov_x, a.pos = d_pos, a.cov_pos = d_cov_pos, a.std_pos = d_std_pos;
  a.max_iter = prm->max_iter, a.min_markers = prm->min_markers, a.lam0 = prm->lam0, a.ftol = prm->ftol, a.xtol = prm->xtol;
  a.kappa = 1.0 / (prm->prior_sigma * prm->prior_sigma);
  a.inv_sigma_iso = 1.0 / prm->sigma_iso;
  const int grid = grid_for(n_frames, 1);       // one frame per workgroup pass, grid-stride beyond the cap
  hipLaunchKernelGGL(k_pose_fit, dim3(grid), dim3(64), 0, (hipStream_t)stream, a);
  ACINO_LAUNCH_CHECK();
  return ACINO_OK;
}

}  // extern "C"
