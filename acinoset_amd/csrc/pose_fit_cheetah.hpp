// What the cheetah's per-frame pose fits share as models of pf_fit_frame<25> (pose_fit_dev.hpp): pose_fit.hip (CheetahFit, from
// 3-D points) and pose_fit_px.hip (CheetahPxFit, from the detections).  Here: the constant box, the FK frame of a state vector,
// the marker Jacobian taken from it, the inverse of the register-resident factor, and CheetahCore<Lds> - the members of a model
// that do not depend on the measurement: the LDS arrays, the active set, factor and solve, cov_x with its symmetric store, the
// positions and the raw Jacobian of the outputs.  Moved here from pose_fit.hip as they stood (same text, same inlining:
// k_pose_fit keeps its code).
//
// Lds is the kernel's LDS block; CheetahCore reads its members F[2] (CovFrame), Jw[NP][PF_ROWS + 1], A and L [NP][PF_LD],
// x, xt, m, g [NP], red[64] and colmask[NP].
#pragma once
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

// the markers that move with state p, into S.colmask (complete after the next barrier)
template <class Lds>
__device__ __forceinline__ void pf_colmask(Lds& S, int lane) {
  if (lane < NP) {
    unsigned mk = 0xFFFFFu;
    if (lane >= 3) {
      mk = 0;
      for (int l = 0; l < NL; ++l)
        if ((c_ancmask[cov_marker_grp(l)] >> c_state_grp[lane]) & 1) mk |= 1u << l;
    }
    S.colmask[lane] = mk;
  }
}

// Jw = U J (RAW: J, every marker) of the frame F, zero outside the markers of a column; U = S.U[l], the six entries of the
// lower-triangular whitening factor (read only without RAW)
template <bool RAW, class Lds>
__device__ __forceinline__ void pf_jacobian(Lds& S, const CovFrame& F, unsigned emask, const int (&piv)[PF_TASKS], int lane) {
#pragma unroll
  for (int k = 0; k < PF_TASKS; ++k) {
    const int t = lane + 64 * k, p = t / NL, l = t - p * NL;
    if (t >= NP * NL) break;
    double w0 = 0.0, w1 = 0.0, w2 = 0.0;
    if (piv[k] != -1 && (RAW || ((emask >> l) & 1u))) {
      double j[3] = {p == 0 ? 1.0 : 0.0, p == 1 ? 1.0 : 0.0, p == 2 ? 1.0 : 0.0};
      if (piv[k] >= 0) rate_cross(F, l, p, piv[k], j);
      if constexpr (RAW) {
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

// The three lower 16 x 16 tiles of a 25 x 25 Gram product (padded to 32) as the matrix cores leave them - lane (i, k) =
// (lane & 15, lane >> 4) holds result[4 r + k][i] in register r - into S.A, mirrored, plus the ridge on the 22 angles
template <class Lds>
__device__ __forceinline__ void pf_store_tiles(Lds& S, const d4& a00, const d4& a10, const d4& a11, double kappa, int lane) {
  const int i = lane & 15, k = lane >> 4;
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

// the cheetah as a model of pf_fit_frame, without its measurement: the constant box, FK frames F[cur] (the iterate's) and
// F[cur ^ 1] (the trial's), A and the factor's rows in Lds.  A model adds eval, linearise, accepted and outputs_at_x.
template <class Lds>
struct CheetahCore {
  static constexpr int RED2 = 32;
  Lds& S;
  const int (&piv)[PF_TASKS];
  const int lane;
  int cur = 0;

  __device__ __forceinline__ CheetahCore(Lds& S_, const int (&piv_)[PF_TASKS], int lane_) : S(S_), piv(piv_), lane(lane_) {}

  __device__ __forceinline__ static constexpr int n_states() { return NP; }
  __device__ __forceinline__ static constexpr int n_slots() { return NL; }
  __device__ __forceinline__ double* x() const { return S.x; }
  __device__ __forceinline__ double* xt() const { return S.xt; }
  __device__ __forceinline__ double* m() const { return S.m; }
  __device__ __forceinline__ double* g() const { return S.g; }
  __device__ __forceinline__ double* red() const { return S.red; }
  __device__ __forceinline__ double* cp() const { return &S.L[0][0]; }      // [60][3]; the factor is not read again

  __device__ __forceinline__ double lo(int p) const { return c_pf_lo[p]; }
  __device__ __forceinline__ double hi(int p) const { return c_pf_hi[p]; }

  __device__ __forceinline__ double diag(int p) const { return S.A[p][p]; }
  // the active set at S.x, one bit per state: at a bound with the gradient pushing outward (oracle active_set, cov_codes)
  __device__ __forceinline__ unsigned active_set(int lane) const {
    bool fixed = false;
    if (lane < NP) {
      const double xv = S.x[lane], gv = S.g[lane], gtol = GRAD_ZERO_REL * S.A[lane][lane];
      fixed = (xv <= c_pf_lo[lane] && gv > gtol) || (xv >= c_pf_hi[lane] && gv < -gtol);
    }
    return (unsigned)__ballot(fixed);
  }

  // pf_factor_rows; the rows are stored to S.L as well, for the products with L^T
  __device__ __forceinline__ bool factor(unsigned fixmask, double lam, int lane, double (&r)[NP], double& dinv) {
    const bool ok = pf_factor_rows<NP, PF_LD, false>(&S.A[0][0], fixmask, lam, lane, r, dinv);
    __syncthreads();                              // (the readers of the previous factor are done)
    if (lane < NP) {
#pragma unroll
      for (int j = 0; j < NP; ++j) S.L[lane][j] = r[j];
    }
    __syncthreads();
    return ok;
  }
  // pf_solve, its back substitution on the rows of S.L read as columns of L^T
  __device__ __forceinline__ double solve(const double (&r)[NP], double dinv, double v, int lane) const {
    const int col = lane < NP ? lane : 0;
    return pf_solve<NP, false>(r, dinv, v, lane, NP, [&](int k) { return &S.L[k][col]; });
  }

  // column c of the inverse by lane c, into row c of S.A (A itself is not read again); then symmetric bit for bit, pinned
  // rows and columns exactly 0
  __device__ __forceinline__ bool cov_x(unsigned fixmask, const double (&r)[NP], double dinv, int lane) {
    bool ok = true;
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
    return ok;
  }
  __device__ __forceinline__ double pos(int t) const { return S.F[cur].pos[t / 3][t % 3]; }
  __device__ __forceinline__ double cov(int p, int q) const { return S.A[p][q]; }
  __device__ __forceinline__ void jacobian_raw(int lane) { pf_jacobian<true>(S, S.F[cur], 0u, piv, lane); }
  __device__ __forceinline__ double jw(int p, int row) const { return S.Jw[p][row]; }
  __device__ __forceinline__ bool moves(int p, int l) const { return (S.colmask[p] >> l) & 1u; }
};

}  // namespace acino
