// The per-frame pose fit, stated once.  Four models instantiate pf_fit_frame<N>: CheetahFit (pose_fit.hip: the cheetah, 25
// states, from 3-D points), CheetahPxFit (pose_fit_px.hip: the cheetah from the detections of every camera), SkelFit<PT>
// (skel_pose_fit.hip: a link program, PT = 16 .. 64 rows, from 3-D points) and SkelPxFit<PT, PINHOLE> (skel_pose_fit_px.hip: a
// link program from the detections); the cheetah's two share CheetahCore (pose_fit_cheetah.hpp), the skeleton's two SkelCore
// (pose_fit_skel.hpp), the two pixel models px_project (pose_fit_px_dev.hpp).  Here: the status codes, the I/O block of both kernels, the admission
// and whitening of a 3-D point with its covariance, the register-resident Cholesky steps and the two substitutions, the
// projected Levenberg-Marquardt controller (active set, damped step on the free states, clip, predicted reduction, trial;
// Nielsen's rule and the ftol / xtol stops on an accepted trial, lam *= nu on a refused one), the epilogue (active set and
// factor at the returned x, the stores, cov_pos = G cov_x G^T) and the argument checks of the two C entries.
//
// One 64-lane wave per frame: every barrier is wave-wide, every loop bound the same in all lanes.  N is a compile-time row
// count (lane i keeps row i of the factor in registers; the pivot column passes between lanes by v_readlane, which needs
// constant lane numbers).  A model M answers, all __device__ __forceinline__:
//   sizes     n_states(), n_slots() (the cheetah's are constants: its loops unroll), RED2 (where the second column of sums
//             starts in red())
//   arrays    x(), xt(), m(), g(), red() in LDS; lo(p), hi(p): the frame's box; cp(): [3 n_slots][3] free for the outputs
//   model     eval(xv, trial): FK at xv and F, the same value in every lane (trial: without touching what belongs to the
//             iterate); linearise(): Jacobian, A and g at x(); accepted(): the trial has become the iterate; diag(p) = A_pp;
//             active_set(lane)
//   factor    factor(fixmask, lam, lane, r, dinv): pf_factor_rows on the model's A plus the store for the back substitution;
//             solve(r, dinv, v, lane): pf_solve with the address of L[k][col] where the model stored it.  A model whose
//             unrolled bodies must keep lane-derived values out of the frame loop (skel_pose_fit.hip: spf_here) makes the lane
//             opaque in these two and in its own pieces; the cheetah passes it through
//   outputs   cov_x(fixmask, r, dinv, lane): A_free^-1 in place of A, false unless finite (each model its own method: they
//             give different bits); outputs_at_x(live); pos(t); cov(p, q); jacobian_raw(lane), jw(p, row); moves(p, l)
#pragma once
#include "fte_kernels.hpp"
#include "ldl3.hpp"

namespace acino {

enum { PF_CONVERGED = 0, PF_MAX_ITER = 1, PF_FEW_MARKERS = 2, PF_NUMERIC = 3 };

// what a pose-fit kernel reads and writes, as the C entries receive it (optional outputs NULL) plus the derived scalars
struct PoseFitIo {
  const double *points, *cov, *x0;
  int64_t n_frames;
  double *x, *cost;
  uint8_t *nmarkers, *status, *iters, *pinned;
  double *cov_x, *pos, *cov_pos, *std_pos;
  int max_iter, min_markers;
  double lam0, ftol, xtol, kappa, inv_sigma_iso;
};

// the checks of both C entries on the parameter block (prm is not NULL); ``slots_text`` names the range of min_markers
inline int pf_check_params(const acino_pose_fit_params* prm, int64_t n_frames, int n_slots, const char* slots_text) {
  ACINO_REQUIRE(n_frames >= 0, "n_frames");
  ACINO_REQUIRE(prm->max_iter >= 1 && prm->max_iter <= 255, "max_iter must be 1..255 (the iteration count is one byte)");
  ACINO_REQUIRE(prm->min_markers >= 1 && prm->min_markers <= n_slots, slots_text);
  ACINO_REQUIRE(prm->lam0 > 0 && prm->lam0 < INFINITY, "lam0 must be > 0");
  ACINO_REQUIRE(prm->ftol > 0 && prm->ftol < INFINITY, "ftol must be > 0");
  ACINO_REQUIRE(prm->xtol > 0 && prm->xtol < INFINITY, "xtol must be > 0");
  ACINO_REQUIRE(prm->prior_sigma > 0 && prm->prior_sigma < INFINITY, "prior_sigma must be > 0");
  ACINO_REQUIRE(prm->sigma_iso > 0 && prm->sigma_iso < INFINITY, "sigma_iso must be > 0");
  return ACINO_OK;
}

inline void pf_fill_io(PoseFitIo& a, const acino_pose_fit_params* prm, const double* d_points, const double* d_cov,
                       const double* d_x0, int64_t n_frames, double* d_x, double* d_cost, uint8_t* d_nmarkers, uint8_t* d_status,
                       uint8_t* d_iters, uint8_t* d_pinned, double* d_cov_x, double* d_pos, double* d_cov_pos, double* d_std_pos) {
  a.points = d_points, a.cov = d_cov, a.x0 = d_x0, a.n_frames = n_frames, a.x = d_x, a.cost = d_cost;
  a.nmarkers = d_nmarkers, a.status = d_status, a.iters = d_iters, a.pinned = d_pinned;
  a.cov_x = d_cov_x, a.pos = d_pos, a.cov_pos = d_cov_pos, a.std_pos = d_std_pos;
  a.max_iter = prm->max_iter, a.min_markers = prm->min_markers, a.lam0 = prm->lam0, a.ftol = prm->ftol, a.xtol = prm->xtol;
  a.kappa = 1.0 / (prm->prior_sigma * prm->prior_sigma);
  a.inv_sigma_iso = 1.0 / prm->sigma_iso;
}

// the value lane ``l`` holds (``l`` the same in every lane: a constant of an unrolled loop)
__device__ __forceinline__ double pf_readlane(double v, int l) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), l), hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
  return __hiloint2double(hi, lo);
}

// np.clip: a NaN stays a NaN
__device__ __forceinline__ double pf_clip(double v, double lo, double hi) { return v != v ? v : fmin(fmax(v, lo), hi); }

// Does the point yp[3] with the covariance s[3][3] (NULL: I sigma_iso^2) enter, and its whitening factor: W = S^-1 = U^T U
// with the lower-triangular U = D^-1/2 L^-1 of S = L D L^T, stored u00 u10 u11 u20 u21 u22 (all 0 where it does not enter).
// It enters when every value is finite and every pivot is above 1e-12 of the trace (the rule of triangulate_mv.hip).
__device__ __forceinline__ bool pf_whiten(const double* __restrict__ yp, const double* __restrict__ s, double inv_sigma_iso,
                                          double (&y)[3], double (&U)[6]) {
  y[0] = yp[0], y[1] = yp[1], y[2] = yp[2];
#pragma unroll
  for (int k = 0; k < 6; ++k) U[k] = 0.0;
  bool enter = m_finite(y[0]) && m_finite(y[1]) && m_finite(y[2]);
  if (s) {
    double c[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      c[k] = s[k];
      enter = enter && m_finite(c[k]);
    }
    Ldl3 f;
    enter = enter && ldl3(c[0], c[1], c[2], c[4], c[5], c[8], 1e-12 * (c[0] + c[4] + c[8]), f);
    if (enter) {
      const double s0 = sqrt(f.i0), s1 = sqrt(f.i1), s2 = sqrt(f.i2);
      U[0] = s0;
      U[1] = -s1 * f.l10;
      U[2] = s1;
      U[3] = s2 * (f.l10 * f.l21 - f.l20);
      U[4] = -s2 * f.l21;
      U[5] = s2;
    }
  } else if (enter) {
    U[0] = U[2] = U[5] = inv_sigma_iso;
  }
  return enter;
}

// Cholesky factor of A + lam diag(A) on the free states (identity rows for the states of ``fix``: the pinned ones and a
// model's padding rows), row i in the registers of lane i: r[j] = L[i][j] for j < i, dinv = 1 / L[i][i].  No LDS traffic and no
// barrier inside the N steps: the pivot column passes between lanes by v_readlane.  A has the leading dimension LD; PACKED:
// A is its lower triangle in an array that holds other things too, so only the entries of the free block are read.  False on
// a pivot that is not above zero (the same value in every lane).
template <int N, int LD, bool PACKED, class Mask>
__device__ __forceinline__ bool pf_factor_rows(const double* A, Mask fix, double lam, int lane, double (&r)[N], double& dinv) {
  const int i = lane < N ? lane : N - 1;          // (the lanes beyond the matrix shadow its last row; nothing reads them)
  const bool fi = (fix >> i) & 1;
#pragma unroll
  for (int j = 0; j < N; ++j) {
    const bool pinned = fi || ((fix >> j) & 1);
    double v = i == j ? 1.0 : 0.0;
    if (!PACKED || !pinned) {
      const double av = A[PACKED && j > i ? j * LD + i : i * LD + j];
      if (!pinned) v = i == j ? av + lam * fmax(av, DIAG_FLOOR) : av;
    }
    r[j] = v;
  }
  bool ok = true;
  dinv = 0.0;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const double dk = pf_readlane(r[k], k);
    ok = ok && dk > 0.0 && m_finite(dk);
    double ik = __builtin_amdgcn_rsq(dk);         // 1 / sqrt(dk): the hardware estimate and two Newton steps
#pragma unroll
    for (int nr = 0; nr < 2; ++nr) ik = fma(0.5 * ik, fma(-dk * ik, ik, 1.0), ik);
    const double lik = r[k] * ik;                 // L[i][k] in the lanes i > k
    r[k] = lik;
    if (lane == k) dinv = ik;
#pragma unroll
    for (int j = k + 1; j < N; ++j) r[j] -= lik * pf_readlane(lik, j);
  }
  return ok;
}

// d = (L L^T)^-1 b, lane p holding entry p: forward substitution on the rows in registers, back substitution on the columns
// of L^T - ``at(k)`` is where the model stored L[k][this lane's column]; GUARD: it is read only below the diagonal of the
// first ``rows`` rows (the others are the identity's) -, the finished entry passed on by v_readlane
template <int N, bool GUARD, class At>
__device__ __forceinline__ double pf_solve(const double (&r)[N], double dinv, double v, int lane, int rows, At&& at) {
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const double zk = pf_readlane(v * dinv, k);
    v = lane == k ? zk : (lane > k ? v - r[k] * zk : v);
  }
#pragma unroll
  for (int k = N - 1; k >= 0; --k) {
    const double xk = pf_readlane(v * dinv, k);
    const double lkc = !GUARD || (k < rows && lane < k) ? *at(k) : 0.0;
    v = lane == k ? xk : (lane < k ? v - lkc * xk : v);
  }
  return v;
}

// ---- the projected Levenberg-Marquardt from x(): the controller of the FTE solve, per frame.  st enters as PF_MAX_ITER.
template <int N, class M>
__device__ __forceinline__ void pf_lm(M& m, const PoseFitIo& a, int lane, int& st, int& it, double& F) {
  const int P = m.n_states();
  F = m.eval(m.x(), false);
  m.linearise();
  double lam = a.lam0, nu = 2.0;
  if (!m_finite(F)) st = PF_NUMERIC;
#pragma unroll 1
  while (st == PF_MAX_ITER && it < a.max_iter) {
    ++it;
    const auto fixmask = m.active_set(lane);
    double r[N], dinv;
    if (!m.factor(fixmask, lam, lane, r, dinv)) {
      st = PF_NUMERIC;
      break;
    }
    const bool free_p = lane < P && !((fixmask >> lane) & 1);
    const double pg = free_p ? m.g()[lane] : 0.0;
    const double d = m.solve(r, dinv, -pg, lane);
    if (lane < P) {
      const double xo = m.x()[lane], xn = pf_clip(xo + d, m.lo(lane), m.hi(lane));
      m.xt()[lane] = xn;
      m.red()[lane] = d * (lam * fmax(m.diag(lane), DIAG_FLOOR) * d - pg);
      m.red()[M::RED2 + lane] = fabs(xn - xo);
    }
    __syncthreads();
    double pred = 0.0, step = 0.0;
    for (int k = 0; k < P; ++k) {
      pred += m.red()[k];
      step = fmax(step, m.red()[M::RED2 + k]);
    }
    pred *= 0.5;
    __syncthreads();
    const double Ft = m.eval(m.xt(), true);
    if (Ft < F) {
      const double dF = F - Ft, gain = pred > 0.0 ? dF / pred : -1.0;
      m.accepted();
      F = Ft;
      if (lane < P) m.x()[lane] = m.xt()[lane];
      __syncthreads();
      m.linearise();
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

// ---- the outputs of frame n at the returned x: the active set, A_free^-1, positions and G cov_x G^T
template <int N, class M>
__device__ __forceinline__ void pf_epilogue(M& m, const PoseFitIo& a, int64_t n, int lane, int st, int it, int n_enter, double F) {
  const int P = m.n_states(), L = m.n_slots(), R3 = 3 * L;
  const double NaN = __builtin_nan("");
  const bool want_cov = a.cov_x || a.cov_pos || a.std_pos;
  bool live = st == PF_CONVERGED || st == PF_MAX_ITER;
  decltype(m.active_set(lane)) fixmask = 0;
  if (live) {
    fixmask = m.active_set(lane);
    double r[N], dinv;
    bool ok = m.factor(fixmask, 0.0, lane, r, dinv) && m_finite(F);
    if (lane < P) ok = ok && m_finite(m.x()[lane]);
    ok = __all(ok);
    if (ok && want_cov) ok = m.cov_x(fixmask, r, dinv, lane);
    if (!ok) {
      st = PF_NUMERIC;
      live = false;
    }
    __syncthreads();
  }
  m.outputs_at_x(live);

  if (lane == 0) {
    a.status[n] = (uint8_t)st;
    if (a.nmarkers) a.nmarkers[n] = (uint8_t)n_enter;
    if (a.iters) a.iters[n] = (uint8_t)it;
    if (a.cost) a.cost[n] = live ? F : NaN;
  }
  if (lane < P) {
    a.x[n * P + lane] = live ? m.x()[lane] : NaN;
    if (a.pinned) a.pinned[n * P + lane] = (uint8_t)(live ? (fixmask >> lane) & 1 : 0);
  }
  if (a.pos)
    for (int t = lane; t < R3; t += 64) a.pos[n * R3 + t] = live ? m.pos(t) : NaN;
  if (a.cov_x)
    for (int t = lane; t < P * P; t += 64) a.cov_x[n * P * P + t] = live ? m.cov(t / P, t % P) : NaN;
  if (a.cov_pos || a.std_pos) {
    double* CP = m.cp();
    if (live) {
      m.jacobian_raw(lane);
      for (int rw = lane; rw < R3; rw += 64) {
        const int l = rw / 3;
        double t[N];
#pragma unroll
        for (int q = 0; q < N; ++q) t[q] = 0.0;
        for (int p = 0; p < P; ++p) {
          if (!m.moves(p, l)) continue;
          const double jp = m.jw(p, rw);
#pragma unroll
          for (int q = 0; q < N; ++q)
            if (q < P) t[q] += jp * m.cov(p, q);
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          double acc = 0.0;
#pragma unroll
          for (int q = 0; q < N; ++q)
            if (q < P) acc += t[q] * m.jw(q, 3 * l + j);
          CP[rw * 3 + j] = acc;
        }
      }
      __syncthreads();
    }
    for (int rw = lane; rw < R3; rw += 64) {
      const int l = rw / 3, i = rw - 3 * l;
      if (a.cov_pos)
#pragma unroll
        for (int j = 0; j < 3; ++j)
          a.cov_pos[(n * L + l) * 9 + i * 3 + j] = live ? 0.5 * (CP[rw * 3 + j] + CP[(3 * l + j) * 3 + i]) : NaN;
      if (a.std_pos && i == 0)
        a.std_pos[n * L + l] = live ? sqrt((CP[(3 * l) * 3] + CP[(3 * l + 1) * 3 + 1]) + CP[(3 * l + 2) * 3 + 2]) : NaN;
    }
  }
}

// one frame after the model's prologue (the slots that enter through pf_whiten, the start clipped to the box in x() and m()):
// the fit and the outputs.  The prologue stays with the kernels - k_pose_fit and k_skel_pose_fit each hold a copy, the
// other's twin: shared, it cost the skeleton kernel 0.5 % (NOTES_perf.md).
template <int N, class M>
__device__ __forceinline__ void pf_fit_frame(M& m, const PoseFitIo& a, int64_t n, int lane, int n_enter) {
  int st = PF_MAX_ITER, it = 0;
  double F = __builtin_nan("");
  if (n_enter < a.min_markers)
    st = PF_FEW_MARKERS;
  else
    pf_lm<N>(m, a, lane, st, it, F);
  pf_epilogue<N>(m, a, n, lane, st, it, n_enter, F);
}

}  // namespace acino
