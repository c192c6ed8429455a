// Per-frame pose fit of a generic skeleton from 3-D points with a covariance each (gfx950, fp64): acino_skel_pose_fit, the
// analogue of pose_fit.hip for a link program.
//
// Per frame the minimiser, over the P = n_active states x inside the frame's box lo <= x <= hi, of
//   F(x) = 1/2 sum_{l enters} (FK_l(x) - y_l)^T W_l (FK_l(x) - y_l) + 1/2 sum_{p >= 3} (x_p - m_p)^2 / prior_sigma^2
// with FK the link program of SkelDev, W_l = S_l^-1 (or I / sigma_iso^2) and m the start clipped to the box, by the projected
// Levenberg-Marquardt that pose_fit.hip runs too: one definition, pf_fit_frame<PT> of pose_fit_dev.hpp (active set,
// damped step on the free states, Nielsen's rule, the stops, the status codes, the stores and cov_pos), instantiated here with
// the model SkelFit<PT>: FK and Jacobian of the link program, the Gram product, where the factor is stored, cov_x, the LDS.
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
// Dynamic LDS, sized from (P, n_pose, n_ops) by spf_layout: Jw as P columns of 4 ceil(3 n_pose / 4) + 1, ONE PT x (PT + 1)
// array that holds A in its lower triangle and the factor's strict lower triangle transposed above it (the factor's diagonal
// stays in registers), one set of link operators and poses (the trial's; the returned point's are evaluated again for the
// outputs), the points and whitening factors.  cov_x = X^T X with X = L^-1: the factor is inverted in its own registers
// (with a second register set for the columns of the inverse, PT = 64 spilled to scratch) and the product runs on the matrix
// cores as A's does.  The shipped human skeleton (P = 36, n_pose = 15) takes 42 KB, the largest
// shape the limits allow (P = 64, n_pose = 65) 157 KB; a shape beyond 160 KB is refused.
#include "pose_fit_dev.hpp"
#include "skel_host.hpp"

namespace acino {

struct SkelPoseFitArgs {
  PoseFitIo io;
  const SkelDev* dev;
  const double *lo, *hi;
};

// offsets into the dynamic LDS, in units of 8 bytes
struct SpfLayout {
  int ldj, ldm;                    // leading dimensions of Jw and of M (odd: columns on unlike banks)
  int Jw, M, y, U, u, rest, pos, opv, vec, red, pm, opm, cm, axs, ent, total;
};
__host__ __device__ inline SpfLayout spf_layout(int P, int PT, int n_pose, int n_ops) {
  SpfLayout L;
  L.ldj = 4 * (((3 * n_pose > P ? 3 * n_pose : P) + 3) / 4) + 1;      // (P: the rows of L^-1 take Jw's place for cov_x)
  L.ldm = PT + 1;                  // (a compile-time constant of the kernel: its offsets are immediates)
  int o = 0;
  auto take = [&](int n) {
    const int at = o;
    o += (n + 1) & ~1;             // (16-byte steps)
    return at;
  };
  L.Jw = take(P * L.ldj);
  L.M = take(PT * L.ldm);          // (PT rows: the tiles are stored whole, the rows beyond P are zeros)
  L.y = take(3 * n_pose);          // y | U | u are consecutive: the outputs' [3 n_pose][3] products take their place
  L.U = take(6 * n_pose);
  L.u = take(3 * n_pose);
  L.rest = take(3 * n_pose);
  L.pos = take(3 * n_pose);
  L.opv = take(12 * (n_ops > 0 ? n_ops : 1));
  L.vec = take(6 * SK_MAXP);       // x, xt, m, g, lo, hi
  L.red = take(3 * SK_MAXP);
  L.pm = take(n_pose);
  L.opm = take(SK_MAXP);
  L.cm = take(2 * SK_MAXP);
  L.axs = take(SK_MAXP / 2);
  L.ent = take((n_pose + 1) / 2);
  L.total = o;
  return L;
}

struct Spf {                       // the carved LDS of one workgroup
  double *Jw, *M, *y, *U, *u, *rest, *pos, *opv, *x, *xt, *m, *g, *lo, *hi, *red;
  unsigned long long *pm, *opm, *cm;   // per slot: the ops on its path; per state: the ops that hang on it, the slots it moves [2]
  int *axs, *ent;                  // per state: its axis (0 phi, 1 theta, 2 psi); per slot: does its point enter
  int P, n_pose, n_ops, ldj, ldm, ks;
};

// The lane index again, opaque to the optimiser: what a loop body derives from it (LDS addresses, the selects of an unrolled
// row) then stays inside the body.  Hoisted out of the frame loop, hundreds of such values outlive every register and are
// spilled to scratch.
__device__ __forceinline__ int spf_here(int lane) {
  asm volatile("" : "+v"(lane));
  return lane;
}

// M off, dM/dphi off, dM/dtheta off, dM/dpsi off of op k at the states xs: the statements of k_skel_assemble
__device__ __forceinline__ void spf_link_op(const SkelDev& D, int k, const double* xs, double* out) {
  const acino_skel_op& o = D.op[k];
  const int f = o.flags;
  double sp = 0, cp = 1, st = 0, ct = 1, sz = 0, cz = 1;
  if (f & 1) sincos(D.amap[k][0] >= 0 ? xs[D.amap[k][0]] : 0.0, &sp, &cp);
  if (f & 2) sincos(D.amap[k][1] >= 0 ? xs[D.amap[k][1]] : 0.0, &st, &ct);
  if (f & 4) sincos(D.amap[k][2] >= 0 ? xs[D.amap[k][2]] : 0.0, &sz, &cz);
  const double Ry[3][3] = {{ct, 0, -st}, {0, 1, 0}, {st, 0, ct}}, dRy[3][3] = {{-st, 0, -ct}, {0, 0, 0}, {ct, 0, -st}};
  const double Rx[3][3] = {{1, 0, 0}, {0, cp, sp}, {0, -sp, cp}}, dRx[3][3] = {{0, 0, 0}, {0, -sp, cp}, {0, -cp, -sp}};
  const double Rz[3][3] = {{cz, sz, 0}, {-sz, cz, 0}, {0, 0, 1}}, dRz[3][3] = {{-sz, cz, 0}, {-cz, -sz, 0}, {0, 0, 0}};
  auto mul = [](const double (&a)[3][3], const double (&b)[3][3], double (&c)[3][3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) c[i][j] = a[i][0] * b[0][j] + a[i][1] * b[1][j] + a[i][2] * b[2][j];
  };
  double RxRy[3][3], M[4][3][3], T1[3][3];
  mul(Rx, Ry, RxRy);
  mul(Rz, RxRy, M[0]);
  mul(dRx, Ry, T1);
  mul(Rz, T1, M[1]);
  mul(Rx, dRy, T1);
  mul(Rz, T1, M[2]);
  mul(dRz, RxRy, M[3]);
  const bool untr = (f & 8) != 0;
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const bool on = m == 0 || ((f >> (m - 1)) & 1);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      double v = 0.0;
      if (on)
        v = untr ? M[m][i][0] * o.off[0] + M[m][i][1] * o.off[1] + M[m][i][2] * o.off[2]
                 : M[m][0][i] * o.off[0] + M[m][1][i] * o.off[1] + M[m][2][i] * o.off[2];
      out[m * 3 + i] = v;
    }
  }
}

// the link operators and the poses of ``xv`` into S.opv and S.pos
__device__ __forceinline__ void spf_frame(const Spf& S, const SkelDev& D, const double* xv, int lane) {
  lane = spf_here(lane);
  if (lane < S.n_ops) spf_link_op(D, lane, xv, S.opv + lane * 12);
  __syncthreads();
  for (int t = lane; t < 3 * S.n_pose; t += 64) {
    const int l = t / 3, c = t - 3 * l;
    double v = xv[c];
    unsigned long long path = S.pm[l];
    while (path) {
      const int k = __ffsll((long long)path) - 1;
      path &= path - 1;
      v = v + S.opv[k * 12 + c];
    }
    S.pos[t] = v;
  }
  __syncthreads();
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

// Jw = U G (RAW: G itself, every slot) from S.opv, zero outside the slots a column moves
template <bool RAW>
__device__ __forceinline__ void spf_jacobian(const Spf& S, int lane) {
  lane = spf_here(lane);
  const int T = S.P * S.n_pose;
  for (int t = lane; t < T; t += 64) {
    const int p = t / S.n_pose, l = t - p * S.n_pose;
    double w0 = 0.0, w1 = 0.0, w2 = 0.0;
    unsigned long long mk = p < 3 ? 0ull : (S.opm[p] & S.pm[l]);
    if ((p < 3 || mk) && (RAW || S.ent[l])) {
      double j0 = p == 0 ? 1.0 : 0.0, j1 = p == 1 ? 1.0 : 0.0, j2 = p == 2 ? 1.0 : 0.0;
      const double* dv0 = S.opv + (1 + S.axs[p]) * 3;
      while (mk) {
        const int k = __ffsll((long long)mk) - 1;
        mk &= mk - 1;
        const double* dv = dv0 + k * 12;
        j0 += dv[0];
        j1 += dv[1];
        j2 += dv[2];
      }
      if (RAW) {
        w0 = j0, w1 = j1, w2 = j2;
      } else {
        const double* U = S.U + 6 * l;
        w0 = U[0] * j0;
        w1 = U[1] * j0 + U[2] * j1;
        w2 = U[3] * j0 + U[4] * j1 + U[5] * j2;
      }
    }
    double* o = S.Jw + p * S.ldj + 3 * l;
    o[0] = w0;
    o[1] = w1;
    o[2] = w2;
  }
  __syncthreads();
}

// The lower tiles of W^T-style products on the fp64 matrix cores: result[r][c] = sum_j W[r][j] W[c][j] over j < 4 ks for the
// rows r, c < P of W (leading dimension ld; rows beyond P count as zeros).  Lane (i, k) = (lane & 15, lane >> 4) feeds
// W[16 a + i][4 s + k] for every tile row a and holds result[16 a + 4 r + k][16 b + i] of tile (a, b) in register r;
// store(row, col, value) is called for every entry with col <= row < PT (zeros beyond P).
template <int PT, class Store>
__device__ __forceinline__ void spf_gram(const double* W, int ld, int ks, int P, int lane, Store&& store) {
  lane = spf_here(lane);
  constexpr int NTL = PT / 16;
  const int i = lane & 15, k = lane >> 4;
  const double* pr[NTL];
  bool in[NTL];
#pragma unroll
  for (int a = 0; a < NTL; ++a) {
    in[a] = 16 * a + i < P;
    pr[a] = W + (in[a] ? 16 * a + i : 0) * ld + k;
  }
  d4 acc[NTL * (NTL + 1) / 2];
#pragma unroll
  for (int t = 0; t < NTL * (NTL + 1) / 2; ++t) acc[t] = d4{0.0, 0.0, 0.0, 0.0};
  for (int s = 0; s < ks; ++s) {
    double v[NTL];
#pragma unroll
    for (int a = 0; a < NTL; ++a) {
      const double h = pr[a][4 * s];
      v[a] = in[a] ? h : 0.0;
    }
    int t = 0;
#pragma unroll
    for (int a = 0; a < NTL; ++a)
#pragma unroll
      for (int b = 0; b <= a; ++b) acc[t] = mfma(v[a], v[b], acc[t]), ++t;
  }
  int t = 0;
#pragma unroll
  for (int a = 0; a < NTL; ++a)
#pragma unroll
    for (int b = 0; b <= a; ++b, ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 16 * a + 4 * r + k, col = 16 * b + i;
        if (a > b || col <= row) store(row, col, acc[t][r]);
      }
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

// X = L^-1 in place of the factor: afterwards lane i holds X[i][c] = r[c] * dinv for c < i and X[i][i] = dinv.  Step k
// broadcasts the finished row k and every later row takes its multiple; r[k] is read for the last time in step k and takes
// the new column's entry, so the inverse needs no registers beyond the factor's.
template <int PT>
__device__ __forceinline__ void spf_invert_factor(double (&r)[PT], double dinv, int lane) {
  lane = spf_here(lane);
#pragma unroll
  for (int k = 0; k < PT; ++k) {
    const double lik = r[k], xkk = pf_readlane(dinv, k);
#pragma unroll
    for (int c = 0; c < k; ++c) {
      const double xkc = pf_readlane(r[c] * dinv, k);
      r[c] = lane > k ? r[c] - lik * xkc : r[c];
    }
    r[k] = lane > k ? -lik * xkk : r[k];
  }
}

// a link program as a model of pf_fit_frame (pose_fit_dev.hpp): the frame's box from the caller, one set of link operators and
// poses (the trial's: the returned point's are evaluated again for the outputs), A and the factor in S.M
template <int PT>
struct SkelFit {
  static constexpr int RED2 = SK_MAXP;
  const Spf& S;
  const SkelDev& D;
  const double kappa;
  const int lane;
  const unsigned long long em0, em1;

  __device__ __forceinline__ int n_states() const { return S.P; }
  __device__ __forceinline__ int n_slots() const { return S.n_pose; }
  __device__ __forceinline__ double* x() const { return S.x; }
  __device__ __forceinline__ double* xt() const { return S.xt; }
  __device__ __forceinline__ double* m() const { return S.m; }
  __device__ __forceinline__ double* g() const { return S.g; }
  __device__ __forceinline__ double* red() const { return S.red; }
  __device__ __forceinline__ double* cp() const { return S.y; }             // (y, U, u are not read by then)

  __device__ __forceinline__ double lo(int p) const { return S.lo[p]; }
  __device__ __forceinline__ double hi(int p) const { return S.hi[p]; }

  __device__ __forceinline__ double eval(const double* xv, bool) {
    spf_frame(S, D, xv, lane);
    return spf_cost(S, xv, kappa, lane);
  }
  __device__ __forceinline__ void linearise() {
    spf_jacobian<false>(S, lane);
    spf_normal<PT>(S, kappa, em0, em1, lane);
  }
  __device__ __forceinline__ void accepted() {}
  __device__ __forceinline__ double diag(int p) const { return S.M[p * (PT + 1) + p]; }
  // the active set at S.x, one bit per state: at a bound with the gradient pushing outward
  __device__ __forceinline__ unsigned long long active_set(int lane) const {
    bool fixed = false;
    if (lane < S.P) fixed = skel_fixed(S.x[lane], S.g[lane], S.M[lane * S.ldm + lane], S.lo[lane], S.hi[lane]);
    return __ballot(fixed);
  }

  // pf_factor_rows with identity rows P .. PT-1; the strict lower triangle goes to S.M above the diagonal, L[k][c] at
  // M[c][k + 1], for the back substitution
  __device__ __forceinline__ bool factor(unsigned long long fixmask, double lam, int lane, double (&r)[PT], double& dinv) {
    lane = spf_here(lane);
    const unsigned long long fix = fixmask | (S.P >= 64 ? 0ull : ~0ull << S.P);
    const bool ok = pf_factor_rows<PT, PT + 1, true>(S.M, fix, lam, lane, r, dinv);
    __syncthreads();                              // (the readers of the previous factor are done)
    if (lane < S.P) {
#pragma unroll
      for (int c = 0; c < PT - 1; ++c)
        if (c < lane) S.M[c * (PT + 1) + lane + 1] = r[c];
    }
    __syncthreads();
    return ok;
  }
  // pf_solve, its back substitution on the columns of L^T in S.M
  __device__ __forceinline__ double solve(const double (&r)[PT], double dinv, double v, int lane) const {
    lane = spf_here(lane);
    const int col = lane < S.P ? lane : 0;
    return pf_solve<PT, true>(r, dinv, v, lane, S.P, [&](int k) { return S.M + col * (PT + 1) + k + 1; });      // (rows P .. PT-1 are the identity's)
  }

  // cov_x = X^T X with X = L^-1: the rows of X from the registers into S.Jw as columns (W[p][i] = X[i][p], zero above the
  // diagonal and in the padding rows), the product on the matrix cores into S.M - neither A nor the factor is read again -,
  // mirrored, so symmetric bit for bit, the rows and columns of pinned states exactly 0
  __device__ __forceinline__ bool cov_x(unsigned long long fixmask, double (&r)[PT], double dinv, int lane) {
    const int P = S.P;
    spf_invert_factor<PT>(r, dinv, lane);
    lane = spf_here(lane);
    const int kpad = (P + 3) & ~3;
    if (lane < kpad) {
#pragma unroll
      for (int p = 0; p < PT; ++p)
        if (p < P) S.Jw[p * S.ldj + lane] = lane >= P || p > lane ? 0.0 : (p == lane ? dinv : r[p] * dinv);
    }
    __syncthreads();
    bool fin = true;
    spf_gram<PT>(S.Jw, S.ldj, kpad / 4, P, lane, [&](int row, int col, double v) {
      if (((fixmask >> row) | (fixmask >> col)) & 1ull) v = 0.0;
      fin = fin && m_finite(v);
      S.M[row * (PT + 1) + col] = v;
      S.M[col * (PT + 1) + row] = v;
    });
    return __all(fin);
  }
  __device__ __forceinline__ void outputs_at_x(bool live) {
    if (live) spf_frame(S, D, S.x, lane);          // (S.opv and S.pos hold the last trial's, which may have been refused)
  }
  __device__ __forceinline__ double pos(int t) const { return S.pos[t]; }
  __device__ __forceinline__ double cov(int p, int q) const { return S.M[p * (PT + 1) + q]; }
  __device__ __forceinline__ void jacobian_raw(int lane) { spf_jacobian<true>(S, lane); }
  __device__ __forceinline__ double jw(int p, int row) const { return S.Jw[p * S.ldj + row]; }
  __device__ __forceinline__ bool moves(int p, int l) const { return (S.cm[2 * p + (l >> 6)] >> (l & 63)) & 1ull; }
};

template <int PT>
__global__ void __launch_bounds__(64) k_skel_pose_fit(SkelPoseFitArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const SkelDev& D = *a.dev;
  const int lane = threadIdx.x;
  const int P = D.n_act, NPOSE = D.n_pose, NOPS = D.n_ops, R3 = 3 * NPOSE;
  const SpfLayout lay = spf_layout(P, PT, NPOSE, NOPS);
  double* base = reinterpret_cast<double*>(smem_raw);
  Spf S;
  S.Jw = base + lay.Jw, S.M = base + lay.M, S.y = base + lay.y, S.U = base + lay.U, S.u = base + lay.u;
  S.rest = base + lay.rest, S.pos = base + lay.pos, S.opv = base + lay.opv;
  S.x = base + lay.vec, S.xt = S.x + SK_MAXP, S.m = S.xt + SK_MAXP, S.g = S.m + SK_MAXP, S.lo = S.g + SK_MAXP, S.hi = S.lo + SK_MAXP;
  S.red = base + lay.red;
  S.pm = reinterpret_cast<unsigned long long*>(base + lay.pm);
  S.opm = reinterpret_cast<unsigned long long*>(base + lay.opm);
  S.cm = reinterpret_cast<unsigned long long*>(base + lay.cm);
  S.axs = reinterpret_cast<int*>(base + lay.axs);
  S.ent = reinterpret_cast<int*>(base + lay.ent);
  S.P = P, S.n_pose = NPOSE, S.n_ops = NOPS, S.ldj = lay.ldj, S.ldm = lay.ldm, S.ks = (R3 + 3) / 4;

  // ---- once per workgroup: the op and slot masks of every state, the rest pose
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

// the params block of skel_program with the four fields this entry reads, everything else at a value skel_validate accepts
static acino_skel_fte_params spf_params(const acino_skel_fte_params* p) {
  acino_skel_fte_params q;
  memset(&q, 0, sizeof(q));
  q.n_frames = 1, q.n_cams = 1;
  q.n_pose = p->n_pose, q.n_ops = p->n_ops, q.n_angles = p->n_angles, q.n_active = p->n_active;
  q.loss = ACINO_SKEL_LOSS_L1;
  q.h = 1.0, q.l1_eps = 1e-2, q.lam0 = 1e-3;
  return q;
}

constexpr size_t SPF_LDS_MAX = 160 * 1024;
static size_t spf_ws_clip() { return skel_align256(sizeof(SkelDev)); }

}  // namespace acino

using namespace acino;

extern "C" {

size_t acino_skel_pose_fit_workspace_bytes(const acino_skel_fte_params* p) {
  if (!p) return 0;
  const acino_skel_fte_params q = spf_params(p);
  if (skel_validate(&q)) return 0;
  return spf_ws_clip() + skel_align256(sizeof(SkelClip));
}

int acino_skel_pose_fit(const acino_pose_fit_params* prm, const acino_skel_fte_params* p, const acino_skel_op* h_ops,
                        const int32_t* h_active, const double* d_points, const double* d_cov, const double* d_x0,
                        const double* d_lo, const double* d_hi, int64_t n_frames, double* d_x, double* d_cost,
                        uint8_t* d_nmarkers, uint8_t* d_status, uint8_t* d_iters, uint8_t* d_pinned, double* d_cov_x,
                        double* d_pos, double* d_cov_pos, double* d_std_pos, void* d_ws, size_t ws_bytes, void* stream) {
  ACINO_REQUIRE(prm != nullptr, "prm");
  ACINO_REQUIRE(p != nullptr, "params");
  const acino_skel_fte_params q = spf_params(p);
  int rc = skel_validate(&q);
  if (rc) return rc;
  if ((rc = pf_check_params(prm, n_frames, p->n_pose, "min_markers must be 1..n_pose"))) return rc;
  ACINO_REQUIRE(h_ops && h_active, "null buffer (h_ops, h_active)");
  SkelDev h;
  if ((rc = skel_program(&q, h_ops, h_active, h))) return rc;
  const SpfLayout lay = spf_layout(h.n_act, h.PT, h.n_pose, h.n_ops);
  const size_t lds = sizeof(double) * (size_t)lay.total;
  ACINO_REQUIRE(lds <= SPF_LDS_MAX, "n_active x n_pose does not fit the pose fit's 160 KB of LDS");
  if (n_frames == 0) return ACINO_OK;
  ACINO_REQUIRE(d_points && d_lo && d_hi && d_x && d_status && d_ws, "null buffer (d_points, d_lo, d_hi, d_x, d_status, d_ws)");
  if ((rc = skel_check_workspace(d_ws, ws_bytes, acino_skel_pose_fit_workspace_bytes(p), "acino_skel_pose_fit_workspace_bytes",
                                 ACINO_ERR_WORKSPACE)))
    return rc;
  hipStream_t s = (hipStream_t)stream;
  SkelDev* d_dev = reinterpret_cast<SkelDev*>(d_ws);
  SkelClip* d_clip = reinterpret_cast<SkelClip*>(reinterpret_cast<char*>(d_ws) + spf_ws_clip());
  if ((rc = skel_upload(h, nullptr, 0, d_dev, d_clip, 1, s))) return rc;      // (no camera: only the link program is read)
  SkelPoseFitArgs a;
  a.dev = d_dev, a.lo = d_lo, a.hi = d_hi;
  pf_fill_io(a.io, prm, d_points, d_cov, d_x0, n_frames, d_x, d_cost, d_nmarkers, d_status, d_iters, d_pinned, d_cov_x, d_pos,
             d_cov_pos, d_std_pos);
  const int grid = grid_for(n_frames, 1);       // one frame per workgroup pass, grid-stride beyond the cap
  return skel_dispatch_pt(h.PT, [&](auto pt) -> int {
    constexpr int T = decltype(pt)::value;
    static PerDeviceOnce attr;
    if (attr.first())
      ACINO_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_skel_pose_fit<T>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                          (int)SPF_LDS_MAX));
    hipLaunchKernelGGL(k_skel_pose_fit<T>, dim3(grid), dim3(64), lds, s, a);
    ACINO_LAUNCH_CHECK();
    return ACINO_OK;
  });
}

}  // extern "C"
