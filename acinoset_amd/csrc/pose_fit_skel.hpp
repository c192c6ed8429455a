// What the skeleton's per-frame pose fits share as models of pf_fit_frame<PT> (pose_fit_dev.hpp): skel_pose_fit.hip (SkelFit,
// from 3-D points) and skel_pose_fit_px.hip (SkelPxFit, from the detections of every camera).  Here: the carved LDS of a link
// program (Spf), its layout around a model's own regions and its carving (spf_layout, spf_carve), the lane made opaque
// (spf_here), the link operators and the poses of a state vector (spf_frame), the pose
// Jacobian taken from them (spf_jacobian), the op and slot masks of every state (spf_masks), the Gram product on the fp64 matrix
// cores (spf_gram, spf_gram_passes), the inverse of the register-resident factor (spf_invert_factor) and SkelCore<PT> - the members of a
// model that do not depend on the measurement: the LDS arrays, the frame's box, the active set, factor and solve, cov_x with its
// symmetric store, the positions and the raw Jacobian of the outputs.  Moved here from skel_pose_fit.hip as they stood (same
// text, same inlining: k_skel_pose_fit keeps its code, instruction for instruction).  A model adds eval, linearise, accepted, outputs_at_x and cp.
// At the end: the host path of both C entries - spf_workspace_bytes, spf_program, spf_upload, spf_launch.
//
// Both kernels: one 64-lane wave per frame, PT = 16, 32, 48, 64 (P rounded up to 16), ONE PT x (PT + 1) array S.M that holds A in
// its lower triangle and the factor's strict lower triangle transposed above it, Jw as P columns of ldj (odd) doubles.
#pragma once
#include "pose_fit_dev.hpp"
#include "skel_host.hpp"

namespace acino {

struct Spf {                       // the carved LDS of one workgroup
  double *Jw, *M, *y, *U, *u, *rest, *pos, *opv, *x, *xt, *m, *g, *lo, *hi, *red;      // (y, U, u, rest: the 3-D measurement's)
  unsigned long long *pm, *opm, *cm;   // per slot: the ops on its path; per state: the ops that hang on it, the slots it moves [2]
  int *axs, *ent;                  // per state: its axis (0 phi, 1 theta, 2 psi); per slot: does its point enter (3-D measurement)
  int P, n_pose, n_ops, ldj, ldm, ks;
};

// offsets into the dynamic LDS, in units of 8 bytes: the regions both fits have; a model's own lie between M and pos (``middle``).
// ``jw_cols``: the columns of Jw when it holds more than the P of the pose (link_scale_dev.hpp: P + K); 0: P
struct SpfLayout {
  int P, n_pose, n_ops;
  int ldj, ldm;                    // leading dimensions of Jw and of M (odd: columns on unlike banks)
  int Jw, M, pos, opv, vec, red, pm, opm, cm, axs;
};
struct SpfTake {                   // the next region of n doubles, in 16-byte steps
  int o = 0;
  __host__ __device__ int operator()(int n) { return (o += (n + 1) & ~1) - ((n + 1) & ~1); }
};
template <class Middle>
__host__ __device__ inline SpfLayout spf_layout(int P, int PT, int n_pose, int n_ops, SpfTake& take, Middle&& middle,
                                                int jw_cols = 0) {
  SpfLayout L;
  L.P = P, L.n_pose = n_pose, L.n_ops = n_ops;
  L.ldj = 4 * (((3 * n_pose > P ? 3 * n_pose : P) + 3) / 4) + 1;      // (P: the rows of L^-1 take Jw's place for cov_x)
  L.ldm = PT + 1;                  // (a compile-time constant of the kernel: its offsets are immediates)
  L.Jw = take((jw_cols ? jw_cols : P) * L.ldj);
  L.M = take(PT * L.ldm);          // (PT rows: the tiles are stored whole, the rows beyond P are zeros)
  middle(take);
  L.pos = take(3 * n_pose);
  L.opv = take(12 * (n_ops > 0 ? n_ops : 1));
  L.vec = take(6 * SK_MAXP);       // x, xt, m, g, lo, hi
  L.red = take(3 * SK_MAXP);
  L.pm = take(n_pose);
  L.opm = take(SK_MAXP);
  L.cm = take(2 * SK_MAXP);
  L.axs = take(SK_MAXP / 2);
  return L;
}

// the members of Spf every model has; ``middle(S)`` sets the model's own between M and pos (y, U, u, rest, ent: NULL unless it
// does).  The pointers are formed in the order of the regions: in another, k_skel_pose_fit gets other scalar address arithmetic
template <class Middle>
__device__ __forceinline__ Spf spf_carve(double* base, const SpfLayout& lay, Middle&& middle) {
  Spf S;
  S.y = S.U = S.u = S.rest = nullptr, S.ent = nullptr;
  S.Jw = base + lay.Jw, S.M = base + lay.M;
  middle(S);
  S.pos = base + lay.pos, S.opv = base + lay.opv;
  S.x = base + lay.vec, S.xt = S.x + SK_MAXP, S.m = S.xt + SK_MAXP, S.g = S.m + SK_MAXP;
  S.lo = S.g + SK_MAXP, S.hi = S.lo + SK_MAXP;
  S.red = base + lay.red;
  S.pm = reinterpret_cast<unsigned long long*>(base + lay.pm);
  S.opm = reinterpret_cast<unsigned long long*>(base + lay.opm);
  S.cm = reinterpret_cast<unsigned long long*>(base + lay.cm);
  S.axs = reinterpret_cast<int*>(base + lay.axs);
  S.P = lay.P, S.n_pose = lay.n_pose, S.n_ops = lay.n_ops, S.ldj = lay.ldj, S.ldm = lay.ldm, S.ks = (3 * lay.n_pose + 3) / 4;
  return S;
}

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

// once per workgroup: per slot the ops on its path (S.pm), per state the ops that hang on it and its axis (S.opm, S.axs), then
// the slots it moves (S.cm); a barrier between the two and none after the second; S.x is left at zero.  k_skel_pose_fit holds
// the twin of these statements as text (skel_pose_fit.hip says why)
__device__ __forceinline__ void spf_masks(const Spf& S, const SkelDev& D, int P, int NPOSE, int NOPS, int lane) {
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
}

// The lower tiles of W^T-style products on the fp64 matrix cores: result[r][c] = sum_j W[r][j] W[c][j] over j < 4 ks for the
// rows r, c < P of W (leading dimension ld; rows beyond P count as zeros).  Lane (i, k) = (lane & 15, lane >> 4) feeds
// W[16 a + i][4 s + k] for every tile row a and holds result[16 a + 4 r + k][16 b + i] of tile (a, b) in register r;
// store(row, col, value) is called for every entry with col <= row < PT (zeros beyond P).  After every pass over the 4 ks
// columns next() is asked for another: it rewrites W in place (a barrier of its own before it returns) and the sum carries on
// in the same tiles - the cameras of skel_pose_fit_px.hip.
template <int PT, class Next, class Store>
__device__ __forceinline__ void spf_gram_passes(const double* W, int ld, int ks, int P, int lane, Next&& next, Store&& store) {
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
  do {
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
  } while (next());
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

// one pass
template <int PT, class Store>
__device__ __forceinline__ void spf_gram(const double* W, int ld, int ks, int P, int lane, Store&& store) {
  spf_gram_passes<PT>(W, ld, ks, P, lane, [] { return false; }, store);
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

// a link program as a model of pf_fit_frame, without its measurement: the frame's box from the caller, one set of link operators
// and poses (the trial's: the returned point's are evaluated again for the outputs), A and the factor in S.M
template <int PT>
struct SkelCore {
  static constexpr int RED2 = SK_MAXP;
  const Spf& S;
  const SkelDev& D;
  const int lane;

  __device__ __forceinline__ int n_states() const { return S.P; }
  __device__ __forceinline__ int n_slots() const { return S.n_pose; }
  __device__ __forceinline__ double* x() const { return S.x; }
  __device__ __forceinline__ double* xt() const { return S.xt; }
  __device__ __forceinline__ double* m() const { return S.m; }
  __device__ __forceinline__ double* g() const { return S.g; }
  __device__ __forceinline__ double* red() const { return S.red; }

  __device__ __forceinline__ double lo(int p) const { return S.lo[p]; }
  __device__ __forceinline__ double hi(int p) const { return S.hi[p]; }

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
  __device__ __forceinline__ double pos(int t) const { return S.pos[t]; }
  __device__ __forceinline__ double cov(int p, int q) const { return S.M[p * (PT + 1) + q]; }
  __device__ __forceinline__ void jacobian_raw(int lane) { spf_jacobian<true>(S, lane); }
  __device__ __forceinline__ double jw(int p, int row) const { return S.Jw[p * S.ldj + row]; }
  __device__ __forceinline__ bool moves(int p, int l) const { return (S.cm[2 * p + (l >> 6)] >> (l & 63)) & 1ull; }
};

// the params block of skel_program with the four fields the pose fits read, everything else at a value skel_validate accepts
inline acino_skel_fte_params spf_params(const acino_skel_fte_params* p) {
  acino_skel_fte_params q;
  memset(&q, 0, sizeof(q));
  q.n_frames = 1, q.n_cams = 1;
  q.n_pose = p->n_pose, q.n_ops = p->n_ops, q.n_angles = p->n_angles, q.n_active = p->n_active;
  q.loss = ACINO_SKEL_LOSS_L1;
  q.h = 1.0, q.l1_eps = 1e-2, q.lam0 = 1e-3;
  return q;
}

constexpr size_t SPF_LDS_MAX = 160 * 1024;
inline size_t spf_ws_clip() { return skel_align256(sizeof(SkelDev)); }

// ---- the host path of both entries, in the order of their checks: spf_program, the entry's 160 KB check of its own layout, its
//      n_frames == 0 return and null-buffer check, spf_upload, spf_launch.  spf_workspace_bytes: both exported *_workspace_bytes
inline size_t spf_workspace_bytes(const acino_skel_fte_params* p) {
  if (!p) return 0;
  const acino_skel_fte_params q = spf_params(p);
  if (skel_validate(&q)) return 0;
  return spf_ws_clip() + skel_align256(sizeof(SkelClip));
}

// the params block checked, then the entry's own parameters (check_fit()), then the link program into h
template <class CheckFit>
inline int spf_program(const acino_skel_fte_params* p, const acino_skel_op* h_ops, const int32_t* h_active, SkelDev& h,
                       CheckFit&& check_fit) {
  ACINO_REQUIRE(p != nullptr, "params");
  const acino_skel_fte_params q = spf_params(p);
  if (int rc = skel_validate(&q)) return rc;
  if (int rc = check_fit()) return rc;
  ACINO_REQUIRE(h_ops && h_active, "null buffer (h_ops, h_active)");
  return skel_program(&q, h_ops, h_active, h);
}

// the workspace checked (``query`` names the entry's function), the link program uploaded into it: d_dev (no camera is read)
inline int spf_upload(const SkelDev& h, const acino_skel_fte_params* p, void* d_ws, size_t ws_bytes, const char* query,
                      hipStream_t s, const SkelDev*& d_dev) {
  if (int rc = skel_check_workspace(d_ws, ws_bytes, spf_workspace_bytes(p), query, ACINO_ERR_WORKSPACE)) return rc;
  SkelDev* dev = reinterpret_cast<SkelDev*>(d_ws);
  d_dev = dev;
  return skel_upload(h, nullptr, 0, dev, reinterpret_cast<SkelClip*>(reinterpret_cast<char*>(d_ws) + spf_ws_clip()), 1, s);
}

// one frame per workgroup pass, grid-stride beyond the cap; the 160 KB opt-in once per device and kernel (``attr``: its static)
template <class K, class Args>
inline int spf_launch(K kernel, PerDeviceOnce& attr, int64_t n_frames, size_t lds, hipStream_t s, const Args& a) {
  if (attr.first())
    ACINO_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                        (int)SPF_LDS_MAX));
  hipLaunchKernelGGL(kernel, dim3(grid_for(n_frames, 1)), dim3(64), lds, s, a);
  ACINO_LAUNCH_CHECK();
  return ACINO_OK;
}

}  // namespace acino
