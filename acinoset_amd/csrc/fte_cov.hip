// Posterior (Laplace) covariance of an FTE trajectory (gfx950, fp64 matrix cores).
//
//   A = blockdiag(H_n) + 2 q (x) D3^T D3      at the context's CURRENT iterate, no Marquardt term; bound-active variables
//                                             pinned (row and column zeroed, diagonal 1) - oracle.fte.solve_banded, lam = 0
//
// is the Gauss-Newton Hessian of the objective F the solve minimises, with its IRLS weights.  The loss is rho(e) = e^2 / 2
// near 0 (common.hpp: redescending) on residuals scaled by 1 / R_meas, the prior q d^2 with q = 1 / (Q_sigma^2 Ts^4): F is a
// negative log-posterior AS IT STANDS, and A^-1 is its Laplace covariance with NO further factor - rad^2 for the angles, m^2
// for the head position and for the marker positions.
//
// A is block tridiagonal in nodes of 3 frames (75 unknowns, identity padding to 80; a ragged last node is padded the same
// way), every clip on a node grid of its own.  With D_k the diagonal blocks and E_k = A[node k, node k + 1] (the constant
// third-difference stencil: <= 3 terms per entry, diagonal in the state index)
//
//   forward   F_0 = D_0,   F_k+1 = D_k+1 - E_k^T F_k^-1 E_k           k_fte_cov_sweep, workgroup (clip, 0)
//   backward  B_M-1 = D_M-1, B_k-1 = D_k-1 - E_k-1 B_k^-1 E_k-1^T     k_fte_cov_sweep, workgroup (clip, 1), concurrently
//   combine   Sigma_k = (A^-1)_kk = (F_k + B_k - D_k)^-1              k_fte_cov_combine, one workgroup per node
//
// exactly (no truncation, no halo).  The sweeps store, per node, the correction they SUBTRACTED (CF_k = E^T F_k-1^-1 E,
// CB_k = E B_k+1^-1 E^T; lower tiles), and the combine forms D_k - CF_k - CB_k from them - F_k + B_k - D_k without ever
// adding and subtracting D_k.  Per node of a sweep: the node in LDS, chol80 (U = L^-T), W = U^T E (a column of W is a
// combination of <= 3 rows of U), then the correction W^T W on the matrix cores.  NOT E^T (U U^T) E: the explicit inverse
// carries an error of cond(F) eps, and D - E^T G E cancels - a last node of ONE frame lost 5 digits that way (7e-6 at 7
// frames, 5e-8 at 121; the numpy restatement shows the same), W^T W is as good as a banded Cholesky solve (3e-10, the
// references' own spread).  The combine inverts explicitly (G = U U^T is its OUTPUT) and writes the node's three 25 x 25
// diagonal blocks and J_l Sigma J_l^T for the 20 markers of each of its frames, J_l = d FK_l / d x from the rotation axes
// the FK chain leaves behind (cheetah_fk.hpp): column a = omega_a x (p_l - pivot_a) for the angles marker l hangs on, e_a
// for the head position.
//
// k_fte_cov_rates (below the combine) reads the same corrections for the covariance of dx, ddx and the marker velocities.
// The sampler (k_fte_sample_factors, k_fte_sample_backsub) and the column solve (k_fte_sample_fwdsub) follow further down.
//
// No workgroup waits for another inside a kernel; a non-positive pivot sets the error word (chol80) and NaNs run through
// the remaining nodes - no trap, no abort.  A translation unit of its own: nothing here is shared with the LM step's kernels
// beyond the device functions of dense80.hpp / bcr_dev.hpp, which stay as they are.
#include "fte_cov.hpp"
#include "fte_cov_dev.hpp"

namespace acino {

CovGrid cov_grid(int64_t n_frames, int64_t clip_len) {
  CovGrid g;
  g.clip = clip_len > 0 ? clip_len : n_frames;
  g.n_clips = (int)(n_frames / g.clip);
  g.nodes_per_clip = (int)((g.clip + 2) / 3);
  return g;
}

size_t cov_workspace_bytes(int64_t n_frames, int64_t clip_len) {
  const CovGrid g = cov_grid(n_frames, clip_len);
  return COV_HEAD_BYTES + 2 * (size_t)g.n_nodes() * COV_TERM_DOUBLES * sizeof(double);
}

namespace {

struct CovArgs {
  const FteConst* cst;
  const acino_fte_state* st;
  const double *x0, *x1, *g0, *g1, *H0, *H1;
  double* terms;           // [2][n_nodes][COV_TERM_DOUBLES]: CF, then CB
  int* err;
  int n_clips, nodes_per_clip;
  long long clip;
  double *cov_x, *cov_pos, *std_pos;
  double *cov_dx, *cov_ddx, *cov_vel, *std_vel;   // k_fte_cov_rates
  double inv_ts;
};

__device__ __forceinline__ CovIn cov_inputs(const CovArgs& A) {
  const int cur = A.st->cur;
  return CovIn{cur ? A.x1 : A.x0, cur ? A.g1 : A.g0, cur ? A.H1 : A.H0};
}

constexpr int COV_TAB = 232;                                        // 9 * NP doubles, padded
constexpr size_t COV_LDS = (2 * MAT + COV_TAB) * sizeof(double) + 2 * BS * sizeof(int);

// D_k into Lm (ACC: on top of what is there), both triangles.  r0: the node's first frame counted inside its clip.
template <bool ACC>
__device__ __forceinline__ void cov_fill(double* Lm, const int* code, const CovIn& in, const FteConst& K, int64_t f0,
                                         int64_t r0, int64_t clip, int tid) {
  for (int e = tid; e < BS * BS; e += 256) {
    const int r = e / BS, c = e % BS;
    double v = 0.0;
    if (code[r] | code[c]) {
      v = r == c ? 1.0 : 0.0;
    } else {
      const int fr = r / NP, p = r % NP, fc = c / NP, q = c % NP;
      if (fr == fc) v = in.H[(f0 + fr) * HPAIRS + hpair(p, q)];
      else if (p == q) v = 2.0 * K.q_w[p] * band_coef(r0 + (fr < fc ? fr : fc), fr < fc ? fc - fr : fr - fc, clip);
    }
    Lm[r * LD + c] = ACC ? Lm[r * LD + c] + v : v;
  }
}

// G = U U^T from the factor chol80 left in Lm (U in the diagonal and strictly-upper tiles), all 80 x 80 entries of Gm
__device__ __forceinline__ void cov_gram(double* Gm, const double* Lm, int wave, int lane) {
  const int li = lane & 15, lk = lane >> 4;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int t = wave + 4 * q;
    if (t < 15) {
      const int ib = tri_i(t), jb = tri_j(t);
      const double* pa = Lm + (ib * 16 + li) * LD + ib * 16 + lk;   // U(ib, k >= ib)[i][kk]
      const double* pb = Lm + (jb * 16 + li) * LD + ib * 16 + lk;   // U(jb, k >= ib)[j][kk]
      d4 acc = {0, 0, 0, 0};
      switch (ib) {
        case 0: acc = mma_seq<20, false>(acc, pa, 4, pb, 4); break;
        case 1: acc = mma_seq<16, false>(acc, pa, 4, pb, 4); break;
        case 2: acc = mma_seq<12, false>(acc, pa, 4, pb, 4); break;
        case 3: acc = mma_seq<8, false>(acc, pa, 4, pb, 4); break;
        default: acc = mma_seq<4, false>(acc, pa, 4, pb, 4); break;
      }
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        Gm[(ib * 16 + lk + 4 * rr) * LD + jb * 16 + li] = acc[rr];
        if (ib != jb) Gm[(jb * 16 + li) * LD + ib * 16 + lk + 4 * rr] = acc[rr];
      }
    }
  }
}

}  // namespace

// grid = 2 * n_clips: workgroup (clip, direction).  Walks the clip's nodes; stores the correction of every node it enters.
// FWD_ONLY (the sampler, below): grid = n_clips, the forward direction alone - the same code, CF_k the same bits.
template <bool FWD_ONLY>
__global__ void __launch_bounds__(256) k_fte_cov_sweep(CovArgs A) {
  extern __shared__ __attribute__((aligned(16))) double cov_smem[];
  double* Lm = cov_smem;
  double* Gm = Lm + MAT;
  double* wtab = Gm + MAT;                          // [(s * 3 + t) * NP + p]: coupling of source frame s with target frame t
  int* code = reinterpret_cast<int*>(wtab + COV_TAB);
  int* coden = code + BS;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int clip_i = FWD_ONLY ? (int)blockIdx.x : (int)blockIdx.x >> 1, back = FWD_ONLY ? 0 : (int)blockIdx.x & 1;
  if (clip_i >= A.n_clips) return;
  const FteConst& K = *A.cst;
  const CovIn in = cov_inputs(A);
  const int M = A.nodes_per_clip;
  const int64_t clip = A.clip, fclip = (int64_t)clip_i * clip;
  const size_t n_nodes = (size_t)A.n_clips * M;
  int k = back ? M - 1 : 0;
  {
    const int64_t r0 = 3 * (int64_t)k;
    cov_codes(code, in, K, fclip + r0, (int)min((int64_t)3, clip - r0), tid);
    __syncthreads();
    cov_fill<false>(Lm, code, in, K, fclip + r0, r0, clip, tid);
  }
  for (int step = 0; step + 1 < M; ++step) {
    const int kn = back ? k - 1 : k + 1;
    const int64_t rs = 3 * (int64_t)k, rn = 3 * (int64_t)kn;
    cov_codes(coden, in, K, fclip + rn, (int)min((int64_t)3, clip - rn), tid);
    __syncthreads();
    // the stencil between node k (source, frames rs + s) and node kn (target, frames rn + t), pinned variables uncoupled
    for (int e = tid; e < 9 * NP; e += 256) {
      const int s = e / (3 * NP), t = (e / NP) % 3, p = e % NP;
      const int dist = back ? 3 + s - t : 3 + t - s;               // frames between the two, > 3: not coupled
      double v = 0.0;
      if (dist <= 3 && code[s * NP + p] == 0 && coden[t * NP + p] == 0)
        v = 2.0 * K.q_w[p] * band_coef(back ? rn + t : rs + s, dist, clip);
      wtab[e] = v;
    }
    chol80(Lm, tid, A.err);
    // W = U^T E, stored transposed: row (t, p) of Wt is a combination of <= 3 ROWS of U (upper triangular: the lower tiles
    // of Lm hold L and are masked out).  Rows 75 .. 79 are zero.
    for (int e = tid; e < BS * BS; e += 256) {
      const int c = e / BS, r = e % BS;
      double v = 0.0;
      if (c < 3 * NP) {
        const int t = c / NP, p = c % NP;
#pragma unroll
        for (int s = 0; s < 3; ++s) {
          const int i = s * NP + p;
          v += r >= i ? wtab[(s * 3 + t) * NP + p] * Lm[i * LD + r] : 0.0;
        }
      }
      Gm[c * LD + r] = v;
    }
    __syncthreads();
    // Lm <- -(W^T W) = -(E^T F^-1 E): the 15 lower tiles on the matrix cores, mirrored
    {
      const int li = lane & 15, lk = lane >> 4;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int t = wave + 4 * q;
        if (t < 15) {
          const int ib = tri_i(t), jb = tri_j(t);
          d4 acc = {0, 0, 0, 0};
          acc = mma_seq<20, false>(acc, Gm + (ib * 16 + li) * LD + lk, 4, Gm + (jb * 16 + li) * LD + lk, 4);
#pragma unroll
          for (int rr = 0; rr < 4; ++rr) {
            Lm[(ib * 16 + lk + 4 * rr) * LD + jb * 16 + li] = -acc[rr];
            if (ib != jb) Lm[(jb * 16 + li) * LD + ib * 16 + lk + 4 * rr] = -acc[rr];
          }
        }
      }
    }
    __syncthreads();
    double2* dst = reinterpret_cast<double2*>(A.terms + ((size_t)back * n_nodes + (size_t)clip_i * M + kn) * COV_TERM_DOUBLES);
    for (int idx = tid; idx < LOWER_ITEMS; idx += 256) {
      int row, col;
      lower_item(idx, row, col);
      dst[idx] = make_double2(-Lm[row * LD + col], -Lm[row * LD + col + 1]);
    }
    __syncthreads();
    cov_fill<true>(Lm, coden, in, K, fclip + rn, rn, clip, tid);
    int* sw = code;
    code = coden;
    coden = sw;
    k = kn;
  }
}

// grid = n_nodes: Sigma_k = (D_k - CF_k - CB_k)^-1, its three diagonal blocks, the markers' covariances.
__global__ void __launch_bounds__(256) k_fte_cov_combine(CovArgs A) {
  extern __shared__ __attribute__((aligned(16))) double cov_smem[];
  double* Lm = cov_smem;
  double* Gm = Lm + MAT;
  double* tr = Gm + MAT;                             // [60][3] diagonal of the markers' covariances
  int* code = reinterpret_cast<int*>(tr + COV_TAB);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const FteConst& K = *A.cst;
  const CovIn in = cov_inputs(A);
  const int M = A.nodes_per_clip;
  const int node = (int)blockIdx.x, clip_i = node / M, k = node % M;
  const int64_t clip = A.clip, r0 = 3 * (int64_t)k, f0 = (int64_t)clip_i * clip + r0;
  const int nlive = (int)min((int64_t)3, clip - r0);
  const size_t n_nodes = (size_t)A.n_clips * M;
  cov_codes(code, in, K, f0, nlive, tid);
  __syncthreads();
  cov_fill<false>(Lm, code, in, K, f0, r0, clip, tid);
  __syncthreads();
  {
    const bool hf = k > 0, hb = k + 1 < M;
    const double2* cf = reinterpret_cast<const double2*>(A.terms + (size_t)node * COV_TERM_DOUBLES);
    const double2* cb = reinterpret_cast<const double2*>(A.terms + (n_nodes + node) * COV_TERM_DOUBLES);
    for (int idx = tid; idx < LOWER_ITEMS; idx += 256) {
      int row, col;
      lower_item(idx, row, col);
      double2 v = make_double2(0.0, 0.0);
      if (hf) v = cf[idx];
      if (hb) {
        const double2 w = cb[idx];
        v.x += w.x;
        v.y += w.y;
      }
      Lm[row * LD + col] -= v.x;
      Lm[row * LD + col + 1] -= v.y;
      if ((row >> 4) != (col >> 4)) {                // (a diagonal tile holds both of its triangles)
        Lm[col * LD + row] -= v.x;
        Lm[(col + 1) * LD + row] -= v.y;
      }
    }
  }
  __syncthreads();
  chol80(Lm, tid, A.err);
  cov_gram(Gm, Lm, wave, lane);
  __syncthreads();
  // a variable held at its bound has no spread; padding is not an unknown
  for (int e = tid; e < BS * BS; e += 256) {
    const int r = e / BS, c = e % BS;
    if (code[r] | code[c]) Gm[r * LD + c] = 0.0;
  }
  __syncthreads();
  if (A.cov_x) {
    for (int e = tid; e < nlive * NP * NP; e += 256) {
      const int fr = e / (NP * NP), p = (e / NP) % NP, q = e % NP;
      A.cov_x[(f0 + fr) * (NP * NP) + p * NP + q] = Gm[(fr * NP + p) * LD + fr * NP + q];
    }
  }
  if (!A.cov_pos && !A.std_pos) return;
  // ---- markers: FK of the node's frames (Lm is free: the factor is spent), J[fr][l][i][p], J Sigma J^T
  CovFrame* F = reinterpret_cast<CovFrame*>(Lm);
  double* J = Lm + 3 * ((sizeof(CovFrame) + 7) / 8);
  for (int task = tid; task < nlive * NP; task += 256) {
    const int fr = task / NP, a = task % NP;
    const double xv = in.x[(f0 + fr + HALO) * NP + a];
    if (a < 3) {
      F[fr].pos[20][a] = xv;
    } else {
      double s, c;
      sincos(xv, &s, &c);
      F[fr].sc[a - 3][0] = s;
      F[fr].sc[a - 3][1] = c;
    }
  }
  __syncthreads();
  for (int task = tid; task < nlive * 3; task += 256) fk_columns(F[task / 3], task % 3);
  __syncthreads();
  for (int task = tid; task < nlive * NL * NP; task += 256) {
    const int fr = task / (NL * NP), l = (task / NP) % NL, p = task % NP;
    double j0 = 0.0, j1 = 0.0, j2 = 0.0;
    if (p < 3) {
      j0 = p == 0 ? 1.0 : 0.0;
      j1 = p == 1 ? 1.0 : 0.0;
      j2 = p == 2 ? 1.0 : 0.0;
    } else {
      const int ga = c_state_grp[p], gm = cov_marker_grp(l);
      if ((c_ancmask[gm] >> ga) & 1) {
        const double* w = F[fr].om[p - 3];
        const double* c = F[fr].pos[c_grp_pivot[ga]];
        const double* m = F[fr].pos[l];
        const double d0 = m[0] - c[0], d1 = m[1] - c[1], d2 = m[2] - c[2];
        j0 = w[1] * d2 - w[2] * d1;
        j1 = w[2] * d0 - w[0] * d2;
        j2 = w[0] * d1 - w[1] * d0;
      }
    }
    double* Jl = J + (size_t)(fr * NL + l) * 3 * NP;
    Jl[p] = j0;
    Jl[NP + p] = j1;
    Jl[2 * NP + p] = j2;
  }
  __syncthreads();
  if (tid < nlive * NL * 3) {
    const int fr = tid / (NL * 3), l = (tid / 3) % NL, i = tid % 3;
    const double* Jl = J + (size_t)(fr * NL + l) * 3 * NP;
    const double* S = Gm + (fr * NP) * LD + fr * NP;
    double o0 = 0.0, o1 = 0.0, o2 = 0.0;
    for (int q = 0; q < NP; ++q) {
      double t = 0.0;
      for (int p = 0; p < NP; ++p) t += Jl[i * NP + p] * S[p * LD + q];
      o0 += t * Jl[q];
      o1 += t * Jl[NP + q];
      o2 += t * Jl[2 * NP + q];
    }
    if (A.cov_pos) {
      double* out = A.cov_pos + ((f0 + fr) * NL + l) * 9 + 3 * i;
      out[0] = o0;
      out[1] = o1;
      out[2] = o2;
    }
    tr[tid] = i == 0 ? o0 : (i == 1 ? o1 : o2);
  }
  __syncthreads();
  if (A.std_pos && tid < nlive * NL) {
    const int fr = tid / NL, l = tid % NL;
    A.std_pos[(f0 + fr) * NL + l] = sqrt(fmax(tr[3 * tid] + tr[3 * tid + 1] + tr[3 * tid + 2], 0.0));
  }
}

// ---- covariance of dx, ddx and of the marker velocities ----------------------------------------------------------------
// Every output is c Sigma c^T for coefficient rows c over a window of <= 3 consecutive frames, which lies in node k or
// across nodes k - 1 and k.  The two nodes, everything before them eliminated into F_k-1 = D_k-1 - CF_k-1 and everything
// behind them into D_k - CB_k, have the joint precision [[F_k-1, E], [E^T, D_k - CB_k]] whose Schur complement is the
// S_k = D_k - CF_k - CB_k of the combine.  With F_k-1 = L1 L1^T, S_k = L2 L2^T, U = L^-T and c = [c_a | c_b]:
//   Y1 = U1^T c_a^T,   Y2 = U2^T (c_b^T - E^T U1 Y1),   c Sigma c^T = Y1^T Y1 + Y2^T Y2
// - sums of squares from the factors.  NOT differences of blocks of A^-1: neighbouring frames are correlated to 1 - 1e-6
// and the blocks, good to 4e-10 themselves, leave cov_ddx 1.8e-8 off when differenced (numpy, sprint, 120 frames).
// The rows go through in batches of 32 (25 states of one frame; 10 markers x 3), stored as rows (Y^T): every product is
// A B^T on the matrix cores and the batch's Gram matrix stays in the accumulators of the four waves across both terms.
namespace {
constexpr int RB = 32;
constexpr size_t COV_RATES_LDS = (3 * MAT + COV_TAB) * sizeof(double) + 2 * BS * sizeof(int);

// <= 3 window frames with their coefficients; loc = frame counted from the first frame of node k - 1 (0..2: node k - 1,
// 3..5: node k), -1: no such member
struct RateBatch {
  int kind, l0;                                          // 0 dx, 1 ddx, 2 marker velocity; first marker of the batch
  double c0, c1, c2;
  int loc0, loc1, loc2;
};

// entry (row c of the batch, column col of node k - 1 (part 0) / node k (part 1)) of the coefficient matrix.
// F[0]: last frame of node k - 1, F[1 + t]: frame t of node k
__device__ __forceinline__ double rate_coef(const RateBatch& B, const CovFrame* F, int c, int part, int col) {
  if (col >= 3 * NP) return 0.0;
  const int loc = part * 3 + col / NP, p = col % NP;
  const double cm = loc == B.loc0 ? B.c0 : (loc == B.loc1 ? B.c1 : (loc == B.loc2 ? B.c2 : 0.0));
  if (cm == 0.0) return 0.0;
  if (B.kind < 2) return c == p ? cm : 0.0;
  if (c >= 30) return 0.0;
  return cm * rate_jac(F[loc - 2], B.l0 + c / 3, c % 3, p);
}

// out[32][80] = in[32][80] U (UT = false) or in U^T (UT = true); U upper triangular with zeros below
template <bool UT>
__device__ __forceinline__ void rates_mul(double* out, const double* in, const double* U, int wave, int lane) {
  const int li = lane & 15, lk = lane >> 4;
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const int t = wave + 4 * q;
    if (t < 10) {
      const int ib = t / 5, jb = t % 5;
      const double* pa = in + (ib * 16 + li) * LD + lk;
      d4 acc = {0, 0, 0, 0};
      if (UT) acc = mma_seq<20, false>(acc, pa, 4, U + (jb * 16 + li) * LD + lk, 4);
      else acc = mma_seq<20, false>(acc, pa, 4, U + lk * LD + jb * 16 + li, 4 * LD);
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) out[(ib * 16 + lk + 4 * rr) * LD + jb * 16 + li] = acc[rr];
    }
  }
}

// tile (wave >> 1, wave & 1) of Y Y^T, Y[32][80]
__device__ __forceinline__ d4 rates_gram(d4 acc, const double* Y, int wave, int lane) {
  const int li = lane & 15, lk = lane >> 4;
  return mma_seq<20, false>(acc, Y + ((wave >> 1) * 16 + li) * LD + lk, 4, Y + ((wave & 1) * 16 + li) * LD + lk, 4);
}

// Lm -= cf + cb (packed lower tiles; either may be null), both triangles
__device__ __forceinline__ void cov_sub_terms(double* Lm, const double2* cf, const double2* cb, int tid) {
  for (int idx = tid; idx < LOWER_ITEMS; idx += 256) {
    int row, col;
    lower_item(idx, row, col);
    double2 v = make_double2(0.0, 0.0);
    if (cf) v = cf[idx];
    if (cb) {
      const double2 w = cb[idx];
      v.x += w.x;
      v.y += w.y;
    }
    Lm[row * LD + col] -= v.x;
    Lm[row * LD + col + 1] -= v.y;
    if ((row >> 4) != (col >> 4)) {
      Lm[col * LD + row] -= v.x;
      Lm[(col + 1) * LD + row] -= v.y;
    }
  }
}
}  // namespace

// grid = n_nodes: cov_dx, cov_ddx, cov_vel, std_vel of the node's frames.  Reads the corrections the sweeps left.
__global__ void __launch_bounds__(256) k_fte_cov_rates(CovArgs A) {
  extern __shared__ __attribute__((aligned(16))) double cov_smem[];
  double* U1 = cov_smem;                             // factor of F_k-1
  double* U2 = U1 + MAT;                             // factor of S_k
  double* X = U2 + MAT;                              // two batch buffers [32][LD] and the FK of four frames
  double* Z = X + RB * LD;
  CovFrame* F = reinterpret_cast<CovFrame*>(Z + RB * LD);
  static_assert(2 * RB * LD * sizeof(double) + 4 * sizeof(CovFrame) <= MAT * sizeof(double), "batch buffers + FK frames");
  double* wtab = X + MAT;
  int* codep = reinterpret_cast<int*>(wtab + COV_TAB);
  int* code = codep + BS;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const FteConst& K = *A.cst;
  const CovIn in = cov_inputs(A);
  const int M = A.nodes_per_clip;
  const int node = (int)blockIdx.x, clip_i = node / M, k = node % M;
  const int64_t clip = A.clip, r0 = 3 * (int64_t)k, f0 = (int64_t)clip_i * clip + r0;
  const int nlive = (int)min((int64_t)3, clip - r0);
  const size_t n_nodes = (size_t)A.n_clips * M;
  const bool prev = k > 0;
  cov_codes(code, in, K, f0, nlive, tid);
  if (prev) cov_codes(codep, in, K, f0 - 3, 3, tid);
  __syncthreads();
  cov_fill<false>(U2, code, in, K, f0, r0, clip, tid);
  if (prev) {
    cov_fill<false>(U1, codep, in, K, f0 - 3, r0 - 3, clip, tid);
    // E = A[node k - 1, node k] (the sweep's table): source frame s of node k - 1, target frame t of node k
    for (int e = tid; e < 9 * NP; e += 256) {
      const int s = e / (3 * NP), t = (e / NP) % 3, p = e % NP;
      const int dist = 3 + t - s;
      double v = 0.0;
      if (dist <= 3 && codep[s * NP + p] == 0 && code[t * NP + p] == 0) v = 2.0 * K.q_w[p] * band_coef(r0 - 3 + s, dist, clip);
      wtab[e] = v;
    }
  }
  __syncthreads();
  {
    const double2* terms = reinterpret_cast<const double2*>(A.terms);
    const size_t T2 = COV_TERM_DOUBLES / 2;
    cov_sub_terms(U2, prev ? terms + (size_t)node * T2 : nullptr, k + 1 < M ? terms + (n_nodes + node) * T2 : nullptr, tid);
    if (k > 1) cov_sub_terms(U1, terms + (size_t)(node - 1) * T2, nullptr, tid);
  }
  __syncthreads();
  chol80(U2, tid, A.err);
  if (prev) chol80(U1, tid, A.err);
  // keep U alone: the lower tiles hold L, the diagonal tiles leftovers below their diagonal
  for (int e = tid; e < BS * BS; e += 256) {
    const int r = e / BS, c = e % BS;
    if (r > c) {
      U2[r * LD + c] = 0.0;
      if (prev) U1[r * LD + c] = 0.0;
    }
  }
  // FK of the last frame of node k - 1 (slot 0) and of the node's own frames (slots 1 ..)
  const bool vel = A.cov_vel || A.std_vel;
  if (vel) {
    for (int task = tid; task < 4 * NP; task += 256) {
      const int slot = task / NP, a = task % NP;
      if (slot == 0 ? prev : slot - 1 < nlive) {
        const double xv = in.x[(f0 + slot - 1 + HALO) * NP + a];
        if (a < 3) {
          F[slot].pos[20][a] = xv;
        } else {
          double s, c;
          sincos(xv, &s, &c);
          F[slot].sc[a - 3][0] = s;
          F[slot].sc[a - 3][1] = c;
        }
      }
    }
    __syncthreads();
    if (tid < 12) {
      const int slot = tid / 3;
      if (slot == 0 ? prev : slot - 1 < nlive) fk_columns(F[slot], tid % 3);
    }
  }
  __syncthreads();
  const double it = A.inv_ts;
  for (int b = 0; b < 12; ++b) {
    RateBatch B;
    const int j = b < 6 ? b >> 1 : (b - 6) >> 1;
    B.kind = b < 6 ? b & 1 : 2;
    B.l0 = b < 6 ? 0 : ((b - 6) & 1) * 10;
    if (j >= nlive) continue;
    if (B.kind == 0 ? !A.cov_dx : (B.kind == 1 ? !A.cov_ddx : !vel)) continue;
    // the window (first frame w0 inside the clip) and its coefficients: k_derivatives with its start-up rules
    const int64_t n = r0 + j;
    int64_t w0 = 0;
    B.c0 = B.c1 = B.c2 = 0.0;
    if (B.kind < 2) {
      if (clip >= 3) {
        w0 = n >= 2 ? n - 2 : 0;
        if (B.kind == 1) {
          B.c0 = it * it;
          B.c1 = -2.0 * it * it;
          B.c2 = it * it;
        } else if (n >= 2) {
          B.c1 = -it;
          B.c2 = it;
        } else if (n == 1) {
          B.c0 = -it;
          B.c1 = it;
        } else {                                       // dx_0 = dx_1 - Ts ddx_2
          B.c0 = -2.0 * it;
          B.c1 = 3.0 * it;
          B.c2 = -it;
        }
      } else if (clip == 2 && B.kind == 0) {           // dx_0 = dx_1, ddx = 0
        B.c0 = -it;
        B.c1 = it;
      }
    } else if (clip >= 2) {                            // v_n from frames n - 1, n; frame 0 repeats frame 1
      w0 = (n >= 1 ? n : 1) - 1;
      B.c0 = -it;
      B.c1 = it;
    }
    const int base = (int)(w0 - (r0 - 3));
    B.loc0 = B.c0 != 0.0 ? base : -1;
    B.loc1 = B.c1 != 0.0 ? base + 1 : -1;
    B.loc2 = B.c2 != 0.0 ? base + 2 : -1;
    const bool need_a = prev && ((B.loc0 >= 0 && B.loc0 < 3) || (B.loc1 >= 0 && B.loc1 < 3) || (B.loc2 >= 0 && B.loc2 < 3));
    d4 gacc = {0, 0, 0, 0};
    if (need_a) {
      if (B.kind < 2) {
        // Y1^T = c_a U1 directly: a row combines <= 3 rows of U1 (the pattern of W = U^T E in the sweep)
        for (int e = tid; e < RB * BS; e += 256) {
          const int c = e / BS, r = e % BS;
          double v = 0.0;
          if (c < NP) {
#pragma unroll
            for (int s = 0; s < 3; ++s) {
              const double cm = s == B.loc0 ? B.c0 : (s == B.loc1 ? B.c1 : (s == B.loc2 ? B.c2 : 0.0));
              const int i = s * NP + c;
              if (cm != 0.0 && codep[i] == 0) v += cm * U1[i * LD + r];
            }
          }
          Z[c * LD + r] = v;
        }
      } else {
        for (int e = tid; e < RB * BS; e += 256) {
          const int c = e / BS, col = e % BS;
          X[c * LD + col] = codep[col] == 0 ? rate_coef(B, F, c, 0, col) : 0.0;
        }
        __syncthreads();
        rates_mul<false>(Z, X, U1, wave, lane);
      }
      __syncthreads();
      gacc = rates_gram(gacc, Z, wave, lane);
      rates_mul<true>(X, Z, U1, wave, lane);           // (U1 Y1)^T
      __syncthreads();
    }
    // (c_b^T - E^T U1 Y1)^T
    for (int e = tid; e < RB * BS; e += 256) {
      const int c = e / BS, col = e % BS;
      double v = code[col] == 0 ? rate_coef(B, F, c, 1, col) : 0.0;
      if (need_a && col < 3 * NP) {
        const int t = col / NP, p = col % NP;
#pragma unroll
        for (int s = 0; s < 3; ++s) v -= X[c * LD + s * NP + p] * wtab[(s * 3 + t) * NP + p];
      }
      Z[c * LD + col] = v;
    }
    __syncthreads();
    rates_mul<false>(X, Z, U2, wave, lane);            // Y2^T
    __syncthreads();
    gacc = rates_gram(gacc, X, wave, lane);
    {
      const int li = lane & 15, lk = lane >> 4;
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) Z[((wave >> 1) * 16 + lk + 4 * rr) * LD + (wave & 1) * 16 + li] = gacc[rr];
    }
    __syncthreads();
    if (B.kind < 2) {
      double* out = (B.kind ? A.cov_ddx : A.cov_dx) + (f0 + j) * (NP * NP);
      for (int e = tid; e < NP * NP; e += 256) out[e] = Z[(e / NP) * LD + e % NP];
    } else {
      if (A.cov_vel && tid < 90) {
        const int ll = tid / 9, i = (tid / 3) % 3, i2 = tid % 3;
        A.cov_vel[((f0 + j) * NL + B.l0 + ll) * 9 + 3 * i + i2] = Z[(3 * ll + i) * LD + 3 * ll + i2];
      }
      if (A.std_vel && tid < 10) {
        const int d = 3 * tid;
        A.std_vel[(f0 + j) * NL + B.l0 + tid] =
            sqrt(fmax(Z[d * LD + d] + Z[(d + 1) * LD + d + 1] + Z[(d + 2) * LD + d + 2], 0.0));
      }
    }
    __syncthreads();
  }
}

// ---- joint samples of the whole trajectory: delta = L^-T z, A = L L^T ---------------------------------------------------
// The forward pivots F_k = D_k - CF_k = L_k L_k^T are the diagonal blocks of the Cholesky factor of A (frame-major order;
// the identity padding decouples), W_k^T = E_k^T U_k its sub-diagonal blocks, U_k = L_k^-T.  Backward substitution:
//   delta_last = U_last z_last,   delta_k = U_k (z_k - U_k^T (E_k delta_k+1))
// - products of the triangular factors only (the rule of the sweeps: never G = U U^T on E delta).  Three launches:
// k_fte_cov_sweep<true> (one workgroup per clip) leaves CF_k; k_fte_sample_factors, one workgroup per node, all in
// parallel, stores U_k^T = L_k^-1 as its 15 lower tiles in the CB half of the workspace (which the forward-only sweep does
// not write); k_fte_sample_backsub, grid (clips, panels of 64 samples), walks the nodes from last to first.
// A fourth kernel uses the same factors for whole solves A^-1 B (launch_fte_solve_columns, further down; the extrinsic
// sensitivity of fte_calib.hip): k_fte_sample_fwdsub, the forward substitution L y = b on the same grid, walks the nodes from
// first to last, and k_fte_sample_backsub<true> then writes L^-T y without x_hat.
namespace {
struct SampleIo {
  const double* z;                                       // [S][N][25]
  double* xs;                                            // [S][N][25]
  long long n_samples, n_frames;
};
constexpr int SPB = 64;                                  // samples per panel: one 16-sample row tile per wave
constexpr size_t SAMPLE_FACT_LDS = MAT * sizeof(double) + BS * sizeof(int);
constexpr size_t SAMPLE_LDS = (MAT + 2 * SPB * LD + COV_TAB) * sizeof(double) + 2 * BS * sizeof(int);

// Samples are held as ROWS (16 per wave, leading dimension LD); Lt = U^T = L^-1, lower triangular, its upper tiles never
// read.  Column tile JB of  in U:  k runs over the tile rows 0 .. JB of U alone (the zero half is skipped).
template <int JB>
__device__ __forceinline__ d4 sample_mul_u(const double* in, const double* Lt, int li, int lk) {
  d4 acc = {0, 0, 0, 0};
  return mma_seq<4 * (JB + 1), false>(acc, in + li * LD + lk, 4, Lt + (JB * 16 + li) * LD + lk, 4);
}
// Column tile IB of  in U^T:  k runs over the tile columns IB .. 4 of U.
template <int IB>
__device__ __forceinline__ d4 sample_mul_ut(const double* in, const double* Lt, int li, int lk) {
  d4 acc = {0, 0, 0, 0};
  return mma_seq<4 * (NT - IB), false>(acc, in + li * LD + IB * 16 + lk, 4, Lt + (IB * 16 + lk) * LD + IB * 16 + li, 4 * LD);
}

struct SampleNode {
  const double* xhat;                                    // the iterate, halo rows included
  const int* code;
  double* xs;
  long long n_samples, n_frames, s_first, f0;            // s_first: the wave's first sample; f0: the node's first frame
  int nlive;
};

// W = z - V U (V = E delta_k+1 as rows; FIRST: the clip's last node, W = z), tile JB of the wave's 16 rows
template <int JB, bool FIRST>
__device__ __forceinline__ void sample_w_tile(double* W, const double* V, const double* Lt, const double (&zv)[4],
                                              const int* code, int li, int lk) {
  d4 acc = {0, 0, 0, 0};
  if (!FIRST) acc = sample_mul_u<JB>(V, Lt, li, lk);
  const int c = JB * 16 + li;
  const bool free_var = code[c] == 0;
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) W[(lk + 4 * rr) * LD + c] = (free_var ? zv[rr] : 0.0) - acc[rr];
}

// delta = W U^T, tile IB: kept as rows for the next node and written out as x_hat + delta for the node's live frames
// (DELTA: as delta alone, exactly 0 for a pinned variable - the solve of launch_fte_solve_columns)
template <int IB, bool DELTA>
__device__ __forceinline__ void sample_d_tile(double* D, const double* W, const double* Lt, const SampleNode& nd, int li,
                                              int lk) {
  const d4 acc = sample_mul_ut<IB>(W, Lt, li, lk);
  const int c = IB * 16 + li;
  const bool out = c < 3 * NP && c / NP < nd.nlive;
  const bool free_var = nd.code[c] == 0;
  const double xh = (out && !DELTA) ? nd.xhat[(nd.f0 + c / NP + HALO) * NP + c % NP] : 0.0;
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    D[(lk + 4 * rr) * LD + c] = acc[rr];
    const long long s = nd.s_first + lk + 4 * rr;
    if (DELTA) {
      if (out && s < nd.n_samples) nd.xs[(s * nd.n_frames + nd.f0) * NP + c] = free_var ? acc[rr] : 0.0;
    } else {
      if (out && s < nd.n_samples) nd.xs[(s * nd.n_frames + nd.f0) * NP + c] = free_var ? xh + acc[rr] : xh;
    }
  }
}
}  // namespace

// grid = n_nodes: F_k = D_k - CF_k, chol80, U_k^T -> the CB slot of the node (packed lower tiles, zeros above the diagonal)
__global__ void __launch_bounds__(256) k_fte_sample_factors(CovArgs A) {
  extern __shared__ __attribute__((aligned(16))) double cov_smem[];
  double* Lm = cov_smem;
  int* code = reinterpret_cast<int*>(Lm + MAT);
  const int tid = threadIdx.x;
  const FteConst& K = *A.cst;
  const CovIn in = cov_inputs(A);
  const int M = A.nodes_per_clip;
  const int node = (int)blockIdx.x, clip_i = node / M, k = node % M;
  if (clip_i >= A.n_clips) return;
  const int64_t clip = A.clip, r0 = 3 * (int64_t)k, f0 = (int64_t)clip_i * clip + r0;
  const size_t n_nodes = (size_t)A.n_clips * M;
  cov_codes(code, in, K, f0, (int)min((int64_t)3, clip - r0), tid);
  __syncthreads();
  cov_fill<false>(Lm, code, in, K, f0, r0, clip, tid);
  __syncthreads();
  if (k > 0) {
    cov_sub_terms(Lm, reinterpret_cast<const double2*>(A.terms + (size_t)node * COV_TERM_DOUBLES), nullptr, tid);
    __syncthreads();
  }
  chol80(Lm, tid, A.err);
  double2* dst = reinterpret_cast<double2*>(A.terms + (n_nodes + node) * COV_TERM_DOUBLES);
  for (int idx = tid; idx < LOWER_ITEMS; idx += 256) {
    int row, col;
    lower_item(idx, row, col);                           // U^T[row][col] = U[col][row]; a diagonal tile holds leftovers below U
    dst[idx] = make_double2(col <= row ? Lm[col * LD + row] : 0.0, col + 1 <= row ? Lm[(col + 1) * LD + row] : 0.0);
  }
}

// grid = (n_clips, panels): the backward substitution of one clip for 64 samples, wave w the samples 16 w .. 16 w + 15 of
// the panel.  A wave reads and writes its own rows of the two panel buffers only; the barriers order the shared factor,
// stencil table and codes.  U_k-1's tiles are requested into registers while node k computes.
// DELTA = false: the sampler (xs = x_hat + delta); true: xs = delta (the second half of a solve A^-1 b).
template <bool DELTA>
__global__ void __launch_bounds__(256) k_fte_sample_backsub(CovArgs A, SampleIo io) {
  extern __shared__ __attribute__((aligned(16))) double cov_smem[];
  double* Lt = cov_smem;
  double* P0 = Lt + MAT;
  double* P1 = P0 + SPB * LD;
  double* wtab = P1 + SPB * LD;                          // [(s * 3 + t) * NP + p]: frame s of node k with frame t of node k + 1
  int* code = reinterpret_cast<int*>(wtab + COV_TAB);
  int* coden = code + BS;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, lk = lane >> 4;
  const int clip_i = (int)blockIdx.x;
  if (clip_i >= A.n_clips) return;
  const FteConst& K = *A.cst;
  const CovIn in = cov_inputs(A);
  const int M = A.nodes_per_clip;
  const int64_t clip = A.clip, fclip = (int64_t)clip_i * clip;
  const size_t n_nodes = (size_t)A.n_clips * M;
  const long long S = io.n_samples, N = io.n_frames;
  const long long s_first = (long long)blockIdx.y * SPB + 16 * wave;
  const bool live = s_first < S;                         // (wave-uniform; a dead wave only keeps the barriers)
  double* Wb = P0 + 16 * wave * LD;                      // W, then the next node's delta source ...
  double* Db = P1 + 16 * wave * LD;                      // ... and back: the two trade places every node
  const double2* ut = reinterpret_cast<const double2*>(A.terms + (n_nodes + (size_t)clip_i * M) * COV_TERM_DOUBLES);
  constexpr int NQ = (LOWER_ITEMS + 255) / 256;
  constexpr size_t T2 = COV_TERM_DOUBLES / 2;
  double2 uf[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int idx = tid + 256 * q;
    if (idx < LOWER_ITEMS) uf[q] = ut[(size_t)(M - 1) * T2 + idx];
  }
  for (int k = M - 1; k >= 0; --k) {
    const int64_t r0 = 3 * (int64_t)k, f0 = fclip + r0;
    const int nlive = (int)min((int64_t)3, clip - r0);
    const bool first = k + 1 == M;
    cov_codes(code, in, K, f0, nlive, tid);
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int idx = tid + 256 * q;
      if (idx < LOWER_ITEMS) {
        int row, col;
        lower_item(idx, row, col);
        Lt[row * LD + col] = uf[q].x;
        Lt[row * LD + col + 1] = uf[q].y;
      }
    }
    if (k > 0) {
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const int idx = tid + 256 * q;
        if (idx < LOWER_ITEMS) uf[q] = ut[(size_t)(k - 1) * T2 + idx];
      }
    }
    double zv[NT][4];
#pragma unroll
    for (int jb = 0; jb < NT; ++jb) {
      const int c = jb * 16 + li;
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const long long s = s_first + lk + 4 * rr;
        zv[jb][rr] = (s < S && c < 3 * NP && c / NP < nlive) ? io.z[(s * N + f0) * NP + c] : 0.0;
      }
    }
    __syncthreads();
    if (!first) {
      for (int e = tid; e < 9 * NP; e += 256) {
        const int s = e / (3 * NP), t = (e / NP) % 3, p = e % NP;
        const int dist = 3 + t - s;
        double v = 0.0;
        if (dist <= 3 && code[s * NP + p] == 0 && coden[t * NP + p] == 0) v = 2.0 * K.q_w[p] * band_coef(r0 + s, dist, clip);
        wtab[e] = v;
      }
      __syncthreads();
      if (live) {                                        // V = E_k delta_k+1, <= 3 stencil terms per entry
        for (int e = lane; e < 16 * BS; e += 64) {
          const int sl = e / BS, r = e % BS;
          double v = 0.0;
          if (r < 3 * NP) {
            const int fr = r / NP, p = r % NP;
#pragma unroll
            for (int t = 0; t < 3; ++t) v += wtab[(fr * 3 + t) * NP + p] * Wb[sl * LD + t * NP + p];
          }
          Db[sl * LD + r] = v;
        }
      }
      __syncthreads();
    }
    if (live) {
      if (first) {
        sample_w_tile<0, true>(Wb, Db, Lt, zv[0], code, li, lk);
        sample_w_tile<1, true>(Wb, Db, Lt, zv[1], code, li, lk);
        sample_w_tile<2, true>(Wb, Db, Lt, zv[2], code, li, lk);
        sample_w_tile<3, true>(Wb, Db, Lt, zv[3], code, li, lk);
        sample_w_tile<4, true>(Wb, Db, Lt, zv[4], code, li, lk);
      } else {
        sample_w_tile<0, false>(Wb, Db, Lt, zv[0], code, li, lk);
        sample_w_tile<1, false>(Wb, Db, Lt, zv[1], code, li, lk);
        sample_w_tile<2, false>(Wb, Db, Lt, zv[2], code, li, lk);
        sample_w_tile<3, false>(Wb, Db, Lt, zv[3], code, li, lk);
        sample_w_tile<4, false>(Wb, Db, Lt, zv[4], code, li, lk);
      }
    }
    __syncthreads();
    if (live) {
      const SampleNode nd{in.x, code, io.xs, S, N, s_first, f0, nlive};
      sample_d_tile<0, DELTA>(Db, Wb, Lt, nd, li, lk);
      sample_d_tile<1, DELTA>(Db, Wb, Lt, nd, li, lk);
      sample_d_tile<2, DELTA>(Db, Wb, Lt, nd, li, lk);
      sample_d_tile<3, DELTA>(Db, Wb, Lt, nd, li, lk);
      sample_d_tile<4, DELTA>(Db, Wb, Lt, nd, li, lk);
    }
    {                                                    // delta_k is the next node's source; this node's codes its neighbour's
      double* sw = Wb;
      Wb = Db;
      Db = sw;
      int* sc = code;
      code = coden;
      coden = sc;
    }
    __syncthreads();
  }
}

namespace {
// The arguments every kernel here takes: inputs, error word, corrections and node grid; no output, inv_ts = 1.
CovArgs cov_args(const PostIn& in, void* d_ws) {
  const CovGrid gr = cov_grid(in.h_c->n_frames, in.h_c->clip_len);
  CovArgs A = {};
  A.cst = in.d_c;
  A.st = in.d_st;
  A.x0 = in.x[0];
  A.x1 = in.x[1];
  A.g0 = in.g[0];
  A.g1 = in.g[1];
  A.H0 = in.H[0];
  A.H1 = in.H[1];
  A.err = reinterpret_cast<int*>(d_ws);
  A.terms = reinterpret_cast<double*>(reinterpret_cast<char*>(d_ws) + COV_HEAD_BYTES);
  A.n_clips = gr.n_clips;
  A.nodes_per_clip = gr.nodes_per_clip;
  A.clip = gr.clip;
  A.inv_ts = 1.0;
  return A;
}

unsigned cov_nodes(const CovArgs& A) { return (unsigned)((int64_t)A.n_clips * A.nodes_per_clip); }

// What the sampler and the column solve start with: the error word cleared, CF_k from the forward sweep, U_k^T of every node
int sample_factors(const CovArgs& A, hipStream_t s) {
  ACINO_HIP_CHECK(set_dyn_lds(k_fte_cov_sweep<true>, COV_LDS));
  ACINO_HIP_CHECK(hipMemsetAsync(A.err, 0, COV_HEAD_BYTES, s));
  if (A.nodes_per_clip > 1) {
    hipLaunchKernelGGL(k_fte_cov_sweep<true>, dim3(A.n_clips), dim3(256), COV_LDS, s, A);
    ACINO_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_fte_sample_factors, dim3(cov_nodes(A)), dim3(256), SAMPLE_FACT_LDS, s, A);
  ACINO_LAUNCH_CHECK();
  return ACINO_OK;
}
}  // namespace

int launch_fte_sample(const PostIn& in, void* d_ws, int64_t n_samples, const double* d_z, double* d_x_samples, hipStream_t s) {
  const CovArgs A = cov_args(in, d_ws);
  const SampleIo io{d_z, d_x_samples, (long long)n_samples, (long long)in.h_c->n_frames};
  const int64_t panels = (n_samples + SPB - 1) / SPB;
  ACINO_HIP_CHECK(set_dyn_lds(k_fte_sample_backsub<false>, SAMPLE_LDS));
  if (int rc = sample_factors(A, s)) return rc;
  hipLaunchKernelGGL(k_fte_sample_backsub<false>, dim3((unsigned)A.n_clips, (unsigned)panels), dim3(256), SAMPLE_LDS, s, A, io);
  ACINO_LAUNCH_CHECK();
  return ACINO_OK;
}

// ---- A^-1 B for panels of right-hand sides: forward substitution, then the sampler's backward substitution ------------
// With A = L L^T and the factors above, L y = b is
//   y_0 = U_0^T b_0,   y_k+1 = U_k+1^T (b_k+1 - E_k^T (U_k y_k))
// - again products of the triangular factors only (never G = U U^T on a right-hand side) -, and k_fte_sample_backsub<true>
// on y gives L^-T y = A^-1 b.  k_fte_sample_fwdsub is the mirror image of the backward substitution: grid (n_clips,
// panels of 64 columns), the columns held as ROWS, 16 per wave, a wave reading and writing its own rows of the two panel
// buffers only, U_k+1's tiles requested into registers while node k computes.  b of a pinned variable counts as 0 (y and
// the solution are exactly 0 there).  No pivot is taken here: the error word is the factors'.
namespace {
// y = W U, tile JB of the wave's 16 rows: kept as rows for the next product and written out for the node's live frames
template <int JB>
__device__ __forceinline__ void fwd_y_tile(double* Y, const double* W, const double* Lt, const int* code, const SampleIo& io,
                                           long long s_first, long long f0, int nlive, int li, int lk) {
  const d4 acc = sample_mul_u<JB>(W, Lt, li, lk);
  const int c = JB * 16 + li;
  const bool out = c < 3 * NP && c / NP < nlive;
  const bool free_var = code[c] == 0;
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    Y[(lk + 4 * rr) * LD + c] = acc[rr];
    const long long s = s_first + lk + 4 * rr;
    if (out && s < io.n_samples) io.xs[(s * io.n_frames + f0) * NP + c] = free_var ? acc[rr] : 0.0;
  }
}
// T = Y U^T, tile IB
template <int IB>
__device__ __forceinline__ void fwd_t_tile(double* T, const double* Y, const double* Lt, int li, int lk) {
  const d4 acc = sample_mul_ut<IB>(Y, Lt, li, lk);
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) T[(lk + 4 * rr) * LD + IB * 16 + li] = acc[rr];
}
}  // namespace

__global__ void __launch_bounds__(256) k_fte_sample_fwdsub(CovArgs A, SampleIo io) {
  extern __shared__ __attribute__((aligned(16))) double cov_smem[];
  double* Lt = cov_smem;
  double* P0 = Lt + MAT;
  double* P1 = P0 + SPB * LD;
  double* wtab = P1 + SPB * LD;                          // [(s * 3 + t) * NP + p]: frame s of node k - 1 with frame t of node k
  int* code = reinterpret_cast<int*>(wtab + COV_TAB);
  int* codep = code + BS;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, lk = lane >> 4;
  const int clip_i = (int)blockIdx.x;
  if (clip_i >= A.n_clips) return;
  const FteConst& K = *A.cst;
  const CovIn in = cov_inputs(A);
  const int M = A.nodes_per_clip;
  const int64_t clip = A.clip, fclip = (int64_t)clip_i * clip;
  const size_t n_nodes = (size_t)A.n_clips * M;
  const long long S = io.n_samples, N = io.n_frames;
  const long long s_first = (long long)blockIdx.y * SPB + 16 * wave;
  const bool live = s_first < S;                         // (wave-uniform; a dead wave only keeps the barriers)
  double* Tb = P0 + 16 * wave * LD;                      // (U_k-1 y_k-1) as rows, then y_k ...
  double* Wb = P1 + 16 * wave * LD;                      // ... b_k - E^T (U y), then U_k y_k: the two trade places every node
  const double2* ut = reinterpret_cast<const double2*>(A.terms + (n_nodes + (size_t)clip_i * M) * COV_TERM_DOUBLES);
  constexpr int NQ = (LOWER_ITEMS + 255) / 256;
  constexpr size_t T2 = COV_TERM_DOUBLES / 2;
  constexpr int NB = 16 * BS / 64;                       // entries of the wave's 16 x 80 rows per lane
  double2 uf[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int idx = tid + 256 * q;
    if (idx < LOWER_ITEMS) uf[q] = ut[idx];
  }
  for (int k = 0; k < M; ++k) {
    const int64_t r0 = 3 * (int64_t)k, f0 = fclip + r0;
    const int nlive = (int)min((int64_t)3, clip - r0);
    cov_codes(code, in, K, f0, nlive, tid);
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int idx = tid + 256 * q;
      if (idx < LOWER_ITEMS) {
        int row, col;
        lower_item(idx, row, col);
        Lt[row * LD + col] = uf[q].x;
        Lt[row * LD + col + 1] = uf[q].y;
      }
    }
    if (k + 1 < M) {
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const int idx = tid + 256 * q;
        if (idx < LOWER_ITEMS) uf[q] = ut[(size_t)(k + 1) * T2 + idx];
      }
    }
    double bv[NB];                                       // entry e = lane + 64 i of the rows: column sl = e / 80, variable r = e % 80
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int e = lane + 64 * i, sl = e / BS, r = e % BS;
      const long long s = s_first + sl;
      bv[i] = (s < S && r < 3 * NP && r / NP < nlive) ? io.z[(s * N + f0) * NP + r] : 0.0;
    }
    __syncthreads();
    if (k > 0) {
      for (int e = tid; e < 9 * NP; e += 256) {
        const int s = e / (3 * NP), t = (e / NP) % 3, p = e % NP;
        const int dist = 3 + t - s;
        double v = 0.0;
        if (dist <= 3 && codep[s * NP + p] == 0 && code[t * NP + p] == 0) v = 2.0 * K.q_w[p] * band_coef(r0 - 3 + s, dist, clip);
        wtab[e] = v;
      }
      __syncthreads();
    }
    if (live) {                                          // W = b_k - E_k-1^T (U_k-1 y_k-1), <= 3 stencil terms per entry
#pragma unroll
      for (int i = 0; i < NB; ++i) {
        const int e = lane + 64 * i, sl = e / BS, r = e % BS;
        double v = 0.0;
        if (k > 0 && r < 3 * NP) {
          const int t = r / NP, p = r % NP;
#pragma unroll
          for (int s = 0; s < 3; ++s) v += wtab[(s * 3 + t) * NP + p] * Tb[sl * LD + s * NP + p];
        }
        Wb[sl * LD + r] = (code[r] == 0 ? bv[i] : 0.0) - v;
      }
    }
    __syncthreads();
    if (live) {                                          // y_k = U_k^T W as rows: W U; kept for the next product and written out
      fwd_y_tile<0>(Tb, Wb, Lt, code, io, s_first, f0, nlive, li, lk);
      fwd_y_tile<1>(Tb, Wb, Lt, code, io, s_first, f0, nlive, li, lk);
      fwd_y_tile<2>(Tb, Wb, Lt, code, io, s_first, f0, nlive, li, lk);
      fwd_y_tile<3>(Tb, Wb, Lt, code, io, s_first, f0, nlive, li, lk);
      fwd_y_tile<4>(Tb, Wb, Lt, code, io, s_first, f0, nlive, li, lk);
    }
    __syncthreads();
    if (live && k + 1 < M) {                             // U_k y_k as rows: y U^T, the next node's source
      fwd_t_tile<0>(Wb, Tb, Lt, li, lk);
      fwd_t_tile<1>(Wb, Tb, Lt, li, lk);
      fwd_t_tile<2>(Wb, Tb, Lt, li, lk);
      fwd_t_tile<3>(Wb, Tb, Lt, li, lk);
      fwd_t_tile<4>(Wb, Tb, Lt, li, lk);
    }
    {
      double* sw = Tb;
      Tb = Wb;
      Wb = sw;
      int* sc = code;
      code = codep;
      codep = sc;
    }
    __syncthreads();
  }
}

int launch_fte_solve_columns(const PostIn& in, void* d_ws, int64_t n_cols, double* d_b, double* d_y, hipStream_t s) {
  const CovArgs A = cov_args(in, d_ws);
  const SampleIo fwd{d_b, d_y, (long long)n_cols, (long long)in.h_c->n_frames};
  const SampleIo back{d_y, d_b, (long long)n_cols, (long long)in.h_c->n_frames};
  const dim3 grid((unsigned)A.n_clips, (unsigned)((n_cols + SPB - 1) / SPB));
  ACINO_HIP_CHECK(set_dyn_lds(k_fte_sample_fwdsub, SAMPLE_LDS));
  ACINO_HIP_CHECK(set_dyn_lds(k_fte_sample_backsub<true>, SAMPLE_LDS));
  if (int rc = sample_factors(A, s)) return rc;
  hipLaunchKernelGGL(k_fte_sample_fwdsub, grid, dim3(256), SAMPLE_LDS, s, A, fwd);
  ACINO_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_fte_sample_backsub<true>, grid, dim3(256), SAMPLE_LDS, s, A, back);
  ACINO_LAUNCH_CHECK();
  return ACINO_OK;
}

int launch_fte_cov_rates(const PostIn& in, void* d_ws, double* d_cov_x, double* d_cov_pos, double* d_std_pos, double* d_cov_dx,
                         double* d_cov_ddx, double* d_cov_vel, double* d_std_vel, double ts, hipStream_t s) {
  CovArgs A = cov_args(in, d_ws);
  A.cov_x = d_cov_x;
  A.cov_pos = d_cov_pos;
  A.std_pos = d_std_pos;
  A.cov_dx = d_cov_dx;
  A.cov_ddx = d_cov_ddx;
  A.cov_vel = d_cov_vel;
  A.std_vel = d_std_vel;
  A.inv_ts = 1.0 / ts;
  const bool blocks = d_cov_x || d_cov_pos || d_std_pos, rates = d_cov_dx || d_cov_ddx || d_cov_vel || d_std_vel;
  ACINO_HIP_CHECK(set_dyn_lds(k_fte_cov_sweep<false>, COV_LDS));
  ACINO_HIP_CHECK(set_dyn_lds(k_fte_cov_combine, COV_LDS));
  ACINO_HIP_CHECK(hipMemsetAsync(d_ws, 0, COV_HEAD_BYTES, s));
  if (A.nodes_per_clip > 1) {
    hipLaunchKernelGGL(k_fte_cov_sweep<false>, dim3(2 * A.n_clips), dim3(256), COV_LDS, s, A);
    ACINO_LAUNCH_CHECK();
  }
  if (blocks) {
    hipLaunchKernelGGL(k_fte_cov_combine, dim3(cov_nodes(A)), dim3(256), COV_LDS, s, A);
    ACINO_LAUNCH_CHECK();
  }
  if (rates) {
    ACINO_HIP_CHECK(set_dyn_lds(k_fte_cov_rates, COV_RATES_LDS));
    hipLaunchKernelGGL(k_fte_cov_rates, dim3(cov_nodes(A)), dim3(256), COV_RATES_LDS, s, A);
    ACINO_LAUNCH_CHECK();
  }
  return ACINO_OK;
}

}  // namespace acino
