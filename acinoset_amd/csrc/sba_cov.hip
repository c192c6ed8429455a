// Error bars of the bundle adjustment: covariance of the camera extrinsics and of every 3-D point at a given iterate.
//
// A = J^T W J of the flat residual (reprojected - points_2d) under the solver's own parametrisation (R <- exp([dw]x) R,
// t <- t + dt, X <- X + dX), W = the Cauchy IRLS weights 1 / (1 + (r / f_scale)^2), NO damping, always fp64.  With every
// camera and point free A has a 7-dimensional null space (world translation, rotation, scale), so the camera covariance
// exists under seven constraints C_g^T d = 0 on the camera parameters only:
//     Sigma_c = N (N^T S N)^-1 N^T,   S = U - sum_p W_p V_p^-1 W_p^T,   N = orthonormal complement of C_g  [6C x (6C - 7)]
//     Sigma_p = V_p^-1 + Y_p Sigma_c Y_p^T,   Y_p = V_p^-1 W_p^T                 (points only: Sigma_p = V_p^-1)
// all multiplied by sigma2 = sum w r^2 / (2 M - dof) unless the caller asks for unit weight.
//
// One code path for 1 .. ACINO_MAX_CAMS cameras, one lane per (point, view) slot: 256 / C points per batch, lane (pl, j) takes
// the j-th observation of its point from the CSR grouping (no slot table).  Three kernels:
//   k_sbacov_lin     linearises at zero damping; per batch the blocks W_pc, Y_pc = W_pc V_p^-1 and the weighted camera rows go
//                    to an LDS slab [point][camera], and every thread keeps up to 36 entries of S in REGISTERS for the whole
//                    kernel, adding the batch's points in point order.  Per-workgroup records, summed in a fixed order by
//                    k_sbacov_reduce (with sum w r^2, the observation and exclusion counts): no floating-point atomics, a
//                    repeated call is bit-identical.
//   k_sbacov_cams    one workgroup: N^T S N in LDS, Cholesky with the pivot test, B = L^-1 N^T, Sigma_c = scale B^T B.
//   k_sbacov_points  the streaming pass: Sigma_c resident in LDS, every lane recomputes its observation, forms Y_a and
//                    Z_a = sum_b Sigma_ab Y_b^T over the views of its point; nothing per observation is written to memory.
// A point whose V_p has an LDL^T pivot <= 3 eps max diag V_p (a single view, or none) carries no information about the
// cameras: it is left out of S, sigma2 and dof and gets NaN.
#include <algorithm>
#include <cmath>
#include <vector>

#include "common.hpp"
#include "sba_dev.hpp"
#include "sba_host.hpp"

namespace acino {

constexpr int CV_T = 256;            // threads per workgroup = (point, view) slots per batch
constexpr int CV_WG = 512;           // at most this many workgroups (= partial records) in the linearisation
constexpr int CV_SLOT = 48;          // slab doubles per (point, camera): W (6 x 3) | Y = W V^-1 (6 x 3) | sqrt(w_d) J_c[d] (2 x 6)
constexpr int CV_Q = (6 * SBA_MAXC + 15) / 16;   // S entries per thread: CV_Q x CV_Q (a 16 x 16 grid of threads over 6C x 6C)
constexpr int CV_CAMS_T = 512;       // threads of the one-workgroup camera kernel

struct CovBuf {
  int C, P, opt_cams;
  long long M;
  double fs;
  const double* intr;    // [C][16]
  const double* Rt;      // [C][12]
  const double* pts;     // [P][3]
  const double* uv;      // [M][2]
  const int* cam_idx;    // [M]
  const int* pt_start;   // [P + 1]
  const int* pt_obs;     // [M]
  double* Spart;         // [n_wg][n n]
  double* scalpart;      // [n_wg][4]: sum w r^2 | observations used | points excluded | bad-input flag
  double* S;             // [n][n]
  double* scal;          // [8]: the four sums | 4 not-PD flag | 5 smallest pivot / largest diagonal
};

// What one lane knows about its (point, view) slot after the shared front end of both point kernels.
struct CovSlot {
  bool on, valid, keep, bad;
  int p, cam;
  double W[18];          // W_pc (6 x 3, row-major)
  double Jc[2][6];       // sqrt(w_d) J_c[d]
  double Vi[6];          // V_p^-1 (packed symmetric)
  double wr2;            // w0 r0^2 + w1 r1^2
};

// Lane (pl, j) of a batch that starts at point pb: the j-th observation of point pb + pl, the point block V_p summed over
// the views in view order through sV, its LDL^T pivots, the exclusion rule and V_p^-1.  Every index that comes from the
// caller's arrays is range-checked before it addresses anything (bad = refuse the call).  Contains one __syncthreads.
template <int MODEL>
__device__ __forceinline__ void cov_slot(const CovBuf& B, int pb, int tid, double* sV, int* sCam, CovSlot& s) {
  const int C = B.C, NB = CV_T / C;
  const bool lane_on = tid < NB * C;
  const int pl = lane_on ? tid / C : 0, j = lane_on ? tid % C : 0;
  s.on = lane_on && pb + pl < B.P;
  s.p = s.on ? pb + pl : pb;
  s.bad = false;
  int o0 = 0, cnt = 0;
  if (s.on) {
    o0 = B.pt_start[s.p];
    cnt = B.pt_start[s.p + 1] - o0;
    if (o0 < 0 || cnt < 0 || cnt > C || (long long)o0 + cnt > B.M) {
      s.bad = true;
      cnt = 0;
    }
  }
  s.valid = s.on && j < cnt;
  int k = 0, c = 0;
  if (s.valid) {
    k = B.pt_obs[o0 + j];
    if (k < 0 || k >= B.M) {
      s.bad = true;
      s.valid = false;
      k = 0;
    }
  }
  if (s.valid) {
    c = B.cam_idx[k];
    if (c < 0 || c >= C) {
      s.bad = true;
      s.valid = false;
      c = 0;
    }
  }
  s.cam = c;
  sCam[tid] = s.valid ? c : -1;
  SbaObs<ACINO_PREC_F64> o;
  {
    double R[12];
    SbaIntr in;
    const double* rp = B.Rt + 12 * c;
    const double* ip = B.intr + SBA_INTR * c;
#pragma unroll
    for (int q = 0; q < 12; ++q) R[q] = rp[q];
    in.fx = ip[0]; in.fy = ip[1]; in.cx = ip[2]; in.cy = ip[3];
#pragma unroll
    for (int q = 0; q < 12; ++q) in.d[q] = (MODEL == 0 && q >= 4) ? 0.0 : ip[4 + q];
    const double X[3] = {B.pts[3 * (size_t)s.p], B.pts[3 * (size_t)s.p + 1], B.pts[3 * (size_t)s.p + 2]};
    sba_observe<ACINO_PREC_F64, true, MODEL, false>(B.fs, R, in, X, B.uv[2 * (size_t)k], B.uv[2 * (size_t)k + 1], o);
  }
  // what a lane without an observation computed is discarded by selects (it may be inf / NaN)
  const double w0 = s.valid ? o.w[0] : 0.0, w1 = s.valid ? o.w[1] : 0.0;
#pragma unroll
  for (int d = 0; d < 2; ++d) {
#pragma unroll
    for (int jj = 0; jj < 3; ++jj) o.Jp[d][jj] = s.valid ? o.Jp[d][jj] : 0.0;
#pragma unroll
    for (int a = 0; a < 6; ++a) o.Jc[d][a] = s.valid ? o.Jc[d][a] : 0.0;
    o.rs[d] = s.valid ? o.rs[d] : 0.0;
  }
  s.wr2 = w0 * o.rs[0] * o.rs[0] + w1 * o.rs[1] * o.rs[1];
  const double q0 = sqrt(w0), q1 = sqrt(w1);
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    s.Jc[0][a] = q0 * o.Jc[0][a];
    s.Jc[1][a] = q1 * o.Jc[1][a];
#pragma unroll
    for (int jj = 0; jj < 3; ++jj) s.W[a * 3 + jj] = w0 * o.Jc[0][a] * o.Jp[0][jj] + w1 * o.Jc[1][a] * o.Jp[1][jj];
  }
  double* pv = sV + 6 * tid;
  pv[0] = w0 * o.Jp[0][0] * o.Jp[0][0] + w1 * o.Jp[1][0] * o.Jp[1][0];
  pv[1] = w0 * o.Jp[0][0] * o.Jp[0][1] + w1 * o.Jp[1][0] * o.Jp[1][1];
  pv[2] = w0 * o.Jp[0][0] * o.Jp[0][2] + w1 * o.Jp[1][0] * o.Jp[1][2];
  pv[3] = w0 * o.Jp[0][1] * o.Jp[0][1] + w1 * o.Jp[1][1] * o.Jp[1][1];
  pv[4] = w0 * o.Jp[0][1] * o.Jp[0][2] + w1 * o.Jp[1][1] * o.Jp[1][2];
  pv[5] = w0 * o.Jp[0][2] * o.Jp[0][2] + w1 * o.Jp[1][2] * o.Jp[1][2];
  __syncthreads();
  double V[6] = {0, 0, 0, 0, 0, 0};
  for (int jj = 0; jj < C; ++jj) {
    const int t2 = pl * C + jj;
    if (s.valid && jj < j && sCam[t2] == c) s.bad = true;       // two observations of one point by one camera
#pragma unroll
    for (int q = 0; q < 6; ++q) V[q] += sV[6 * t2 + q];
  }
  // V = L D L^T; the point is kept when every pivot is above 3 eps max diag V
  const double tol = 3.0 * 2.220446049250313e-16 * fmax(V[0], fmax(V[3], V[5]));
  const double d0 = V[0];
  bool keep = cnt >= 2 && d0 > tol;                        // (one view: rank 2 exactly, whatever the rounding of the last pivot says)
  const double i0 = keep ? 1.0 / d0 : 0.0;
  const double l10 = V[1] * i0, l20 = V[2] * i0;
  const double d1 = V[3] - l10 * V[1];
  keep = keep && d1 > tol;
  const double i1 = keep ? 1.0 / d1 : 0.0;
  const double b21 = V[4] - l20 * V[1];
  const double l21 = b21 * i1;
  const double d2 = V[5] - l20 * V[2] - l21 * b21;
  keep = keep && d2 > tol;
  const double i2 = keep ? 1.0 / d2 : 0.0;
  s.keep = keep;
  // V^-1 = M^T D^-1 M with M = L^-1 = [1 0 0; -l10 1 0; m20 -l21 1]
  const double m20 = l10 * l21 - l20;
  s.Vi[0] = i0 + l10 * l10 * i1 + m20 * m20 * i2;
  s.Vi[1] = -l10 * i1 - m20 * l21 * i2;
  s.Vi[2] = m20 * i2;
  s.Vi[3] = i1 + l21 * l21 * i2;
  s.Vi[4] = -l21 * i2;
  s.Vi[5] = i2;
}

// Y = W V^-1 (6 x 3)
__device__ __forceinline__ void cov_y(const double (&W)[18], const double (&Vi)[6], double (&Y)[18]) {
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    const double x0 = W[r * 3], x1 = W[r * 3 + 1], x2 = W[r * 3 + 2];
    Y[r * 3] = x0 * Vi[0] + x1 * Vi[1] + x2 * Vi[2];
    Y[r * 3 + 1] = x0 * Vi[1] + x1 * Vi[3] + x2 * Vi[4];
    Y[r * 3 + 2] = x0 * Vi[2] + x1 * Vi[4] + x2 * Vi[5];
  }
}

__host__ __device__ inline size_t cov_lin_lds(int C) { return ((size_t)(CV_T / C) * C * CV_SLOT + CV_T * 6) * 8 + CV_T * 4; }
__host__ __device__ inline size_t cov_pts_lds(int C) { return ((size_t)36 * C * C + CV_T * 18 + CV_T * 6) * 8 + CV_T * 4; }

template <int MODEL>
__global__ void __launch_bounds__(CV_T) k_sbacov_lin(CovBuf B, int batches_per_wg, int n_batch) {
  extern __shared__ __attribute__((aligned(16))) double cv_smem[];
  __shared__ double sred[4][4];
  const int tid = threadIdx.x, C = B.C, NB = CV_T / C, n = 6 * C, nn = n * n;
  double* slab = cv_smem;                                  // [NB][C][CV_SLOT]
  double* sV = slab + (size_t)NB * C * CV_SLOT;            // [CV_T][6]
  int* sCam = reinterpret_cast<int*>(sV + CV_T * 6);       // [CV_T]
  // S in registers: the threads form a 16 x 16 grid, thread (ti, tj) owns the entries (ti + 16 qi, tj + 16 qj) - per point
  // it reads its (up to) six rows of Y and six rows of W once and adds their outer product
  const int ti = tid >> 4, tj = tid & 15, nq = (n + 15) / 16;
  int offA[CV_Q], offB[CV_Q];                              // row i / row j of S in a point's slab: camera slot * CV_SLOT + r, r = row % 6
  unsigned long long same = 0;                             // bit 6 qi + qj: both rows belong to one camera (the U_c block)
#pragma unroll
  for (int qi = 0; qi < CV_Q; ++qi) {
    const int i = min(ti + 16 * qi, n - 1), jc = min(tj + 16 * qi, n - 1);
    offA[qi] = (i / 6) * CV_SLOT + i % 6;
    offB[qi] = (jc / 6) * CV_SLOT + jc % 6;
  }
#pragma unroll
  for (int qi = 0; qi < CV_Q; ++qi)
#pragma unroll
    for (int qj = 0; qj < CV_Q; ++qj)
      if (min(ti + 16 * qi, n - 1) / 6 == min(tj + 16 * qj, n - 1) / 6) same |= 1ull << (6 * qi + qj);
  double acc[CV_Q][CV_Q];
#pragma unroll
  for (int qi = 0; qi < CV_Q; ++qi)
#pragma unroll
    for (int qj = 0; qj < CV_Q; ++qj) acc[qi][qj] = 0.0;
  double swr2 = 0.0, nobs = 0.0, nexcl = 0.0, bad = 0.0;
  const int b0 = min(blockIdx.x * batches_per_wg, n_batch), b1 = min(b0 + batches_per_wg, n_batch);
  for (int b = b0; b < b1; ++b) {
    const int pb = b * NB, nb = min(NB, B.P - pb);
    if (B.opt_cams)
      for (int e = tid; e < nb * C * CV_SLOT; e += CV_T) slab[e] = 0.0;
    CovSlot s;
    cov_slot<MODEL>(B, pb, tid, sV, sCam, s);               // (its barrier also orders the zeroing before the writes below)
    if (s.bad) bad = 1.0;
    if (s.valid && s.keep) {
      swr2 += s.wr2;
      nobs += 1.0;
      if (B.opt_cams) {
        double Y[18];
        cov_y(s.W, s.Vi, Y);
        double* sl = slab + ((size_t)(s.p - pb) * C + s.cam) * CV_SLOT;
#pragma unroll
        for (int q = 0; q < 18; ++q) {
          sl[q] = s.W[q];
          sl[18 + q] = Y[q];
        }
#pragma unroll
        for (int a = 0; a < 6; ++a) {
          sl[36 + a] = s.Jc[0][a];
          sl[42 + a] = s.Jc[1][a];
        }
      }
    }
    if (s.on && tid % C == 0 && !s.keep) nexcl += 1.0;
    __syncthreads();
    if (B.opt_cams) {
#pragma unroll 1
      for (int pp = 0; pp < nb; ++pp) {
        const double* sp = slab + (size_t)pp * C * CV_SLOT;
        double ya[CV_Q][3], ua[CV_Q][2], wb[CV_Q][3], ub[CV_Q][2];
#pragma unroll
        for (int q = 0; q < CV_Q; ++q)
          if (q < nq) {
            // pa / pb2 = slot + r.  In a slot: W row r at 3 r, Y row r at 18 + 3 r, the two camera rows' entry r at 36 + r, 42 + r
            const double* pa = sp + offA[q];
            const double* pb2 = sp + offB[q];
            const int ra = offA[q] % CV_SLOT, rb = offB[q] % CV_SLOT;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
              ya[q][k] = pa[18 + 2 * ra + k];
              wb[q][k] = pb2[2 * rb + k];
            }
            ua[q][0] = pa[36];
            ua[q][1] = pa[42];
            ub[q][0] = pb2[36];
            ub[q][1] = pb2[42];
          }
#pragma unroll
        for (int qi = 0; qi < CV_Q; ++qi)
#pragma unroll
          for (int qj = 0; qj < CV_Q; ++qj)
            if (qi < nq && qj < nq) {
              double v = acc[qi][qj] - (ya[qi][0] * wb[qj][0] + ya[qi][1] * wb[qj][1] + ya[qi][2] * wb[qj][2]);
              const double u = ua[qi][0] * ub[qj][0] + ua[qi][1] * ub[qj][1];
              acc[qi][qj] = ((same >> (6 * qi + qj)) & 1ull) ? v + u : v;
            }
      }
    }
    __syncthreads();
  }
  double red[4] = {swr2, nobs, nexcl, bad};
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    for (int off = 32; off > 0; off >>= 1) red[q] += __shfl_down(red[q], off, 64);
    if ((tid & 63) == 0) sred[q][tid >> 6] = red[q];
  }
  __syncthreads();
  if (tid < 4) B.scalpart[4 * blockIdx.x + tid] = (sred[tid][0] + sred[tid][1]) + (sred[tid][2] + sred[tid][3]);
  if (B.opt_cams) {
#pragma unroll
    for (int qi = 0; qi < CV_Q; ++qi)
#pragma unroll
      for (int qj = 0; qj < CV_Q; ++qj) {
        const int i = ti + 16 * qi, jc = tj + 16 * qj;
        if (i < n && jc < n) B.Spart[(size_t)blockIdx.x * nn + i * n + jc] = acc[qi][qj];
      }
  }
}

// the records in workgroup order: S, and (block 0) the four scalar sums
__global__ void __launch_bounds__(256) k_sbacov_reduce(CovBuf B, int n_wg) {
  const int nn = 36 * B.C * B.C, e = blockIdx.x * 256 + threadIdx.x;
  if (B.opt_cams && e < nn) {
    double s = 0.0;
    for (int w = 0; w < n_wg; ++w) s += B.Spart[(size_t)w * nn + e];
    B.S[e] = s;
  }
  if (blockIdx.x == 0 && threadIdx.x < 4) {
    double s = 0.0;
    for (int w = 0; w < n_wg; ++w) s += B.scalpart[4 * w + threadIdx.x];
    B.scal[threadIdx.x] = s;
  }
}

// Sigma_c = scale N (N^T S N)^-1 N^T by one workgroup.  Nm [n][m] (row-major, orthonormal columns), T1 [n][m] and Bm [m][n]
// are scratch in global memory (written and read by this workgroup only, barriers in between), the m x m matrix lives in LDS.
// A Cholesky pivot <= m eps max diag(N^T S N) raises scal[4] and every entry of the result is NaN.
__global__ void __launch_bounds__(CV_CAMS_T)
k_sbacov_cams(CovBuf B, const double* Nm, int m, double* T1, double* Bm, double scale, double* cov) {
  extern __shared__ __attribute__((aligned(16))) double cv_smem[];
  __shared__ double sflag[2];
  const int n = 6 * B.C, ld = m + 1, tid = threadIdx.x;
  double* sM = cv_smem;                                    // [m][m + 1], lower triangle
  for (int e = tid; e < n * m; e += CV_CAMS_T) {
    const int i = e / m, k = e - i * m;
    double v = 0.0;
    for (int jj = 0; jj < n; ++jj) v += 0.5 * (B.S[i * n + jj] + B.S[jj * n + i]) * Nm[jj * m + k];
    T1[e] = v;
  }
  __syncthreads();
  for (int e = tid; e < m * m; e += CV_CAMS_T) {
    const int k = e / m, l = e - k * m;
    if (l > k) continue;
    double v = 0.0;
    for (int i = 0; i < n; ++i) v += Nm[i * m + k] * T1[i * m + l];
    sM[k * ld + l] = v;
  }
  __syncthreads();
  if (tid == 0) {
    double mx = 0.0;
    for (int k = 0; k < m; ++k) mx = fmax(mx, sM[k * ld + k]);
    sflag[0] = mx;
    sflag[1] = 0.0;
  }
  __syncthreads();
  const double mx = sflag[0], tol = (double)m * 2.220446049250313e-16 * mx;
  double minpiv = INFINITY;                                // (thread 0's copy is the one that is used)
  for (int jc = 0; jc < m; ++jc) {
    if (tid == 0) {
      double d = sM[jc * ld + jc];
      minpiv = fmin(minpiv, d);
      if (!(d > tol)) {
        sflag[1] = 1.0;
        minpiv = fmin(minpiv, isnan(d) ? -INFINITY : d);
        d = 1.0;
      }
      sM[jc * ld + jc] = sqrt(d);
    }
    __syncthreads();
    const double dj = sM[jc * ld + jc];
    for (int i = jc + 1 + tid; i < m; i += CV_CAMS_T) sM[i * ld + jc] /= dj;
    __syncthreads();
    const int rem = m - jc - 1;
    for (int e = tid; e < rem * rem; e += CV_CAMS_T) {
      const int i = jc + 1 + e / rem, k = jc + 1 + e % rem;
      if (k <= i) sM[i * ld + k] -= sM[i * ld + jc] * sM[k * ld + jc];
    }
    __syncthreads();
  }
  // B = L^-1 N^T: one column per thread, forward substitution
  if (tid < n) {
    for (int k = 0; k < m; ++k) {
      double v = Nm[tid * m + k];
      for (int l = 0; l < k; ++l) v -= sM[k * ld + l] * Bm[l * n + tid];
      Bm[k * n + tid] = v / sM[k * ld + k];
    }
  }
  __syncthreads();
  const bool notpd = sflag[1] != 0.0;
  for (int e = tid; e < n * n; e += CV_CAMS_T) {
    const int i = e / n, jj = e - i * n;
    double v = 0.0;
    for (int k = 0; k < m; ++k) v += Bm[k * n + i] * Bm[k * n + jj];
    cov[e] = notpd ? (double)NAN : scale * v;
  }
  if (tid == 0) {
    B.scal[4] = sflag[1];
    B.scal[5] = mx > 0.0 ? minpiv / mx : -INFINITY;
  }
}

// The streaming pass over the points.  covc = the (already scaled) camera covariance [6C][6C] or null for points only; per point
// Sigma_p = scale V_p^-1 + sum_{a, b seen} Y_a^T Sigma_ab Y_b with Y_a = W_pa V_p^-1 (6 x 3), packed xx xy xz yy yz zz.
template <int MODEL>
__global__ void __launch_bounds__(CV_T)
k_sbacov_points(CovBuf B, const double* __restrict__ covc, double scale, double* __restrict__ cov_points,
                double* __restrict__ std_points, int batches_per_wg, int n_batch) {
  extern __shared__ __attribute__((aligned(16))) double cv_smem[];
  const int tid = threadIdx.x, C = B.C, n = 6 * C, nn = covc ? n * n : 0;
  double* sSig = cv_smem;                                  // [n][n]
  double* sY = sSig + nn;                                  // [CV_T][18]
  double* sV = sY + CV_T * 18;                             // [CV_T][6]: the V shares, then the Q shares
  int* sCam = reinterpret_cast<int*>(sV + CV_T * 6);       // [CV_T]
  for (int e = tid; e < nn; e += CV_T) sSig[e] = covc[e];
  const int NB = CV_T / C;
  const int b0 = min(blockIdx.x * batches_per_wg, n_batch), b1 = min(b0 + batches_per_wg, n_batch);
  for (int b = b0; b < b1; ++b) {
    const int pb = b * NB;
    CovSlot s;
    cov_slot<MODEL>(B, pb, tid, sV, sCam, s);
    const bool live = s.valid && s.keep && !s.bad;
    double Y[18];
    cov_y(s.W, s.Vi, Y);
    if (covc) {
#pragma unroll
      for (int q = 0; q < 18; ++q) sY[18 * tid + q] = live ? Y[q] : 0.0;
    }
    __syncthreads();                                       // (Y of the batch complete; every lane has read its V shares)
    double Q[6] = {0, 0, 0, 0, 0, 0};
    if (covc && live) {
      const int base = tid - tid % C;                      // slot 0 of this lane's point
      double Z[18];
#pragma unroll
      for (int q = 0; q < 18; ++q) Z[q] = 0.0;
      for (int jb = 0; jb < C; ++jb) {
        const int cb = sCam[base + jb];
        if (cb < 0) continue;
        const double* yb = sY + 18 * (base + jb);
        const double* sg = sSig + (size_t)(6 * s.cam) * n + 6 * cb;
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
          for (int t = 0; t < 6; ++t) {
            const double g = sg[r * n + t];
            Z[r * 3] += g * yb[t * 3];
            Z[r * 3 + 1] += g * yb[t * 3 + 1];
            Z[r * 3 + 2] += g * yb[t * 3 + 2];
          }
      }
#pragma unroll
      for (int r = 0; r < 6; ++r) {
        Q[0] += Y[r * 3] * Z[r * 3];
        Q[1] += Y[r * 3] * Z[r * 3 + 1];
        Q[2] += Y[r * 3] * Z[r * 3 + 2];
        Q[3] += Y[r * 3 + 1] * Z[r * 3 + 1];
        Q[4] += Y[r * 3 + 1] * Z[r * 3 + 2];
        Q[5] += Y[r * 3 + 2] * Z[r * 3 + 2];
      }
    }
#pragma unroll
    for (int q = 0; q < 6; ++q) sV[6 * tid + q] = Q[q];
    __syncthreads();
    if (s.on && tid % C == 0) {
      double out[6];
#pragma unroll
      for (int q = 0; q < 6; ++q) out[q] = scale * s.Vi[q];
      for (int jj = 0; jj < C; ++jj)
#pragma unroll
        for (int q = 0; q < 6; ++q) out[q] += sV[6 * (tid + jj) + q];
      const bool ok = s.keep && !s.bad;
      if (cov_points) {
#pragma unroll
        for (int q = 0; q < 6; ++q) cov_points[6 * (size_t)s.p + q] = ok ? out[q] : (double)NAN;
      }
      if (std_points) std_points[s.p] = ok ? sqrt(fmax(out[0] + out[3] + out[5], 0.0)) : (double)NAN;
    }
    __syncthreads();                                       // (the shares are read before the next batch overwrites them)
  }
}

struct CovLayout {
  size_t Spart, scalpart, S, N, T1, Bm, scal, total;
};
static CovLayout cov_layout(int n_cams) {
  const size_t nn = (size_t)36 * n_cams * n_cams;
  SbaTake take;
  CovLayout L;
  L.Spart = take((size_t)CV_WG * nn * 8);                  // partial records
  L.scalpart = take((size_t)CV_WG * 4 * 8);                // scalar partials
  L.S = take(nn * 8);
  L.N = take(nn * 8);                                      // the gauge complement N [n][n - 7]
  L.T1 = take(nn * 8);
  L.Bm = take(nn * 8);                                     // B = L^-1 N^T
  L.scal = take(64);
  L.total = take.off + 1024;
  return L;
}

// Orthonormal complement of the n x 7 constraint block G (row-major, overwritten): Householder QR, N = columns 7 .. n - 1 of Q
// as [n][n - 7] row-major.  false when G has rank below 7 (a diagonal entry of R at or below n eps max column norm).
static bool gauge_complement(std::vector<double>& G, int n, std::vector<double>& N) {
  const int g = 7, m = n - g;
  double cmax = 0.0;
  for (int k = 0; k < g; ++k) {
    double s = 0.0;
    for (int i = 0; i < n; ++i) s += G[i * g + k] * G[i * g + k];
    if (!(s == s) || std::isinf(s)) return false;
    cmax = fmax(cmax, sqrt(s));
  }
  const double tol = (double)n * 2.220446049250313e-16 * cmax;
  std::vector<double> vs((size_t)g * n, 0.0);
  for (int k = 0; k < g; ++k) {
    double nrm = 0.0;
    for (int i = k; i < n; ++i) nrm += G[i * g + k] * G[i * g + k];
    nrm = sqrt(nrm);
    if (!(nrm > tol)) return false;
    double* v = &vs[(size_t)k * n];
    const double alpha = G[k * g + k] >= 0.0 ? -nrm : nrm;
    for (int i = k; i < n; ++i) v[i] = G[i * g + k];
    v[k] -= alpha;
    double vn = 0.0;
    for (int i = k; i < n; ++i) vn += v[i] * v[i];
    vn = sqrt(vn);
    for (int i = k; i < n; ++i) v[i] /= vn;
    for (int c = k; c < g; ++c) {
      double d = 0.0;
      for (int i = k; i < n; ++i) d += v[i] * G[i * g + c];
      for (int i = k; i < n; ++i) G[i * g + c] -= 2.0 * d * v[i];
    }
  }
  // Q e_col = H_0 ... H_6 e_col for the columns behind the seventh
  N.assign((size_t)n * m, 0.0);
  std::vector<double> q(n);
  for (int col = 0; col < m; ++col) {
    for (int i = 0; i < n; ++i) q[i] = i == g + col ? 1.0 : 0.0;
    for (int k = g - 1; k >= 0; --k) {
      const double* v = &vs[(size_t)k * n];
      double d = 0.0;
      for (int i = k; i < n; ++i) d += v[i] * q[i];
      for (int i = k; i < n; ++i) q[i] -= 2.0 * d * v[i];
    }
    for (int i = 0; i < n; ++i) N[(size_t)i * m + col] = q[i];
  }
  return true;
}

}  // namespace acino

using namespace acino;

extern "C" {

size_t acino_sizeof_sba_cov_info(void) { return sizeof(acino_sba_cov_info); }

size_t acino_sba_covariance_workspace_bytes(int n_cams, int64_t n_points, int64_t n_obs) {
  if (n_cams < 1 || n_cams > SBA_MAXC || n_points < 0 || n_obs < 0) return 0;
  return cov_layout(n_cams).total;
}

int acino_sba_covariance(const acino_sba_params* prm, const double* d_intr, const double* d_Rt, const double* d_pts,
                         const double* d_uv, const int32_t* d_cam_idx, const int32_t* d_pt_start, const int32_t* d_pt_obs,
                         int gauge, int ref_cam, int scale_cam, const double* h_gauge, int scale, void* d_ws, size_t ws_bytes,
                         double* d_cov_cams, double* d_cov_points, double* d_std_points, acino_sba_cov_info* info,
                         void* stream) {
  if (int e = sba_check_problem(prm, info, d_intr && d_Rt && d_pts && d_uv && d_cam_idx && d_pt_start && d_pt_obs && d_ws, d_ws,
                                ws_bytes, acino_sba_covariance_workspace_bytes, ACINO_ERR_WORKSPACE, "SBA covariance: "))
    return e;
  ACINO_REQUIRE(scale == ACINO_SBA_SCALE_RESIDUAL || scale == ACINO_SBA_SCALE_UNIT, "scale: 0 residual, 1 unit");
  const int C = prm->n_cams, opt = prm->optimize_cameras ? 1 : 0, n = 6 * C, m = n - 7;
  if (opt) {
    ACINO_REQUIRE(C >= 2, "the covariance of the extrinsics needs at least two cameras");
    ACINO_REQUIRE(d_cov_cams, "d_cov_cams");
    ACINO_REQUIRE(gauge == ACINO_SBA_GAUGE_BASELINE || gauge == ACINO_SBA_GAUGE_FREE || gauge == ACINO_SBA_GAUGE_CUSTOM,
                  "gauge: 0 baseline, 1 free, 2 custom");
    if (gauge == ACINO_SBA_GAUGE_BASELINE)
      ACINO_REQUIRE(ref_cam >= 0 && ref_cam < C && scale_cam >= 0 && scale_cam < C && ref_cam != scale_cam,
                    "ref_cam and scale_cam: two different cameras");
    if (gauge == ACINO_SBA_GAUGE_CUSTOM) ACINO_REQUIRE(h_gauge, "custom gauge without a constraint matrix");
  }
  hipStream_t s = (hipStream_t)stream;
  const size_t P = (size_t)prm->n_points, nn = (size_t)n * n;
  const CovLayout L = cov_layout(C);
  char* w = (char*)d_ws;
  CovBuf B;
  B.C = C;
  B.P = (int)P;
  B.M = prm->n_obs;
  B.opt_cams = opt;
  B.fs = prm->f_scale;
  B.intr = d_intr;
  B.Rt = d_Rt;
  B.pts = d_pts;
  B.uv = d_uv;
  B.cam_idx = d_cam_idx;
  B.pt_start = d_pt_start;
  B.pt_obs = d_pt_obs;
  B.Spart = (double*)(w + L.Spart);
  B.scalpart = (double*)(w + L.scalpart);
  B.S = (double*)(w + L.S);
  double *d_N = (double*)(w + L.N), *d_T1 = (double*)(w + L.T1), *d_Bm = (double*)(w + L.Bm);
  B.scal = (double*)(w + L.scal);

  info->status = 0;
  info->n_points_excluded = 0;
  info->n_obs_used = 0;
  info->dof = 0;
  info->sigma2 = info->sum_w_r2 = info->min_pivot_ratio = NAN;
  // every way out of a singular problem: NaN outputs, status 5, ACINO_ERR_NUMERIC
  auto numeric = [&](const char* what) -> int {
    if (opt) ACINO_HIP_CHECK(hipMemsetAsync(d_cov_cams, 0xFF, nn * 8, s));               // (all bits set: a NaN)
    if (d_cov_points) ACINO_HIP_CHECK(hipMemsetAsync(d_cov_points, 0xFF, P * 6 * 8, s));
    if (d_std_points) ACINO_HIP_CHECK(hipMemsetAsync(d_std_points, 0xFF, P * 8, s));
    ACINO_HIP_CHECK(hipStreamSynchronize(s));
    info->status = 5;
    set_error("SBA covariance: %s", what);
    return ACINO_ERR_NUMERIC;
  };

  typedef void (*LinKernel)(CovBuf, int, int);
  typedef void (*PointsKernel)(CovBuf, const double*, double, double*, double*, int, int);
  const LinKernel lin_k[2] = {k_sbacov_lin<0>, k_sbacov_lin<1>};                 // [camera model]
  const PointsKernel points_k[2] = {k_sbacov_points<0>, k_sbacov_points<1>};
  static PerDeviceOnce once;
  if (once.first()) {                                      // more than 64 KB of dynamic LDS: the largest any camera count asks for
    size_t lin = 0, pts = 0;
    for (int c = 1; c <= SBA_MAXC; ++c) {
      lin = std::max(lin, cov_lin_lds(c));
      pts = std::max(pts, cov_pts_lds(c));
    }
    for (int k = 0; k < 2; ++k) {
      ACINO_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(lin_k[k]), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lin));
      ACINO_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(points_k[k]), hipFuncAttributeMaxDynamicSharedMemorySize, (int)pts));
    }
  }

  // ---- (a) linearisation at zero damping
  const int NB = CV_T / C;
  const int n_batch = (int)((P + NB - 1) / NB);
  const int bpw = (n_batch + CV_WG - 1) / CV_WG, n_wg = (n_batch + bpw - 1) / bpw;
  ACINO_HIP_CHECK(hipMemsetAsync(B.scal, 0, 64, s));
  hipLaunchKernelGGL(lin_k[prm->camera_model], dim3(n_wg), dim3(CV_T), cov_lin_lds(C), s, B, bpw, n_batch);
  ACINO_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_sbacov_reduce, dim3((unsigned)((nn + 255) / 256)), dim3(256), 0, s, B, n_wg);
  ACINO_LAUNCH_CHECK();
  double hs[8], hRt[12 * SBA_MAXC];
  ACINO_HIP_CHECK(hipMemcpyAsync(hs, B.scal, 64, hipMemcpyDeviceToHost, s));
  if (opt) ACINO_HIP_CHECK(hipMemcpyAsync(hRt, d_Rt, (size_t)C * 12 * 8, hipMemcpyDeviceToHost, s));
  ACINO_HIP_CHECK(hipStreamSynchronize(s));
  ACINO_REQUIRE(hs[3] == 0.0, "SBA covariance: observation lists out of range, a camera index out of range, or two observations "
                              "of one point by one camera");
  const int64_t n_used = (int64_t)hs[1], n_excl = (int64_t)hs[2], kept = (int64_t)P - n_excl;
  info->sum_w_r2 = hs[0];
  info->n_obs_used = n_used;
  info->n_points_excluded = (int32_t)n_excl;
  info->dof = 3 * kept + (opt ? n - 7 : 0);
  if (2 * n_used <= info->dof) return numeric("no more residuals than degrees of freedom (2 M <= dof)");
  info->sigma2 = hs[0] / (double)(2 * n_used - info->dof);
  const double mult = scale == ACINO_SBA_SCALE_RESIDUAL ? info->sigma2 : 1.0;

  // ---- (b) the gauge on the host (7 columns), the camera covariance by one workgroup
  if (opt) {
    std::vector<double> G((size_t)n * 7, 0.0), N;
    if (gauge == ACINO_SBA_GAUGE_CUSTOM) {
      for (size_t e = 0; e < (size_t)n * 7; ++e) G[e] = h_gauge[e];
    } else if (gauge == ACINO_SBA_GAUGE_FREE) {
      // the camera rows of the seven generators: translation dt_c = -R_c e, rotation dw_c = -R_c e, scale dt_c = t_c
      for (int c = 0; c < C; ++c)
        for (int i = 0; i < 3; ++i) {
          for (int k = 0; k < 3; ++k) {
            G[(size_t)(6 * c + 3 + i) * 7 + k] = -hRt[12 * c + 3 * i + k];
            G[(size_t)(6 * c + i) * 7 + 3 + k] = -hRt[12 * c + 3 * i + k];
          }
          G[(size_t)(6 * c + 3 + i) * 7 + 6] = hRt[12 * c + 9 + i];
        }
    } else {
      // the pose of ref_cam held (six unit constraints), and the distance between the centres c = -R^T t of ref_cam and scale_cam
      for (int q = 0; q < 6; ++q) G[(size_t)(6 * ref_cam + q) * 7 + q] = 1.0;
      double cen[2][3], u[3], un = 0.0;
      const int cams[2] = {ref_cam, scale_cam};
      for (int a = 0; a < 2; ++a)
        for (int k = 0; k < 3; ++k) {
          const double* R = hRt + 12 * cams[a];
          cen[a][k] = -(R[k] * R[9] + R[3 + k] * R[10] + R[6 + k] * R[11]);
        }
      for (int k = 0; k < 3; ++k) {
        u[k] = cen[1][k] - cen[0][k];
        un += u[k] * u[k];
      }
      un = sqrt(un);
      const double* Rs = hRt + 12 * scale_cam;
      double Ru[3];
      for (int i = 0; i < 3; ++i) Ru[i] = (Rs[3 * i] * u[0] + Rs[3 * i + 1] * u[1] + Rs[3 * i + 2] * u[2]) / un;   // (un = 0: NaN, refused below)
      const double* t = Rs + 9;
      const double tx[3] = {t[1] * Ru[2] - t[2] * Ru[1], t[2] * Ru[0] - t[0] * Ru[2], t[0] * Ru[1] - t[1] * Ru[0]};
      for (int i = 0; i < 3; ++i) {
        G[(size_t)(6 * scale_cam + i) * 7 + 6] = tx[i];
        G[(size_t)(6 * scale_cam + 3 + i) * 7 + 6] = -Ru[i];
      }
    }
    if (!gauge_complement(G, n, N)) return numeric("the gauge constraints have rank below 7");
    ACINO_HIP_CHECK(hipMemcpyAsync(d_N, N.data(), (size_t)n * m * 8, hipMemcpyHostToDevice, s));
    ACINO_HIP_CHECK(hipStreamSynchronize(s));              // (N is a local: the copy must have left it)
    hipLaunchKernelGGL(k_sbacov_cams, dim3(1), dim3(CV_CAMS_T), (size_t)m * (m + 1) * 8, s, B, d_N, m, d_T1, d_Bm, mult, d_cov_cams);
    ACINO_LAUNCH_CHECK();
    ACINO_HIP_CHECK(hipMemcpyAsync(hs, B.scal, 64, hipMemcpyDeviceToHost, s));
    ACINO_HIP_CHECK(hipStreamSynchronize(s));
    info->min_pivot_ratio = hs[5];
    if (hs[4] != 0.0) return numeric("the reduced camera system is not positive definite under this gauge");
  }

  // ---- (c) the points
  if (d_cov_points || d_std_points) {
    const double* covc = opt ? d_cov_cams : nullptr;
    const size_t lds = cov_pts_lds(opt ? C : 0);
    hipLaunchKernelGGL(points_k[prm->camera_model], dim3(n_wg), dim3(CV_T), lds, s, B, covc, mult, d_cov_points, d_std_points, bpw, n_batch);
    ACINO_LAUNCH_CHECK();
  }
  return ACINO_OK;
}

}  // extern "C"
