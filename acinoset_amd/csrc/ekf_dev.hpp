// Device code the EKF kernels of ekf.hip share with the covariance kernels of ekf_cov.hip: the dimensions of the filter,
// the parameter tables, the kernel constants, the workspace's rounding, the tile product and the covariance prediction.  Moved here from ekf.hip as
// they stood (same text, same inlining: the kernels of ekf.hip keep their code); the two tables are `static` now that two
// translation units hold them.
#pragma once
#include "cheetah_fk.hpp"
#include "dense80.hpp"

namespace acino {

constexpr int EP = 25;            // pose parameters (qb_list order)
constexpr int ES = 75;            // states: pose, velocity, acceleration
constexpr int EKF_MAXC = 6;
constexpr int EROWS = EKF_MAXC * 2 * NL;   // 240
constexpr int PLD = 81;           // leading dimension of the covariance in LDS: 80 x 81, zero beyond 75 (no masks on tiles)
constexpr int PR = 80;            // its padded row count
constexpr int VLD = 28;           // leading dimension of V = P[:, :25] A (80 x 28, zero beyond 75 x 25)
constexpr int HLD = 27;           // leading dimension of Hq
constexpr int SLD = 27;           // leading dimension of the 25 x 25 (+1) work matrices
constexpr int NVAR = EP + 1;      // base pose + one forward-difference variant per parameter

// EKF parameter (qb_list order, :734-746) -> active-state index of the kinematic chain
// (0-2 xyz, 3-5 phi0,phi1,phi3, 6-19 theta0-13, 20-24 psi0,1,3,4,5)
static __device__ const int8_t c_ekf2act[EP] = {0, 1, 2, 3, 6, 20, 4, 7, 21, 8, 5, 9, 22, 10, 23, 11, 24, 12, 13, 14, 15, 16, 17, 18, 19};
static __device__ const double c_qb_list[EP] = {5.0,  5.0,  5.0,   10.0,  10.0,  10.0,  5.0,   25.0,  5.0,   50.0,  5.0,   50.0, 25.0,
                                                100.0, 30.0, 140.0, 40.0, 350.0, 200.0, 350.0, 200.0, 450.0, 400.0, 450.0, 400.0};

// Host: the arrays of the workspace (include/acinoset_hip.h, read-back contract) each start at a multiple of 256 bytes.
static inline size_t a256(size_t v) { return (v + 255) / 256 * 256; }

struct EkfK {
  int n_frames, n_cams, pivoting;
  double sT, dlc_thresh, max_pixel_err, eps;
};

// C = A B on the matrix cores with 16 x 16 output tiles dealt to the four waves; KS k-steps of 4.  The operands and
// the result go through accessors (a_at(row, k), b_at(k, col), c_out(row, col, value)) that mask the padding.
template <int KS, class FA, class FB, class FC>
__device__ __forceinline__ void tile_gemm(int tiles_m, int tiles_n, int wave, int li, int lk, FA a_at, FB b_at, FC c_out) {
  for (int t = wave; t < tiles_m * tiles_n; t += 4) {
    const int ti = t / tiles_n, tj = t % tiles_n;
    double av[KS], bv[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      av[s] = a_at(16 * ti + li, 4 * s + lk);
      bv[s] = b_at(4 * s + lk, 16 * tj + li);
    }
    d4 acc = {0, 0, 0, 0};
#pragma unroll
    for (int s = 0; s < KS; ++s) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[s], bv[s], acc, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 4; ++r) c_out(16 * ti + lk + 4 * r, 16 * tj + li, acc[r]);
  }
}

// Entry (i, j) of each of the nine 25 x 25 blocks of F P F^T + Q (:761-766, :733-757), F = [[I, a1 I, a2 I], [0, I, a1 I],
// [0, 0, I]].  Reads and writes the same nine positions, so src == dst is fine with one thread per (i, j).  The
// smoother's gain kernel rebuilds P_pred[i+1] from P_est[i] with this same code - the filter does not store it.
__device__ __forceinline__ void predict_cov_entry(const double* src, int lds, double* dst, int ldd, int i, int j, double sT) {
  const double a1 = sT, a2 = sT * sT / 2;
  double p[3][3], r[3][3];
#pragma unroll
  for (int bi = 0; bi < 3; ++bi)
#pragma unroll
    for (int bj = 0; bj < 3; ++bj) p[bi][bj] = src[(bi * EP + i) * lds + bj * EP + j];
#pragma unroll
  for (int bj = 0; bj < 3; ++bj) {
    r[0][bj] = p[0][bj] + a1 * p[1][bj] + a2 * p[2][bj];
    r[1][bj] = p[1][bj] + a1 * p[2][bj];
    r[2][bj] = p[2][bj];
  }
  double qd = 0.0;
  if (i == j) {
    const double h = c_qb_list[i] / 2;
    qd = h * h;
  }
  const double s2 = sT * sT;
  const double qc[3][3] = {{s2 * s2 / 4, s2 * sT / 2, s2 / 2}, {s2 * sT / 2, s2, sT}, {s2 / 2, sT, 1.0}};
#pragma unroll
  for (int bi = 0; bi < 3; ++bi) {
    dst[(bi * EP + i) * ldd + j] = r[bi][0] + a1 * r[bi][1] + a2 * r[bi][2] + qc[bi][0] * qd;
    dst[(bi * EP + i) * ldd + EP + j] = r[bi][1] + a1 * r[bi][2] + qc[bi][1] * qd;
    dst[(bi * EP + i) * ldd + 2 * EP + j] = r[bi][2] + qc[bi][2] * qd;
  }
}

}  // namespace acino
