// Device functions the posterior kernels of fte_cov.hip share with fte_calib.hip: the inputs at the current iterate, the
// pinned set of a node, the FK frame with its rotation axes and the marker Jacobian taken from them.  Moved here from
// fte_cov.hip as they stood (same text, same inlining: the kernels of fte_cov.hip keep their code).
#pragma once
#include "bcr_dev.hpp"
#include "cheetah_fk.hpp"

namespace acino {

struct CovIn {
  const double *x, *g, *H;
};

// code[row] of a node whose first frame is global frame f0 and which holds nlive frames of its clip:
// 0 free, 1 bound-active (the solve's rule: build_finish, oracle active_set), 2 padding / no such frame
__device__ __forceinline__ void cov_codes(int* code, const CovIn& in, const FteConst& K, int64_t f0, int nlive, int tid) {
  if (tid < BS) {
    int c = 2;
    const int fr = tid / NP, p = tid % NP;
    if (tid < 3 * NP && fr < nlive) {
      const int64_t n = f0 + fr;
      const double d = in.H[n * HPAIRS + hpair(p, p)];              // (measurement part + smoothness diagonal)
      const double xv = in.x[(n + HALO) * NP + p], gv = in.g[n * NP + p];
      const double gtol = GRAD_ZERO_REL * d;
      c = ((xv <= K.lo[p] && gv > gtol) || (xv >= K.hi[p] && gv < -gtol)) ? 1 : 0;
    }
    code[tid] = c;
  }
}

struct CovFrame {
  static constexpr bool kHasOm = true;
  double sc[22][2];
  double pos[21][3];
  double om[22][3];
};
// the rotation group whose frame carries marker l (cheetah_fk.hpp: fk_columns)
__device__ __forceinline__ int cov_marker_grp(int l) {
  // {0, 0, 0, 1, 2, 3, 4, 5, 2, 6, 7, 2, 8, 9, 3, 10 | 11, 3, 12, 13}, one nibble per marker (arithmetic, not a table)
  const unsigned long long lo = 0xA398276254321000ull, hi = 0xDC3Bull;
  return (int)(((l < 16 ? lo : hi) >> (4 * (l & 15))) & 15);
}

// d FK_l / d x_p, component i: omega_p x (p_l - pivot) for an angle marker l hangs on, e_p for the head position
__device__ __forceinline__ double rate_jac(const CovFrame& F, int l, int i, int p) {
  if (p < 3) return p == i ? 1.0 : 0.0;
  const int ga = c_state_grp[p], gm = cov_marker_grp(l);
  if (!((c_ancmask[gm] >> ga) & 1)) return 0.0;
  const double* w = F.om[p - 3];
  const double* c = F.pos[c_grp_pivot[ga]];
  const double* m = F.pos[l];
  const double d0 = m[0] - c[0], d1 = m[1] - c[1], d2 = m[2] - c[2];
  return i == 0 ? w[1] * d2 - w[2] * d1 : (i == 1 ? w[2] * d0 - w[0] * d2 : w[0] * d1 - w[1] * d0);
}

// rate_jac in two halves, for a caller that walks the tables once and evaluates many frames: the index into F.pos of the
// pivot of angle p (>= 3) when marker l hangs on it, else -1 ...
__device__ __forceinline__ int rate_pivot(int l, int p) {
  const int ga = c_state_grp[p];
  return ((c_ancmask[cov_marker_grp(l)] >> ga) & 1) ? c_grp_pivot[ga] : -1;
}
// ... and d FK_l / d x_p = omega_p x (p_l - pivot), all three components
__device__ __forceinline__ void rate_cross(const CovFrame& F, int l, int p, int pivot, double out[3]) {
  const double* w = F.om[p - 3];
  const double* c = F.pos[pivot];
  const double* m = F.pos[l];
  const double d0 = m[0] - c[0], d1 = m[1] - c[1], d2 = m[2] - c[2];
  out[0] = w[1] * d2 - w[2] * d1;
  out[1] = w[2] * d0 - w[0] * d2;
  out[2] = w[0] * d1 - w[1] * d0;
}

// Host: the opt-in of one kernel to `bytes` of dynamic LDS on the current device.  Made per call, beside the launch.
template <class Kernel>
inline hipError_t set_dyn_lds(Kernel* kernel, size_t bytes) {
  return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

}  // namespace acino
