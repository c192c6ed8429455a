// What the per-frame pose fits share - pose_fit.hip (the cheetah model) and skel_pose_fit.hip (a link program): the status
// codes, the admission and whitening of a 3-D point with its covariance, and the lane read of the register-resident
// factorisations.  Nothing here depends on the shape of the model.
#pragma once
#include "ldl3.hpp"

namespace acino {

enum { PF_CONVERGED = 0, PF_MAX_ITER = 1, PF_FEW_MARKERS = 2, PF_NUMERIC = 3 };

// the value lane ``l`` holds (``l`` the same in every lane: a constant of an unrolled loop)
__device__ __forceinline__ double pf_readlane(double v, int l) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), l), hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
  return __hiloint2double(hi, lo);
}

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

}  // namespace acino
