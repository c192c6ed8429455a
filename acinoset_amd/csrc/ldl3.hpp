// L D L^T of a symmetric 3 x 3 matrix with a pivot test, its solve and its inverse (gfx950, fp64): the admission rule of the
// multi-view triangulation (triangulate_mv.hip) and of the marker covariances the pose fit takes (pose_fit.hip).
#pragma once
#include "common.hpp"

namespace acino {

// M = L D L^T of a symmetric 3 x 3 (upper entries m00 m01 m02 m11 m12 m22): unit lower L and the reciprocal pivots.  False
// when a pivot d_i (the square of the Cholesky diagonal) is not above ``tol``.
struct Ldl3 {
  double l10, l20, l21, i0, i1, i2;
};
__device__ __forceinline__ bool ldl3(double m00, double m01, double m02, double m11, double m12, double m22, double tol,
                                     Ldl3& f) {
  if (!(m00 > tol)) return false;
  f.i0 = rcp64(m00);
  f.l10 = m01 * f.i0;
  f.l20 = m02 * f.i0;
  const double d1 = m11 - f.l10 * m01;
  if (!(d1 > tol)) return false;
  f.i1 = rcp64(d1);
  const double b21 = m12 - f.l20 * m01;
  f.l21 = b21 * f.i1;
  const double d2 = m22 - f.l20 * m02 - f.l21 * b21;
  if (!(d2 > tol)) return false;
  f.i2 = rcp64(d2);
  return true;
}
__device__ __forceinline__ void ldl3_solve(const Ldl3& f, double b0, double b1, double b2, double& x0, double& x1,
                                           double& x2) {
  const double z1 = b1 - f.l10 * b0, z2 = b2 - f.l20 * b0 - f.l21 * z1;
  x2 = z2 * f.i2;
  x1 = z1 * f.i1 - f.l21 * x2;
  x0 = b0 * f.i0 - f.l10 * x1 - f.l20 * x2;
}
// the upper entries of M^-1 = L^-T D^-1 L^-1
__device__ __forceinline__ void ldl3_inverse(const Ldl3& f, double inv[6]) {
  const double m10 = -f.l10, m21 = -f.l21, m20 = f.l10 * f.l21 - f.l20;
  inv[0] = f.i0 + m10 * m10 * f.i1 + m20 * m20 * f.i2;
  inv[1] = m10 * f.i1 + m20 * m21 * f.i2;
  inv[2] = m20 * f.i2;
  inv[3] = f.i1 + m21 * m21 * f.i2;
  inv[4] = m21 * f.i2;
  inv[5] = f.i2;
}

}  // namespace acino
