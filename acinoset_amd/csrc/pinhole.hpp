// The OpenCV "standard" pinhole camera (cv2.projectPoints: rational + tangential + thin-prism distortion), shared by the
// point-wise camera kernels and the FTE assembly; and what a kernel template needs to take the camera model as a parameter:
// the record type of a model (CamRec) and one projection-with-Jacobian call for either record (project_jac).
#pragma once
#include <type_traits>

#include "common.hpp"

namespace acino {

// ---- pinhole camera record (32 doubles, see acinoset_hip.h) --------------------------------
struct Pin {
  double fx, fy, cx, cy;
  double d[14];           // k1 k2 p1 p2 k3 k4 k5 k6 s1 s2 s3 s4 tx ty (the tilt tx, ty is refused by calib.pinhole_record)
  double R[9];
  double t[3];
  double pad0, pad1;
};
static_assert(sizeof(Pin) == ACINO_PINHOLE_STRIDE * sizeof(double), "pinhole record layout");

// cv2.projectPoints of a camera-frame point and d(uv)/d(Xc); the skew entry of K is ignored, as OpenCV does.  The algebra
// of pinhole_cam<JAC> (sba.hip), with the two reciprocals 1 / z and 1 / (1 + k4 r^2 + k5 r^4 + k6 r^6) by rcp64 as in the
// rest of the per-point camera arithmetic.
template <bool JAC>
__device__ __forceinline__ void pinhole_project(const Pin& c, double xc, double yc, double zc, double uv[2], double J[2][3]) {
  const double* k = c.d;
  const double iz = rcp64(zc);
  const double a = xc * iz, b = yc * iz;
  const double r2 = a * a + b * b, r4 = r2 * r2, r6 = r4 * r2;
  const double num = 1 + k[0] * r2 + k[1] * r4 + k[4] * r6;
  const double iden = rcp64(1 + k[5] * r2 + k[6] * r4 + k[7] * r6);
  const double rad = num * iden;
  const double xd = a * rad + 2 * k[2] * a * b + k[3] * (r2 + 2 * a * a) + k[8] * r2 + k[9] * r4;
  const double yd = b * rad + k[2] * (r2 + 2 * b * b) + 2 * k[3] * a * b + k[10] * r2 + k[11] * r4;
  uv[0] = c.fx * xd + c.cx;
  uv[1] = c.fy * yd + c.cy;
  if (JAC) {
    const double dnum = k[0] + 2 * k[1] * r2 + 3 * k[4] * r4, dden = k[5] + 2 * k[6] * r2 + 3 * k[7] * r4;
    const double drad = (dnum - rad * dden) * iden;                  // d rad / d r2
    const double sx = k[8] + 2 * k[9] * r2, sy = k[10] + 2 * k[11] * r2;
    const double dx_da = rad + 2 * a * a * drad + 2 * k[2] * b + 6 * k[3] * a + 2 * a * sx;
    const double dx_db = 2 * a * b * drad + 2 * k[2] * a + 2 * k[3] * b + 2 * b * sx;
    const double dy_da = 2 * a * b * drad + 2 * k[2] * a + 2 * k[3] * b + 2 * a * sy;
    const double dy_db = rad + 2 * b * b * drad + 6 * k[2] * b + 2 * k[3] * a + 2 * b * sy;
    const double du_da = c.fx * dx_da, du_db = c.fx * dx_db, dv_da = c.fy * dy_da, dv_db = c.fy * dy_db;
    J[0][0] = du_da * iz;
    J[0][1] = du_db * iz;
    J[0][2] = -(du_da * a + du_db * b) * iz;
    J[1][0] = dv_da * iz;
    J[1][1] = dv_db * iz;
    J[1][2] = -(dv_da * a + dv_db * b) * iz;
  }
}

// cv2.undistortPoints of one pixel (no R / P): the 5-step fixed point of OpenCV's default criteria (MAX_ITER, 5, 0.01).
__device__ __forceinline__ void undistort_pinhole_pt(const Pin& c, double u, double v, double& x, double& y) {
  const double* k = c.d;
  double x0 = (u - c.cx) / c.fx, y0 = (v - c.cy) / c.fy;
  x = x0;
  y = y0;
  for (int j = 0; j < 5; ++j) {
    double r2 = x * x + y * y;
    double icdist = (1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2) / (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2);
    if (icdist < 0) {
      x = x0;
      y = y0;
      break;
    }
    double dx = 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x) + k[8] * r2 + k[9] * r2 * r2;
    double dy = k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y + k[10] * r2 + k[11] * r2 * r2;
    x = (x0 - dx) * icdist;
    y = (y0 - dy) * icdist;
  }
}

// ---- the camera model as a template parameter: PINHOLE ? Pin : Cam.  The structs that hold both kinds of record give the
//      record of camera ci by cam_rec<PINHOLE>(owner, ci) (fte_kernels.hpp: FteConst, skel_dev.hpp: SkelDev).
template <bool PINHOLE>
using CamRec = std::conditional_t<PINHOLE, Pin, Cam>;

// Pixel and d(uv)/d(X_cam) of a camera-frame point, the report kernels' call: the FTE assembly's own functions in its order.
__device__ __forceinline__ void project_jac(const Cam& c, double xc, double yc, double zc, double uv[2], double J[2][3]) {
  FisheyeNlp fp;
  fisheye_nlp_uv(c, xc, yc, zc, fp, uv[0], uv[1]);
  fisheye_nlp_jac(c, fp, J[0], J[1]);
}
__device__ __forceinline__ void project_jac(const Pin& c, double xc, double yc, double zc, double uv[2], double J[2][3]) {
  pinhole_project<true>(c, xc, yc, zc, uv, J);
}

// calibration-level projection of a camera-frame point and d(uv)/d(Xc).  Fisheye: project_points_fisheye - the r > 1e-8
// branch and the record's skew, u = fx (xd + alpha yd) + cx -, the algebra of fisheye_cam<true> (sba_dev.hpp) plus the skew.
__device__ __forceinline__ void mv_project(const Cam& c, double xc, double yc, double zc, double uv[2], double J[2][3]) {
  const double iz = rcp64(zc);
  const double a = xc * iz, b = yc * iz;
  const double r2 = a * a + b * b;
  const double r = sqrt(r2);
  const double th = atan(r), th2 = th * th;
  const double thd = th * (1 + th2 * (c.k1 + th2 * (c.k2 + th2 * (c.k3 + th2 * c.k4))));
  const bool small = !(r > 1e-8);
  const double ir = small ? 0.0 : rcp64(r);
  const double m = small ? 1.0 : thd * ir;
  const double xd = a * m, yd = b * m;
  uv[0] = c.fx * (xd + c.alpha * yd) + c.cx;
  uv[1] = c.fy * yd + c.cy;
  double dm_da = 0.0, dm_db = 0.0;
  if (!small) {
    const double dthd = 1 + th2 * (3 * c.k1 + th2 * (5 * c.k2 + th2 * (7 * c.k3 + th2 * 9 * c.k4)));
    const double dm_dr = (dthd * rcp64(1 + r2) * r - thd) * (ir * ir);
    dm_da = dm_dr * a * ir;
    dm_db = dm_dr * b * ir;
  }
  const double dxd_da = m + a * dm_da, dxd_db = a * dm_db, dyd_da = b * dm_da, dyd_db = m + b * dm_db;
  const double du_da = c.fx * (dxd_da + c.alpha * dyd_da), du_db = c.fx * (dxd_db + c.alpha * dyd_db);
  const double dv_da = c.fy * dyd_da, dv_db = c.fy * dyd_db;
  J[0][0] = du_da * iz;
  J[0][1] = du_db * iz;
  J[0][2] = -(du_da * a + du_db * b) * iz;
  J[1][0] = dv_da * iz;
  J[1][1] = dv_db * iz;
  J[1][2] = -(dv_da * a + dv_db * b) * iz;
}
__device__ __forceinline__ void mv_project(const Pin& c, double xc, double yc, double zc, double uv[2], double J[2][3]) {
  pinhole_project<true>(c, xc, yc, zc, uv, J);
}

}  // namespace acino
