// Device functions of the bundle adjustment that more than one translation unit calls (sba.hip, sba_cov.hip): the two camera
// models with d(uv)/d(Xc), and one observation's residual, IRLS weights and Jacobian rows under the solver's parametrisation.
#pragma once
#include <type_traits>

#include "common.hpp"

namespace acino {

constexpr int SBA_MAXC = ACINO_MAX_CAMS;

struct SbaIntr {
  double fx, fy, cx, cy;
  double d[12];   // fisheye: k1..k4 ; pinhole (cv2.projectPoints): k1 k2 p1 p2 k3 k4 k5 k6 s1 s2 s3 s4
};
constexpr int SBA_INTR = 16;

// cv2.fisheye projection of a camera-frame point and d(uv)/d(Xc)
template <bool JAC>
__device__ __forceinline__ void fisheye_cam(const SbaIntr& c, const double Xc[3], double uv[2], double J[2][3]) {
  // (three divisions instead of seven: 1 / z, 1 / r, 1 / (1 + r^2) - an fp64 division is ~12 instructions, four of them at quarter rate)
  const double iz = 1.0 / Xc[2];
  const double a = Xc[0] * iz, b = Xc[1] * iz;
  const double r2 = a * a + b * b;
  const double r = sqrt(r2);
  const double th = atan(r), th2 = th * th;
  const double thd = th * (1 + th2 * (c.d[0] + th2 * (c.d[1] + th2 * (c.d[2] + th2 * c.d[3]))));
  const bool small = !(r > 1e-8);
  const double ir = small ? 0.0 : 1.0 / r;
  const double m = small ? 1.0 : thd * ir;
  uv[0] = c.fx * a * m + c.cx;
  uv[1] = c.fy * b * m + c.cy;
  if (JAC) {
    double dm_da = 0.0, dm_db = 0.0;
    if (!small) {
      const double dthd = 1 + th2 * (3 * c.d[0] + th2 * (5 * c.d[1] + th2 * (7 * c.d[2] + th2 * 9 * c.d[3])));
      const double dm_dr = (dthd / (1 + r2) * r - thd) * (ir * ir);
      dm_da = dm_dr * a * ir;
      dm_db = dm_dr * b * ir;
    }
    const double du_da = c.fx * (m + a * dm_da), du_db = c.fx * a * dm_db;
    const double dv_da = c.fy * b * dm_da, dv_db = c.fy * (m + b * dm_db);
    J[0][0] = du_da * iz;
    J[0][1] = du_db * iz;
    J[0][2] = -(du_da * a + du_db * b) * iz;
    J[1][0] = dv_da * iz;
    J[1][1] = dv_db * iz;
    J[1][2] = -(dv_da * a + dv_db * b) * iz;
  }
}

// cv2.projectPoints (rational + tangential + thin-prism model; the skew entry of K is ignored, as OpenCV does)
template <bool JAC>
__device__ __forceinline__ void pinhole_cam(const SbaIntr& c, const double Xc[3], double uv[2], double J[2][3]) {
  const double* k = c.d;
  const double iz = 1.0 / Xc[2];
  const double a = Xc[0] * iz, b = Xc[1] * iz;
  const double r2 = a * a + b * b, r4 = r2 * r2, r6 = r4 * r2;
  const double num = 1 + k[0] * r2 + k[1] * r4 + k[4] * r6;
  const double iden = 1.0 / (1 + k[5] * r2 + k[6] * r4 + k[7] * r6);
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

template <int PREC>
struct SbaObs {
  typedef typename std::conditional<PREC == ACINO_PREC_F64, double, float>::type acc_t;
  acc_t Jp[2][3], Jc[2][6], w[2], rs[2];
  double cost;
};
template <int PREC, bool JAC, int MODEL, bool COST = true>
__device__ __forceinline__ void sba_observe(double fs, const double (&R)[12], const SbaIntr& in, const double (&X)[3],
                                            double u, double v, SbaObs<PREC>& o) {
  typedef typename SbaObs<PREC>::acc_t acc_t;
  const double RX[3] = {R[0] * X[0] + R[1] * X[1] + R[2] * X[2], R[3] * X[0] + R[4] * X[1] + R[5] * X[2],
                        R[6] * X[0] + R[7] * X[1] + R[8] * X[2]};
  const double Xc[3] = {RX[0] + R[9], RX[1] + R[10], RX[2] + R[11]};
  double uvp[2], Jpi[2][3];
  if (MODEL == 0) fisheye_cam<JAC>(in, Xc, uvp, Jpi);
  else pinhole_cam<JAC>(in, Xc, uvp, Jpi);
  const double r0 = uvp[0] - u, r1 = uvp[1] - v;
  const double ifs2 = 1.0 / (fs * fs);
  const double z0 = r0 * r0 * ifs2, z1 = r1 * r1 * ifs2;
  o.cost = COST ? 0.5 * fs * fs * (log1p(z0) + log1p(z1)) : 0.0;
  if (JAC) {
    if (PREC == ACINO_PREC_F64) {
      o.w[0] = 1.0 / (1.0 + z0);
      o.w[1] = 1.0 / (1.0 + z1);
      o.rs[0] = r0;
      o.rs[1] = r1;
    } else {
      o.rs[0] = bf16_round((float)r0);
      o.rs[1] = bf16_round((float)r1);
      const float fi = (float)ifs2;
      o.w[0] = 1.0f / (1.0f + (float)o.rs[0] * (float)o.rs[0] * fi);
      o.w[1] = 1.0f / (1.0f + (float)o.rs[1] * (float)o.rs[1] * fi);
    }
    auto st = [](double x) -> acc_t { return PREC == ACINO_PREC_F64 ? (acc_t)x : (acc_t)bf16_round((float)x); };
#pragma unroll
    for (int d = 0; d < 2; ++d) {
#pragma unroll
      for (int j = 0; j < 3; ++j) o.Jp[d][j] = st(Jpi[d][0] * R[j] + Jpi[d][1] * R[3 + j] + Jpi[d][2] * R[6 + j]);
      o.Jc[d][0] = st(Jpi[d][1] * (-RX[2]) + Jpi[d][2] * RX[1]);      // d(Xc)/d(dw) = -[RX]x ;  d(Xc)/d(dt) = I
      o.Jc[d][1] = st(Jpi[d][0] * RX[2] - Jpi[d][2] * RX[0]);
      o.Jc[d][2] = st(-Jpi[d][0] * RX[1] + Jpi[d][1] * RX[0]);
      o.Jc[d][3] = st(Jpi[d][0]);
      o.Jc[d][4] = st(Jpi[d][1]);
      o.Jc[d][5] = st(Jpi[d][2]);
    }
  }
}

}  // namespace acino
