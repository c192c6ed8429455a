// Robust N-view triangulation with a covariance per point (gfx950, fp64): acino_triangulate_multiview.
//
// Per (frame, marker) the minimiser X of the per-coordinate Cauchy cost of the calibration-level reprojection residuals
//   F(X) = sum_{c in V} 0.5 f^2 (log1p(r_u^2 / f^2) + log1p(r_v^2 / f^2)),   r = pi_c(X) - (u, v)
// over the cameras V with a valid detection (likelihood > thresh, finite pixel, undistortion succeeded), started at the
// N-view ray midpoint and refined by a damped Gauss-Newton iteration of its own: one thread per point, one launch, no host
// round trip, no atomics.  At the returned X: A = sum J^T W J (W the Cauchy IRLS weights - the matrix of
// sba.covariance(optimize_cameras=False)), cov = sigma_px^2 A^-1, wssr = sum w r^2 and, optionally, the sensitivity of X to
// every camera's extrinsics S = -A^-1 [J_c^T W_c Jc_c] under R <- exp([dw]x) R, t <- t + dt.
//
// The launch shape is k_triangulate_pairs': 256 consecutive (frame, marker) items per workgroup pass, their detections one
// contiguous span of whole frames staged in LDS when it fits in 60 KB (read from HBM otherwise), camera records staged once,
// a grid-stride loop over grid_for.  A thread keeps X, the gradient, the six entries of the matrix and the trial state in
// registers and re-reads its detections from the stage in every iteration; the cameras of V are a 16-bit mask.
#include "common.hpp"
#include "ldl3.hpp"
#include "pinhole.hpp"

namespace acino {

enum { MV_XTOL = 0, MV_MAX_ITER = 1, MV_FEW_VIEWS = 2, MV_NUMERIC = 3 };

__device__ __forceinline__ bool mv_undistort(const Cam& c, double u, double v, double& x, double& y) {
  return undistort_fisheye_pt(c, u, v, 10, 1e-8, x, y);
}
__device__ __forceinline__ bool mv_undistort(const Pin& c, double u, double v, double& x, double& y) {
  undistort_pinhole_pt(c, u, v, x, y);
  return true;
}

// What one pass over the cameras of V leaves at X: the cost, its gradient, a 3 x 3 matrix (upper entries) and sum w r^2.
struct MvSums {
  double F, g0, g1, g2, a00, a01, a02, a11, a12, a22, wssr;
  bool behind;          // z_c <= 0 for some camera of V
};

// CURV: the matrix of the step, sum J^T h J with the curvature of the loss floored so that it stays positive definite,
// h = max(rho'', 0.1 w), rho'' = (1 - z) / (1 + z)^2;  else the matrix of the outputs, h = w = 1 / (1 + z), z = r^2 / f^2.
template <bool PINHOLE>
__device__ __forceinline__ void mv_eval(const CamRec<PINHOLE>* __restrict__ c, const double* base, int64_t cam_stride,
                                        int n_cams, unsigned mask, double X0, double X1, double X2, double fs2, double ifs2,
                                        bool curv, MvSums& s) {
  s.F = s.g0 = s.g1 = s.g2 = s.a00 = s.a01 = s.a02 = s.a11 = s.a12 = s.a22 = s.wssr = 0.0;
  s.behind = false;
  for (int ci = 0; ci < n_cams; ++ci) {
    if (!((mask >> ci) & 1u)) continue;
    const CamRec<PINHOLE>& cm = c[ci];
    const double* d = base + (int64_t)ci * cam_stride;
    const double xc = cm.R[0] * X0 + cm.R[1] * X1 + cm.R[2] * X2 + cm.t[0];
    const double yc = cm.R[3] * X0 + cm.R[4] * X1 + cm.R[5] * X2 + cm.t[1];
    const double zc = cm.R[6] * X0 + cm.R[7] * X1 + cm.R[8] * X2 + cm.t[2];
    if (!(zc > 0.0)) s.behind = true;
    double uv[2], J[2][3];
    mv_project(cm, xc, yc, zc, uv, J);
    const double r[2] = {uv[0] - d[0], uv[1] - d[1]};
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const double z = r[k] * r[k] * ifs2;
      const double w = rcp64(1.0 + z);
      const double h = curv ? fmax((1.0 - z) * w * w, 0.1 * w) : w;
      const double j0 = J[k][0] * cm.R[0] + J[k][1] * cm.R[3] + J[k][2] * cm.R[6];
      const double j1 = J[k][0] * cm.R[1] + J[k][1] * cm.R[4] + J[k][2] * cm.R[7];
      const double j2 = J[k][0] * cm.R[2] + J[k][1] * cm.R[5] + J[k][2] * cm.R[8];
      const double wr = w * r[k];
      s.F += 0.5 * fs2 * log1p(z);
      s.wssr += wr * r[k];
      s.g0 += j0 * wr;
      s.g1 += j1 * wr;
      s.g2 += j2 * wr;
      const double h0 = h * j0, h1 = h * j1;
      s.a00 += h0 * j0;
      s.a01 += h0 * j1;
      s.a02 += h0 * j2;
      s.a11 += h1 * j1;
      s.a12 += h1 * j2;
      s.a22 += h * j2 * j2;
    }
  }
}

template <bool PINHOLE>
__global__ void __launch_bounds__(256)
k_triangulate_multiview(const double* __restrict__ det, int64_t n_frames, int n_cams, int n_markers, double thresh,
                        double f_scale, double sigma_px, double xtol, int max_iter, const double* __restrict__ cams,
                        double* __restrict__ points, double* __restrict__ cov, double* __restrict__ wssr,
                        uint8_t* __restrict__ nviews, uint8_t* __restrict__ status, uint8_t* __restrict__ iters,
                        double* __restrict__ sens, int stage_doubles) {
  typedef CamRec<PINHOLE> Rec;
  constexpr int STRIDE = PINHOLE ? ACINO_PINHOLE_STRIDE : ACINO_CAM_STRIDE;
  extern __shared__ __attribute__((aligned(16))) double stage[];
  __shared__ Rec c[ACINO_MAX_CAMS];
  for (int i = threadIdx.x; i < n_cams * STRIDE; i += blockDim.x) reinterpret_cast<double*>(c)[i] = cams[i];
  const int64_t total = n_frames * n_markers;
  const int64_t cam_stride = (int64_t)n_markers * 3;
  const int64_t frame_doubles = (int64_t)n_cams * cam_stride;
  const double fs2 = f_scale * f_scale, ifs2 = 1.0 / fs2, xtol2 = xtol * xtol, NaN = __builtin_nan("");
  for (int64_t idx0 = blockIdx.x * (int64_t)256; idx0 < total; idx0 += (int64_t)gridDim.x * 256) {
    const int64_t nf0 = idx0 / n_markers;
    int64_t nf1 = (idx0 + 255) / n_markers;
    if (nf1 > n_frames - 1) nf1 = n_frames - 1;
    const int64_t span = (nf1 - nf0 + 1) * frame_doubles;
    const bool staged = span <= stage_doubles;
    __syncthreads();                              // the previous pass is done with the stage (and c[] is complete)
    if (staged) {
      const double* src = det + nf0 * frame_doubles;
      for (int64_t e = threadIdx.x; e < span; e += 256) stage[e] = src[e];
    }
    __syncthreads();
    const int64_t idx = idx0 + threadIdx.x;
    if (idx >= total) continue;
    const int64_t n = idx / n_markers;
    const int l = (int)(idx - n * n_markers);
    const double* base = staged ? stage + (n - nf0) * frame_doubles + (int64_t)l * 3
                                : det + n * frame_doubles + (int64_t)l * 3;

    // ---- the view set and the ray midpoint: sum (I - w w^T) X = sum (I - w w^T) o,  o = -R^T t,  w = R^T (x, y, 1) / |.|
    unsigned mask = 0;
    int nv = 0;
    double m00 = 0, m01 = 0, m02 = 0, m11 = 0, m12 = 0, m22 = 0, b0 = 0, b1 = 0, b2 = 0;
    for (int ci = 0; ci < n_cams; ++ci) {
      const double* d = base + (int64_t)ci * cam_stride;
      const double u = d[0], v = d[1], lik = d[2];
      if (!(lik > thresh && m_finite(u) && m_finite(v))) continue;
      const Rec& cm = c[ci];
      double x, y;
      if (!mv_undistort(cm, u, v, x, y)) continue;
      mask |= 1u << ci;
      ++nv;
      const double in = rsqrt(x * x + y * y + 1.0);
      const double w0 = (cm.R[0] * x + cm.R[3] * y + cm.R[6]) * in, w1 = (cm.R[1] * x + cm.R[4] * y + cm.R[7]) * in,
                   w2 = (cm.R[2] * x + cm.R[5] * y + cm.R[8]) * in;
      const double o0 = -(cm.R[0] * cm.t[0] + cm.R[3] * cm.t[1] + cm.R[6] * cm.t[2]),
                   o1 = -(cm.R[1] * cm.t[0] + cm.R[4] * cm.t[1] + cm.R[7] * cm.t[2]),
                   o2 = -(cm.R[2] * cm.t[0] + cm.R[5] * cm.t[1] + cm.R[8] * cm.t[2]);
      const double wo = w0 * o0 + w1 * o1 + w2 * o2;
      m00 += 1.0 - w0 * w0;
      m01 -= w0 * w1;
      m02 -= w0 * w2;
      m11 += 1.0 - w1 * w1;
      m12 -= w1 * w2;
      m22 += 1.0 - w2 * w2;
      b0 += o0 - w0 * wo;
      b1 += o1 - w1 * wo;
      b2 += o2 - w2 * wo;
    }

    int st = MV_XTOL, it = 0;
    double X0 = NaN, X1 = NaN, X2 = NaN, inv[6] = {NaN, NaN, NaN, NaN, NaN, NaN}, ws = NaN;
    Ldl3 f;
    if (nv < 2) {
      st = MV_FEW_VIEWS;
    } else if (!ldl3(m00, m01, m02, m11, m12, m22, 1e-12 * (m00 + m11 + m22), f)) {
      st = MV_NUMERIC;
    } else {
      ldl3_solve(f, b0, b1, b2, X0, X1, X2);
      // ---- damped Gauss-Newton: (H + lam diag H) d = -g; a trial that raises F or leaves the front of a camera of V is
      //      rejected (lam x 10), an accepted one divides lam by 10; the iteration ends on a step shorter than xtol
      MvSums s, tr;
      mv_eval<PINHOLE>(c, base, cam_stride, n_cams, mask, X0, X1, X2, fs2, ifs2, true, s);
      double lam = 1e-3;
      st = MV_MAX_ITER;
#pragma unroll 1
      while (it < max_iter) {
        ++it;
        double d0 = 0, d1 = 0, d2 = 0;
        const bool pd = ldl3(s.a00 * (1.0 + lam), s.a01, s.a02, s.a11 * (1.0 + lam), s.a12, s.a22 * (1.0 + lam), 0.0, f);
        if (pd) ldl3_solve(f, -s.g0, -s.g1, -s.g2, d0, d1, d2);
        const double T0 = X0 + d0, T1 = X1 + d1, T2 = X2 + d2;
        bool ok = false;
        if (pd) {
          mv_eval<PINHOLE>(c, base, cam_stride, n_cams, mask, T0, T1, T2, fs2, ifs2, true, tr);
          ok = !tr.behind && tr.F <= s.F;
        }
        if (ok) {
          X0 = T0;
          X1 = T1;
          X2 = T2;
          s = tr;
          lam = fmax(lam * 0.1, 1e-12);
        } else {
          lam = fmin(lam * 10.0, 1e12);
        }
        if (pd && d0 * d0 + d1 * d1 + d2 * d2 < xtol2) {
          st = MV_XTOL;
          break;
        }
      }
      // ---- the outputs at the returned X: A with the IRLS weights, its inverse, sum w r^2
      mv_eval<PINHOLE>(c, base, cam_stride, n_cams, mask, X0, X1, X2, fs2, ifs2, false, s);
      ws = s.wssr;
      const bool pdA = ldl3(s.a00, s.a01, s.a02, s.a11, s.a12, s.a22, 1e-12 * (s.a00 + s.a11 + s.a22), f);
      if (pdA) ldl3_inverse(f, inv);
      bool fin = pdA && m_finite(X0) && m_finite(X1) && m_finite(X2) && m_finite(ws);
#pragma unroll
      for (int k = 0; k < 6; ++k) fin = fin && m_finite(inv[k]);
      if (!fin) {
        st = MV_NUMERIC;
        X0 = X1 = X2 = ws = NaN;
#pragma unroll
        for (int k = 0; k < 6; ++k) inv[k] = NaN;
      }
    }

    points[idx * 3 + 0] = X0;
    points[idx * 3 + 1] = X1;
    points[idx * 3 + 2] = X2;
    nviews[idx] = (uint8_t)nv;
    status[idx] = (uint8_t)st;
    if (iters) iters[idx] = (uint8_t)it;
    if (wssr) wssr[idx] = ws;
    if (cov) {
      const double s2 = sigma_px * sigma_px;
      double* o = cov + idx * 9;
      o[0] = s2 * inv[0];
      o[1] = o[3] = s2 * inv[1];
      o[2] = o[6] = s2 * inv[2];
      o[4] = s2 * inv[3];
      o[5] = o[7] = s2 * inv[4];
      o[8] = s2 * inv[5];
    }
    if (sens) {
      // ---- S = -A^-1 [G_0 .. G_{C-1}], G_c = J_c^T W_c Jc_c, camera by camera, stored straight out; the cameras outside V
      //      get exact zeros, a point that is not returned NaN
      const int64_t row = 6 * (int64_t)n_cams;
      double* so = sens + idx * 3 * row;
      const bool live = st == MV_XTOL || st == MV_MAX_ITER;
      for (int ci = 0; ci < n_cams; ++ci) {
        double* oc = so + 6 * ci;
        if (!live || !((mask >> ci) & 1u)) {
          const double fill = live ? 0.0 : NaN;
#pragma unroll
          for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int k = 0; k < 6; ++k) oc[i * row + k] = fill;
          continue;
        }
        const Rec& cm = c[ci];
        const double* d = base + (int64_t)ci * cam_stride;
        const double rx = cm.R[0] * X0 + cm.R[1] * X1 + cm.R[2] * X2, ry = cm.R[3] * X0 + cm.R[4] * X1 + cm.R[5] * X2,
                     rz = cm.R[6] * X0 + cm.R[7] * X1 + cm.R[8] * X2;
        double uv[2], J[2][3];
        mv_project(cm, rx + cm.t[0], ry + cm.t[1], rz + cm.t[2], uv, J);
        double P[3][2], Jc[2][6];                  // P = A^-1 J_c^T W_c (3 x 2)
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          const double r = uv[k] - d[k];
          const double w = rcp64(1.0 + r * r * ifs2);
          const double j0 = J[k][0] * cm.R[0] + J[k][1] * cm.R[3] + J[k][2] * cm.R[6];
          const double j1 = J[k][0] * cm.R[1] + J[k][1] * cm.R[4] + J[k][2] * cm.R[7];
          const double j2 = J[k][0] * cm.R[2] + J[k][1] * cm.R[5] + J[k][2] * cm.R[8];
          P[0][k] = w * (inv[0] * j0 + inv[1] * j1 + inv[2] * j2);
          P[1][k] = w * (inv[1] * j0 + inv[3] * j1 + inv[4] * j2);
          P[2][k] = w * (inv[2] * j0 + inv[4] * j1 + inv[5] * j2);
          Jc[k][0] = J[k][2] * ry - J[k][1] * rz;      // d(Xc)/d(dw) = -[R X]x ;  d(Xc)/d(dt) = I
          Jc[k][1] = J[k][0] * rz - J[k][2] * rx;
          Jc[k][2] = J[k][1] * rx - J[k][0] * ry;
          Jc[k][3] = J[k][0];
          Jc[k][4] = J[k][1];
          Jc[k][5] = J[k][2];
        }
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
          for (int k = 0; k < 6; ++k) oc[i * row + k] = -(P[i][0] * Jc[0][k] + P[i][1] * Jc[1][k]);
      }
    }
  }
}

}  // namespace acino

using namespace acino;

extern "C" {

size_t acino_sizeof_tri_mv_params(void) { return sizeof(acino_tri_mv_params); }

int acino_triangulate_multiview(const acino_tri_mv_params* prm, const double* d_det, int64_t n_frames, int n_cams,
                                int n_markers, const double* d_cams, double* d_points, double* d_cov, double* d_wssr,
                                uint8_t* d_nviews, uint8_t* d_status, uint8_t* d_iters, double* d_sens, void* stream) {
  ACINO_REQUIRE(prm != nullptr, "prm");
  ACINO_REQUIRE(n_frames >= 0 && n_markers >= 0, "sizes (n_frames, n_markers)");
  ACINO_REQUIRE(n_cams >= 1 && n_cams <= ACINO_MAX_CAMS, "n_cams must be 1..16");
  ACINO_REQUIRE(prm->camera_model == 0 || prm->camera_model == 1, "camera_model must be 0 (fisheye) or 1 (pinhole)");
  ACINO_REQUIRE(prm->max_iter >= 1 && prm->max_iter <= 255, "max_iter must be 1..255 (the iteration count is one byte)");
  ACINO_REQUIRE(prm->f_scale > 0 && prm->f_scale < INFINITY, "f_scale must be > 0");
  ACINO_REQUIRE(prm->sigma_px > 0 && prm->sigma_px < INFINITY, "sigma_px must be > 0");
  ACINO_REQUIRE(prm->xtol > 0 && prm->xtol < INFINITY, "xtol must be > 0");
  if (n_frames == 0 || n_markers == 0) return ACINO_OK;
  ACINO_REQUIRE(d_det && d_cams && d_points && d_nviews && d_status, "null buffer (d_det, d_cams, d_points, d_nviews, d_status)");
  // whole frames covering 256 consecutive (frame, marker) items; rigs whose span exceeds 60 KB read HBM directly
  const int64_t frames = 256 / n_markers + 2;
  int64_t stage = frames * n_cams * n_markers * 3;
  if (stage * 8 > 60 * 1024) stage = 0;        // (static LDS - the camera records, at most 4 KB - shares the 64 KB that need no opt-in)
  const int grid = grid_for(n_frames * n_markers, 256);
  if (prm->camera_model == 1)
    hipLaunchKernelGGL(k_triangulate_multiview<true>, dim3(grid), dim3(256), (size_t)stage * 8, (hipStream_t)stream, d_det,
                       n_frames, n_cams, n_markers, prm->thresh, prm->f_scale, prm->sigma_px, prm->xtol, prm->max_iter, d_cams,
                       d_points, d_cov, d_wssr, d_nviews, d_status, d_iters, d_sens, (int)stage);
  else
    hipLaunchKernelGGL(k_triangulate_multiview<false>, dim3(grid), dim3(256), (size_t)stage * 8, (hipStream_t)stream, d_det,
                       n_frames, n_cams, n_markers, prm->thresh, prm->f_scale, prm->sigma_px, prm->xtol, prm->max_iter, d_cams,
                       d_points, d_cov, d_wssr, d_nviews, d_status, d_iters, d_sens, (int)stage);
  ACINO_LAUNCH_CHECK();
  return ACINO_OK;
}

}  // extern "C"
