// The skeleton assembly kernel, one template for the solve (skel_fte.hip) and the covariance's Fisher assembly (skel_cov.hip):
// one workgroup per frame - link program, projection + 2x3 Jacobian per (pose, camera), the residual Jacobian rows A[r][p] in LDS,
// H_n = A^T W A, g_n, cost.  (Frame index n runs over the frames of all clips; `which` = 0: the clips' current iterate, 1: their
// trial iterate.)  The variants are template parameters, every branch on them an `if constexpr`:
//   PINHOLE  the camera record (SkelDev::pins for SkelDev::cams) and the projection with its 2x3 Jacobian: cv2.projectPoints
//            (pinhole.hpp) for the reference's fisheye pt3d_to_2d.  The product with R, the residual, the curvature and the
//            singular-plane cut are the same statements.
//   ROBUST   the measurement loss is the redescending rho of common.hpp on the same scaled residual e (acino_skel_fte_params::loss
//            = ACINO_SKEL_LOSS_REDESCENDING; a, b, c = 3, 10, 20): cost rho(e), gradient w rho'(|e|) sign(e), curvature w^2 h(e)
//            with the clipped secant h - for the L1 loss |e| with the IRLS curvature w^2 / max(|e|, l1_eps).  A dropped row
//            (w = 0) contributes nothing under either.
//   FISHER   = one trailing argument `double* opv_out` (the pack Opv is {double}; the solve's kernels have no such argument,
//            Opv = {}).  The block that goes to H is the Fisher information J^T diag(w^2) J of the stated Laplace model - under
//            ROBUST the Gauss-Newton curvature w^2 h(e) - instead of the IRLS curvature; g, hd and the cost stay the solver's own,
//            they feed its pin rule; the link operators go to opv_out.
// A kernel template with `if constexpr` compiles every instantiation to the code a hand-written kernel would have (DESIGN.md
// section 8, scripts/isa_diff.py); a shared __device__ function, once inlined, does not.
#pragma once
#include "skel_dev.hpp"

namespace acino {

template <bool JAC, bool PINHOLE, bool ROBUST, class... Opv>
__global__ void __launch_bounds__(256)
k_skel_assemble(const SkelDev* __restrict__ dev, const SkelClip* __restrict__ clip, int which, const double* __restrict__ x0,
                const double* __restrict__ x1, const double* __restrict__ meas, const double* __restrict__ wgt,
                double* __restrict__ H0, double* __restrict__ H1, double* __restrict__ g0, double* __restrict__ g1,
                double* __restrict__ hd0, double* __restrict__ hd1, double* __restrict__ c0, double* __restrict__ c1,
                Opv* __restrict__... opv_out) {
  constexpr bool FISHER = sizeof...(Opv) == 1;
  static_assert(sizeof...(Opv) <= 1 && (std::is_same_v<Opv, double> && ...), "opv_out is one double*, or absent");
  static_assert(JAC || !FISHER, "the Fisher assembly always wants the Jacobian");
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const SkelDev& D = *dev;
  const int tid = threadIdx.x, n = blockIdx.x;
  const SkelClip& cs = clip[n / D.n_frames];
  if (cs.status != 0) return;                               // (the clip is finished)
  const int buf = cs.cur ^ which;
  const double* __restrict__ x = buf ? x1 : x0;
  double* __restrict__ H = buf ? H1 : H0;
  double* __restrict__ g = buf ? g1 : g0;
  double* __restrict__ hd = buf ? hd1 : hd0;
  double* __restrict__ cost_part = buf ? c1 : c0;
  const int P = D.n_act, C = D.n_cams, NPOSE = D.n_pose, NOPS = D.n_ops, R = D.n_rows, lda = P | 1;
  double* xs = reinterpret_cast<double*>(smem_raw);          // [64] active states of this frame
  double* opv = xs + SK_MAXP;                                 // [n_ops][4][3]: M off, dM/dphi off, dM/dtheta off, dM/dpsi off
  double* pos = opv + ACINO_SKEL_MAX_OPS * 12;                // [n_pose][3]
  double* jrow = pos + (ACINO_SKEL_MAX_OPS + 1) * 3;          // [R][3] projection Jacobian row
  double* gsr = jrow + SK_MAXROWS * 3;                        // [R] d cost / d residual
  double* hwr = gsr + SK_MAXROWS;                             // [R] IRLS curvature weight
  double* red = hwr + SK_MAXROWS;                             // [8]
  double* A = red + 8;                                        // [R][lda]
  double* fwr = A + (size_t)R * lda;                          // [R] FISHER only: weight w^2 of a kept row (0 for a dropped one)
  if (tid < P) xs[tid] = x[(size_t)n * P + tid];
  __syncthreads();
  // ---- link operators: R_loc = Rz(psi) Rx(phi) Ry(theta) of the parent's own angles (reference sign convention)
  if (tid < NOPS) {
    const acino_skel_op& o = D.op[tid];
    const int f = o.flags;
    double sp = 0, cp = 1, st = 0, ct = 1, sz = 0, cz = 1;
    if (f & 1) sincos(D.amap[tid][0] >= 0 ? xs[D.amap[tid][0]] : 0.0, &sp, &cp);
    if (f & 2) sincos(D.amap[tid][1] >= 0 ? xs[D.amap[tid][1]] : 0.0, &st, &ct);
    if (f & 4) sincos(D.amap[tid][2] >= 0 ? xs[D.amap[tid][2]] : 0.0, &sz, &cz);
    const double Ry[3][3] = {{ct, 0, -st}, {0, 1, 0}, {st, 0, ct}}, dRy[3][3] = {{-st, 0, -ct}, {0, 0, 0}, {ct, 0, -st}};
    const double Rx[3][3] = {{1, 0, 0}, {0, cp, sp}, {0, -sp, cp}}, dRx[3][3] = {{0, 0, 0}, {0, -sp, cp}, {0, -cp, -sp}};
    const double Rz[3][3] = {{cz, sz, 0}, {-sz, cz, 0}, {0, 0, 1}}, dRz[3][3] = {{-sz, cz, 0}, {-cz, -sz, 0}, {0, 0, 0}};
    auto mul = [](const double (&a)[3][3], const double (&b)[3][3], double (&c)[3][3]) {
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) c[i][j] = a[i][0] * b[0][j] + a[i][1] * b[1][j] + a[i][2] * b[2][j];
    };
    double RxRy[3][3], M[4][3][3], T1[3][3], T2[3][3];
    mul(Rx, Ry, RxRy);
    mul(Rz, RxRy, M[0]);                 // R_loc
    mul(dRx, Ry, T1);
    mul(Rz, T1, M[1]);                   // d / d phi
    mul(Rx, dRy, T1);
    mul(Rz, T1, M[2]);                   // d / d theta
    mul(dRz, RxRy, M[3]);                // d / d psi
    (void)T2;
    const bool untr = (f & 8) != 0;      // bit 3: R_loc itself, else its transpose
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const bool on = m == 0 || ((f >> (m - 1)) & 1);
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        double v = 0.0;
        if (on) {
          v = untr ? M[m][i][0] * o.off[0] + M[m][i][1] * o.off[1] + M[m][i][2] * o.off[2]
                   : M[m][0][i] * o.off[0] + M[m][1][i] * o.off[1] + M[m][2][i] * o.off[2];
        }
        opv[(tid * 4 + m) * 3 + i] = v;
      }
    }
  }
  __syncthreads();
  if constexpr (FISHER) {
    double* __restrict__ out = (opv_out, ...);
    for (int e = tid; e < NOPS * 12; e += 256) out[(size_t)n * NOPS * 12 + e] = opv[e];
  }
  if (tid < 3) {                         // poses, coordinate by coordinate, in program order
    for (int s = 0; s < NPOSE; ++s) pos[s * 3 + tid] = xs[tid];
    for (int k = 0; k < NOPS; ++k) pos[D.op[k].child * 3 + tid] = pos[D.op[k].parent * 3 + tid] + opv[(k * 4) * 3 + tid];
  }
  __syncthreads();
  double my_cost = 0.0;
  // ---- projection of every (pose, camera): residuals, cost, Jacobian rows (pt3d_to_2d, build.py:457-481)
  if (tid < NPOSE * C) {
    const int l = tid / C, c = tid % C;
    const auto& cam = cam_rec<PINHOLE>(D, c);
    const double px = pos[l * 3], py = pos[l * 3 + 1], pz = pos[l * 3 + 2];
    const double* mz = meas + (((size_t)n * C + c) * NPOSE + l) * 2;
    const double um = mz[0], vm = mz[1];
    double w = wgt[((size_t)n * C + c) * NPOSE + l];
    if (!(m_finite(um) && m_finite(vm))) w = 0.0;
    const double xc = cam.R[0] * px + cam.R[1] * py + cam.R[2] * pz + cam.t[0];
    const double yc = cam.R[3] * px + cam.R[4] * py + cam.R[5] * pz + cam.t[1];
    const double zc = cam.R[6] * px + cam.R[7] * py + cam.R[8] * pz + cam.t[2];
    if (fabs(zc) < 1e-9) w = 0.0;        // (the singular plane itself; no other cut, as the reference)
    const int r0 = 2 * tid;
    double ju[3] = {0, 0, 0}, jv[3] = {0, 0, 0}, gu = 0, gv = 0, hu = 0, hv = 0;
    // The loss block - cost after the residuals, then d cost / d residual and the curvature weight after the Jacobian rows - stands
    // once under each camera branch: written once behind the branch, or as two local lambdas called from both, the JAC kernels
    // compile to other code (the same instructions in another order, other registers; scripts/isa_diff.py).
    double rho_u, rho_v, drho_u = 0, drho_v = 0, h_u = 0, h_v = 0;          // ROBUST only
    if (w != 0.0) {
      if constexpr (PINHOLE) {
        // cv2.projectPoints and d(uv)/d(X_cam) (pinhole.hpp); the fisheye branch's r^2 + 1e-12 of pt3d_to_2d is not part of it
        double uv[2], Jc[2][3];
        pinhole_project<JAC>(cam, xc, yc, zc, uv, Jc);
        const double eu = w * (uv[0] - um), ev = w * (uv[1] - vm);
        if constexpr (ROBUST) {
          redescending<JAC>(D.loss, eu, rho_u, drho_u, h_u);
          redescending<JAC>(D.loss, ev, rho_v, drho_v, h_v);
          my_cost = rho_u + rho_v;
        } else {
          my_cost = fabs(eu) + fabs(ev);
        }
        if (JAC) {
#pragma unroll
          for (int j = 0; j < 3; ++j) {
            ju[j] = Jc[0][0] * cam.R[j] + Jc[0][1] * cam.R[3 + j] + Jc[0][2] * cam.R[6 + j];
            jv[j] = Jc[1][0] * cam.R[j] + Jc[1][1] * cam.R[3 + j] + Jc[1][2] * cam.R[6 + j];
          }
          if constexpr (ROBUST) {
            gu = w * drho_u * (eu > 0 ? 1.0 : (eu < 0 ? -1.0 : 0.0));
            gv = w * drho_v * (ev > 0 ? 1.0 : (ev < 0 ? -1.0 : 0.0));
            hu = w * w * h_u;
            hv = w * w * h_v;
          } else {
            gu = w * (eu > 0 ? 1.0 : (eu < 0 ? -1.0 : 0.0));
            gv = w * (ev > 0 ? 1.0 : (ev < 0 ? -1.0 : 0.0));
            hu = w * w / fmax(fabs(eu), D.l1_eps);
            hv = w * w / fmax(fabs(ev), D.l1_eps);
          }
        }
      } else {
        const double iz = 1.0 / zc;
        const double a = xc * iz, b = yc * iz;
        const double r2 = a * a + b * b + 1e-12;
        const double r = sqrt(r2), ir = 1.0 / r;
        const double th = atan(r), th2 = th * th;
        const double poly = 1 + th2 * (cam.k1 + th2 * (cam.k2 + th2 * (cam.k3 + th2 * cam.k4)));
        const double thD = th * poly, m = thD * ir;
        const double eu = w * (cam.fx * a * m + cam.cx - um), ev = w * (cam.fy * b * m + cam.cy - vm);
        if constexpr (ROBUST) {
          redescending<JAC>(D.loss, eu, rho_u, drho_u, h_u);
          redescending<JAC>(D.loss, ev, rho_v, drho_v, h_v);
          my_cost = rho_u + rho_v;
        } else {
          my_cost = fabs(eu) + fabs(ev);
        }
        if (JAC) {
          const double dthD = 1 + th2 * (3 * cam.k1 + th2 * (5 * cam.k2 + th2 * (7 * cam.k3 + th2 * 9 * cam.k4)));
          const double dm_dr = (dthD / (1 + r2) * r - thD) * (ir * ir);
          const double dm_da = dm_dr * a * ir, dm_db = dm_dr * b * ir;
          const double du_da = cam.fx * (m + a * dm_da), du_db = cam.fx * a * dm_db;
          const double dv_da = cam.fy * b * dm_da, dv_db = cam.fy * (m + b * dm_db);
          const double uc0 = du_da * iz, uc1 = du_db * iz, uc2 = -(du_da * a + du_db * b) * iz;
          const double vc0 = dv_da * iz, vc1 = dv_db * iz, vc2 = -(dv_da * a + dv_db * b) * iz;
#pragma unroll
          for (int j = 0; j < 3; ++j) {
            ju[j] = uc0 * cam.R[j] + uc1 * cam.R[3 + j] + uc2 * cam.R[6 + j];
            jv[j] = vc0 * cam.R[j] + vc1 * cam.R[3 + j] + vc2 * cam.R[6 + j];
          }
          if constexpr (ROBUST) {
            gu = w * drho_u * (eu > 0 ? 1.0 : (eu < 0 ? -1.0 : 0.0));
            gv = w * drho_v * (ev > 0 ? 1.0 : (ev < 0 ? -1.0 : 0.0));
            hu = w * w * h_u;
            hv = w * w * h_v;
          } else {
            gu = w * (eu > 0 ? 1.0 : (eu < 0 ? -1.0 : 0.0));
            gv = w * (ev > 0 ? 1.0 : (ev < 0 ? -1.0 : 0.0));
            hu = w * w / fmax(fabs(eu), D.l1_eps);
            hv = w * w / fmax(fabs(ev), D.l1_eps);
          }
        }
      }
    }
    if (JAC) {
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        jrow[r0 * 3 + j] = ju[j];
        jrow[(r0 + 1) * 3 + j] = jv[j];
      }
      gsr[r0] = gu;
      gsr[r0 + 1] = gv;
      hwr[r0] = hu;
      hwr[r0 + 1] = hv;
      if constexpr (FISHER && ROBUST) {
        fwr[r0] = hu;                        // w^2 h(e): the Gauss-Newton curvature of the stated objective, u and v separately
        fwr[r0 + 1] = hv;
      } else if constexpr (FISHER) {
        fwr[r0] = fwr[r0 + 1] = w * w;
      }
    }
  }
  if (JAC) {
    for (int e = tid; e < R * lda; e += 256) A[e] = 0.0;
    __syncthreads();
    // residual Jacobian: root columns, then one entry per (row, op on the pose's path, enabled angle of the op's parent)
    for (int e = tid; e < R * 3; e += 256) A[(e / 3) * lda + e % 3] = jrow[e];
    for (int e = tid; e < R * NOPS; e += 256) {
      const int r = e / NOPS, k = e % NOPS, l = r / (2 * C);
      if ((D.pmask[l] >> k) & 1ull) {
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
          const int p = D.amap[k][ax];
          if (p >= 0) {
            const double* dv = opv + (k * 4 + 1 + ax) * 3;
            A[r * lda + p] = jrow[r * 3] * dv[0] + jrow[r * 3 + 1] * dv[1] + jrow[r * 3 + 2] * dv[2];
          }
        }
      }
    }
    __syncthreads();
    // H_n = A^T W A (upper pairs, mirrored), g_n = A^T gs (+ the smoothness terms, as the cheetah assembly)
    const double b0 = band_coef(n % D.n_frames, 0, D.n_frames);      // (position inside the clip)
    for (int e = tid; e < P * P; e += 256) {
      const int p = e / P, pc = e % P;
      if (pc < p) continue;
      double s = 0.0;
      if constexpr (FISHER) {
        for (int r = 0; r < R; ++r) s += fwr[r] * A[r * lda + p] * A[r * lda + pc];
        if (p == pc) {
          double sd = 0.0;                                        // the solver's diagonal, in its own summation order
          for (int r = 0; r < R; ++r) sd += hwr[r] * A[r * lda + p] * A[r * lda + pc];
          hd[(size_t)n * P + p] = sd + 2.0 * D.q * b0;
          s += 2.0 * D.q * b0;
        }
      } else {
        for (int r = 0; r < R; ++r) s += hwr[r] * A[r * lda + p] * A[r * lda + pc];
        if (p == pc) {
          s += 2.0 * D.q * b0;
          hd[(size_t)n * P + p] = s;
        }
      }
      H[((size_t)n * P + p) * P + pc] = s;
      H[((size_t)n * P + pc) * P + p] = s;
    }
  }
  if (tid < P) {
    const double* xc = x + (size_t)n * P + tid;
    const int nl = n % D.n_frames;                            // position inside the clip: no coupling across clips
    if (nl >= 3) {
      const double d3 = xc[0] - 3.0 * xc[-P] + 3.0 * xc[-2 * P] - xc[-3 * P];
      my_cost += D.q * d3 * d3;
    }
    if (JAC) {
      double gs = 0.0;
#pragma unroll
      for (int k = -3; k <= 3; ++k) {
        const int nn = nl + k;
        if (nn < 0 || nn >= D.n_frames) continue;
        const double bc = k >= 0 ? band_coef(nl, k, D.n_frames) : band_coef(nn, -k, D.n_frames);
        gs += bc * xc[k * P];
      }
      double gm = 0.0;
      for (int r = 0; r < R; ++r) gm += gsr[r] * A[r * lda + tid];
      g[(size_t)n * P + tid] = gm + 2.0 * D.q * gs;
    }
  }
  for (int off = 32; off > 0; off >>= 1) my_cost += __shfl_down(my_cost, off, 64);
  if ((tid & 63) == 0) red[tid >> 6] = my_cost;
  __syncthreads();
  if (tid == 0) cost_part[n] = (red[0] + red[1]) + (red[2] + red[3]);
}

// the eight kernels of the solve and the four of the Fisher assembly, as function-pointer types
using SkelAssembleKernel = decltype(&k_skel_assemble<true, false, false>);
using SkelFisherKernel = decltype(&k_skel_assemble<true, false, false, double>);

}  // namespace acino
