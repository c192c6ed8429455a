// A skeleton-FTE iterate seen in image space (gfx950, fp64): per (clip, frame, camera, pose slot) the predicted pixel, its
// 2 x 2 covariance J_pi sym(cov_pos) J_pi^T, the residual against the detection, a gating distance under the stated Laplace
// noise and flags (acinoset_hip.h: acino_skel_fte_reprojection).  The generic-skeleton counterpart of fte_reproj.hip.
//
// One launch over all n_clips * N frames (frames are independent: clip boundaries mean nothing here).  A workgroup of 256
// threads handles SKR_FPB frames in three phases with a barrier between them:
//   A  one thread per (frame, link op): M(parent's own angles) off into LDS - R_loc = Rz(psi) Rx(phi) Ry(theta) of the
//      enabled angles, itself or transposed, as skel_pose_row and the assembly body evaluate it; no derivatives
//   B  one thread per (frame, coordinate): the link program in order, pose[child] = pose[parent] + op
//   C  the workgroup's nf * C * n_pose (frame, camera, pose slot) entries dealt to the threads in OUTPUT order, so every
//      output array is written as one contiguous run per workgroup.  Fisheye: fisheye_nlp_uv / fisheye_nlp_jac (pt3d_to_2d's
//      arithmetic, r^2 + 1e-12 included); pinhole: pinhole_project<true>.
// The problem description - sizes, the link program, the active index of every op's parent angles: 2.9 KB - travels as a kernel
// argument, and the camera records are read where the caller keeps them: no workspace, no upload, no synchronisation, no
// atomics.  LDS: SKR_FPB * (64 * 3 + 65 * 3) doubles = 24.2 KB whatever the skeleton (six workgroups per CU by LDS; the
// register count decides).  A streaming kernel: 24 B of detection and weight and the slot's 72 B of cov_pos (shared by the C
// cameras through the cache) in, up to 81 B out per entry, a few hundred fp64 operations with one atan in between.
// acino_skel_fte_reprojection_weights adds the curvature weights of the params block's loss (16 B per entry more; under the
// redescending loss two exp per weighted entry).
#include "skel_host.hpp"

namespace acino {

constexpr int SKR_FPB = 8;         // frames per workgroup

struct SkelReprojArgs {            // by value in the kernel-argument segment (limit 4 KB)
  int32_t n_cams, n_pose, n_ops, n_act;
  acino_skel_op op[ACINO_SKEL_MAX_OPS];
  int8_t amap[ACINO_SKEL_MAX_OPS][4];
};
static_assert(sizeof(SkelReprojArgs) <= 3072, "the kernel-argument segment holds 4 KB");

// ROBUST (acino_skel_fte_params::loss = ACINO_SKEL_LOSS_REDESCENDING): weight_out takes the curvature weight h(w res_d) the
// robust solve gives each component of a weighted detection (fte_reproj.hip's `weight`), and the gating distance uses the
// Gaussian core of that loss - rho(e) = e^2 / 2 near 0: noise of scale 1 / w, variance 1 / w^2 - in place of the Laplace
// variance 2 / w^2.  Without it weight_out, when asked for, is 1 for a weighted detection: L1 rejects nothing.
template <bool PINHOLE, bool ROBUST = false>
__global__ void __launch_bounds__(256)
k_skel_reproj(const SkelReprojArgs A, long long n_total, const double* __restrict__ meas, const double* __restrict__ wgt,
              const double* __restrict__ cams, const double* __restrict__ x, const double* __restrict__ cov_pos, double gate_w,
              double* __restrict__ uv_out, double* __restrict__ cov_out, double* __restrict__ res_out,
              double* __restrict__ m2_out, uint8_t* __restrict__ flags_out, const LossC loss, double* __restrict__ weight_out) {
  __shared__ double opv[SKR_FPB][ACINO_SKEL_MAX_OPS][3];          // M off of every op
  __shared__ double pos[SKR_FPB][ACINO_SKEL_MAX_OPS + 1][3];      // poses
  const int tid = threadIdx.x;
  const int C = A.n_cams, NPOSE = A.n_pose, NOPS = A.n_ops, P = A.n_act;
  const long long f0 = (long long)blockIdx.x * SKR_FPB;
  const int nf = (int)min((long long)SKR_FPB, n_total - f0);
  // ---- A: link operators
  for (int task = tid; task < nf * NOPS; task += 256) {
    const int f = task / NOPS, k = task - f * NOPS;
    const double* xs = x + (f0 + f) * P;
    const acino_skel_op& o = A.op[k];
    const int fl = o.flags;
    double sp = 0, cp = 1, st = 0, ct = 1, sz = 0, cz = 1;
    if (fl & 1) sincos(A.amap[k][0] >= 0 ? xs[A.amap[k][0]] : 0.0, &sp, &cp);
    if (fl & 2) sincos(A.amap[k][1] >= 0 ? xs[A.amap[k][1]] : 0.0, &st, &ct);
    if (fl & 4) sincos(A.amap[k][2] >= 0 ? xs[A.amap[k][2]] : 0.0, &sz, &cz);
    // Rx Ry, then Rz (Rx Ry): Ry = [ct 0 -st; 0 1 0; st 0 ct], Rx = [1 0 0; 0 cp sp; 0 -sp cp], Rz = [cz sz 0; -sz cz 0; 0 0 1]
    const double q[3][3] = {{ct, 0.0, -st}, {sp * st, cp, sp * ct}, {cp * st, -sp, cp * ct}};
    double M[3][3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      M[0][j] = cz * q[0][j] + sz * q[1][j];
      M[1][j] = -sz * q[0][j] + cz * q[1][j];
      M[2][j] = q[2][j];
    }
    const bool untr = (fl & 8) != 0;     // bit 3: R_loc itself, else its transpose
#pragma unroll
    for (int i = 0; i < 3; ++i)
      opv[f][k][i] = untr ? M[i][0] * o.off[0] + M[i][1] * o.off[1] + M[i][2] * o.off[2]
                          : M[0][i] * o.off[0] + M[1][i] * o.off[1] + M[2][i] * o.off[2];
  }
  __syncthreads();
  // ---- B: the chain, one thread per (frame, coordinate), in program order
  if (tid < nf * 3) {
    const int f = tid / 3, j = tid - f * 3;
    const double root = x[(f0 + f) * P + j];
    for (int s = 0; s < NPOSE; ++s) pos[f][s][j] = root;
    for (int k = 0; k < NOPS; ++k) pos[f][A.op[k].child][j] = pos[f][A.op[k].parent][j] + opv[f][k][j];
  }
  __syncthreads();
  // ---- C: one (frame, camera, pose slot) per thread and turn
  const double nan = __builtin_nan("");
  const int per_frame = C * NPOSE;
  for (int task = tid; task < nf * per_frame; task += 256) {
    const int f = task / per_frame, rem = task - f * per_frame;
    const int ci = rem / NPOSE, l = rem - ci * NPOSE;
    const long long n = f0 + f;
    const long long e = f0 * per_frame + task;                    // = (n * C + ci) * n_pose + l
    const double px = pos[f][l][0], py = pos[f][l][1], pz = pos[f][l][2];
    const double um = meas[2 * e], vm = meas[2 * e + 1], w = wgt[e];
    const bool finite = m_finite(um) && m_finite(vm);
    const double* cam = cams + (size_t)ci * (PINHOLE ? ACINO_PINHOLE_STRIDE : ACINO_CAM_STRIDE);
    const double* Rc = cam + (PINHOLE ? offsetof(Pin, R) : offsetof(Cam, R)) / sizeof(double);
    const double* tc = cam + (PINHOLE ? offsetof(Pin, t) : offsetof(Cam, t)) / sizeof(double);
    const double xc = Rc[0] * px + Rc[1] * py + Rc[2] * pz + tc[0];
    const double yc = Rc[3] * px + Rc[4] * py + Rc[5] * pz + tc[1];
    const double zc = Rc[6] * px + Rc[7] * py + Rc[8] * pz + tc[2];
    const bool behind = zc < 1e-6, sing = fabs(zc) < 1e-9;
    const bool weighted = w != 0.0 && finite && !sing;            // the assembly's rule (skel_assemble.hpp)
    double u = nan, v = nan, ru = nan, rv = nan, m2 = nan, s00 = nan, s01 = nan, s11 = nan;
    double hu = weighted ? 1.0 : 0.0, hv = hu;
    if (!sing) {
      double jc[2][3];
      if (PINHOLE) {
        double uv[2];
        pinhole_project<true>(*reinterpret_cast<const Pin*>(cam), xc, yc, zc, uv, jc);
        u = uv[0];
        v = uv[1];
      } else {
        FisheyeNlp fp;
        const Cam& fc = *reinterpret_cast<const Cam*>(cam);
        fisheye_nlp_uv(fc, xc, yc, zc, fp, u, v);
        fisheye_nlp_jac(fc, fp, jc[0], jc[1]);
      }
      if (finite) {
        ru = u - um;
        rv = v - vm;
      }
      if (ROBUST && weighted) {
        double rho, drho;
        redescending<true>(loss, w * (u - um), rho, drho, hu);
        redescending<true>(loss, w * (v - vm), rho, drho, hv);
      }
      const double wg = w > 0.0 ? w : gate_w;
      if (cov_pos) {
        double ju[3], jv[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          ju[j] = jc[0][0] * Rc[j] + jc[0][1] * Rc[3 + j] + jc[0][2] * Rc[6 + j];
          jv[j] = jc[1][0] * Rc[j] + jc[1][1] * Rc[3 + j] + jc[1][2] * Rc[6 + j];
        }
        const double* S = cov_pos + (n * NPOSE + l) * 9;
        double tu[3], tv[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          tu[i] = S[3 * i] * ju[0] + S[3 * i + 1] * ju[1] + S[3 * i + 2] * ju[2];
          tv[i] = S[3 * i] * jv[0] + S[3 * i + 1] * jv[1] + S[3 * i + 2] * jv[2];
        }
        s00 = ju[0] * tu[0] + ju[1] * tu[1] + ju[2] * tu[2];
        s11 = jv[0] * tv[0] + jv[1] * tv[1] + jv[2] * tv[2];
        s01 = 0.5 * ((ju[0] * tv[0] + ju[1] * tv[1] + ju[2] * tv[2]) + (jv[0] * tu[0] + jv[1] * tu[1] + jv[2] * tu[2]));
        const double r2 = (ROBUST ? 1.0 : 2.0) / (wg * wg);        // variance of Laplace noise of scale 1 / wg (ROBUST: Gaussian)
        const double a00 = s00 + r2, a11 = s11 + r2;
        m2 = (a11 * ru * ru - 2.0 * s01 * ru * rv + a00 * rv * rv) / (a00 * a11 - s01 * s01);
      } else {
        m2 = (ru * ru + rv * rv) * ((ROBUST ? 1.0 : 0.5) * wg * wg);
      }
    }
    if (uv_out) {
      uv_out[2 * e] = u;
      uv_out[2 * e + 1] = v;
    }
    if (cov_out) {
      cov_out[4 * e] = s00;
      cov_out[4 * e + 1] = s01;
      cov_out[4 * e + 2] = s01;
      cov_out[4 * e + 3] = s11;
    }
    if (res_out) {
      res_out[2 * e] = ru;
      res_out[2 * e + 1] = rv;
    }
    if (m2_out) m2_out[e] = m2;
    if (flags_out) flags_out[e] = (uint8_t)((weighted ? 1 : 0) | (behind ? 2 : 0) | (sing ? 4 : 0));
    if (weight_out) {
      weight_out[2 * e] = hu;
      weight_out[2 * e + 1] = hv;
    }
  }
}

}  // namespace acino

using namespace acino;

// the body of both entries (d_weight: NULL from the entry without it)
static int skel_reproject(const acino_skel_fte_params* p, int n_clips, int camera_model, const acino_skel_op* h_ops,
                          const int32_t* h_active, const double* d_meas, const double* d_w, const double* d_cams,
                          const double* d_x, const double* d_cov_pos, double gate_w, double* d_uv, double* d_cov_uv,
                          double* d_res, double* d_mahal2, uint8_t* d_flags, double* d_weight, void* stream) {
  int rc = skel_check_batch(p, n_clips, false, camera_model, h_ops && h_active && d_meas && d_w && d_cams && d_x);
  if (rc) return rc;
  ACINO_REQUIRE(gate_w > 0 && gate_w <= 1.79769313486231570e308, "gate_w > 0 and finite");
  ACINO_REQUIRE(d_uv || d_cov_uv || d_res || d_mahal2 || d_flags || d_weight,
                "no output: at least one of d_uv, d_cov_uv, d_res, d_mahal2, d_flags");
  ACINO_REQUIRE(!d_cov_uv || d_cov_pos, "d_cov_uv needs d_cov_pos");
  const long long NT = (long long)p->n_frames * n_clips;      // frames of all clips
  SkelDev h;                                                 // (the host half of the record: the checks of skel_program)
  if ((rc = skel_program(p, h_ops, h_active, h))) return rc;
  SkelReprojArgs a;
  memset(&a, 0, sizeof(a));
  a.n_cams = p->n_cams;
  a.n_pose = p->n_pose;
  a.n_ops = p->n_ops;
  a.n_act = p->n_active;
  memcpy(a.op, h.op, sizeof(a.op));
  memcpy(a.amap, h.amap, sizeof(a.amap));
  const unsigned nb = (unsigned)((NT + SKR_FPB - 1) / SKR_FPB);
  const auto kernel = p->loss == ACINO_SKEL_LOSS_REDESCENDING
                          ? skel_camera_kernel(camera_model, k_skel_reproj<false, true>, k_skel_reproj<true, true>)
                          : skel_camera_kernel(camera_model, k_skel_reproj<false>, k_skel_reproj<true>);
  hipLaunchKernelGGL(kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, a, NT, d_meas, d_w, d_cams, d_x, d_cov_pos, gate_w, d_uv,
                     d_cov_uv, d_res, d_mahal2, d_flags, h.loss, d_weight);
  ACINO_LAUNCH_CHECK();
  return ACINO_OK;
}

extern "C" {

int acino_skel_fte_reprojection(const acino_skel_fte_params* p, int n_clips, int camera_model, const acino_skel_op* h_ops,
                                const int32_t* h_active, const double* d_meas, const double* d_w, const double* d_cams,
                                const double* d_x, const double* d_cov_pos, double gate_w, double* d_uv, double* d_cov_uv,
                                double* d_res, double* d_mahal2, uint8_t* d_flags, void* stream) {
  return skel_reproject(p, n_clips, camera_model, h_ops, h_active, d_meas, d_w, d_cams, d_x, d_cov_pos, gate_w, d_uv, d_cov_uv, d_res,
                        d_mahal2, d_flags, nullptr, stream);
}

int acino_skel_fte_reprojection_weights(const acino_skel_fte_params* p, int n_clips, int camera_model, const acino_skel_op* h_ops,
                                        const int32_t* h_active, const double* d_meas, const double* d_w, const double* d_cams,
                                        const double* d_x, const double* d_cov_pos, double gate_w, double* d_uv, double* d_cov_uv,
                                        double* d_res, double* d_mahal2, uint8_t* d_flags, double* d_weight, void* stream) {
  return skel_reproject(p, n_clips, camera_model, h_ops, h_active, d_meas, d_w, d_cams, d_x, d_cov_pos, gate_w, d_uv, d_cov_uv, d_res,
                        d_mahal2, d_flags, d_weight, stream);
}

}  // extern "C"
