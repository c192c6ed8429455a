// What the generic-skeleton kernels share - skel_fte.hip (the solve), skel_cov.hip (covariance and observability at an iterate),
// skel_sample.hip (joint samples), skel_calib.hip (the sensitivity to the extrinsics), skel_links.hip (the sensitivity to the
// link lengths) and skel_reproj.hip (the image-space report): the device-resident problem description, the controller state of a clip, the bound-active rule, the link program's forward kinematics, the parameter checks and the
// host-side compilation of the link program into SkelDev.  The host layer on top of it (entry checks, upload, dispatch,
// read-back) is skel_host.hpp.
#pragma once
#include <cstddef>
#include <cstring>
#include <vector>

#include "dense80.hpp"
#include "pinhole.hpp"

namespace acino {

constexpr int SK_MAXP = 64;        // active states per frame
constexpr int SK_MAXROWS = 256;    // residual rows per frame = 2 * poses * cameras

struct SkelDev {                   // device-resident description of one problem
  int32_t n_frames, n_cams, n_pose, n_ops, n_act, PT, n_rows, pad;
  double q;                        // model weight / h^4
  double l1_eps, lam_floor;
  acino_skel_op op[ACINO_SKEL_MAX_OPS];
  int8_t amap[ACINO_SKEL_MAX_OPS][4];              // per op: active index of the parent's phi, theta, psi (-1: none)
  unsigned long long pmask[ACINO_SKEL_MAX_OPS + 1];  // per pose slot: the ops on its path from the root
  Cam cams[ACINO_MAX_CAMS];
  Pin pins[ACINO_MAX_CAMS];        // the pinhole model's records (k_skel_assemble<., true, ...>); appended: the offsets above stay
  LossC loss;                      // the redescending loss's constants (a, b, c = 3, 10, 20); appended: the offsets above stay
  int32_t loss_kind, pad1;         // ACINO_SKEL_LOSS_L1 / ACINO_SKEL_LOSS_REDESCENDING: which measurement loss the problem states
};

template <bool PINHOLE>
__host__ __device__ __forceinline__ decltype(auto) cam_rec(const SkelDev& D, int c) {
  if constexpr (PINHOLE) return (D.pins[c]);
  else return (D.cams[c]);
}

struct SkelClip {                  // controller state of one clip (device)
  double F, lam, nu, gnorm, cost0, Ft, pred, step;
  int32_t cur, status, it, accepted, pivot_err, pad;
};

// the solver's bound-active rule: at a bound with the gradient pushing outward (d0: the IRLS diagonal of that variable)
__device__ __forceinline__ bool skel_fixed(double xv, double gv, double d0, double lo, double hi) {
  const double gtol = GRAD_ZERO_REL * d0;
  return (xv <= lo && gv > gtol) || (xv >= hi && gv < -gtol);
}

// poses of one frame from its active states: the link program, pose[child] = pose[parent] + M(parent's own angles) off
// (states outside the active set are 0).  xs[n_act] -> out[n_pose][3]; out is read back (a slot's parent), by this thread only.
__device__ __forceinline__ void skel_pose_row(const SkelDev& D, const double* __restrict__ xs, double* __restrict__ out) {
  for (int s = 0; s < D.n_pose; ++s)
    for (int j = 0; j < 3; ++j) out[s * 3 + j] = xs[j];
  for (int k = 0; k < D.n_ops; ++k) {
    const acino_skel_op& o = D.op[k];
    double Rm[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    if (o.flags & 2) {
      double s, c;
      sincos(D.amap[k][1] >= 0 ? xs[D.amap[k][1]] : 0.0, &s, &c);
      Rm[0][0] = c; Rm[0][2] = -s; Rm[2][0] = s; Rm[2][2] = c;
    }
    if (o.flags & 1) {
      double s, c;
      sincos(D.amap[k][0] >= 0 ? xs[D.amap[k][0]] : 0.0, &s, &c);
      for (int j = 0; j < 3; ++j) {
        const double r1 = Rm[1][j], r2 = Rm[2][j];
        Rm[1][j] = c * r1 + s * r2;
        Rm[2][j] = -s * r1 + c * r2;
      }
    }
    if (o.flags & 4) {
      double s, c;
      sincos(D.amap[k][2] >= 0 ? xs[D.amap[k][2]] : 0.0, &s, &c);
      for (int j = 0; j < 3; ++j) {
        const double r0 = Rm[0][j], r1 = Rm[1][j];
        Rm[0][j] = c * r0 + s * r1;
        Rm[1][j] = -s * r0 + c * r1;
      }
    }
    for (int i = 0; i < 3; ++i) {
      const double d = (o.flags & 8) ? Rm[i][0] * o.off[0] + Rm[i][1] * o.off[1] + Rm[i][2] * o.off[2]
                                     : Rm[0][i] * o.off[0] + Rm[1][i] * o.off[1] + Rm[2][i] * o.off[2];
      out[o.child * 3 + i] = out[o.parent * 3 + i] + d;
    }
  }
}

// column p of the pose Jacobian G_l (3 x n_act) of slot l: [I | d(M off)/d(angle) of the ops on the slot's path], from the link
// operators opv[n_ops][4][3] the assembly leaves (k_skel_cov_pose, k_skel_calib_rhs, k_skel_calib_combine, k_skel_links_rhs,
// k_skel_links_combine)
__device__ __forceinline__ void skel_pose_jac_col(const SkelDev& D, const double* __restrict__ opv, int l, int p, double (&gc)[3]) {
  gc[0] = p == 0 ? 1.0 : 0.0;
  gc[1] = p == 1 ? 1.0 : 0.0;
  gc[2] = p == 2 ? 1.0 : 0.0;
  const unsigned long long path = D.pmask[l];
  for (int k = 0; k < D.n_ops; ++k) {
    if (!((path >> k) & 1ull)) continue;
#pragma unroll
    for (int ax = 0; ax < 3; ++ax)
      if (D.amap[k][ax] == p) {
        const double* dv = opv + (k * 4 + 1 + ax) * 3;
        gc[0] += dv[0];
        gc[1] += dv[1];
        gc[2] += dv[2];
      }
  }
}

// dynamic LDS of the assembly kernels (skel_assemble.hpp), without the Fisher weights of the covariance's assembly
inline size_t skel_assemble_lds(int n_rows, int P) {
  return sizeof(double) * (SK_MAXP + ACINO_SKEL_MAX_OPS * 12 + (ACINO_SKEL_MAX_OPS + 1) * 3 + SK_MAXROWS * 5 + 8 +
                           (size_t)n_rows * (P | 1));
}

inline int skel_validate(const acino_skel_fte_params* p) {
  ACINO_REQUIRE(p != nullptr, "params");
  ACINO_REQUIRE(p->n_frames >= 1, "n_frames >= 1");
  ACINO_REQUIRE(p->n_cams >= 1 && p->n_cams <= ACINO_MAX_CAMS, "n_cams in 1..16");
  ACINO_REQUIRE(p->n_pose >= 1 && p->n_pose <= ACINO_SKEL_MAX_OPS + 1, "n_pose");
  ACINO_REQUIRE(p->n_ops >= 0 && p->n_ops <= ACINO_SKEL_MAX_OPS, "n_ops <= ACINO_SKEL_MAX_OPS");
  ACINO_REQUIRE(p->n_angles >= 1, "n_angles");
  ACINO_REQUIRE(p->n_active >= 3 && p->n_active <= SK_MAXP, "n_active in 3..64 (x, y, z and the angles that move a pose)");
  ACINO_REQUIRE(2 * p->n_pose * p->n_cams <= SK_MAXROWS, "2 * n_pose * n_cams <= 256 residual rows per frame");
  ACINO_REQUIRE(p->n_pose * p->n_cams <= 256, "n_pose * n_cams <= 256");
  ACINO_REQUIRE(p->h > 0 && p->model_weight >= 0 && p->l1_eps > 0, "h > 0, model_weight >= 0, l1_eps > 0");
  ACINO_REQUIRE(p->lam0 > 0 && p->max_iter >= 0, "lam0 > 0, max_iter >= 0");
  ACINO_REQUIRE(p->loss == ACINO_SKEL_LOSS_L1 || p->loss == ACINO_SKEL_LOSS_REDESCENDING, "loss: 0 L1, 1 redescending");
  return ACINO_OK;
}

// The host half of SkelDev (everything but the camera records, which are copied on the device): sizes, constants, the link
// program, the active index of every op's parent angles, the ops on every pose's path.  h_ops / h_active must not be NULL.
inline int skel_program(const acino_skel_fte_params* p, const acino_skel_op* h_ops, const int32_t* h_active, SkelDev& h) {
  const int N = p->n_frames, P = p->n_active, PT = (P + 15) / 16 * 16, L = p->n_angles;
  memset(&h, 0, sizeof(h));
  h.n_frames = N;
  h.n_cams = p->n_cams;
  h.n_pose = p->n_pose;
  h.n_ops = p->n_ops;
  h.n_act = P;
  h.PT = PT;
  h.n_rows = 2 * p->n_pose * p->n_cams;
  h.q = p->model_weight / (p->h * p->h * p->h * p->h);
  h.l1_eps = p->l1_eps;
  h.lam_floor = DIAG_FLOOR;
  h.loss = make_loss(3.0, 10.0, 20.0);                       // the reference's only call (build.py:307); the scale is r_meas
  h.loss_kind = p->loss;
  ACINO_REQUIRE(h_active[0] == 0 && h_active[1] == 1 && h_active[2] == 2, "the first three active states are x, y, z");
  std::vector<int> where(3 + 3 * L, -1);
  for (int a = 0; a < P; ++a) {
    ACINO_REQUIRE(h_active[a] >= 0 && h_active[a] < 3 + 3 * L && (a == 0 || h_active[a] > h_active[a - 1]),
                  "active state indices must be increasing and inside [0, 3 + 3 L)");
    where[h_active[a]] = a;
  }
  std::vector<unsigned long long> path(p->n_pose, 0ull);
  for (int k = 0; k < p->n_ops; ++k) {
    const acino_skel_op& o = h_ops[k];
    ACINO_REQUIRE(o.child >= 0 && o.child < p->n_pose && o.parent >= 0 && o.parent < p->n_pose, "op slot out of range");
    ACINO_REQUIRE(o.angle >= 0 && o.angle < L, "op angle index out of range");
    h.op[k] = o;
    for (int ax = 0; ax < 3; ++ax) {
      const int st = 3 + ax * L + o.angle;
      const int a = ((o.flags >> ax) & 1) ? where[st] : -1;
      ACINO_REQUIRE(!((o.flags >> ax) & 1) || a >= 0, "an enabled angle of a parent part is missing from the active states");
      h.amap[k][ax] = (int8_t)a;
    }
    h.amap[k][3] = -1;
    path[o.child] = path[o.parent] | (1ull << k);          // (a slot defined twice keeps its last definition, as the poses)
  }
  for (int l = 0; l < p->n_pose; ++l) h.pmask[l] = path[l];
  return ACINO_OK;
}

}  // namespace acino
