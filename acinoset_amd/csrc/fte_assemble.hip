// FTE residual / Jacobian / normal-equation assembly (gfx950, fp64).
//
// Reference: cheetah FK src/all_optimizations.py:66-190, projection pt3d_to_2d :193-209, weights
// :243-252,302-315, objective :486-500, loss src/build.py:382-395.
//
// One workgroup handles FPB frames in five LDS-staged phases:
//   A  sin/cos of the 22 active angles                       (frame, angle)
//   B  kinematic chain, column-parallel: RI_k[:,j], marker coordinate j, axis component j
//                                                            (frame, column j)
//   C  projection + analytic 2x3 Jacobian + robust weights for all cameras (the reference's fisheye pt3d_to_2d, or the
//      cv2.projectPoints pinhole model in k_fte_assemble_pinhole); per marker the
//      3x3 M_l = sum_c J^T W J, v_l = sum_c J^T w rho' and their 6x6 "spatial" form
//      Lambda_l = S_l^T M_l S_l, f_l = S_l^T v_l with S_l = [I, -[p_l]x]          (frame, marker)
//   D  subtree sums of Lambda / f over the kinematic tree     (frame, component)
//   E  H[a][b] = xi_a . (Lambda_sub(b) xi_b), g[b] = xi_b . f_sub(b) + smoothness      (frame, state)
// where xi = (pivot x omega, omega) is the joint twist: dp_l/dq_a = omega_a x (p_l - pivot_a).
// J (240x25 per frame) is never materialised; only H_n (25x25) and g_n leave the workgroup.
#include "cheetah_fk.hpp"
#include "dense80.hpp"

namespace acino {

// 6 408 B per frame: 8 frames = 51 KB per workgroup, so THREE workgroups share a CU (12 waves: the projection phase is a
// chain of fp64 transcendentals per thread and lives on latency hiding).  Two arrays share storage with one that is dead
// by the time they are written: the twists (phase C) take the place of sin / cos (phases A-B), the subtree sums (phase D)
// are written over the first NGRP rows of the per-marker blocks, column by column by the thread that has just read it.
struct FrameLds {
  static constexpr bool kHasOm = true;
  union {
    double sc[22][2];     // phases A-B: sin, cos of active angle (index a-3)
    double xi[22][6];     // phase C on: twist (pivot x omega, omega)
  };
  double pos[21][3];      // markers 0..19, head = 20
  double om[22][3];       // rotation axis of active angle in the inertial frame
  double lam[NL][27];     // per-marker 6x6 symmetric (21) + wrench (6); after phase D rows 0..NGRP-1 = subtree sums
};
static_assert(NGRP <= NL, "subtree sums are stored over the per-marker blocks");

// index of (i,j), i<=j, in the packed upper triangle of a 6x6
__device__ __forceinline__ int tri6(int i, int j) { return i * 6 - (i * (i - 1)) / 2 + (j - i); }

// float twin of redescending<> (common.hpp) for the mixed-precision rows of ACINO_PREC_BF16_ROWS
struct LossF {
  float a, b, c, ea, eb, ec, d0, t4, icb;
};
template <bool DERIV>
__device__ __forceinline__ void redescending_f(const LossF& L, float err, float& rho, float& drho, float& h) {
  const float e = fabsf(err);
  const float u = __expf(-e);
  const float da = 1.0f + L.ea * u, db = 1.0f + L.eb * u, dc = 1.0f + L.ec * u;
  const float inv = __frcp_rn(da * db * dc);
  const float sa = inv * (db * dc), sb = inv * (da * dc), sc = inv * (da * db);
  const float cb = L.c - L.b;
  const float t2 = L.a * e - L.a * L.a * 0.5f;
  const float ce = (L.c - e) * L.icb;
  const float t3 = L.a * L.b - L.a * L.a * 0.5f + (L.a * cb * 0.5f) * (1.0f - ce * ce);
  rho = (1.0f - sa) * 0.5f * e * e + (sa - sb) * t2 + (sb - sc) * t3 + sc * L.t4;
  if (DERIV) {
    const float dsa = sa * (1.0f - sa), dsb = sb * (1.0f - sb), dsc = sc * (1.0f - sc);
    drho = -dsa * 0.5f * e * e + (1.0f - sa) * e + (dsa - dsb) * t2 + (sa - sb) * L.a + (dsb - dsc) * t3 +
           (sb - sc) * (L.a * ce) + dsc * L.t4;
    const float hh = e > 1e-6f ? (drho - L.d0) * __frcp_rn(e) : 1.0f;
    h = fminf(fmaxf(hh, 0.0f), 1.0f);
  }
}

// PREC = ACINO_PREC_F64: everything fp64.  PREC = ACINO_PREC_BF16_ROWS (BASELINE config 5): camera-frame coordinates
// in fp64, projection / Jacobian / robust weights in fp32, the scaled residuals and the 2x3 Jacobian ROWS rounded to
// bf16, M_l and v_l accumulated in fp32; from Lambda_l on (phases C-tail, D, E) fp64 as before.  The cost is summed in
// fp64 from the UNROUNDED fp32 residuals (accept / reject decisions need more than 8 bits).
// SPLIT = 2 (short chains: fewer workgroups than the chip holds at once, so only the latency of ONE workgroup counts) deals the
// cameras of a (frame, marker) to two lanes next to each other - contiguous halves of the camera list, summed left + right:
// 8 frames x 20 markers x 2 = 320 threads, three cameras per lane instead of six.  (For long chains it loses: the kernel keeps
// ~165 registers, five-wave workgroups fit twice on a CU where four-wave ones fit three times - NOTES_perf.md round 6.)
template <bool JAC, int PREC, int SPLIT = 1>
__global__ void __launch_bounds__(SPLIT == 2 ? 2 * FPB * NL : 256)
k_fte_assemble(const FteConst* __restrict__ cst, const acino_fte_state* __restrict__ st, int which,
               const double* __restrict__ det, const double* __restrict__ x0, const double* __restrict__ x1,
               double* __restrict__ H0, double* __restrict__ H1, double* __restrict__ g0, double* __restrict__ g1,
               double* __restrict__ hd0, double* __restrict__ hd1, double* __restrict__ cost_partials,
               int* __restrict__ nbehind, int respect_status) {
#define ACINO_ASM_PINHOLE 0
#include "fte_assemble_body.inc"
#undef ACINO_ASM_PINHOLE
}

// The pinhole model (FteConst::camera_model == CAMERA_PINHOLE), fp64 only: a kernel name of its own, so that the fisheye
// kernels' names - which the profiling tools look up - and their code stay as they are.
template <bool JAC, int SPLIT>
__global__ void __launch_bounds__(SPLIT == 2 ? 2 * FPB * NL : 256)
k_fte_assemble_pinhole(const FteConst* __restrict__ cst, const acino_fte_state* __restrict__ st, int which,
                       const double* __restrict__ det, const double* __restrict__ x0, const double* __restrict__ x1,
                       double* __restrict__ H0, double* __restrict__ H1, double* __restrict__ g0, double* __restrict__ g1,
                       double* __restrict__ hd0, double* __restrict__ hd1, double* __restrict__ cost_partials,
                       int* __restrict__ nbehind, int respect_status) {
  constexpr int PREC = ACINO_PREC_F64;
#define ACINO_ASM_PINHOLE 1
#include "fte_assemble_body.inc"
#undef ACINO_ASM_PINHOLE
}

// ---- plain FK kernels (positions only) -----------------------------------------------------
__global__ void __launch_bounds__(256)
k_fk(const double* __restrict__ q, int64_t n_frames, int stride, int halo, int active_only, double* __restrict__ pos) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  FrameLds* F = reinterpret_cast<FrameLds*>(smem_raw);
  const int tid = threadIdx.x;
  const int64_t f0 = (int64_t)blockIdx.x * FPB;
  const int nf = (int)min((int64_t)FPB, n_frames - f0);
  const int8_t act[NP] = {0, 1, 2, 3, 4, 6, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 34, 35, 36};
  for (int task = tid; task < nf * NP; task += blockDim.x) {
    int f = task / NP, a = task - f * NP;
    double xv = q[(f0 + f + halo) * stride + (active_only ? a : act[a])];
    if (a < 3) {
      F[f].pos[20][a] = xv;
    } else {
      double s, c;
      sincos(xv, &s, &c);
      F[f].sc[a - 3][0] = s;
      F[f].sc[a - 3][1] = c;
    }
  }
  __syncthreads();
  for (int task = tid; task < nf * 3; task += blockDim.x) fk_columns(F[task / 3], task % 3);
  __syncthreads();
  for (int task = tid; task < nf * NL * 3; task += blockDim.x) {
    int f = task / (NL * 3), r = task - f * NL * 3;
    pos[(f0 + f) * NL * 3 + r] = F[f].pos[r / 3][r % 3];
  }
}

int n_assemble_blocks(int n_frames) { return (n_frames + FPB - 1) / FPB; }

// The 16 assembly kernels: [ACINO_PREC_* of the fisheye model, then the pinhole model][need_jac][SPLIT - 1]
using AssembleKernel = void (*)(const FteConst*, const acino_fte_state*, int, const double*, const double*, const double*,
                                double*, double*, double*, double*, double*, double*, double*, int*, int);
constexpr int ASM_ROW_PINHOLE = 3;
static_assert(ACINO_PREC_F64 == 0 && ACINO_PREC_BF16_ROWS == 1 && ACINO_PREC_BF16_RES == 2, "rows of kAssemble");
static const AssembleKernel kAssemble[4][2][2] = {
    {{k_fte_assemble<false, ACINO_PREC_F64, 1>, k_fte_assemble<false, ACINO_PREC_F64, 2>},
     {k_fte_assemble<true, ACINO_PREC_F64, 1>, k_fte_assemble<true, ACINO_PREC_F64, 2>}},
    {{k_fte_assemble<false, ACINO_PREC_BF16_ROWS, 1>, k_fte_assemble<false, ACINO_PREC_BF16_ROWS, 2>},
     {k_fte_assemble<true, ACINO_PREC_BF16_ROWS, 1>, k_fte_assemble<true, ACINO_PREC_BF16_ROWS, 2>}},
    {{k_fte_assemble<false, ACINO_PREC_BF16_RES, 1>, k_fte_assemble<false, ACINO_PREC_BF16_RES, 2>},
     {k_fte_assemble<true, ACINO_PREC_BF16_RES, 1>, k_fte_assemble<true, ACINO_PREC_BF16_RES, 2>}},
    {{k_fte_assemble_pinhole<false, 1>, k_fte_assemble_pinhole<false, 2>},
     {k_fte_assemble_pinhole<true, 1>, k_fte_assemble_pinhole<true, 2>}},
};

int launch_assemble(const FteConst* d_c, const FteConst& h_c, const acino_fte_state* d_st, int which,
                    const double* d_det, double* const x[2], double* const H[2], double* const g[2],
                    double* const hd[2], double* d_cost_partials, int* d_nbehind, bool need_jac, bool respect_status, hipStream_t s) {
  const int nb = n_assemble_blocks(h_c.n_frames);
  if (nb == 0) return ACINO_OK;
  const size_t lds = sizeof(FrameLds) * FPB + 64;
  static PerDeviceOnce attr;
  static int cus_of[64] = {};
  int dev = 0;
  ACINO_HIP_CHECK(hipGetDevice(&dev));
  if (attr.first()) {
    for (const auto& by_jac : kAssemble)
      for (const auto& by_split : by_jac)
        for (AssembleKernel k : by_split)
          ACINO_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    int cus = 0;
    ACINO_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    if (dev >= 0 && dev < 64) cus_of[dev] = cus;
  }
  // short chains - a workgroup per CU at most - take the camera-split variant: what counts there is the latency of one
  // workgroup, and its longest phase is the serial loop over the cameras (999 frames: 27.6 -> 23.9 us; with two workgroups on a
  // CU it loses already - 3 331 frames: 30 -> 43 us)
  int split = (dev >= 0 && dev < 64 && nb <= cus_of[dev]) ? 2 : 1;
  if (const char* e = getenv("ACINO_ASM_SPLIT")) split = atoi(e) == 2 ? 2 : 1;
  // (the pinhole model is fp64 only: acino_fte_create_pinhole / set_precision refuse the rest)
  const bool bf16 = h_c.precision == ACINO_PREC_BF16_ROWS || h_c.precision == ACINO_PREC_BF16_RES;
  const int row = h_c.camera_model == CAMERA_PINHOLE ? ASM_ROW_PINHOLE : (bf16 ? h_c.precision : ACINO_PREC_F64);
  hipLaunchKernelGGL(kAssemble[row][need_jac ? 1 : 0][split - 1], dim3(nb), dim3(split == 2 ? 2 * FPB * NL : 256), lds, s, d_c,
                     d_st, which, d_det, x[0], x[1], H[0], H[1], g[0], g[1], hd[0], hd[1], d_cost_partials, d_nbehind,
                     respect_status ? 1 : 0);
  ACINO_LAUNCH_CHECK();
  return ACINO_OK;
}

static int fk_attr() {
  static PerDeviceOnce attr;
  if (attr.first())
    ACINO_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_fk),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)(sizeof(FrameLds) * FPB)));
  return ACINO_OK;
}

int launch_fk(const double* d_q, int64_t n, double* d_pos, hipStream_t s) {
  if (n == 0) return ACINO_OK;
  if (int rc = fk_attr()) return rc;
  hipLaunchKernelGGL(k_fk, dim3((unsigned)((n + FPB - 1) / FPB)), dim3(256), sizeof(FrameLds) * FPB, s, d_q, n,
                     ACINO_N_STATES, 0, 0, d_pos);
  ACINO_LAUNCH_CHECK();
  return ACINO_OK;
}

int launch_fk_active(const double* d_xa_halo, int64_t n, double* d_pos, hipStream_t s) {
  if (n == 0) return ACINO_OK;
  if (int rc = fk_attr()) return rc;
  hipLaunchKernelGGL(k_fk, dim3((unsigned)((n + FPB - 1) / FPB)), dim3(256), sizeof(FrameLds) * FPB, s, d_xa_halo,
                     n, NP, HALO, 1, d_pos);
  ACINO_LAUNCH_CHECK();
  return ACINO_OK;
}

}  // namespace acino

extern "C" int acino_cheetah_fk(const double* d_q, int64_t n_frames, double* d_pos, void* stream) {
  using namespace acino;
  ACINO_REQUIRE(n_frames >= 0, "n_frames");
  if (n_frames == 0) return ACINO_OK;
  ACINO_REQUIRE(d_q && d_pos, "null buffer");
  return launch_fk(d_q, n_frames, d_pos, (hipStream_t)stream);
}
