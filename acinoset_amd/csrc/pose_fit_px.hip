// Per-frame cheetah pose fit from the detections of every camera (gfx950, fp64): acino_cheetah_pose_fit_px.
//
// Per frame the minimiser, over the 25 active states x inside the box of the FTE, of
//   F(x) = 1/sigma_px^2 sum_{(c,l) valid} sum_{k in (u,v)} 1/2 f^2 log1p(r_k^2 / f^2) + 1/2 sum_{p = 3..24} (x_p - m_p)^2 / prior_sigma^2
// with r = pi_c(FK_l(x)) - z_{n,c,l}: the calibration-level projection and the per-coordinate Cauchy loss of
// triangulate_mv.hip (mv_project, pinhole.hpp), a detection valid when its likelihood is above thresh and its pixel finite.
// No triangulation stands between a detection and the skeleton: a marker one camera sees enters.  Gradient and matrix carry the
// IRLS weight w = 1 / (1 + r_k^2 / f^2), J = (J_pi R_c) J_FK; the same A serves step, predicted reduction, active set and
// outputs, so the frame after its prologue is pf_fit_frame<25> of pose_fit_dev.hpp as pose_fit.hip runs it, and this file is its
// third model, CheetahPxFit: CheetahCore of pose_fit_cheetah.hpp (FK frames, raw marker Jacobian, register-resident factor,
// cov_x) plus the measurement, whose arithmetic is pose_fit_px_dev.hpp's, shared with skel_pose_fit_px.hip.
//
// One 64-lane wave per frame, one launch, a grid-stride loop over the frames.  Static LDS 34 016 bytes: two FK frames, the raw
// J_FK as 25 columns of 60, one camera's weighted rows Jc as 26 columns of 40 (the rows of the Cholesky factor lie over them:
// linearise is done with Jc before the next factor is stored), A, and a group of three cameras' 2 x 3 blocks and residuals.
// Dynamic LDS: the n_cams camera records (once per launch) and the frame's detections, 672 bytes per fisheye camera, 736 per
// pinhole camera (4 032 at 6 cameras: 38 048 bytes in all, four workgroups per CU; 45 792 at 16 pinhole cameras).
//   eval       the 20 C (camera, marker) pairs over the lanes, pair t = lane + 64 k: project, add the two log terms; the
//              ridge terms by lanes 3..24; the 64 partial sums by a butterfly of lane exchanges, whose additions pair the same
//              operands in every lane: every lane holds the same bits, the same from run to run.  +inf when a valid pair has
//              z_c <= 0.
//   linearise  J_FK once.  Then three cameras at a time, 20 markers each over 60 lanes: a lane projects its marker and leaves
//              sqrt(w) / sigma_px * (J_pi R_c) (2 x 3) and sqrt(w) / sigma_px * r.  Then camera by camera: the 500 (state,
//              marker) entries of Jc = that block times J_FK[l] over the lanes (exact zeros for an invalid detection and
//              outside a column's markers), the 40 weighted residuals beside them as a 26th column, and 10 k-steps of 4 rows
//              into the three accumulator tiles of pf_normal on the fp64 matrix cores, carried across the cameras.  Row 25 of
//              the product is Jc^T (sqrt(w) r / sigma_px) = g without its ridge: the gradient comes out of the tiles that give
//              A, summed in (camera, row) order by the k-steps.  A camera without a valid detection is skipped.  The full
//              40 C x 25 Jacobian is never in LDS.  (Measured at 10 000 frames x 6 cameras, NOTES_perf.md: 10.96 ms with g by a
//              loop over each column's markers per camera, 47 080 bytes of LDS and one camera projected at a time; 7.60 ms with g
//              from the tiles and 35 168 bytes; 6.37 ms with three cameras projected at a time.)
//   outputs    the count of valid detections (uint16: it exceeds a byte) and the weights at the returned x, stored by the
//              model (outputs_at_x); PoseFitIo's nmarkers is NULL.
#include "pose_fit_cheetah.hpp"
#include "pose_fit_px_dev.hpp"

namespace acino {

constexpr int PX_ROWS = 2 * NL;       // 40 rows of one camera: (u, v) of marker l in rows 2 l, 2 l + 1
constexpr int PX_GROUP = 3;           // cameras projected in one pass: 20 markers each over 60 of the 64 lanes

struct PxLds {
  CovFrame F[2];
  double Jw[NP][PF_ROWS + 1];   // (+ 1: columns on unlike LDS banks) column p of J_FK, zero outside the column's markers
  union {                       // (linearise is done with Jc before the next factor is stored)
    double Jc[NP + 1][PX_ROWS + 1];   // column p of one camera's weighted rows; column 25: sqrt(w) / sigma_px * r
    double L[NP][PF_LD];        // rows of the Cholesky factor (pf_factor)
  };
  double A[NP][PF_LD];          // sum w J^T J / sigma_px^2 + diag(kappa); the inverse of the free block for the outputs
  double jr[PX_GROUP][NL][6];   // of a group of cameras: sqrt(w) / sigma_px * (J_pi R_c) of marker l, the row of u, the row of v
  double ur[PX_GROUP][PX_ROWS]; // and sqrt(w) / sigma_px * r
  double x[NP], xt[NP], m[NP], g[NP];
  double red[64];
  unsigned colmask[NP];         // the markers that move with state p
  unsigned vmask[ACINO_MAX_CAMS];   // the markers with a valid detection in camera c
};

template <bool PINHOLE>
struct CheetahPxFit : CheetahCore<PxLds> {
  typedef PxLds Lds;
  typedef CheetahCore<Lds> Core;
  using Core::S;
  using Core::cur;
  using Core::lane;
  using Core::piv;
  const PxArgs& b;
  const CamRec<PINHOLE>* const cams;     // the records and the frame's detections, in the dynamic LDS
  const double* const det;
  const double kappa;
  const int64_t n;
  const int n_det;

  __device__ __forceinline__ CheetahPxFit(Lds& S_, const int (&piv_)[PF_TASKS], int lane_, const PxArgs& b_,
                                          const CamRec<PINHOLE>* cams_, const double* det_, double kappa_, int64_t n_, int n_det_)
      : Core(S_, piv_, lane_), b(b_), cams(cams_), det(det_), kappa(kappa_), n(n_), n_det(n_det_) {}

  // F(xv): FK into the iterate's frame or the trial's, the pairs over the lanes, the same sum in every lane
  __device__ __forceinline__ double eval(const double* xv, bool trial) {
    CovFrame& T = S.F[trial ? cur ^ 1 : cur];
    pf_frame(T, xv, lane);
    double part = 0.0;
    bool behind = false;
    const int pairs = NL * b.n_cams;
    for (int t = lane; t < pairs; t += 64) {
      const int c = t / NL, l = t - c * NL;
      if (!((S.vmask[c] >> l) & 1u)) continue;
      part += px_pair_cost(b, cams[c], T.pos[l], det, t, behind);
    }
    return px_cost_finish(part, xv, S.m, kappa, NP, lane, b, behind);
  }

  // J_FK, then A and g at S.x camera by camera
  __device__ __forceinline__ void linearise() {
    const CovFrame& F = S.F[cur];
    pf_jacobian<true>(S, F, 0u, piv, lane);
    const int i = lane & 15, k4 = lane >> 4;
    const bool upper = 16 + i < NP + 1;           // (column 25, the residuals, rides in the upper tiles: their row 9 is g)
    const double *plo = &S.Jc[i][k4], *phi = &S.Jc[upper ? 16 + i : 0][k4];
    d4 a00 = {0.0, 0.0, 0.0, 0.0}, a10 = a00, a11 = a00;
    const int cg = (lane >= NL) + (lane >= 2 * NL) + (lane >= 3 * NL), lg = lane - cg * NL;   // lane = 20 cg + lg
#pragma unroll 1
    for (int c0 = 0; c0 < b.n_cams; c0 += PX_GROUP) {
      // ---- three cameras at a time over 60 lanes: lane (cg, lg) projects marker lg in camera c0 + cg
      if (cg < PX_GROUP) {
        const int c = c0 + cg;
        double jr[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, u[2] = {0.0, 0.0};
        if (c < b.n_cams && ((S.vmask[c] >> lg) & 1u)) px_pair_rows(b, cams[c], F.pos[lg], det, NL, c, lg, jr, u);
#pragma unroll
        for (int k = 0; k < 6; ++k) S.jr[cg][lg][k] = jr[k];
        S.ur[cg][2 * lg] = u[0];
        S.ur[cg][2 * lg + 1] = u[1];
      }
      __syncthreads();
      // ---- then camera by camera: its 40 rows of Jc, the residuals beside them, the three tiles
#pragma unroll 1
      for (int cc = 0; cc < PX_GROUP && c0 + cc < b.n_cams; ++cc) {
        const unsigned vm = S.vmask[c0 + cc];
        if (vm == 0u) continue;                   // (the same in every lane)
#pragma unroll
        for (int k = 0; k < PF_TASKS; ++k) {
          const int t = lane + 64 * k, p = t / NL, l = t - p * NL;
          if (t >= NP * NL) break;
          double v0 = 0.0, v1 = 0.0;
          if (piv[k] != -1 && ((vm >> l) & 1u)) {
            const double *a = &S.Jw[p][3 * l], *q = S.jr[cc][l];
            v0 = q[0] * a[0] + q[1] * a[1] + q[2] * a[2];
            v1 = q[3] * a[0] + q[4] * a[1] + q[5] * a[2];
          }
          S.Jc[p][2 * l] = v0;
          S.Jc[p][2 * l + 1] = v1;
        }
        if (lane < PX_ROWS) S.Jc[NP][lane] = S.ur[cc][lane];
        __syncthreads();
        double lo[PX_ROWS / 4], hi[PX_ROWS / 4];
#pragma unroll
        for (int s = 0; s < PX_ROWS / 4; ++s) {
          lo[s] = plo[4 * s];
          const double h = phi[4 * s];
          hi[s] = upper ? h : 0.0;
        }
#pragma unroll
        for (int s = 0; s < PX_ROWS / 4; ++s) {
          a00 = mfma(lo[s], lo[s], a00);
          a10 = mfma(hi[s], lo[s], a10);
          a11 = mfma(hi[s], hi[s], a11);
        }
        __syncthreads();                          // (Jc is free for the next camera, jr and ur after the last of the group)
      }
    }
    pf_store_tiles(S, a00, a10, a11, kappa, lane);
    if (k4 == 1) {                                // result[16 + 4 r + k4][.] with 4 r + k4 = 9: Jc^T (sqrt(w) r / sigma_px)
      S.g[i] = i >= 3 ? a10[2] + kappa * (S.x[i] - S.m[i]) : a10[2];
      if (16 + i < NP) S.g[16 + i] = a11[2] + kappa * (S.x[16 + i] - S.m[16 + i]);
    }
    __syncthreads();
  }
  __device__ __forceinline__ void accepted() { cur ^= 1; }

  // the count of valid detections and, at the returned x (F[cur]), the weight every coordinate ended with
  __device__ __forceinline__ void outputs_at_x(bool live) {
    px_store_outputs(b, cams, det, NL, n, n_det, live, lane, [&](int c, int l) { return (S.vmask[c] >> l) & 1u; },
                     [&](int l) { return S.F[cur].pos[l]; });
  }
};

template <bool PINHOLE>
__global__ void __launch_bounds__(64) k_pose_fit_px(PoseFitIo a, PxArgs b) {
  constexpr int STRIDE = PINHOLE ? ACINO_PINHOLE_STRIDE : ACINO_CAM_STRIDE;
  __shared__ PxLds S;
  extern __shared__ __attribute__((aligned(16))) double px_dyn[];      // n_cams records, then the frame's detections
  double* const det = px_dyn + b.n_cams * STRIDE;
  const int lane = threadIdx.x;
  pf_colmask(S, lane);
  for (int e = lane; e < b.n_cams * STRIDE; e += 64) px_dyn[e] = b.cams[e];
  int piv[PF_TASKS];
  pf_tasks(lane, piv);
  const int frame_doubles = b.n_cams * NL * 3;
  for (int64_t n = blockIdx.x; n < a.n_frames; n += gridDim.x) {
    __syncthreads();                              // the previous frame is done with S (colmask and cams are complete)
    const double* src = b.det + n * frame_doubles;
    for (int e = lane; e < frame_doubles; e += 64) det[e] = src[e];
    __syncthreads();
    // ---- the valid detections, camera by camera
    int n_det = 0;
    for (int c = 0; c < b.n_cams; ++c) {
      bool valid = false;
      if (lane < NL) {
        const double* d = &det[(c * NL + lane) * 3];
        valid = px_valid(d, b.thresh);
      }
      const unsigned vm = (unsigned)(__ballot(valid) & 0xFFFFFull);
      if (lane == 0) S.vmask[c] = vm;
      n_det += __popc(vm);
    }
    // ---- the caller's start, clipped to the box: the first iterate and the centre of the ridge
    if (lane < NP) {
      const double v = pf_clip(a.x0[n * NP + lane], c_pf_lo[lane], c_pf_hi[lane]);
      S.m[lane] = v;
      S.x[lane] = v;
    }
    __syncthreads();
    CheetahPxFit<PINHOLE> m(S, piv, lane, b, reinterpret_cast<const CamRec<PINHOLE>*>(px_dyn), det, a.kappa, n, n_det);
    pf_fit_frame<NP>(m, a, n, lane, n_det);
  }
}

}  // namespace acino

using namespace acino;

extern "C" {

size_t acino_sizeof_pose_fit_px_params(void) { return sizeof(acino_pose_fit_px_params); }

int acino_cheetah_pose_fit_px(const acino_pose_fit_px_params* prm, const double* d_det, int64_t n_frames, int n_cams,
                              const double* d_cams, const double* d_x0, double* d_x, double* d_cost, uint16_t* d_ndet,
                              uint8_t* d_status, uint8_t* d_iters, uint8_t* d_pinned, double* d_cov_x, double* d_pos,
                              double* d_cov_pos, double* d_std_pos, double* d_weight, void* stream) {
  ACINO_REQUIRE(prm != nullptr, "prm");
  acino_pose_fit_params fit;
  if (int rc = px_check_params(prm, n_frames, n_cams, ACINO_N_MARKERS, "min_detections must be 1..20 n_cams", fit)) return rc;
  if (n_frames == 0) return ACINO_OK;
  ACINO_REQUIRE(d_det && d_cams && d_x0 && d_x && d_status, "null buffer (d_det, d_cams, d_x0, d_x, d_status)");
  PoseFitIo a;
  pf_fill_io(a, &fit, nullptr, nullptr, d_x0, n_frames, d_x, d_cost, nullptr, d_status, d_iters, d_pinned, d_cov_x, d_pos,
             d_cov_pos, d_std_pos);
  PxArgs b;
  px_fill_args(b, prm, d_det, d_cams, n_cams, d_ndet, d_weight);
  const int grid = grid_for(n_frames, 1);       // one frame per workgroup pass, grid-stride beyond the cap
  const size_t record = prm->camera_model == 1 ? ACINO_PINHOLE_STRIDE : ACINO_CAM_STRIDE;
  const size_t dyn = (size_t)n_cams * (record + ACINO_N_MARKERS * 3) * sizeof(double);    // at most 11 776 bytes: no opt-in needed
  if (prm->camera_model == 1)
    hipLaunchKernelGGL(k_pose_fit_px<true>, dim3(grid), dim3(64), dyn, (hipStream_t)stream, a, b);
  else
    hipLaunchKernelGGL(k_pose_fit_px<false>, dim3(grid), dim3(64), dyn, (hipStream_t)stream, a, b);
  ACINO_LAUNCH_CHECK();
  return ACINO_OK;
}

}  // extern "C"
