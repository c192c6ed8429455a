/*
 * acinoset_hip.h - C ABI of libacinoset_hip.so (MI355X / gfx950, fp64).
 *
 * Drop-in boundary for the AcinoSet triangulation + Full-Trajectory-Estimation hot path.
 * The reference (pure Python) has no FFI; these are the entry points a binding for that path
 * binds, one per reference interface it replaces (paths relative to the AcinoSet tree):
 *
 *   acino_undistort_fisheye          cv2.fisheye.undistortPoints      src/calib/calib.py:124-125
 *   acino_triangulate_fisheye        triangulate_points_fisheye       src/calib/calib.py:121-130
 *   acino_triangulate_pinhole        triangulate_points               src/calib/calib.py:52-61
 *   acino_project_fisheye            project_points_fisheye           src/calib/calib.py:132-136
 *   acino_project_pinhole            project_points                   src/calib/calib.py:64-66
 *   acino_triangulate_pairs          get_pairwise_3d_points_from_df   src/calib/calib.py:394-423 (triangulate_func = triangulate_points_fisheye)
 *   acino_triangulate_pairs_pinhole  get_pairwise_3d_points_from_df   src/calib/calib.py:394-423 (triangulate_func = triangulate_points; app.py:215-218)
 *   acino_reproject_residuals        project(triangulate(.)) - pts    src/calib/calib.py:312-316 (cost_func_points_only)
 *   acino_triangulate_reproject      the two above fused (one pass over the detections)
 *   acino_triangulate_multiview      (no counterpart) robust N-view triangulation with a covariance per point, from the
 *                                    same dense detections as acino_triangulate_pairs
 *   acino_cheetah_pose_fit           (no counterpart) per-frame pose with error bars from 3-D marker points and their
 *                                    covariances (the outputs of acino_triangulate_multiview)
 *   acino_skel_pose_fit              (no counterpart) the same for a skeleton's link program (acino_skel_fte_*)
 *   acino_cheetah_pose_fit_px        (no counterpart) per-frame pose with error bars from the detections themselves: the
 *                                    reprojection error of the skeleton in every camera, robust weight per coordinate
 *   acino_skel_pose_fit_px           (no counterpart) the same for a skeleton's link program
 *   acino_cheetah_fk                 pose_to_3d                       src/all_optimizations.py:66-190
 *   acino_fte_*                      the Pyomo model + opt.solve()    src/all_optimizations.py:283-556
 *
 * Conventions
 *   - every function returns 0 on success or a negative acino_status; no C++ exception and no
 *     abort crosses the boundary; acino_last_error_string() describes the last failure (thread-local).
 *   - all pointers named d_* are DEVICE pointers (HBM), caller-allocated and caller-owned; the
 *     library allocates no device memory.  FTE scratch is one caller buffer whose size comes
 *     from acino_fte_workspace_bytes().
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); all work is stream-ordered,
 *     nothing synchronises the device unless stated.
 *   - all arrays are dense, C-contiguous, double (fp64) unless stated.
 */
#ifndef ACINOSET_HIP_H
#define ACINOSET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ACINO_ABI_VERSION 3   /* 2: acino_fte_params grew (chunk_nodes, refine_sweeps), 17 profiler classes, status 5-7 / numeric_err bit mask;
                               * 3: acino_skel_fte_* (generic-skeleton FTE), debug-stamp buffer of 72 entries with the selectors at [64], [65] */

typedef enum acino_status {
  ACINO_OK = 0,
  ACINO_ERR_INVALID_ARG = -1,
  ACINO_ERR_HIP = -2,            /* a HIP runtime call or kernel launch failed        */
  ACINO_ERR_WORKSPACE = -3,      /* workspace too small / misaligned                 */
  ACINO_ERR_NO_DEVICE = -4,
  ACINO_ERR_UNSUPPORTED = -5,
  ACINO_ERR_NUMERIC = -6,        /* non-positive pivot in the block factorisation    */
  ACINO_ERR_CALLBACK = -7        /* a caller-supplied reduction callback failed      */
} acino_status;

/* ---- camera records -------------------------------------------------------------------------
 * Fisheye camera: 24 doubles  [fx fy cx cy | k1 k2 k3 k4 | R(9,row-major) | t(3) | alpha 0 0 0]
 * Pinhole camera: 32 doubles  [fx fy cx cy | d(14: k1 k2 p1 p2 k3 k4 k5 k6 s1 s2 s3 s4 tx ty) | R(9) | t(3) | 0 0]
 * (alpha = K[0][1]/fx, OpenCV's skew; zero for every reference rig.  The point-wise, pair and EKF kernels honour it; the
 * FTE NLP projection and every pinhole path ignore it, as their references do; the bundle adjustment refuses it.  All of it
 * under test on unlike, skewed cameras: tests/test_gpu_unlike_rig.py.) */
#define ACINO_CAM_STRIDE 24
#define ACINO_PINHOLE_STRIDE 32
#define ACINO_MAX_CAMS 16
#define ACINO_MAX_PAIR_CAMS 8   /* dense pair path: the pair mask is one byte (pairs (c, c+1), c < 7) */
#define ACINO_N_MARKERS 20     /* cheetah markers (all_optimizations.py:170-179)            */
#define ACINO_N_STATES 45      /* x,y,z, phi_0..13, theta_0..13, psi_0..13                   */
#define ACINO_N_ACTIVE 25      /* states with Q != 0 (all_optimizations.py:245-252)          */

const char* acino_last_error_string(void);
int acino_abi_version(void);
/* sha256 prefix over every HIP source and header this binary was built from (acinoset_amd/_lib.py::source_hash):
 * build() and the profile stamps compare it instead of file times. */
const char* acino_build_id(void);
/* Number of visible HIP devices, or a negative status. */
int acino_device_count(void);

/* ---- point-wise camera model (a-1, a-2) ------------------------------------------------------ */
/* d_pts[M][2] pixel -> d_out[M][2] normalised coordinates; OpenCV criteria (max_iter=10, eps=1e-8);
 * non-converged / sign-flipped points are written as -1e6 like OpenCV >= 4.5. */
int acino_undistort_fisheye(const double* d_pts, int64_t m, const double* d_cam24, double* d_out,
                            int max_iter, double eps, void* stream);
/* Two-view triangulation: undistort both, 4x4 DLT, smallest right-singular vector, dehomogenise.
 * d_pts1/d_pts2 [M][2], d_cam_a/d_cam_b one camera record each, d_out[M][3]. */
int acino_triangulate_fisheye(const double* d_pts1, const double* d_pts2, int64_t m,
                              const double* d_cam_a24, const double* d_cam_b24, double* d_out, void* stream);
int acino_triangulate_pinhole(const double* d_pts1, const double* d_pts2, int64_t m,
                              const double* d_cam_a32, const double* d_cam_b32, double* d_out, void* stream);
/* d_obj[M][3] -> d_out[M][2]. */
int acino_project_fisheye(const double* d_obj, int64_t m, const double* d_cam24, double* d_out, void* stream);
int acino_project_pinhole(const double* d_obj, int64_t m, const double* d_cam32, double* d_out, void* stream);

/* ---- dense adjacent-pair triangulation (a-3, BASELINE configs[1]) ---------------------------
 * d_det[N][C][L][3] = (x, y, likelihood).  A detection is valid iff likelihood > thresh.
 * For each (frame, marker): triangulate every adjacent camera pair (c, c+1) with both valid, take
 * the Kahan-compensated mean in pair order (what pandas' groupby().mean() computes).
 * d_tri[N][L][3] (NaN when no pair), d_npairs[N][L] u8, d_pairmask[N][L] u8 (bit c = pair (c,c+1)).
 * d_npairs / d_pairmask may be NULL.  1 <= n_cams <= ACINO_MAX_PAIR_CAMS. */
int acino_triangulate_pairs(const double* d_det, int64_t n_frames, int n_cams, int n_markers, double thresh,
                            const double* d_cams24, double* d_tri, uint8_t* d_npairs, uint8_t* d_pairmask,
                            void* stream);
/* Initial iterate of the FTE solve from the dense triangulation d_tri[N][n_markers][3] (NaN = no pair), formed on the device
 * (acinoset_amd.fte.triangulation_init; the reference's own initialisation is the nose line, all_optimizations.py:268-277,
 * which acinoset_amd.fte.nose_line_init restates): d_xa[N][n_active] <- 0 except columns 0..2 = mean of the finite ones among
 * markers 0, 1, 2 (eyes, nose) and column psi_column = np.unwrap(atan2) of marker 2 - marker 3 (neck_base -> nose), each
 * np.interp'ed over the frames that lack it (held flat at the ends).  *d_flag (preset to 0 by the caller) <- 1 when no frame
 * has a head marker.  One launch; d_scratch: acino_fte_triangulation_init_scratch_bytes(N), 8-byte aligned. */
size_t acino_fte_triangulation_init_scratch_bytes(int64_t n_frames);
int acino_fte_triangulation_init(const double* d_tri, int64_t n_frames, int n_markers, double* d_xa, int n_active,
                                 int psi_column, void* d_scratch, size_t scratch_bytes, int32_t* d_flag, void* stream);
/* The same index path with the injected pinhole pair (calib.py:52-61): d_cams32 = C pinhole records. */
int acino_triangulate_pairs_pinhole(const double* d_det, int64_t n_frames, int n_cams, int n_markers, double thresh,
                                    const double* d_cams32, double* d_tri, uint8_t* d_npairs, uint8_t* d_pairmask,
                                    void* stream);
/* The two calls below in one pass over d_det (BASELINE configs[1]: triangulation + reprojection residual of the
 * triangulated points in every camera): d_tri / d_npairs / d_pairmask as acino_triangulate_pairs, d_res / d_sums as
 * acino_reproject_residuals applied to d_tri. */
int acino_triangulate_reproject(const double* d_det, int64_t n_frames, int n_cams, int n_markers, double thresh,
                                const double* d_cams24, double* d_tri, uint8_t* d_npairs, uint8_t* d_pairmask,
                                double* d_res, double* d_sums, void* stream);
/* Reprojection residual of d_pts3[N][L][3] in every camera against d_det:
 * d_res[N][C][L][2] = project(pts3) - det.xy where det valid and pts3 finite, else NaN.
 * d_sums[4] (may be NULL) += {count, sum r, sum r^2, 0.5*sum log1p(r^2)} over valid residual components. */
int acino_reproject_residuals(const double* d_pts3, const double* d_det, int64_t n_frames, int n_cams,
                              int n_markers, double thresh, const double* d_cams24, double* d_res,
                              double* d_sums, void* stream);

/* ---- robust N-view triangulation with a covariance per point (csrc/triangulate_mv.hip) -------
 * Per (frame, marker), over V = the cameras whose detection has likelihood > thresh, finite pixels and a successful
 * undistortion (fisheye: the OpenCV criteria (10, 1e-8); pinhole: always): the minimiser X of
 *   F(X) = sum_{c in V} 0.5 f^2 (log1p(r_u^2 / f^2) + log1p(r_v^2 / f^2)),  r = pi_c(X) - (u, v),  f = f_scale,
 * pi_c the calibration-level projection (acino_project_fisheye with the record's skew / acino_project_pinhole).  Start: the
 * N-view ray midpoint.  Iteration: a damped Gauss-Newton per point on sum J^T h J, h = max(rho'', 0.1 w); a trial that
 * raises F or leaves the front of a camera of V is rejected; it ends on a step shorter than xtol [m] or after max_iter
 * trials.  One launch, no synchronisation.  At the returned X, with W the Cauchy IRLS weights w = 1 / (1 + r^2 / f^2):
 *   d_points[N][L][3]
 *   d_cov[N][L][3][3]    sigma_px^2 (sum J_c^T W_c J_c)^-1, symmetric bit for bit (the matrix of acino_sba_covariance with
 *                        the cameras fixed)
 *   d_wssr[N][L]         sum w r^2
 *   d_nviews[N][L]       |V|
 *   d_status[N][L]       0 stopped on xtol, 1 max_iter reached, 2 fewer than two views, 3 numeric (the start's matrix or A
 *                        with a pivot d_i of L D L^T at or below 1e-12 of its trace, or a non-finite value);
 *                        points, cov, wssr (and sens) are NaN for 2 and 3
 *   d_iters[N][L]        trials made
 *   d_sens[N][L][3][6C]  -A^-1 [G_0 .. G_{C-1}], G_c = J_c^T W_c Jc_c, Jc_c the derivative with respect to (dw, dt) under
 *                        R <- exp([dw]x) R, t <- t + dt (the parametrisation of acino_sba_covariance); the columns of the
 *                        cameras outside V are exactly 0
 * d_cov, d_wssr, d_iters, d_sens may be NULL.  1 <= n_cams <= ACINO_MAX_CAMS. */
typedef struct acino_tri_mv_params {
  int32_t camera_model;   /* 0 fisheye (24-double records), 1 pinhole (32) */
  int32_t max_iter;       /* 1..255 */
  double thresh, f_scale, sigma_px, xtol;
} acino_tri_mv_params;
size_t acino_sizeof_tri_mv_params(void);
int acino_triangulate_multiview(const acino_tri_mv_params* prm, const double* d_det, int64_t n_frames, int n_cams,
                                int n_markers, const double* d_cams, double* d_points, double* d_cov, double* d_wssr,
                                uint8_t* d_nviews, uint8_t* d_status, uint8_t* d_iters, double* d_sens, void* stream);

/* ---- per-frame cheetah pose fit from 3-D markers with a covariance each (csrc/pose_fit.hip) -------
 * Per frame n, from d_points[N][20][3] (metres) and d_cov[N][20][3][3] - the points / cov layout of
 * acino_triangulate_multiview -, over the 25 active states x (the order of acino_fk_active) inside the box of the FTE:
 *   F(x) = 1/2 sum_{l enters} (FK_l(x) - y_l)^T W_l (FK_l(x) - y_l) + 1/2 sum_{p = 3..24} (x_p - m_p)^2 / prior_sigma^2.
 * A marker enters when its 3 + 9 values are finite and S_l = L D L^T has every pivot above 1e-12 of its trace (the rule of
 * acino_triangulate_multiview); W_l = S_l^-1, or I / sigma_iso^2 for every finite point with d_cov NULL.  m = the start
 * clipped to the box: the ridge acts on the 22 angles only, defines the states no entering marker moves and keeps A
 * positive definite whenever one marker enters.  F is a negative log-posterior as it stands (acino_fte_covariance).
 * Start: d_x0[N][25], or with d_x0 NULL the mean of the entering markers among 0, 1, 2 (of all entering markers when none of
 * them enters) in columns 0..2, psi_0 = atan2 of (marker 2 - marker 3) when both enter, every other state 0.
 * Iteration: the projected Levenberg-Marquardt of acino_fte_solve per frame - active set "at a bound with the gradient
 * pushing outward, |g_p| > 1e-14 A_pp", (A + lam diag A) d = -g on the free states with A = sum J_l^T W_l J_l + the ridge,
 * the trial clipped to the box and accepted when F falls, Nielsen's damping; it ends on dF <= ftol |F|, on a step <= xtol,
 * on lam > 1e16 or after max_iter trials.  One launch (one 64-lane wave per frame), no synchronisation.  At the returned x:
 *   d_x[N][25], d_cost[N], d_nmarkers[N] (markers that entered), d_iters[N] (trials made)
 *   d_status[N]           0 stopped on ftol or xtol, 1 max_iter reached or lam overflowed, 2 fewer than min_markers enter,
 *                         3 numeric (a pivot not above zero or a non-finite value); every floating-point output of the
 *                         frame is NaN (and d_pinned 0) for 2 and 3
 *   d_pinned[N][25]       the active set
 *   d_cov_x[N][25][25]    A_free^-1 without a Marquardt term, rows and columns of pinned states exactly 0 (as
 *                         acino_fte_covariance), symmetric bit for bit
 *   d_pos[N][20][3]       FK(x)
 *   d_cov_pos[N][20][3][3]  J_l cov_x J_l^T, symmetric bit for bit;  d_std_pos[N][20] = sqrt((c00 + c11) + c22)
 * Any output but d_x and d_status may be NULL.  Argument validation happens before any device call; n_frames == 0 is a
 * no-op. */
typedef struct acino_pose_fit_params {
  int32_t max_iter;       /* 1..255 */
  int32_t min_markers;    /* 1..20 */
  double lam0, ftol, xtol, prior_sigma, sigma_iso;   /* all > 0; prior_sigma [rad], sigma_iso [m] */
} acino_pose_fit_params;
size_t acino_sizeof_pose_fit_params(void);
int acino_cheetah_pose_fit(const acino_pose_fit_params* prm, const double* d_points, const double* d_cov,
                           const double* d_x0, int64_t n_frames, double* d_x, double* d_cost, uint8_t* d_nmarkers,
                           uint8_t* d_status, uint8_t* d_iters, uint8_t* d_pinned, double* d_cov_x, double* d_pos,
                           double* d_cov_pos, double* d_std_pos, void* stream);

/* ---- per-frame cheetah pose fit from the detections of every camera (csrc/pose_fit_px.hip) -------
 * Per frame n, from d_det[N][C][20][3] (x, y, likelihood) and d_cams - the layouts of acino_triangulate_multiview,
 * 1 <= n_cams <= ACINO_MAX_CAMS -, over the 25 active states x inside the box of the FTE:
 *   F(x) = 1/sigma_px^2 sum_{(c,l) valid} sum_{k in (u,v)} 1/2 f^2 log1p(r_k^2 / f^2)
 *        + 1/2 sum_{p = 3..24} (x_p - m_p)^2 / prior_sigma^2,      r = pi_c(FK_l(x)) - z_{n,c,l},  f = f_scale,
 * pi_c the calibration-level projection of acino_triangulate_multiview and its per-coordinate Cauchy loss.  A detection is
 * valid when its likelihood is above thresh and both pixel values are finite: a marker one camera sees enters, and no
 * triangulation stands between a detection and the skeleton.  m = the start d_x0[N][25] (required) clipped to the box.
 * Gradient and matrix carry the IRLS weight w = 1 / (1 + r_k^2 / f^2): g = sum w r J / sigma_px^2 + ridge and
 * A = sum w J^T J / sigma_px^2 + ridge with J = (J_pi R_c) J_FK; the same A serves the step, the predicted reduction, the
 * active set and the outputs, so cov_x = A_free^-1 is the matrix family of acino_triangulate_multiview and
 * acino_sba_covariance carried to the states.  An x that puts a marker with a valid detection at z_c <= 0 in that camera has
 * F = +inf: as a trial it is refused, as a start it gives status 3.  Iteration, stops, active set, status codes, NaN
 * conventions and the bit-symmetric covariances are those of acino_cheetah_pose_fit, with "fewer than min_detections valid
 * detections" for status 2.  One launch (one 64-lane wave per frame), no synchronisation, no workspace.  At the returned x:
 *   d_x, d_cost, d_status, d_iters, d_pinned, d_cov_x, d_pos, d_cov_pos, d_std_pos   as acino_cheetah_pose_fit
 *   d_ndet[N]              uint16: the valid detections of the frame (at most 20 C)
 *   d_weight[N][C][20][2]  the w every coordinate ended with, exactly 0 for an invalid detection, NaN for status 2 and 3
 * Any output but d_x and d_status may be NULL.  Argument validation happens before any device call; n_frames == 0 is a
 * no-op. */
typedef struct acino_pose_fit_px_params {
  int32_t camera_model;     /* 0 fisheye (24-double records), 1 pinhole (32) */
  int32_t max_iter;         /* 1..255 */
  int32_t min_detections;   /* 1..20 n_cams */
  int32_t reserved;         /* 0 */
  double lam0, ftol, xtol, prior_sigma;   /* all > 0; prior_sigma [rad] */
  double thresh;            /* not NaN */
  double f_scale, sigma_px; /* > 0 [px] */
} acino_pose_fit_px_params;
size_t acino_sizeof_pose_fit_px_params(void);
int acino_cheetah_pose_fit_px(const acino_pose_fit_px_params* prm, const double* d_det, int64_t n_frames, int n_cams,
                              const double* d_cams, const double* d_x0, double* d_x, double* d_cost, uint16_t* d_ndet,
                              uint8_t* d_status, uint8_t* d_iters, uint8_t* d_pinned, double* d_cov_x, double* d_pos,
                              double* d_cov_pos, double* d_std_pos, double* d_weight, void* stream);

/* ---- cheetah forward kinematics (a-4) ---------------------------------------------------------
 * d_q[N][45] full state -> d_pos[N][20][3]. */
int acino_cheetah_fk(const double* d_q, int64_t n_frames, double* d_pos, void* stream);

/* ---- Full Trajectory Estimation (a-5 .. a-11) -------------------------------------------------
 * Reduced problem of the reference NLP: unknowns xa[N][25] (active states),
 *   F = sum rho(w*(pi_c(FK_l(x_n)) - z)) + sum_{n>=3} q_p (x_n - 3x_{n-1} + 3x_{n-2} - x_{n-3})_p^2,
 * box bounds lo/hi, solved by a projected Levenberg-Marquardt whose Gauss-Newton system is
 * block-tridiagonal in super-blocks of 3 frames and solved by block cyclic reduction.
 * Active set: a variable sitting ON a bound whose gradient entry pushes outward is pinned for the iteration (step exactly
 * 0); "pushes" means |g_i| > 1e-14 * H_ii, i.e. a gradient below a Newton step of 1e-14 counts as zero.  Damping is
 * Marquardt's lam * diag(H); a diagonal entry that is exactly 0 (clips of < 4 frames with an unobserved state) is damped
 * by lam * 1e-30 and keeps its variable where it is. */
typedef struct acino_fte_params {
  int32_t n_frames;        /* local frames on this GPU                                      */
  int32_t n_cams;
  int64_t n_global;        /* frames in the whole sequence (== n_frames on one GPU)         */
  int64_t n_offset;        /* global index of local frame 0 (multiple of 3 when > 0)        */
  int32_t pin_left;        /* 1: local chain starts with a separator owned by the left rank */
  int32_t pin_right;       /* 1: the last local super-block is a separator (not eliminated) */
  double dlc_thresh;       /* likelihood threshold (all_optimizations.py:304)               */
  double inv_r_meas;       /* 1/R, R = 5 px (all_optimizations.py:243)                      */
  double redesc_a, redesc_b, redesc_c;   /* 3, 10, 20 (all_optimizations.py:25-27)          */
  double q_w[ACINO_N_ACTIVE];            /* (1/Q_p) / Ts^4 per active state                 */
  double lo[ACINO_N_ACTIVE], hi[ACINO_N_ACTIVE];   /* box bounds (+-inf = free)             */
  double lam0;             /* initial LM damping                                            */
  double ftol, xtol, gtol; /* stopping tolerances (0 disables a test)                       */
  double lam_max;          /* damping ceiling (0 = 1e16)                                    */
  int32_t clamp_lambda;    /* 0: stop with status 4 when lam exceeds lam_max; 1: clamp and keep iterating */
  int32_t shared_gpu;      /* 1: other solver contexts run on this GPU at the same time (batched clips, several ranks on one
                            * device): kernels that spin-wait on other workgroups (the fused back-substitution tail) are
                            * replaced by their per-level forms - concurrent spin-waiting kernels could fill the CUs */
  int64_t clip_len;        /* 0: the frames are ONE sequence.  > 0: the frames are n_frames / clip_len independent clips of
                            * this many frames laid end to end (BASELINE config 5): the smoothness prior does not couple
                            * frames of different clips, everything else - kernels, schedule, one LM controller over the
                            * sum of the clips' costs - is unchanged.  Single-GPU contexts only. */
  int32_t precision;       /* ACINO_PREC_F64 (0, default) or ACINO_PREC_BF16_ROWS (1) = BASELINE config 5's "bf16 residuals
                            * with fp32 accumulate": FK and camera-frame coordinates in fp64, projection / 2x3 Jacobian /
                            * robust weights in fp32, every per-(frame, camera, marker) residual and Jacobian ROW rounded
                            * to bf16 (round-to-nearest-even) before it enters the normal equations, the per-marker
                            * M_l = sum J^T W J and v_l = sum J^T w rho' accumulated in fp32; everything from the 6x6
                            * spatial blocks onward - subtree sums, H, g, the smoothness prior with its 1/Ts^4 weights, the
                            * band factorisation, the LM controller and the cost - stays fp64. */
  int32_t bcr_levels;      /* 0 (default): complete block cyclic reduction.  K > 0: INCOMPLETE reduction - after K levels the
                            * couplings between the remaining nodes (3 * 2^K frames apart) are dropped and every remaining
                            * node is solved on its own.  The dropped blocks decay geometrically with the node distance
                            * (the Gauss-Newton matrix is banded SPD); their normalised size
                            * eps = max || L_b^-1 C L_a^-T ||_F is MEASURED on the device every iteration
                            * (acino_fte_state::trunc_eps) - the solve's relative energy-norm error is <= eps / (1 - eps) -
                            * and an iteration with eps > trunc_tol stops the solve with status 7 instead of returning an
                            * unverified step.  Single-GPU contexts only (no pinned separators). */
  double trunc_tol;        /* admissible eps of an incomplete reduction (0 = 1e-10)                                */
  int32_t own_first;       /* overlapping-window sharding (acinoset_amd/dist.py WindowedFTE): the n_frames of this context */
  int32_t own_count;       /* are a WINDOW [n_offset, n_offset + n_frames) of the sequence, of which only the local frames
                            * [own_first, own_first + own_count) are owned: the whole window is assembled and solved
                            * (frames outside it keep delta = 0), but cost, predicted reduction, step and gradient norms
                            * count owned frames only.  own_count = 0 (default): every frame is owned. */
  int32_t chunk_nodes;     /* linear solver of single-GPU contexts (no pinned separators).  0 (default): chunked
                            * substructuring (csrc/chunk.hip) - the chain of 3-frame nodes is cut into runs of an
                            * automatically chosen length, one workgroup eliminates the interior nodes of a run in order
                            * with every operand in LDS, block cyclic reduction solves the chain of the runs' separators.
                            * m >= 2: the same with m nodes per run (m - 1 interior + 1 separator).  -1: block cyclic
                            * reduction over the whole chain (the round-1/2 solver).  With chunking, bcr_levels counts
                            * reduction levels of the SEPARATOR chain. */
  int32_t refine_sweeps;   /* incomplete reduction (bcr_levels > 0): block-Jacobi sweeps that re-introduce the dropped
                            * couplings after the truncated solve (0 = none).  In theory r sweeps leave a relative
                            * energy-norm error <= (2 eps)^(r+1) / (1 - 2 eps).  What the device CHECKS against trunc_tol with
                            * r > 0 is an a-posteriori estimate from the sweeps themselves (eps is not measured then):
                            * rho / (1 - rho) * max|last update| / max|x| with rho = a ratio of the max-norms of consecutive
                            * updates: of the first two sweeps and - while those are above the rounding level, 2^-44 max|x| -
                            * of the last two, the larger of both (r = 1, or a first update already at rounding: rho = 1/2
                            * assumed); rho > 1/2 refuses the step (status 7).  The estimate is written to
                            * acino_fte_state::trunc_eps. */
} acino_fte_params;
#define ACINO_PREC_F64 0
#define ACINO_PREC_BF16_ROWS 1
#define ACINO_PREC_BF16_RES 2    /* as BF16_ROWS but only the residual rows are rounded to bf16; Jacobian rows stay fp32 */

/* LM state mirrored in device memory (read back with acino_fte_get_state). */
typedef struct acino_fte_state {
  double cost;             /* F at the current iterate (this rank's share when sharded)     */
  double cost_trial;
  double lam, nu;
  double gain, pred, step_inf, gnorm_inf;
  int32_t iter;            /* LM iterations performed                                       */
  int32_t accepted;
  int32_t status;          /* 0 running, 1 ftol, 2 xtol, 3 gtol, 4 lambda overflow, 5 numeric (non-positive pivot),
                            * 6 device synchronisation timeout (backsub tail), 7 dropped couplings above trunc_tol */
  int32_t cur;             /* which of the two iterate buffers is current                   */
  int32_t n_behind;        /* weighted detections with z_cam < 1e-6 (kept, as the reference)  */
  int32_t last_accept;
  int32_t pad0, pad1;
  double trunc_eps;        /* incomplete reduction: what was compared with trunc_tol in the last iteration - the measured
                            * size of the dropped couplings, or (refine_sweeps > 0) the sweeps' error estimate (0: complete) */
} acino_fte_state;

typedef struct acino_fte_ctx acino_fte_ctx;   /* opaque host handle */

/* sizeof() of the two ABI structs as this library was compiled (bindings assert their own layout against it). */
size_t acino_sizeof_fte_params(void);
size_t acino_sizeof_fte_state(void);
size_t acino_fte_workspace_bytes(const acino_fte_params* p);
/* Creates a handle over caller-owned buffers.  d_det[N][C][L=20][3], d_cams24[C][24],
 * d_workspace >= acino_fte_workspace_bytes(p), 256-byte aligned.  Synchronises the stream once. */
int acino_fte_create(acino_fte_ctx** out, const acino_fte_params* p, const double* d_det,
                     const double* d_cams24, void* d_workspace, size_t workspace_bytes, void* stream);
/* The same problem on the OpenCV pinhole camera (cv2.projectPoints: k1 k2 p1 p2 k3 k4 k5 k6 s1 s2 s3 s4, skew ignored,
 * the tilted model tau_x = tau_y = 0): d_cams32[C][32] pinhole records, everything else as acino_fte_create - the
 * workspace size, every call on the handle, clips, graphs, profiling.  fp64 only: p->precision other than
 * ACINO_PREC_F64, or a later acino_fte_set_precision to a bf16 mode, is ACINO_ERR_INVALID_ARG. */
int acino_fte_create_pinhole(acino_fte_ctx** out, const acino_fte_params* p, const double* d_det,
                             const double* d_cams32, void* d_workspace, size_t workspace_bytes, void* stream);
int acino_fte_destroy(acino_fte_ctx* ctx);
/* Layout the linear solver chooses for these parameters: out[0] = nodes per run of the chunked solver (0: block cyclic
 * reduction over the whole chain), out[1] = runs, out[2] = separators, out[3] = reduction levels of the reduced chain
 * (the separators, or the whole chain) when nothing is truncated.  A caller that wants an incomplete reduction picks
 * bcr_levels from the node distance it implies: 3 * max(out[0], 1) * 2^bcr_levels frames. */
int acino_fte_plan(const acino_fte_params* p, int32_t* out);
/* Loads the initial iterate (d_x0[N][25], clipped to the bounds), restarts the LM controller and evaluates
 * cost / gradient / Gauss-Newton blocks.  = load_x + eval(0) + control(NULL, init=1). */
int acino_fte_set_x(acino_fte_ctx* ctx, const double* d_x0, void* stream);
/* One LM iteration, entirely stream-ordered (no host sync): damped block system -> block cyclic reduction ->
 * trial iterate -> residuals, Jacobians, normal-equation assembly at the trial -> accept/reject + lambda. */
int acino_fte_step(acino_fte_ctx* ctx, void* stream);
/* on != 0: acino_fte_step captures its launch sequence into a hipGraph on first use and replays it afterwards
 * (needs a non-null stream; ignored while profiling is active and for sharded contexts). */
int acino_fte_enable_graph(acino_fte_ctx* ctx, int on);
/* Up to max_iter LM iterations (the device stops by itself on convergence; the host peeks every 8 steps);
 * synchronises at the end and fills *out (may be NULL). */
int acino_fte_solve(acino_fte_ctx* ctx, int max_iter, acino_fte_state* out, void* stream);
int acino_fte_get_state(acino_fte_ctx* ctx, acino_fte_state* out, void* stream);   /* synchronises */
/* Current iterate -> d_x[N][25]; positions d_pos[N][20][3]; dx/ddx by the reference's backward-Euler
 * relations (all_optimizations.py:369-383).  Any output may be NULL.  Synchronises. */
int acino_fte_get_result(acino_fte_ctx* ctx, double ts, double* d_x, double* d_pos, double* d_dx, double* d_ddx,
                         void* stream);
/* Switches the arithmetic of the assembly for the following evaluations (ACINO_PREC_*): a mixed-precision solve is
 * finished ("polished") with a few fp64 iterations this way.  Drops the captured step graph; the next
 * acino_fte_step re-evaluates nothing by itself - call acino_fte_reevaluate to refresh cost / gradient / blocks of
 * the current iterate in the new precision before stepping. */
int acino_fte_set_precision(acino_fte_ctx* ctx, int precision);
/* Re-evaluates the CURRENT iterate (cost, gradient, Gauss-Newton blocks) and restarts the controller's stopping
 * state (status -> running; lambda kept, or back to lam0 when the run had ended in lambda overflow). */
int acino_fte_reevaluate(acino_fte_ctx* ctx, void* stream);
/* Copies n frames of the current (which = 0) or trial (which = 1) iterate, starting at local frame `first`
 * (-3 <= first, first + n <= n_frames + 3: the three halo rows on either side are addressable), to d_buf[n][25]
 * (import = 0) or from it (import = 1).  The overlapping-window driver exchanges its edge slabs with these. */
int acino_fte_copy_frames(acino_fte_ctx* ctx, int which, int import, int first, int n, double* d_buf, void* stream);
/* Cost only at d_x[N][25] -> d_cost[1]; evaluated in the trial buffer (call between LM steps). */
int acino_fte_cost(acino_fte_ctx* ctx, const double* d_x, double* d_cost, void* stream);
/* Gradient d_g[N][25] and Gauss-Newton blocks d_h[N][25][25] (measurement part + smoothness diagonal) of the
 * CURRENT iterate, for parity checks.  Either may be NULL. */
int acino_fte_get_grad_hess(acino_fte_ctx* ctx, double* d_g, double* d_h, void* stream);
/* Posterior covariance of the trajectory at the context's CURRENT iterate (csrc/fte_cov.hip).  With
 *   A = blockdiag(H_n) + 2 q (x) D3^T D3   (no Marquardt term; H_n and the active set as the context holds them, the
 *                                           bound-active variables pinned: row and column zeroed, diagonal 1)
 * the Gauss-Newton Hessian of the solve's objective F, the outputs are blocks of A^-1, all fp64:
 *   d_cov_x[N][25][25]     the diagonal 25 x 25 blocks of A^-1, one per frame; rows / columns of variables held at a bound
 *                          are exactly 0
 *   d_cov_pos[N][20][3][3] J_l cov_x[n] J_l^T, J_l the 3 x 25 Jacobian of marker l's position (the FK of acino_fk_active)
 *   d_std_pos[N][20]       sqrt(trace(cov_pos)): one error bar per marker and frame, in metres
 * Any of the three may be NULL (not all).  UNITS: F counts a scaled residual e as rho(e) = e^2 / 2 near 0 and the prior as
 * q d^2, i.e. F is a negative log-posterior as it stands and A^-1 its Laplace covariance with no further factor: rad^2 for
 * angles, m^2 for the head position and the markers.
 * The call is exact (two pivot sweeps per clip over nodes of 3 frames + one inversion per node), reads the context's current
 * H / gradient / iterate - after acino_fte_load_x run acino_fte_reevaluate first - and leaves the context's solver state,
 * buffers and captured graphs untouched.  d_ws: caller-owned, acino_fte_covariance_workspace_bytes(params) bytes, 256-byte
 * aligned (ACINO_ERR_WORKSPACE otherwise).  It synchronises the stream once, to read the error word: a non-positive pivot
 * is ACINO_ERR_NUMERIC.  ACINO_ERR_UNSUPPORTED (no launch) for sharded, pinned or windowed contexts (n_global != n_frames,
 * pin_left / pin_right, own_count > 0) and for contexts in a bf16 precision. */
size_t acino_fte_covariance_workspace_bytes(const acino_fte_params* p);
int acino_fte_covariance(acino_fte_ctx* ctx, void* d_ws, size_t ws_bytes, double* d_cov_x, double* d_cov_pos,
                         double* d_std_pos, void* stream);
/* The same call with error bars for what a user takes from dx / ddx and from the speed of a marker (a superset: any of
 * the seven outputs may be NULL, not all; ONE run of the sweeps serves them all; the first three are bit-identical to
 * acino_fte_covariance).  ts > 0: the frame period, as in acino_fte_get_result.  With Sigma_win the 75 x 75 block of
 * A^-1 over a window of three consecutive frames of the frame's own clip (rows / columns of pinned variables 0):
 *   d_cov_dx[N][25][25]    C Sigma_win C^T, C = c (x) I_25 with the three scalars that make dx_n out of the window;
 *                          (rad/s)^2, (m/s)^2
 *   d_cov_ddx[N][25][25]   the same for ddx_n; (rad/s^2)^2, (m/s^2)^2
 *   d_cov_vel[N][20][3][3] covariance of the marker velocity v_n,l = (p_l(x_n) - p_l(x_n-1)) / ts, linearised:
 *                          (J_l(x_n) e_n - J_l(x_n-1) e_n-1) / ts for the estimation errors e; (m/s)^2
 *   d_std_vel[N][20]       sqrt(trace(cov_vel)), m/s
 * dx_n / ddx_n are those of acino_fte_get_result / acino_fte_derivatives taken per clip.  n >= 2: the window is
 * (x_n-2, x_n-1, x_n), dx_n = (x_n - x_n-1) / ts, ddx_n = (x_n - 2 x_n-1 + x_n-2) / ts^2.  START-UP FRAMES n = 0, 1 of a
 * clip: the window is frames 0..2 of the clip, ddx_0 = ddx_1 = ddx_2, dx_1 = (x_1 - x_0) / ts, dx_0 = dx_1 - ts ddx_2;
 * cov_vel / std_vel of frame 0 repeat frame 1.  Clips of 2 frames: ddx = 0, dx_0 = dx_1; of 1 frame: everything 0.
 * No further factor (see above).  The velocity of two neighbouring frames is NOT bounded by cov_x: the prior correlates
 * them almost perfectly, and sqrt(2 diag cov_x) / ts overstates the spread of dx by orders of magnitude.
 * Workspace (the same byte count), statuses, synchronisation and what the call leaves untouched: as acino_fte_covariance. */
size_t acino_fte_covariance_rates_workspace_bytes(const acino_fte_params* p);
int acino_fte_covariance_rates(acino_fte_ctx* ctx, double ts, void* d_ws, size_t ws_bytes, double* d_cov_x, double* d_cov_pos,
                               double* d_std_pos, double* d_cov_dx, double* d_cov_ddx, double* d_cov_vel, double* d_std_vel,
                               void* stream);
/* Joint draws of the WHOLE trajectory from the same Laplace posterior: what the two entries above give as diagonal blocks,
 * this one gives as samples, so that any statistic of any functional across frames (stride length, mean speed over a
 * stride, the phase between two feet) is a line of numpy on them.  A = the matrix of acino_fte_covariance at the CURRENT
 * iterate, unknowns ordered frame-major (n, p), A = L L^T its Cholesky factor.  For the caller's d_z[S][N][25]
 *   d_x_samples[s] = x_hat + delta(s),   delta(s) = L^-T z(s),   z of a pinned variable counted as 0 (delta exactly 0 there)
 * so Cov(delta) = A^-1 for standard-normal z (E[delta_n delta_n^T] = cov_x[n], E[delta_n delta_m^T] the block (n, m) of
 * A^-1).  The map z -> delta is deterministic: the library owns no random generator, and the result for one clip does not
 * depend on the other clips of the context.  d_pos_samples[S][N][20][3] (may be NULL): acino_fk_active of every sample -
 * the real FK, not its linearisation.  dx / ddx of a sample: acino_fte_derivatives on d_x_samples[s] (per clip).
 * Three launches: the forward pivot sweep of the covariance (one workgroup per clip), the factors U_k = L_k^-T of all nodes
 * in parallel, one backward substitution per clip and panel of 64 samples, delta_k = U_k (z_k - U_k^T (E_k delta_k+1)).
 * n_samples >= 1; d_z must not alias the outputs (ACINO_ERR_INVALID_ARG, before any device call, as for a NULL d_z /
 * d_x_samples).  Workspace (the same byte count), ACINO_ERR_WORKSPACE / _UNSUPPORTED / _NUMERIC, the one synchronisation
 * and what the call leaves untouched: as acino_fte_covariance. */
size_t acino_fte_sample_workspace_bytes(const acino_fte_params* p);
int acino_fte_sample(acino_fte_ctx* ctx, int64_t n_samples, const double* d_z, void* d_ws, size_t ws_bytes,
                     double* d_x_samples, double* d_pos_samples, void* stream);
/* Error bars that include the CALIBRATION: the sensitivity S = d x_hat / d c of the whole trajectory to the camera
 * extrinsics, and the "consider" covariance S Sigma_c S^T it gives for a covariance Sigma_c of the extrinsics.
 * All quantities are at the context's CURRENT iterate.  A, the pinned (bound-active) set and the node grid are those of
 * acino_fte_covariance.
 * Camera parameters are c = [dw_0, dt_0, ..., dw_C-1, dt_C-1], applied as R_c <- exp([dw]x) R_c, t_c <- t_c + dt.  This is
 * the order and parametrisation of acino_sba_covariance, so cov_cams plugs in unchanged.
 * For a detection (n, c, l) with world point p = FK_l(x_n):
 *   J_x = J_pi J_l (2 x 25).
 *   J_c = J_pi R_c^T [ -[R_c p]x | I_3 ] (2 x 6), the derivative of the predicted pixel with respect to (dw_c, dt_c).
 *   J_pi = d uv / d p in the world frame, from the context's own camera model, fisheye or pinhole.
 *   The per-component weight is w^2 h, with w and h exactly as the assembly forms them.  h is the weight
 *   acino_fte_reprojection reports; w = 0 below the likelihood threshold, for non-finite pixels and on the singular plane.
 * The cross term and the solve:
 *   G_n[:, 6c:6c+6] = sum over l and both pixel components of J_x^T (w^2 h) J_c, shape [25, 6C] per frame.
 *   S = -A^-1 G, shape [N, 25, 6C].
 *   Rows of G for pinned variables are 0, so rows of S for pinned variables are exactly 0.
 * S is the shift of the minimiser of the solver's own quadratic model per unit change of the extrinsics.  It uses the same
 * Gauss-Newton / secant-weight approximation that A^-1 itself makes.  S is NOT a derivative of the Levenberg-Marquardt end
 * point: a finite difference of re-solves with perturbed cameras agrees with it on well-determined states (about 1 %) and
 * is meaningless along the flat valleys of the objective, where the end point depends on the path.
 * Given Sigma_c = d_cov_cams[6C][6C] (e.g. cov_cams of acino_sba_covariance; only PSD - a held camera has zero rows - so it
 * is multiplied, T = S_n Sigma_c, then T S_n^T, never factored):
 *   d_sens[N][25][6C]          S
 *   d_cov_x_cal[N][25][25]     S_n Sigma_c S_n^T, symmetric to the bit
 *   d_cov_pos_cal[N][20][3][3] J_l cov_x_cal[n] J_l^T, symmetric to the bit
 *   d_std_pos_cal[N][20]       sqrt(trace(cov_pos_cal)), metres
 * Any output may be NULL, but not all of them; a cov / std output without d_cov_cams is ACINO_ERR_INVALID_ARG.  Argument
 * checks come before any device call.  The total covariance of a trajectory solved on a calibration that came from OTHER data
 * is cov_x + cov_x_cal; it is NOT valid for extrinsics refined on the same clips (the two errors are then correlated).
 * The calibration term is perfectly correlated across frames: smoothing does not average it out.
 * Launches: k_fte_calib_rhs (-G as 6C columns), the sampler's forward sweep and factors, one forward and one backward
 * substitution per clip and panel of 64 columns, k_fte_calib_combine.  Every clip on its own node grid; the result for one
 * clip does not depend on the others.  Workspace: the covariance workspace + 2 * 6C * N * 25 doubles, 256-byte aligned
 * (ACINO_ERR_WORKSPACE otherwise); ACINO_ERR_UNSUPPORTED, ACINO_ERR_NUMERIC, the one synchronisation and what the call leaves
 * untouched (solver state, buffers, captured graphs): as acino_fte_covariance. */
size_t acino_fte_calibration_workspace_bytes(const acino_fte_params* p);
int acino_fte_calibration_sensitivity(acino_fte_ctx* ctx, const double* d_cov_cams /* [6C][6C] or NULL */, void* d_ws,
                                      size_t ws_bytes, double* d_sens, double* d_cov_x_cal, double* d_cov_pos_cal,
                                      double* d_std_pos_cal, void* stream);
/* The solve seen in IMAGE space, at the CURRENT iterate: for every (frame n, camera c, marker l), with p = FK_l(x_n) (the
 * FK of acino_fk_active) and (uv, J_pi, z_cam) the projection of the context's own camera model - the device function the
 * assembly calls: the reference's pt3d_to_2d for acino_fte_create, cv2.projectPoints for acino_fte_create_pinhole -,
 * J_pi = d uv / d p (2 x 3, world frame), z = the detection:
 *   d_uv[N][C][20][2]        predicted pixel.  NaN on the singular plane abs(z_cam) < 1e-9 (which the assembly drops); behind
 *                            the camera it is the mirrored projection the solve itself penalises (bit 1 of the flags)
 *   d_cov_uv[N][C][20][2][2] J_pi cov_pos[n][l] J_pi^T, px^2, both off-diagonal entries the same bits (cov_pos enters by its
 *                            symmetric part).  Needs d_cov_pos [N][20][3][3], normally d_cov_pos of acino_fte_covariance at
 *                            the same iterate: d_cov_uv without d_cov_pos is ACINO_ERR_INVALID_ARG.  NaN where uv is
 *   d_res[N][C][20][2]       uv - z for every detection whose x and y are finite, whatever its likelihood; NaN otherwise and
 *                            where uv is NaN
 *   d_weight[N][C][20][2]    the Gauss-Newton curvature weight h in [0, 1] of the redescending loss at e = inv_r_meas *
 *                            abs(res), per component: what the solve made of the detection (1: used as measured, towards 0:
 *                            redescended).  Exactly 0 where the assembly gives the detection no weight (likelihood <=
 *                            dlc_thresh, non-finite, singular plane)
 *   d_mahal2[N][C][20]       res^T (cov_uv + R^2 I)^-1 res, R = 1 / inv_r_meas: the squared gating distance of the
 *                            detection under the posterior predictive (chi-square, 2 degrees of freedom); with d_cov_pos ==
 *                            NULL res^T res / R^2.  NaN where res is
 *   d_flags[N][C][20] (u8)   bit 0: the assembly weights this detection; bit 1: z_cam < 1e-6 (what n_behind counts among
 *                            the detections above the threshold); bit 2: singular plane
 * Any output may be NULL (not all).  Argument checks come before any device call.  ONE launch of a streaming kernel:
 * stream-ordered, no synchronisation, no allocation, no workspace; the context's solver state, buffers and captured graphs
 * are untouched.  It reads the iterate alone, in fp64 whatever the context's precision, so it is valid for every context
 * (clips; sharded / windowed contexts: their local frames). */
int acino_fte_reprojection(acino_fte_ctx* ctx, const double* d_cov_pos, double* d_uv, double* d_cov_uv, double* d_res,
                           double* d_weight, double* d_mahal2, uint8_t* d_flags, void* stream);
/* Live per-kernel timing for bench.py: HIP events recorded on the launch stream around every kernel between
 * begin and end.  end synchronises and returns, per class {elim, elim_deep, update0, update, update_deep, backsub0,
 * backsub, trial, assemble, totals, control, backsub_tail, trunc_check, chunk_sweep, sep_combine, chunk_backsub, refine} (one class per kernel), the summed event time in ms, the launch
 * count and the work units (chain nodes for the block-reduction kernels, frames for trial/assemble; may be NULL). */
#define ACINO_PROF_CLASSES 17
int acino_fte_profile_begin(acino_fte_ctx* ctx);
/* Test aid: copies an internal buffer of the linear solver to d_out (at most n doubles).  what: 0 = the solution vector
 * per 3-frame node [n_nodes][80] (after acino_fte_backsub_local); separator-side buffers of the chunked solver: 1 = D,
 * 2 = b, 3 = coupling blocks, 4 = left-run contributions AL (5 is not assigned: ACINO_ERR_INVALID_ARG); 6 = G_k of the
 * interior nodes (lower 16 x 16 tiles), 7 = f_k = F_k x_L, [80] per interior node (T_k is not stored). */
int acino_fte_debug_read(acino_fte_ctx* ctx, int what, double* d_out, int64_t n, void* stream);
/* Debug aid: phase timestamps (wall_clock64 ticks) of ONE workgroup of the elimination kernel / the chunk sweep ->
 * d_dbg[0..63] of a caller buffer of ACINO_DEBUG_STAMP_ENTRIES (72) int64 entries; the caller sets d_dbg[64] = workgroup
 * index and d_dbg[65] = reduction level (k_bcr_elim) or node of the run (k_chunk_sweep) to stamp (read by every launch
 * while enabled).  NULL disables. */
#define ACINO_DEBUG_STAMP_ENTRIES 72
int acino_fte_debug_stamps(acino_fte_ctx* ctx, long long* d_dbg);
int acino_fte_profile_end(acino_fte_ctx* ctx, double* ms_by_class, int* launches_by_class, int64_t* units_by_class,
                          void* stream);
/* Stand-alone helpers: dx/ddx of a trajectory d_x[N][25]; FK of active states d_xa[N][25] -> d_pos[N][20][3]. */
int acino_fte_derivatives(const double* d_x, int64_t n_frames, double ts, double* d_dx, double* d_ddx, void* stream);
int acino_fk_active(const double* d_xa, int64_t n_frames, double* d_pos, void* stream);

/* ---- pieces of one LM iteration, for the multi-GPU driver (acinoset_amd/dist.py) ---------------
 * A sharded sequence gives every rank a contiguous frame block; the last super-block (3 frames) of every
 * rank but the last is a SEPARATOR that the rank does not eliminate (pin_right), and every rank but the
 * first sees its left neighbour's separator as chain node 0 (pin_left).  Per iteration:
 *   reduce_local -> export_separators -> [all-reduce SUM] -> solve_separators -> backsub_local -> trial
 *   -> export_edges(1) -> [all-gather] -> set_halo(1) -> eval(1) -> export_partials -> [all-gather + combine]
 *   -> control(total, 0).
 * `which`: 0 = current iterate, 1 = trial iterate (resolved on the device). */
#define ACINO_BS 80
/* Doubles in the exchange record of ONE separator: D[80][80] | C[80][80] = block(next separator, this one) | b[80]. */
#define ACINO_SEP_DOUBLES (2 * ACINO_BS * ACINO_BS + ACINO_BS)
int acino_fte_load_x(acino_fte_ctx* ctx, const double* d_x0, void* stream);
/* d_halo_l[3][25] = the 3 frames left of the shard, d_halo_r[3][25] the 3 frames right of it; NULL = zeros
 * (sequence end: the coefficients there are zero anyway). */
int acino_fte_set_halo(acino_fte_ctx* ctx, int which, const double* d_halo_l, const double* d_halo_r, void* stream);
/* Residuals + Jacobians + assembly of iterate `which`; local sums {cost, pred, step_inf, gnorm_inf,
 * n_behind, 0, 0, 0} are left in the context (export_partials copies them to d_partial[8]). */
int acino_fte_eval(acino_fte_ctx* ctx, int which, void* stream);
int acino_fte_export_partials(acino_fte_ctx* ctx, double* d_partial, void* stream);
/* Accept/reject + lambda update from d_total[8] (NULL = this context's own sums); init=1 only records the
 * cost of the freshly loaded iterate. */
int acino_fte_control(acino_fte_ctx* ctx, const double* d_total, int init, void* stream);
int acino_fte_reduce_local(acino_fte_ctx* ctx, void* stream);
/* WRITES this rank's contributions into d_sep[world-1][ACINO_SEP_DOUBLES] (caller zero-fills before;
 * contributions of different ranks never overlap except D and b, which the all-reduce sums). */
int acino_fte_export_separators(acino_fte_ctx* ctx, double* d_sep, int rank, int world, void* stream);
size_t acino_sep_scratch_bytes(int n_sep);
/* Solves the all-reduced separator chain (every rank redundantly): d_sep_x[n_sep][80]. */
int acino_solve_separators(const double* d_sep, int n_sep, double* d_sep_x, void* d_scratch, size_t scratch_bytes,
                           void* stream);
int acino_fte_backsub_local(acino_fte_ctx* ctx, const double* d_sep_x, int rank, int world, void* stream);
int acino_fte_trial(acino_fte_ctx* ctx, void* stream);
/* First / last 3 frames of iterate `which` -> d_edge[6][25]. */
int acino_fte_export_edges(acino_fte_ctx* ctx, int which, double* d_edge, void* stream);

/* ---- sparse bundle adjustment ------------------------------------------------------
 * Replaces scipy.optimize.least_squares(method='trf', loss='cauchy', f_scale=...) inside
 * bundle_adjust_points_and_extrinsics (src/calib/calib.py:345-390) and bundle_adjust_points_only
 * (src/calib/calib.py:307-341).  Cost = sum over observations and both pixel axes of 0.5 f^2 log1p((r/f)^2),
 * scipy's definition, so costs compare 1:1 with `res.cost`.  Observations arrive flat: uv[M][2], cam_idx[M]; the host
 * also supplies the CSR grouping by point (pt_start[P+1], pt_obs[M]).  Poses are [R row-major 9 | t 3] per camera and
 * are updated in place together with the points.  A (point, camera) pair may carry at most ONE observation (refused with
 * ACINO_ERR_INVALID_ARG otherwise).  Up to seven cameras take the fused path: one GPU lane per (point, camera) slot, the
 * 6 x 3 coupling blocks never leave the chip, the Schur complement onto the cameras is accumulated on the fp64 matrix
 * cores (workspace: n_points x (n_cams x 4 + 144) B).  More cameras - or the environment variable ACINO_SBA_UNFUSED, an
 * independent cross-check - take the table path: coupling blocks in a dense table [point][camera] (n_points x n_cams x 144 B),
 * Schur complement by LDS atomics. */
typedef struct acino_sba_params {
  int32_t n_cams;
  int32_t optimize_cameras;   /* 0 = points only (calib.py:327), 1 = points + extrinsics (calib.py:369) */
  int64_t n_points;
  int64_t n_obs;
  double f_scale;             /* Cauchy scale in px: 1 (scipy default, calib.py:381) or 50 (calib.py:327,335) */
  double lam0;                /* initial Marquardt damping (1e-3) */
  double ftol;                /* stop when an accepted step lowers the cost by <= ftol * cost */
  double gtol;                /* stop when ||J^T W r||_inf <= gtol */
  int32_t max_iter;
  int32_t camera_model;       /* 0 = cv2.fisheye (app.py:220-223), 1 = cv2.projectPoints pinhole (app.py:215-218) */
  int32_t precision;          /* ACINO_PREC_F64 (0) or ACINO_PREC_BF16_ROWS (1): BASELINE config 5's "bf16 residuals with fp32
                               * accumulate" for the extrinsic refinement - residuals and Jacobian rows rounded to bf16, the
                               * point / coupling / camera blocks accumulated in fp32; cost, Schur complement, camera solve
                               * and updates fp64 */
  int32_t pad0;
} acino_sba_params;
typedef struct acino_sba_info {
  double cost_initial, cost_final, gnorm_inf, lam;
  int32_t iterations, accepted;
  int32_t status;             /* 0 max_iter, 1 ftol, 3 gtol, 4 lambda overflow, 5 numeric failure */
  int32_t pad0;
} acino_sba_info;
size_t acino_sizeof_sba_params(void);
size_t acino_sizeof_sba_info(void);
size_t acino_sba_workspace_bytes(int n_cams, int64_t n_points, int64_t n_obs);
/* d_intr[C][16] = fx fy cx cy | 12 distortion coefficients (fisheye: k1..k4, rest 0; pinhole: k1 k2 p1 p2 k3 k4 k5 k6
 * s1..s4); d_res_before / d_res_after [M][2] (projected - observed, as calib.py:316,359) or NULL. */
int acino_sba_solve(const acino_sba_params* prm, const double* d_intr, double* d_Rt, double* d_pts,
                    const double* d_uv, const int32_t* d_cam_idx, const int32_t* d_pt_start, const int32_t* d_pt_obs,
                    void* d_ws, size_t ws_bytes, double* d_res_before, double* d_res_after, acino_sba_info* info,
                    void* stream);
/* The same solve with the POINTS sharded over several processes / GPUs and the cameras replicated (BASELINE config 5,
 * "the SBA extrinsic refinement adds a 36x36 camera-block + 36-vector all-reduce per
 * iteration").  Every rank passes its own points and observations and identical camera poses; `reduce` must combine
 * n doubles at d_buf (device memory inside d_ws) over all ranks in place - op 0: sum, op 1: max - and return 0; it is
 * called after the stream has been synchronised, once at entry (max of the input-check flag: a rank with a duplicate (point,
 * camera) pair or a camera index out of range makes EVERY rank return ACINO_ERR_INVALID_ARG together) and five times per LM
 * iteration (max point gradient; camera blocks + camera
 * gradient, 27 n_cams doubles; the Schur complement and its right-hand side, (6 n_cams)^2 + 6 n_cams; the predicted
 * reduction; the trial cost - and the initial cost once).  All ranks take identical
 * decisions and leave with identical poses.  reduce == NULL is acino_sba_solve. */
typedef int (*acino_reduce_fn)(void* user, double* d_buf, int64_t n, int op, void* stream);
int acino_sba_solve_sharded(const acino_sba_params* prm, const double* d_intr, double* d_Rt, double* d_pts,
                            const double* d_uv, const int32_t* d_cam_idx, const int32_t* d_pt_start,
                            const int32_t* d_pt_obs, void* d_ws, size_t ws_bytes, double* d_res_before,
                            double* d_res_after, acino_sba_info* info, acino_reduce_fn reduce, void* reduce_user,
                            void* stream);

/* ---- error bars of the bundle adjustment: covariance of the extrinsics and of the points at a given iterate ------------
 * A = J^T W J of the flat residual under the solver's parametrisation (R <- exp([dw]x) R, t <- t + dt; camera parameter
 * order [dw, dt]), W = the Cauchy IRLS weights 1 / (1 + (r / f_scale)^2), no damping, always fp64 (acino_sba_params is
 * reused unchanged; lam0, ftol, gtol, max_iter and precision are ignored).  With optimize_cameras A has a 7-dimensional null
 * space (world translation, rotation, scale); the camera covariance is taken under seven constraints on the camera
 * parameters, Sigma_c = N (N^T S N)^-1 N^T with S the undamped reduced camera system and N the orthonormal complement of the
 * 6C x 7 constraint block:
 *   ACINO_SBA_GAUGE_BASELINE  the pose of ref_cam held and the distance between the centres of ref_cam and scale_cam held
 *   ACINO_SBA_GAUGE_FREE      the camera rows of the seven generators: Sigma_c is the Moore-Penrose inverse of S
 *   ACINO_SBA_GAUGE_CUSTOM    h_gauge[6C][7] (HOST memory, row-major): the caller's constraints
 * Points: Sigma_p = V_p^-1 + Y_p Sigma_c Y_p^T, Y_p = V_p^-1 W_p^T (optimize_cameras = 0: Sigma_p = V_p^-1, no gauge, the
 * gauge arguments and d_cov_cams are ignored).  A point whose V_p has an LDL^T pivot <= 3 eps max diag V_p (one view or none)
 * is left out of S, of sigma2 and of dof, counted in n_points_excluded, and gets NaN.
 * scale = ACINO_SBA_SCALE_RESIDUAL multiplies every covariance by sigma2 = sum w r^2 / (2 M - dof), dof = 3 P' + 6C - 7
 * (3 P' for points only; P' points kept, M their observations); ACINO_SBA_SCALE_UNIT returns the unit-weight inverse.
 *   d_cov_cams[6C][6C]   d_cov_points[P][6] (xx xy xz yy yz zz; may be NULL)   d_std_points[P] = sqrt(trace) (may be NULL)
 * The workspace is the caller's, 256-byte aligned (ACINO_ERR_WORKSPACE otherwise).  A singular problem - 2 M <= dof, gauge
 * constraints of rank below 7, or a Cholesky pivot of N^T S N at or below (6C - 7) eps max diag (a camera no point sees, too
 * few points, a constraint block that does not fix the gauge) - is ACINO_ERR_NUMERIC with info->status = 5 and every output
 * NaN.  optimize_cameras with one camera, ref_cam == scale_cam, an observation list or camera index out of range and two
 * observations of one point by one camera are ACINO_ERR_INVALID_ARG.  The call synchronises the stream (two or three times).
 * Sums go through per-workgroup partials added in a fixed order: a repeated call is bit-identical. */
#define ACINO_SBA_GAUGE_BASELINE 0
#define ACINO_SBA_GAUGE_FREE 1
#define ACINO_SBA_GAUGE_CUSTOM 2
#define ACINO_SBA_SCALE_RESIDUAL 0
#define ACINO_SBA_SCALE_UNIT 1
typedef struct acino_sba_cov_info {
  double sigma2;              /* sum_w_r2 / (2 n_obs_used - dof); NaN when 2 M <= dof */
  double sum_w_r2;
  double min_pivot_ratio;     /* smallest Cholesky pivot of N^T S N over its largest diagonal entry (NaN for points only) */
  int64_t dof;
  int64_t n_obs_used;         /* observations of the points kept */
  int32_t n_points_excluded;
  int32_t status;             /* 0 ok, 5 numeric */
} acino_sba_cov_info;
size_t acino_sizeof_sba_cov_info(void);
size_t acino_sba_covariance_workspace_bytes(int n_cams, int64_t n_points, int64_t n_obs);
int acino_sba_covariance(const acino_sba_params* prm, const double* d_intr, const double* d_Rt, const double* d_pts,
                         const double* d_uv, const int32_t* d_cam_idx, const int32_t* d_pt_start, const int32_t* d_pt_obs,
                         int gauge, int ref_cam, int scale_cam, const double* h_gauge, int scale, void* d_ws, size_t ws_bytes,
                         double* d_cov_cams, double* d_cov_points, double* d_std_points, acino_sba_cov_info* info,
                         void* stream);

/* ---- generic-skeleton forward kinematics (src/build.py:28-86) ---------------------------
 * The host compiles a skeleton dictionary into <= ACINO_SKEL_MAX_OPS link operations, evaluated in order for every
 * frame:  pose[child] = pose[parent] + M @ off,  M = R_loc or R_loc^T of the PARENT part's own angles
 * (phi, theta, psi at q[3+angle], q[3+L+angle], q[3+2L+angle]; R_loc = Rz(psi) Rx(phi) Ry(theta) restricted to the
 * dofs in flags bits 0..2; bit 3 set = use R_loc, clear = R_loc^T).  All n_pose slots start at the root (x, y, z). */
#define ACINO_SKEL_MAX_OPS 64
typedef struct acino_skel_op {
  int32_t child, parent, angle, flags;
  double off[3];
} acino_skel_op;
/* d_q[N][3 + 3 L] -> d_pos[N][n_pose][3]; h_ops is a HOST array. */
int acino_skeleton_fk(const double* d_q, int64_t n_frames, int n_angles, int n_pose, const acino_skel_op* h_ops,
                      int n_ops, double* d_pos, void* stream);

/* ---- generic-skeleton Full Trajectory Estimation (src/build.py:28-335: build_model + solve_optimisation) -------------
 * The skeleton-driven NLP of the reference in reduced form (oracle/skel_fte.py):
 *   min  sum |w_ncl (pi_c(pose_l(x_n))_d - z_ncld)|  +  sum_{n>=3,p} (model_weight / h^4) (x_n - 3 x_n-1 + 3 x_n-2 - x_n-3)_p^2
 *   s.t. lo[n][p] <= x[n][p] <= hi[n][p]
 * over the n_active states that move a pose (x, y, z and the enabled angles of parent parts; h_active[n_active] holds
 * their indices in the full state [x y z | phi | theta | psi], increasing, starting 0, 1, 2 - every other state stays at
 * its initial 0 as in the reference).  h_ops is the link program of acino_skeleton_fk.  d_meas[N][C][n_pose][2] and
 * d_w[N][C][n_pose] are indexed by POSE SLOT: the caller pairs slots with detections (the reference pairs by position in
 * the skeleton's marker list, build.py:113-128,288-292) and sets w = 1/R where likelihood > threshold, else 0.
 * d_x[N][n_active]: initial iterate in, solution out.  d_pos[N][n_pose][3] (may be NULL): poses of the solution.
 * Solved by the projected Levenberg-Marquardt of the cheetah path (L1 loss: IRLS curvature w^2 / max(|e|, l1_eps), cost
 * and gradient those of |e|); the controller runs on the device (one status word per clip read back per iteration).
 * Limits: n_active <= 64, 2 n_pose C <= 256.
 * The measurement loss is the params block's `loss`, read by EVERY acino_skel_fte_* entry.  ACINO_SKEL_LOSS_L1 (0) is the problem
 * above.  ACINO_SKEL_LOSS_REDESCENDING replaces |e| by the reference's redescending_loss rho(e) (build.py:382-395, commented out at
 * :307) with its only constants a, b, c = 3, 10, 20 in scaled residual units (the scale is the caller's 1 / w): cost sum rho(e)
 * over the kept rows, d cost / d e = rho'(|e|) sign(e), Gauss-Newton curvature w^2 h(e) with h = clip((rho'(e) - rho'(0+)) / e,
 * 0, 1) - the loss and the conventions of acino_fte_*; l1_eps is then not read.  Prior, bounds, pin rule, controller and
 * factorisation are the same.  From a far start every residual lies beyond c, where rho is constant: the solve is meant to start
 * at the L1 solution (build.solve_models does that).  Any other value of `loss` is ACINO_ERR_INVALID_ARG. */
#define ACINO_SKEL_LOSS_L1 0
#define ACINO_SKEL_LOSS_REDESCENDING 1
typedef struct acino_skel_fte_params {
  int32_t n_frames, n_cams, n_pose, n_ops, n_angles, n_active;
  int32_t max_iter;
  int32_t loss;               /* ACINO_SKEL_LOSS_L1 (0: what the field held while it was reserved) or _REDESCENDING */
  double h;                   /* time step (build.py:131: 1/120)                           */
  double model_weight;        /* build.py:186-191: 0.002 for every state                    */
  double l1_eps;              /* floor of |e| in the IRLS weight (scaled residual units)     */
  double lam0, ftol, xtol, gtol, lam_max;
} acino_skel_fte_params;
typedef struct acino_skel_fte_info {
  double cost_initial, cost_final, gnorm_inf, lam;
  int32_t iterations, accepted;
  int32_t status;             /* 0 max_iter, 1 ftol, 2 xtol, 3 gtol, 4 lambda overflow, 5 numeric failure */
  int32_t pad0;
} acino_skel_fte_info;
size_t acino_sizeof_skel_fte_params(void);
size_t acino_sizeof_skel_fte_info(void);
size_t acino_skel_fte_workspace_bytes(const acino_skel_fte_params* p);
int acino_skel_fte_solve(const acino_skel_fte_params* p, const acino_skel_op* h_ops, const int32_t* h_active,
                         const double* d_meas, const double* d_w, const double* d_cams24, const double* d_lo,
                         const double* d_hi, double* d_x, double* d_pos, void* d_workspace, size_t workspace_bytes,
                         acino_skel_fte_info* info, void* stream);
/* The same for n_clips independent clips of n_frames frames each in one call (same skeleton, same cameras; the reference
 * solves windows of N = 100 frames, build.py:131-133 - a video is many of them): every array gains a leading clip index
 * (d_meas[n_clips][N][C][n_pose][2], d_x[n_clips][N][n_active], ..., infos[n_clips]); no coupling across clips; one
 * workgroup per clip walks its banded factorisation, every clip has its own Levenberg-Marquardt controller on the device
 * and stops on its own criteria.  With n_clips > 1 and infos given, a clip that fails numerically (infos[b].status = 5) does
 * NOT fail the call: the other clips' results stand and the return value is ACINO_OK; the caller reads the status per clip.
 * (n_clips = 1, or no infos: ACINO_ERR_NUMERIC as acino_skel_fte_solve.) */
size_t acino_skel_fte_workspace_bytes_batch(const acino_skel_fte_params* p, int n_clips);
int acino_skel_fte_solve_batch(const acino_skel_fte_params* p, int n_clips, const acino_skel_op* h_ops, const int32_t* h_active,
                               const double* d_meas, const double* d_w, const double* d_cams24, const double* d_lo,
                               const double* d_hi, double* d_x, double* d_pos, void* d_workspace, size_t workspace_bytes,
                               acino_skel_fte_info* infos, void* stream);
/* The same two entries on the OpenCV pinhole camera (cv2.projectPoints: k1 k2 p1 p2 k3 k4 k5 k6 s1 s2 s3 s4, skew ignored,
 * the tilted model tau_x = tau_y = 0): d_cams32[C][32] pinhole records in place of d_cams24, every other argument, the
 * workspace size and the solver as above.  fp64. */
int acino_skel_fte_solve_pinhole(const acino_skel_fte_params* p, const acino_skel_op* h_ops, const int32_t* h_active,
                                 const double* d_meas, const double* d_w, const double* d_cams32, const double* d_lo,
                                 const double* d_hi, double* d_x, double* d_pos, void* d_workspace, size_t workspace_bytes,
                                 acino_skel_fte_info* info, void* stream);
int acino_skel_fte_solve_batch_pinhole(const acino_skel_fte_params* p, int n_clips, const acino_skel_op* h_ops,
                                       const int32_t* h_active, const double* d_meas, const double* d_w, const double* d_cams32,
                                       const double* d_lo, const double* d_hi, double* d_x, double* d_pos, void* d_workspace,
                                       size_t workspace_bytes, acino_skel_fte_info* infos, void* stream);

/* ---- error bars of the generic-skeleton FTE: per-frame covariance of the states and of every pose slot --------------------
 * Evaluated at the iterate d_x[n_clips][N][n_active] (normally the solution of acino_skel_fte_solve*), unknowns frame-major:
 *   A = blockdiag_n( sum_{c,l,d} w_ncl^2 J_ncld^T J_ncld ) + 2 q D3^T D3,   q = model_weight / h^4
 * with J the 1 x n_active rows of the solve's own assembly (rows it drops - w = 0, non-finite measurements, |z_cam| < 1e-9 -
 * contribute nothing) and D3 the third-difference operator of a clip.  This is the Fisher information of the model the
 * objective states (sum |w r| is the negative log-likelihood of Laplace noise of scale 1 / w: information w^2) plus the prior;
 * A^-1 is the asymptotic covariance of the L1 estimate.  The IRLS curvature w^2 / max(|e|, l1_eps) of the solver is NOT used,
 * every detection the caller gave a weight counts fully (outliers are not discounted), and there is no Marquardt term.
 * Bound-active variables are pinned as the solver pins them (at a bound with its own gradient pushing outward): their rows
 * and columns are exactly 0 in every output.  Outputs (fp64, any may be NULL but not all three):
 *   d_cov_x  [n_clips][N][n_active][n_active]  diagonal blocks of A^-1
 *   d_cov_pos[n_clips][N][n_pose][3][3]        G_l cov_x G_l^T, G_l the 3 x n_active Jacobian of pose slot l
 *   d_std_pos[n_clips][N][n_pose]              sqrt(trace(cov_pos)), metres
 * camera_model 0: d_cams = fisheye records [C][24]; 1: pinhole records [C][32].  h_ops / h_active / d_meas / d_w / d_lo / d_hi as
 * the solve; limits as the solve (n_active <= 64, 2 n_pose C <= 256); arguments are validated before any device call.  The
 * workspace is the caller's, 256-byte aligned (ACINO_ERR_WORKSPACE otherwise).  A pivot that is not above zero (a state observed
 * in no frame of the clip) makes the clip singular: h_status[b] = 5 (else 0) and its outputs are NaN; with n_clips > 1 and
 * h_status given the call returns ACINO_OK and the other clips stand, otherwise ACINO_ERR_NUMERIC.  One stream synchronisation,
 * to read the status words.  One workgroup per clip walks the factorisation and the Takahashi recursion: meant for batches.
 * With p->loss = ACINO_SKEL_LOSS_REDESCENDING the blocks are sum w^2 h(e) J^T J - the Gauss-Newton curvature of the stated
 * objective at d_x, the definition of acino_fte_covariance: a detection the loss rejects (h ~ 0) adds nothing, and unlike the L1
 * Fisher matrix A depends on the residuals.  Which rows are kept, the pin rule (with the robust solver's own g and diagonal),
 * the outputs and the status rules are the same, and so they are for acino_skel_fte_sample*, _covariance_pinned and
 * _covariance_rates; acino_skel_fte_observability and pin_unobserved go by the kept rows (w^2), whatever their h. */
size_t acino_skel_fte_covariance_workspace_bytes(const acino_skel_fte_params* p, int n_clips);
int acino_skel_fte_covariance(const acino_skel_fte_params* p, int n_clips, int camera_model /* 0 fisheye: d_cams24, 1 pinhole: d_cams32 */,
                              const acino_skel_op* h_ops, const int32_t* h_active, const double* d_meas, const double* d_w,
                              const double* d_cams, const double* d_lo, const double* d_hi, const double* d_x,
                              double* d_cov_x, double* d_cov_pos, double* d_std_pos, int32_t* h_status /* [n_clips], may be NULL */,
                              void* d_ws, size_t ws_bytes, void* stream);

/* ---- joint posterior samples of the generic-skeleton FTE trajectory ---------------------------------------------------------
 * The other use of the same matrix: with A exactly the matrix of acino_skel_fte_covariance at d_x (Fisher blocks with w^2,
 * 2 q D3^T D3, bound-active variables pinned, unknowns frame-major, no Marquardt term) and A = L L^T its banded Cholesky factor,
 *   d_x_samples[b][s] = d_x[b] + delta,   delta = L_b^-T z[b][s],   z of a pinned variable counted as 0
 * for the caller's d_z[n_clips][S][N][n_active] (S = n_samples).  For standard-normal z, Cov(delta) = A^-1 with every
 * cross-frame block: the samples are joint draws of the whole trajectory from the Laplace posterior - what step length, mean
 * speed over a stride or the range of a joint angle over a clip are computed from.  delta is exactly 0 at pinned variables
 * whatever z holds there.  The map is deterministic - the library owns no random generator - and delta(s) depends on z(s)
 * alone: the same bits whatever other samples or clips share the call.  Samples are NOT clipped to the box [d_lo, d_hi]: the
 * Laplace posterior is a Gaussian, and only the pinned variables are held.  Outputs (fp64):
 *   d_x_samples  [n_clips][S][N][n_active]
 *   d_pos_samples[n_clips][S][N][n_pose][3]   may be NULL; the forward kinematics of every sample itself (the link program on
 *                                             the sample's active states, every other state 0) - not the linearisation
 * Argument conventions, limits (n_active <= 64, 2 n_pose C <= 256), workspace alignment, h_status, the return rules and the one
 * stream synchronisation are those of acino_skel_fte_covariance: a singular clip (a pivot not above zero) gets h_status[b] = 5
 * and NaN samples; with n_clips > 1 and h_status given the other clips stand and the call returns ACINO_OK, otherwise
 * ACINO_ERR_NUMERIC.  n_samples < 1, a NULL d_z or d_x_samples, and d_z overlapping either output are ACINO_ERR_INVALID_ARG
 * before any device call.  The factorisation is one workgroup per clip; the back-substitution runs on a grid of (panels of 64
 * samples, clips). */
size_t acino_skel_fte_sample_workspace_bytes(const acino_skel_fte_params* p, int n_clips, int64_t n_samples);
int acino_skel_fte_sample(const acino_skel_fte_params* p, int n_clips, int camera_model /* 0 fisheye: d_cams24, 1 pinhole: d_cams32 */,
                          const acino_skel_op* h_ops, const int32_t* h_active, const double* d_meas, const double* d_w,
                          const double* d_cams, const double* d_lo, const double* d_hi, const double* d_x, int64_t n_samples,
                          const double* d_z /* [n_clips][S][N][n_active] */, double* d_x_samples /* [n_clips][S][N][n_active] */,
                          double* d_pos_samples /* [n_clips][S][N][n_pose][3], may be NULL */,
                          int32_t* h_status /* [n_clips], may be NULL */, void* d_ws, size_t ws_bytes, void* stream);

/* ---- which states does a clip observe?  Pinning the unobserved ones in the two posterior entries ----------------------------
 * With H_F[n] the Fisher block of frame n at d_x (sum_{c,l,d} w^2 J^T J: the blocks of acino_skel_fte_covariance WITHOUT the prior)
 * and ACINO_SKEL_UNOBS_REL = 1e-24, per clip b and active state p:
 *   info[b][p]       = sum_n H_F[n][p][p], over the clip's frames in frame order (the same bits whatever else shares the batch)
 *   n_seen[b][p]     = the number of frames with H_F[n][p][p] > ACINO_SKEL_UNOBS_REL * max_q info[b][q]
 *   unobserved[b][p] = info[b][p] <= ACINO_SKEL_UNOBS_REL * max_q info[b][q]       (1 or 0)
 * (a Jacobian entry that is zero only up to rounding is ~1e-16 relative, its square ~1e-32; a clip without any weighted detection
 * has max info = 0 and every state unobserved).  An unobserved state makes A singular - the prior alone leaves its quadratic
 * drift free - and acino_skel_fte_covariance / _sample report status 5 for the clip.  Two active states of the reference's shipped
 * human skeleton (the psi angles of "chin" and "hip2": every link they rotate lies along the rotation's own axis) are unobserved
 * on every clip; so are the joints of a limb no camera detects in the clip.
 *
 * acino_skel_fte_observability: the Fisher assembly and one small reduction (one workgroup per clip) on `stream`; no
 * factorisation, no synchronisation, nothing read from host memory after the return.  Outputs on the device, each
 * [n_clips][n_active], any may be NULL but not all three: d_info (fp64), d_n_seen (int32), d_unobserved (uint8).  Leading
 * arguments, limits and workspace rules as acino_skel_fte_covariance (d_lo / d_hi are not read: the rule knows no bounds); both
 * camera models.  n_seen is the diagnostic for a clip that stays singular although nothing is unobserved: the prior's quadratic
 * drift needs a state to be seen in three frames.
 *
 * acino_skel_fte_covariance_pinned / acino_skel_fte_sample_pinned: the two entries above with two more arguments at the end.
 *   pin_unobserved  0: the entry above, bit for bit.  1: every unobserved state of a clip is pinned in EVERY frame of the clip,
 *                   by the rule of a bound pin (row and column 0, diagonal 1, the prior's couplings dropped) and in addition to
 *                   the bound pins; everything else about A is unchanged.  cov_x has rows and columns exactly 0 there, delta
 *                   of a sample is exactly 0 there whatever z holds.  A pose slot l of frame n with a nonzero entry of G_l[n] in
 *                   the column of an unobserved state gets std_pos = +inf and all nine entries of cov_pos NaN: its spread is
 *                   not finite under the stated model; every other slot gets G_l cov_x G_l^T.  pos_samples of such a slot show
 *                   NO spread from that state (it is held at x): the mask is how the caller finds out.  The factorisation
 *                   still decides singularity: a state seen in one or two frames is not pinned, and the clip stays status 5.
 *                   Any other value: ACINO_ERR_INVALID_ARG.
 *   d_unobserved    NULL, or [n_clips][n_active] (uint8, device): the mask of the rule above, written whether or not
 *                   pin_unobserved is set; it tells the zeros that mean "undetermined" from those of a bound pin.
 * Their workspace queries take pin_unobserved too (0 for a value outside {0, 1}); the size they return covers either value and
 * a d_unobserved request, and is what these two entries need unless pin_unobserved == 0 and d_unobserved == NULL. */
#define ACINO_SKEL_UNOBS_REL 1e-24
size_t acino_skel_fte_observability_workspace_bytes(const acino_skel_fte_params* p, int n_clips);
int acino_skel_fte_observability(const acino_skel_fte_params* p, int n_clips, int camera_model /* 0 fisheye: d_cams24, 1 pinhole: d_cams32 */,
                                 const acino_skel_op* h_ops, const int32_t* h_active, const double* d_meas, const double* d_w,
                                 const double* d_cams, const double* d_lo, const double* d_hi, const double* d_x,
                                 double* d_info, int32_t* d_n_seen, uint8_t* d_unobserved, void* d_ws, size_t ws_bytes,
                                 void* stream);
size_t acino_skel_fte_covariance_pinned_workspace_bytes(const acino_skel_fte_params* p, int n_clips, int pin_unobserved);
int acino_skel_fte_covariance_pinned(const acino_skel_fte_params* p, int n_clips, int camera_model, const acino_skel_op* h_ops,
                                     const int32_t* h_active, const double* d_meas, const double* d_w, const double* d_cams,
                                     const double* d_lo, const double* d_hi, const double* d_x, double* d_cov_x,
                                     double* d_cov_pos, double* d_std_pos, int32_t* h_status /* [n_clips], may be NULL */,
                                     void* d_ws, size_t ws_bytes, void* stream, int pin_unobserved,
                                     uint8_t* d_unobserved /* [n_clips][n_active], may be NULL */);
size_t acino_skel_fte_sample_pinned_workspace_bytes(const acino_skel_fte_params* p, int n_clips, int64_t n_samples,
                                                    int pin_unobserved);
int acino_skel_fte_sample_pinned(const acino_skel_fte_params* p, int n_clips, int camera_model, const acino_skel_op* h_ops,
                                 const int32_t* h_active, const double* d_meas, const double* d_w, const double* d_cams,
                                 const double* d_lo, const double* d_hi, const double* d_x, int64_t n_samples,
                                 const double* d_z, double* d_x_samples, double* d_pos_samples,
                                 int32_t* h_status /* [n_clips], may be NULL */, void* d_ws, size_t ws_bytes, void* stream,
                                 int pin_unobserved, uint8_t* d_unobserved /* [n_clips][n_active], may be NULL */);

/* ---- error bars for the rates of the generic-skeleton FTE: dx, ddx and the pose velocities -------------------------------------
 * acino_skel_fte_covariance_rates: acino_skel_fte_covariance_pinned with four more outputs.  A, the bound pins, pin_unobserved,
 * the status rules, the limits, both camera models and the workspace rules are exactly those of that entry, and its three
 * outputs are bit-identical to it.  Let e be the estimation error of a clip, Cov(e) = A^-1 with the rows and columns of pinned
 * variables 0.  Every new output is the covariance C S_win C^T of a linear map of a window of at most three consecutive frames
 * of the frame's own clip (a window never reaches into another clip of the batch); h = p->h:
 *   dx, ddx   what the Python layer returns beside x (build._finite_diff_states; NOT the rule of acino_fte_derivatives):
 *               N >= 3, n >= 2:  window (n-2, n-1, n);  dx_n = (x_n - x_n-1) / h,  ddx_n = (x_n - 2 x_n-1 + x_n-2) / h^2
 *               N >= 3, n < 2:   window (0, 1, 2);  ddx_0 = ddx_1 = ddx_2,  dx_1 = (x_1 - x_0) / h,
 *                                dx_0 = dx_1 - h ddx_1 = (-2 x_0 + 3 x_1 - x_2) / h
 *               N = 2:           ddx = 0,  dx_1 = (x_1 - x_0) / h,  dx_0 = 0  (the cheetah rule has dx_0 = dx_1)
 *               N = 1:           everything 0
 *   v_n,l     the velocity of pose slot l, (pose_l(x_n) - pose_l(x_n-1)) / h, linearised as (G_l(x_n) e_n - G_l(x_n-1) e_n-1) / h
 *             with G_l the pose Jacobian of d_cov_pos; frame 0 of a clip repeats frame 1; N = 1: 0
 * Outputs (fp64, device; any of the seven may be NULL, but not all of them):
 *   d_cov_dx, d_cov_ddx [n_clips][N][n_active][n_active]   (unit/s)^2 and (unit/s^2)^2
 *   d_cov_vel           [n_clips][N][n_pose][3][3]         (m/s)^2
 *   d_std_vel           [n_clips][N][n_pose]               sqrt(trace(cov_vel)), m/s
 * sqrt(2 diag cov_x) / h is NOT a bar on dx: the third-difference prior correlates neighbouring frames almost perfectly, and
 * the cross-frame blocks of the window - which lie inside the factor's band, so the result is exact - cancel most of it.
 * A variable pinned in frame a contributes nothing from frame a: block S_ab of A^-1 has row p dropped if p is pinned in frame
 * a and column q dropped if q is pinned in frame b.  With pin_unobserved = 1, cov_dx and cov_ddx are exactly 0 in the rows and
 * columns of the unobserved states, and a slot whose G_l has a nonzero entry in such a column in frame n or in frame n-1 gets
 * std_vel = +inf and cov_vel = NaN (as std_pos).  A singular clip: status 5 and every new output NaN; in a batch with h_status
 * the other clips stand.  One run of the factorisation serves all outputs; arguments are validated before any device call;
 * one stream synchronisation.  The workspace query returns what acino_skel_fte_covariance_pinned_workspace_bytes returns: the
 * rates are streamed from the blocks the recursion leaves in the workspace, one workgroup per frame. */
size_t acino_skel_fte_covariance_rates_workspace_bytes(const acino_skel_fte_params* p, int n_clips, int pin_unobserved);
int acino_skel_fte_covariance_rates(const acino_skel_fte_params* p, int n_clips, int camera_model, const acino_skel_op* h_ops,
                                    const int32_t* h_active, const double* d_meas, const double* d_w, const double* d_cams,
                                    const double* d_lo, const double* d_hi, const double* d_x, double* d_cov_x,
                                    double* d_cov_pos, double* d_std_pos, double* d_cov_dx, double* d_cov_ddx,
                                    double* d_cov_vel, double* d_std_vel, int32_t* h_status /* [n_clips], may be NULL */,
                                    void* d_ws, size_t ws_bytes, void* stream, int pin_unobserved,
                                    uint8_t* d_unobserved /* [n_clips][n_active], may be NULL */);

/* ---- generic-skeleton FTE error bars that include the calibration: sensitivity to the camera extrinsics ---------------------
 * acino_skel_fte_calibration_sensitivity: S = -A^-1 G, the sensitivity of the trajectory to the extrinsics, and the "consider"
 * covariance S Sigma S^T it gives for a covariance Sigma of the extrinsics.  All quantities are at the caller's iterate
 * d_x[n_clips][N][n_active].  A, the bound pins, pin_unobserved, the status rules, the limits, both camera models and the
 * leading arguments are exactly those of acino_skel_fte_covariance_pinned.
 * Camera parameters are c = [dw_0, dt_0, ..., dw_C-1, dt_C-1], applied as R_c <- exp([dw]x) R_c, t_c <- t_c + dt: the order
 * and units of acino_sba_covariance (and calib.extrinsic_cov), so its cov_cams plugs in unchanged.
 * For a row (n, c, l, d) that the assembly keeps - it drops a row when w = 0, when the measurement is non-finite, or when
 * |z_cam| < 1e-9 - with p = pose_l(x_n):
 *   J_x = J_pi G_l (2 x n_active), J_pi and G_l those of the Fisher assembly and of d_cov_pos.
 *   J_c = J_pi R_c^T [ -[R_c p]x | I_3 ] (2 x 6), the derivative of the predicted pixel with respect to (dw_c, dt_c).
 *   The weight is w^2: the Fisher weight of the stated Laplace model, the same statement A makes.  It is NOT the IRLS
 *   curvature; it depends neither on the residual nor on l1_eps.
 *   G_n[:, 6c:6c+6] = sum over l, d of J_x^T w^2 J_c;  S = -A^-1 G, shape [n_clips][N][n_active][6C].
 *   Rows of G for pinned variables (bound pins and, with pin_unobserved, unobserved pins) are 0: rows of S are EXACTLY 0 there.
 * S is the shift of the minimiser of the expected (Fisher) quadratic model per unit change of the extrinsics, consistent with
 * the A^-1 the covariance reports.  It is NOT a derivative of the L1 / Levenberg-Marquardt end point.
 * With Sigma = d_cov_cams[6C][6C] (e.g. cov_cams of acino_sba_covariance; only PSD - a held camera has zero rows - so it is
 * multiplied, T = S_n Sigma, then T S_n^T, and never factored):
 *   d_sens       [n_clips][N][n_active][6C]         S
 *   d_cov_x_cal  [n_clips][N][n_active][n_active]   S_n Sigma S_n^T, symmetric to the bit
 *   d_cov_pos_cal[n_clips][N][n_pose][3][3]         G_l cov_x_cal G_l^T, symmetric to the bit
 *   d_std_pos_cal[n_clips][N][n_pose]               sqrt(trace(cov_pos_cal)), metres
 * Any output may be NULL, but not all of them; a cov / std output without d_cov_cams is ACINO_ERR_INVALID_ARG.  With
 * pin_unobserved = 1 a slot whose G_l has a nonzero entry in the column of an unobserved state gets std_pos_cal = +inf and NaN
 * cov_pos_cal (the rule of d_std_pos).  A singular clip gets status 5 and NaN in every output; in a batch with h_status the
 * other clips stand.  The result of one clip is the same bits whatever else shares the call.
 * The total covariance of a trajectory is cov + cov_cal ONLY for a calibration obtained from OTHER data than the clips being
 * solved; it is not valid for extrinsics refined on the same clips (the two errors are then correlated).  The calibration term
 * is perfectly correlated across frames: smoothing does not average it out.
 * Limit: n_cams <= ACINO_MAX_CAMS = 16 (96 columns), checked with every other argument before any device call.  Launches on
 * `stream`: the Fisher assembly and build of the covariance, k_skel_calib_rhs (-G as 6C columns), k_skel_factor, one forward
 * (k_skel_fwdsub) and one backward substitution per clip and panel of 64 columns, k_skel_calib_combine; one synchronisation.
 * Workspace: the pinned covariance workspace plus two column buffers [n_clips][6C][N][n_active], 256-byte aligned
 * (ACINO_ERR_WORKSPACE otherwise); the query returns 0 outside the limits.
 * Defined for the L1 loss only: with p->loss != ACINO_SKEL_LOSS_L1 the call returns ACINO_ERR_INVALID_ARG (the message names the
 * loss) before any device call. */
size_t acino_skel_fte_calibration_workspace_bytes(const acino_skel_fte_params* p, int n_clips, int pin_unobserved);
int acino_skel_fte_calibration_sensitivity(const acino_skel_fte_params* p, int n_clips, int camera_model, const acino_skel_op* h_ops,
                                           const int32_t* h_active, const double* d_meas, const double* d_w, const double* d_cams,
                                           const double* d_lo, const double* d_hi, const double* d_x,
                                           const double* d_cov_cams /* [6C][6C] or NULL */, double* d_sens, double* d_cov_x_cal,
                                           double* d_cov_pos_cal, double* d_std_pos_cal,
                                           int32_t* h_status /* [n_clips], may be NULL */, void* d_ws, size_t ws_bytes,
                                           void* stream, int pin_unobserved,
                                           uint8_t* d_unobserved /* [n_clips][n_active], may be NULL */);

/* ---- generic-skeleton FTE error bars that include the link lengths: sensitivity to the links' log-scales ---------------------
 * acino_skel_fte_link_sensitivity: what the calibration entry above does for the extrinsics, for the body's dimensions.  Every
 * op k of the link program belongs to a group h_group[k] in -1 .. n_groups-1 (-1: its offset stays fixed; the convention of
 * acino_skel_link_scale, n_groups in 1..16) and theta_g is the log-scale of group g, theta = 0 the offsets of h_ops as given:
 *   pos_l(x, theta) = root + sum over the ops k on l's path of exp(theta_g(k)) M_k(x) off_k
 *   D_l[:, g] = d pos_l / d theta_g = the sum of M_k(x) off_k over the ops of group g on l's path         (the direct term)
 *   G_n[p, g] = sum over c, l of G_l[:, p] . (w^2 J_pi^T J_pi) D_l[:, g]                                   (the cross term)
 * with G_l, J_pi, the kept rows (w = 0, a non-finite measurement and |z_cam| < 1e-9 are dropped) and the Fisher weight w^2 of
 * the calibration entry: neither the residuals nor l1_eps enter, and the smoothness prior does not depend on theta.
 *   S = -A^-1 G, [n_clips][N][n_active][K]; A, the bound pins, pin_unobserved, the status rules, the limits, both camera models
 *   and the leading arguments are exactly those of acino_skel_fte_covariance_pinned; rows of pinned variables are EXACTLY 0.
 *   T_l = G_l S_n + D_l (3 x K): a pose moves through the states AND directly.
 * With Sigma = d_cov_links[K][K], a covariance of the log-scales (e.g. cov_log_scales of a length fit; only PSD - a held group
 * has zero rows - so it is multiplied and never factored):
 *   d_sens    [n_clips][N][n_active][K]          S
 *   d_dpos    [n_clips][N][n_pose][3][K]         T_l
 *   d_cov_x   [n_clips][N][n_active][n_active]   S_n Sigma S_n^T, symmetric to the bit
 *   d_cov_pos [n_clips][N][n_pose][3][3]         T_l Sigma T_l^T, symmetric to the bit
 *   d_std_pos [n_clips][N][n_pose]               sqrt(trace(cov_pos)), metres
 * Any output may be NULL, but not all of them; d_cov_x, d_cov_pos or d_std_pos without d_cov_links is ACINO_ERR_INVALID_ARG.
 * d_unknown[K] (uint8, may be NULL) marks groups whose length the caller cannot bound: a slot whose path holds an op of such a
 * group gets std_pos = +inf and NaN cov_pos; the group's column of S and T_l is reported all the same.  With pin_unobserved = 1 a
 * slot whose G_l has a nonzero entry in the column of an unobserved state gets std_pos = +inf and NaN cov_pos (the rule of
 * d_std_pos of the covariance); its T_l is the derivative with the unobserved states held.  A singular clip gets status 5 and NaN
 * in every output; in a batch with h_status the other clips stand.  The result of one clip is the same bits whatever else shares
 * the call.
 * The total covariance of a trajectory is cov + cov_links ONLY for a Sigma obtained from OTHER data than the clip being solved, or
 * an honest prior; lengths fitted to the same clip have errors correlated with the trajectory's.  The term is perfectly correlated
 * across frames: smoothing does not average it out.
 * Every argument is checked before any device call: n_groups in 1..16, every h_group[k] in -1..n_groups-1, the loss L1
 * (p->loss != ACINO_SKEL_LOSS_L1 is ACINO_ERR_INVALID_ARG, as above).  Launches on `stream`: the Fisher assembly and build of the
 * covariance, k_skel_links_rhs (-G as K columns), k_skel_factor, one forward (k_skel_fwdsub) and one backward substitution per
 * clip (K <= 16 columns: one panel), k_skel_links_combine; one synchronisation.
 * Workspace: the pinned covariance workspace plus two column buffers [n_clips][16][N][n_active], 256-byte aligned
 * (ACINO_ERR_WORKSPACE otherwise); the query returns 0 outside the limits. */
size_t acino_skel_fte_link_workspace_bytes(const acino_skel_fte_params* p, int n_clips, int pin_unobserved);
int acino_skel_fte_link_sensitivity(const acino_skel_fte_params* p, int n_clips, int camera_model, const acino_skel_op* h_ops,
                                    const int32_t* h_active, const double* d_meas, const double* d_w, const double* d_cams,
                                    const double* d_lo, const double* d_hi, const double* d_x,
                                    const int32_t* h_group /* [n_ops] */, int n_groups,
                                    const double* d_cov_links /* [K][K] or NULL */, const uint8_t* d_unknown /* [K] or NULL */,
                                    double* d_sens, double* d_dpos, double* d_cov_x, double* d_cov_pos, double* d_std_pos,
                                    int32_t* h_status /* [n_clips], may be NULL */, void* d_ws, size_t ws_bytes, void* stream,
                                    int pin_unobserved, uint8_t* d_unobserved /* [n_clips][n_active], may be NULL */);

/* ---- the link lengths fitted JOINTLY with the generic-skeleton FTE trajectory: the reduced system of the log-scales -----------
 * acino_skel_fte_link_fit_system: theta, h_group, n_groups, A, G, D_l, the kept rows, the pins, pin_unobserved, the status rules,
 * the limits and the leading arguments are those of acino_skel_fte_link_sensitivity above.  With e = w (uv - meas),
 * J_theta = J_pi D_l and F(x, theta) the solver's own objective of a clip (data term plus smoothness), per clip at d_x:
 *   d_cost   [n_clips]         F(x, 0), the value the solve reports
 *   d_c      [n_clips][K]      dF/dtheta at fixed x = sum w sign(e) J_theta (the solver's gradient convention gu = w sign(eu))
 *   d_C      [n_clips][K][K]   sum w^2 J_theta^T J_theta, symmetric to the bit
 *   d_S      [n_clips][K][K]   C - G^T A^-1 G = C - Y^T Y, Y = L^-1 G (rows of pinned variables 0), symmetric to the bit
 *   d_r      [n_clips][K]      c - G^T A^-1 g_x, g_x the solver's gradient of F in the active states at x, 0 at pinned rows: the
 *                              Schur right-hand side of the quadratic model, correct to first order where x is not stationary
 *   d_sens   [n_clips][N][n_active][K]   (may be NULL) -A^-1 G: the bits of d_sens of acino_skel_fte_link_sensitivity
 *   d_newton [n_clips][N][n_active]      (may be NULL) -A^-1 g_x, the Fisher-scoring step of the trajectory
 * [[A, G], [G^T, C]] is the information of the joint posterior over (trajectory, log-scales): S is the information of theta with
 * the trajectory eliminated, and with Sigma = (sum over the clips that share theta of S)^-1 as d_cov_links the sums
 * cov + cov_links of the sensitivity entry ARE the marginals of the joint posterior (A^-1 + S_x Sigma S_x^T, S_x = -A^-1 G).
 * Clips that share theta add their S and r.  A group on no weighted slot's path has exact zeros in its row, column and entries.
 * The first five outputs are required.  A singular clip gets status 5 and NaN in every output; in a batch with h_status the
 * other clips stand.  No atomics, every sum in a fixed order: the result of one clip is the same bits whatever else shares the
 * call, and a second call repeats the first.
 * Every argument is checked before any device call, with the sensitivity entry's texts (n_groups in 1..16, h_group, the loss
 * L1).  Launches on `stream`: the Fisher assembly and build of the covariance, k_skel_link_fit_rhs ([-G | -g_x] as K + 1 columns,
 * the frames' C_n and c_n), k_skel_factor, one forward and one backward substitution per clip, k_skel_link_fit_reduce; one
 * synchronisation.  Workspace: the pinned covariance workspace, two column buffers [n_clips][17][N][n_active] and the frames'
 * partials [n_clips N][16][17], 256-byte aligned (ACINO_ERR_WORKSPACE otherwise); the query returns 0 outside the limits. */
size_t acino_skel_fte_link_fit_workspace_bytes(const acino_skel_fte_params* p, int n_clips, int pin_unobserved);
int acino_skel_fte_link_fit_system(const acino_skel_fte_params* p, int n_clips, int camera_model, const acino_skel_op* h_ops,
                                   const int32_t* h_active, const double* d_meas, const double* d_w, const double* d_cams,
                                   const double* d_lo, const double* d_hi, const double* d_x,
                                   const int32_t* h_group /* [n_ops] */, int n_groups, double* d_S, double* d_r, double* d_C,
                                   double* d_c, double* d_cost, double* d_sens /* may be NULL */, double* d_newton /* may be NULL */,
                                   int32_t* h_status /* [n_clips], may be NULL */, void* d_ws, size_t ws_bytes, void* stream,
                                   int pin_unobserved, uint8_t* d_unobserved /* [n_clips][n_active], may be NULL */);

/* ---- a generic-skeleton FTE iterate in image space: predicted pixels, their covariance, residuals, gating ----------------
 * Evaluated at the iterate d_x[n_clips][N][n_active] (normally the solution of acino_skel_fte_solve*).  Per entry
 * (b, n, c, l) = (clip, frame, camera, pose slot), the layout of d_meas[n_clips][N][C][n_pose][2] / d_w[n_clips][N][C][n_pose]:
 *   pose = FK_l(x[b][n])        the link program on the active states, every other state 0
 *   (uv, J_pi, z_cam)           the projection of camera c (camera_model 0: fisheye records d_cams[C][24], pt3d_to_2d's
 *                               arithmetic; 1: pinhole records d_cams[C][32], cv2.projectPoints) and its 2 x 3 Jacobian with
 *                               respect to the world point
 *   z, w                        the entries of d_meas and d_w; finite: both components of z finite; sing: |z_cam| < 1e-9;
 *                               wg = (w > 0 ? w : gate_w)
 * Outputs (any may be NULL, but not all of them):
 *   d_uv    [..][2]     the predicted pixel; NaN on the singular plane
 *   d_cov_uv[..][2][2]  J_pi sym(cov_pos[b][n][l]) J_pi^T in px^2, cov_pos = d_cov_pos[n_clips][N][n_pose][3][3] (normally that
 *                       of acino_skel_fte_covariance at the same d_x); both off-diagonal entries carry the same bits; NaN where uv
 *                       is NaN; a NaN cov_pos (a singular clip) propagates.  Asking for it with d_cov_pos == NULL is
 *                       ACINO_ERR_INVALID_ARG
 *   d_res   [..][2]     uv - z for every finite detection WHATEVER its weight; NaN otherwise and where uv is NaN
 *   d_mahal2[..]        res^T (cov_uv + (2 / wg^2) I)^-1 res; with d_cov_pos == NULL: res^T res wg^2 / 2; NaN where res is NaN.
 *                       The stated noise model is Laplace of scale 1 / w per component, variance 2 / w^2: this is a
 *                       MOMENT-MATCHED gating distance under the posterior predictive, NOT an exact chi-square - the noise is
 *                       not Gaussian, so a chi-square quantile with 2 degrees of freedom is a convention for the gate, not a
 *                       coverage statement.  gate_w (> 0, finite) is the scale used for detections the caller gave no positive
 *                       weight (low likelihood): whether they agree with the trajectory all the same can then be asked
 *   d_flags [..]  (u8)  bit 0: the assembly weights this row (w != 0, finite, not singular: the solve's own rule);
 *                       bit 1: z_cam < 1e-6 (behind the camera); bit 2: the singular plane
 * The L1 objective pulls every weighted detection with the same force w however wrong it is - outliers are not discounted - and
 * nothing else in a skeleton solve's results says which detections they are.  No factorisation is involved: the call also serves
 * a skeleton whose covariance is singular (uv / res / flags; NaN cov_uv and mahal2 where the caller's cov_pos is NaN).
 * h_ops / h_active / d_meas / d_w / d_cams as the solve (d_meas RAW: a NaN detection gives a NaN residual); limits as the solve.
 * Every argument is validated before any device call (the params block, the link program and the active states as the solve
 * checks them; n_clips >= 1; camera_model 0 or 1; gate_w; NULL inputs; all outputs NULL).  ONE streaming kernel on `stream`:
 * the problem description travels as a kernel argument, so the call takes no workspace, allocates nothing, copies nothing and
 * does not synchronise; the device arrays must stay valid until the stream reaches it. */
int acino_skel_fte_reprojection(const acino_skel_fte_params* p, int n_clips, int camera_model /* 0 fisheye: d_cams24, 1 pinhole: d_cams32 */,
                                const acino_skel_op* h_ops, const int32_t* h_active, const double* d_meas, const double* d_w,
                                const double* d_cams, const double* d_x,
                                const double* d_cov_pos /* [n_clips][N][n_pose][3][3] or NULL */, double gate_w, double* d_uv,
                                double* d_cov_uv, double* d_res, double* d_mahal2, uint8_t* d_flags, void* stream);
/* The same call with one more output, which may be NULL (and counts as an output):
 *   d_weight[..][2]     the curvature weight of each component of the detection under the params block's loss: with
 *                       ACINO_SKEL_LOSS_REDESCENDING h(w res_d) in [0, 1] for a row the assembly weights (bit 0 of the flags) - 1: the
 *                       detection counts fully, ~0: the solve has rejected it - and 0 otherwise; with ACINO_SKEL_LOSS_L1 1 for a
 *                       weighted row (L1 rejects nothing) and 0 otherwise.
 * Under ACINO_SKEL_LOSS_REDESCENDING BOTH entries use the noise variance 1 / wg^2 in d_mahal2 in place of 2 / wg^2 (the loss is
 * e^2 / 2 in its core: Gaussian noise of scale 1 / w); without d_cov_pos: res^T res wg^2.  Everything else is as above. */
int acino_skel_fte_reprojection_weights(const acino_skel_fte_params* p, int n_clips, int camera_model, const acino_skel_op* h_ops,
                                        const int32_t* h_active, const double* d_meas, const double* d_w, const double* d_cams,
                                        const double* d_x, const double* d_cov_pos, double gate_w, double* d_uv, double* d_cov_uv,
                                        double* d_res, double* d_mahal2, uint8_t* d_flags, double* d_weight, void* stream);

/* ---- per-frame pose fit of a skeleton from 3-D points with a covariance each (csrc/skel_pose_fit.hip) -------------------
 * acino_cheetah_pose_fit for a link program.  Per frame n, from d_points[N][n_pose][3] (metres; slot l is pose slot l of the
 * link program) and d_cov[N][n_pose][3][3], over the P = n_active states x inside the frame's box d_lo[n] <= x <= d_hi[n]:
 *   F(x) = 1/2 sum_{l enters} (FK_l(x) - y_l)^T W_l (FK_l(x) - y_l) + 1/2 sum_{p >= 3} (x_p - m_p)^2 / prior_sigma^2.
 * The entry rule of a slot, W_l, m, the ridge (on the angles only, never on x, y, z), the iteration, its stops and the status
 * codes are those of acino_cheetah_pose_fit; acino_pose_fit_params is reused with min_markers in 1..n_pose.
 * Start: d_x0[N][P], or with d_x0 NULL every angle 0 and x, y, z the mean over the entering slots, in slot order, of
 * y_l - rest_l, rest the poses of the zero state; clipped to the box.
 * Of p ONLY n_pose, n_ops, n_angles and n_active are read (limits as acino_skel_fte_solve; no camera, no frame count, no
 * solver field); h_ops / h_active as the solve.  The dynamic LDS of a frame is sized from (n_active, n_pose, n_ops): 157 KB
 * for the largest shape the limits allow (64 states, 65 slots), 42 KB for the shipped human skeleton; a shape beyond
 * 160 KB would be ACINO_ERR_INVALID_ARG.
 * At the returned x (every floating-point output of a frame is NaN, and d_pinned 0, for status 2 and 3):
 *   d_x[N][P], d_cost[N], d_nmarkers[N] (slots that entered), d_status[N], d_iters[N] (trials made), d_pinned[N][P]
 *   d_cov_x[N][P][P]          A_free^-1 without a Marquardt term, rows and columns of pinned states exactly 0, symmetric
 *                             bit for bit
 *   d_pos[N][n_pose][3]       FK(x)
 *   d_cov_pos[N][n_pose][3][3]  G_l cov_x G_l^T for every slot, with or without a point, symmetric bit for bit;
 *   d_std_pos[N][n_pose]      sqrt((c00 + c11) + c22)
 * Any output but d_x and d_status may be NULL.  d_ws: acino_skel_pose_fit_workspace_bytes(p) bytes, 256-byte aligned (the
 * device copy of the link program; 0: p is outside the limits).  Argument validation happens before any device call;
 * n_frames == 0 is a no-op.  One launch (one 64-lane wave per frame), no synchronisation: d_ws and the device arrays must
 * stay valid until the stream reaches it. */
size_t acino_skel_pose_fit_workspace_bytes(const acino_skel_fte_params* p);
int acino_skel_pose_fit(const acino_pose_fit_params* prm, const acino_skel_fte_params* p, const acino_skel_op* h_ops,
                        const int32_t* h_active, const double* d_points /* [N][n_pose][3] */,
                        const double* d_cov /* [N][n_pose][3][3] or NULL */, const double* d_x0 /* [N][P] or NULL */,
                        const double* d_lo, const double* d_hi /* [N][P] */, int64_t n_frames, double* d_x, double* d_cost,
                        uint8_t* d_nmarkers, uint8_t* d_status, uint8_t* d_iters, uint8_t* d_pinned, double* d_cov_x,
                        double* d_pos, double* d_cov_pos, double* d_std_pos, void* d_ws, size_t ws_bytes, void* stream);

/* ---- per-frame pose of a skeleton from the detections of every camera (csrc/skel_pose_fit_px.hip) ------------------
 * acino_cheetah_pose_fit_px for a link program: per frame the minimiser, over the P = n_active states inside the frame's
 * box d_lo[n] <= x <= d_hi[n], of
 *   F(x) = 1/sigma_px^2 sum_{(c,l) valid} sum_{k in (u,v)} 1/2 f^2 log1p(r_k^2 / f^2) + 1/2 sum_{p >= 3} (x_p - m_p)^2 / prior_sigma^2
 * with r = pi_c(FK_l(x)) - d_det[n][c][l][0..1], FK the link program, pi_c the calibration-level projection of
 * acino_triangulate_multiview, f = f_scale, m the start clipped to the box; a detection (x, y, likelihood) is valid when its
 * likelihood is above thresh and both pixel values are finite.  The controller, the status codes and the outputs are
 * acino_skel_pose_fit's, the parameter block, d_cams (n_cams records of the stated camera model), d_ndet and d_weight
 * acino_cheetah_pose_fit_px's with n_pose slots in place of the 20 markers: min_detections in 1..n_pose n_cams,
 *   d_det[N][C][n_pose][3], d_ndet[N] uint16, d_weight[N][C][n_pose][2] (exactly 0 for an invalid detection, NaN for status
 *   2 and 3).
 * d_x0 [N][P] is required: there is no triangulated point to derive a start from.  ``reserved`` of the block: 0; bit 0 set
 * makes the kernel sum the gradient state by state even where it could take it from the matrix product (same minimiser,
 * other rounding; a measurement switch).  Any output but d_x and d_status may be NULL.  d_ws:
 * acino_skel_pose_fit_px_workspace_bytes(p) bytes, 256-byte aligned (0: p is outside the limits).  A shape whose LDS exceeds
 * 160 KB is refused.  Argument validation happens before any device call; n_frames == 0 is a no-op.  One launch (one 64-lane
 * wave per frame), no synchronisation. */
size_t acino_skel_pose_fit_px_workspace_bytes(const acino_skel_fte_params* p);
int acino_skel_pose_fit_px(const acino_pose_fit_px_params* prm, const acino_skel_fte_params* p, const acino_skel_op* h_ops,
                           const int32_t* h_active, const double* d_det /* [N][C][n_pose][3] */, int64_t n_frames, int n_cams,
                           const double* d_cams, const double* d_x0 /* [N][P] */, const double* d_lo,
                           const double* d_hi /* [N][P] */, double* d_x, double* d_cost, uint16_t* d_ndet, uint8_t* d_status,
                           uint8_t* d_iters, uint8_t* d_pinned, double* d_cov_x, double* d_pos, double* d_cov_pos,
                           double* d_std_pos, double* d_weight, void* d_ws, size_t ws_bytes, void* stream);

/* ---- link lengths of a skeleton from the pose fits of a clip (csrc/skel_link_scale.hip) -------------------------------
 * One log-scale theta_g per group of links, off_k -> exp(theta_g(k)) off_k; h_group[n_ops] names the group of every op
 * (0 .. n_groups-1, or -1 for an op whose offset stays fixed), n_groups = K in 1..16.  h_ops carries the CURRENT, already
 * scaled, offsets: the derivative of a pose with respect to theta_g at that point is the sum of M_k off_k over the ops of
 * group g on its path.  Per frame n with d_status[n] < 2, at the pose d_x[n] (the output of acino_skel_pose_fit on the same
 * d_points / d_cov / prior_sigma / sigma_iso, d_m its ridge centre - read for p >= 3 only -, d_pinned its active set), the
 * joint Gauss-Newton system of (pose, theta) with the pose eliminated on the free states F (lam = 0):
 *   A = Jw^T Jw + kappa, B = Jw^T Js, C = Js^T Js, g = Jw^T u + kappa (x - m), c = Js^T u    (u: the whitened residuals)
 *   d_S[N][K][K]   C - B_F^T A_FF^-1 B_F, symmetric bit for bit      d_r[N][K]   c - B_F^T A_FF^-1 g_F
 *   d_F[N]         the pose fit's objective at d_x[n]                d_used[N]   1 where the frame entered
 *   d_frame_status[N]  d_status[n], or 3 where A_FF has no Cholesky factor
 *   d_sens[N][P][K]    -A_FF^-1 B_F, the pose's sensitivity to the log-scales; rows of pinned states exactly 0
 * A frame with d_status[n] >= 2 or without a factor gets zeros in d_S, d_r and d_F, NaN in d_sens and d_used[n] = 0.  A
 * group that no entering slot of the frame hangs on has exact zeros in its row and column of d_S and in d_r.
 * d_total[K K + K + 2]: S, r, F and the number of used frames summed over the frames in frame order by a second launch, one
 * entry per lane, no atomics: the same bits on every call.  d_sens and d_total may be NULL, as d_cov (sigma_iso is read then).
 * d_ws: acino_skel_link_scale_workspace_bytes(p) bytes, 256-byte aligned (0: p is outside the limits).  Of p the fields that
 * acino_skel_pose_fit reads.  n_groups outside 1..16, a group outside -1..K-1, a NULL required buffer and a shape whose LDS
 * exceeds 160 KB are ACINO_ERR_INVALID_ARG before any device call; n_frames == 0 is a no-op.  No synchronisation. */
size_t acino_skel_link_scale_workspace_bytes(const acino_skel_fte_params* p);
int acino_skel_link_scale(const acino_skel_fte_params* p, const acino_skel_op* h_ops, const int32_t* h_active,
                          const int32_t* h_group /* [n_ops] */, int n_groups, double prior_sigma, double sigma_iso,
                          const double* d_points /* [N][n_pose][3] */, const double* d_cov /* [N][n_pose][3][3] or NULL */,
                          const double* d_x, const double* d_m /* [N][P] */, const uint8_t* d_pinned /* [N][P] */,
                          const uint8_t* d_status /* [N] */, int64_t n_frames, double* d_S, double* d_r, double* d_F,
                          uint8_t* d_used, uint8_t* d_frame_status, double* d_sens, double* d_total, void* d_ws,
                          size_t ws_bytes, void* stream);

/* ---- link lengths of a skeleton from the pixel pose fits of a clip (csrc/skel_link_scale_px.hip) -----------------------
 * acino_skel_link_scale for the objective of acino_skel_pose_fit_px: the groups, h_ops (the CURRENT offsets), the outputs,
 * d_total, the group rules and their messages are acino_skel_link_scale's; the measurement - prm, d_det [N][C][n_pose][3],
 * n_cams, d_cams - is acino_skel_pose_fit_px's.  Per frame n with d_status[n] < 2, at the pose d_x[n] (the output of
 * acino_skel_pose_fit_px on the same d_det / d_cams / prm, d_m its ridge centre - its start clipped to the box, read for
 * p >= 3 only -, d_pinned its active set) and with the IRLS weights w = 1 / (1 + r^2 / f^2) at d_x[n]:
 *   Jc  = sqrt(w) / sigma_px (J_pi R_c) G_l,   Jsc = sqrt(w) / sigma_px (J_pi R_c) d_gl    (d_gl: d pose_l / d theta_g)
 *   A = sum_c Jc^T Jc + kappa, B = sum_c Jc^T Jsc, C = sum_c Jsc^T Jsc, g = sum_c Jc^T u + kappa (x - m), c = sum_c Jsc^T u
 *   d_S = C - B_F^T A_FF^-1 B_F (symmetric bit for bit),  d_r = c - B_F^T A_FF^-1 g_F,  d_sens = -A_FF^-1 B_F
 *   d_F[N]  the pixel pose fit's objective at d_x[n] (the Cauchy cost and the ridge)
 * g and c carry w r, the exact gradient of the Cauchy cost: d_r is the derivative of min_x F_n in theta to first order; d_S
 * is the IRLS Gauss-Newton curvature.  A group that no valid detection of the frame hangs on has exact zeros in its row and
 * column of d_S and in d_r.  Of prm: thresh, f_scale, sigma_px, prior_sigma and camera_model are read; the block is checked
 * as acino_skel_pose_fit_px checks it (max_iter, min_detections, lam0, ftol, xtol must be valid and are not read).
 * d_ws: acino_skel_link_scale_px_workspace_bytes(p) bytes, 256-byte aligned (0: p is outside the limits).  A shape whose LDS
 * exceeds 160 KB is refused, like every other invalid argument, before any device call; n_frames == 0 is a no-op.  Two
 * launches (one 64-lane wave per frame; the sums), no atomics, no synchronisation. */
size_t acino_skel_link_scale_px_workspace_bytes(const acino_skel_fte_params* p);
int acino_skel_link_scale_px(const acino_pose_fit_px_params* prm, const acino_skel_fte_params* p, const acino_skel_op* h_ops,
                             const int32_t* h_active, const int32_t* h_group /* [n_ops] */, int n_groups,
                             const double* d_det /* [N][C][n_pose][3] */, int64_t n_frames, int n_cams, const double* d_cams,
                             const double* d_x, const double* d_m /* [N][P] */, const uint8_t* d_pinned /* [N][P] */,
                             const uint8_t* d_status /* [N] */, double* d_S, double* d_r, double* d_F, uint8_t* d_used,
                             uint8_t* d_frame_status, double* d_sens, double* d_total, void* d_ws, size_t ws_bytes,
                             void* stream);

/* ---- extended Kalman filter + RTS smoother (src/all_optimizations.py:569-865) ---------
 * One call filters and smooths n_seq independent sequences of n_frames frames (same rig).  States are the reference's
 * 75 = 3 x 25 [pose | velocity | acceleration], pose parameters in the order of qb_list (:734-746).  d_det is
 * [n_seq][n_frames][n_cams][20][3] (x, y, likelihood), d_states0 [n_seq][75] the state BEFORE the first prediction
 * (:700-711), d_est / d_smooth [n_seq][n_frames][75] the filtered and the smoothed states (:848-856 slices them into
 * x, dx, ddx), d_outliers [n_seq] the gated pixel pairs (:818).  Model constants (P0, Q, R, the 3-sigma gate, the
 * forward-difference step 1e-3) are the reference's literals.  The predicted covariances are not stored: the smoother
 * rebuilds P_pred[i+1] = F P_est[i] F^T + Q from the filtered one with the filter's own arithmetic.
 *
 * Workspace read-back contract.  After acino_ekf_run / acino_ekf_run_pinhole has returned ACINO_OK, the caller-owned
 * workspace holds, from its first byte and in this order, three arrays of doubles, each rounded up to a multiple of
 * 256 bytes (T = n_seq * n_frames):
 *   P_est  [n_seq][n_frames][75][75]  at 0                     the filtered covariances (:829), exactly symmetric (the lower
 *                                                              triangle of the update, mirrored)
 *   A      [n_seq][n_frames][75][75]  at a256(T*75*75*8)       the smoother gains A_i = P_est[i] F^T inv(P_pred[i+1]) (:840),
 *                                                              each stored TRANSPOSED (element [c][r] is A_i[r][c]) and
 *                                                              written for the frames 1 .. n_frames-2 only: the slots of
 *                                                              frame 0 and frame n_frames-1, and every slot when
 *                                                              n_frames < 3, keep whatever the caller's buffer held
 *   x_pred [n_seq][n_frames][75]      at 2 * a256(T*75*75*8)   the predicted states, rounded to float32 (:628)
 * with a256(v) = (v + 255) / 256 * 256.  Everything behind x_pred, from 2 * a256(T*75*75*8) + a256(T*75*8) to
 * acino_ekf_workspace_bytes, is private to the library and may change without notice. */
typedef struct acino_ekf_params {
  int64_t n_frames;
  int32_t n_seq;
  int32_t n_cams;             /* <= 6 */
  double fps;
  double dlc_thresh;          /* likelihood < thresh -> measurement sigma = cam_width (:805-808) */
  double cam_width;           /* camera_resolution[0], the reference's max_pixel_err (:611) */
  int32_t smoother_pivoting;  /* 0: Cholesky of P_pred, Gauss-Jordan with partial pivoting only where a pivot fails;
                                 1: always the pivoting solver (the reference's np.linalg.inv makes no definiteness
                                 assumption, :840) */
  int32_t reserved;
} acino_ekf_params;
size_t acino_sizeof_ekf_params(void);
size_t acino_ekf_workspace_bytes(int64_t n_frames, int n_seq);
int acino_ekf_run(const acino_ekf_params* prm, const double* d_det, const double* d_cams24, const double* d_states0,
                  void* d_ws, size_t ws_bytes, double* d_est, double* d_smooth, int32_t* d_outliers, void* stream);
/* The same filter on the OpenCV pinhole camera: d_cams32[n_cams][32] pinhole records in place of d_cams24; the same
 * parameters, workspace size and smoother.  fp64. */
int acino_ekf_run_pinhole(const acino_ekf_params* prm, const double* d_det, const double* d_cams32, const double* d_states0,
                          void* d_ws, size_t ws_bytes, double* d_est, double* d_smooth, int32_t* d_outliers, void* stream);
/* Covariances of the filter and the smoother: an opt-in second pass, no change to the calls above.  Both functions are
 * stream-ordered (no host synchronisation), keep no state and need no workspace of their own.  fp64.
 *
 * acino_ekf_smoothed_covariance reads P_est and A from the workspace of a run that returned ACINO_OK (same prm, the
 * read-back contract above; d_ws 256-byte aligned, ws_bytes >= acino_ekf_workspace_bytes) and writes
 * d_P_smooth [n_seq][n_frames][75][75], the second half of Rauch-Tung-Striebel:
 *   P_s[i] = P_est[i] + A_i (P_s[i+1] - P_pred[i+1]) A_i^T   for i = n_frames-2 .. 1,
 * P_pred[i+1] = F P_est[i] F^T + Q rebuilt with the filter's own arithmetic.  Every P_s[i] is exactly symmetric.  The
 * frames 0 and n_frames-1 (every frame when n_frames < 3) receive P_est bit for bit: the reference's smoother returns
 * the filtered state there (:836-839), and this is the covariance of the state d_smooth reports.  The 3-sigma gate does
 * not enter any covariance: a gated pair has its residual zeroed, the gain and (I - K H) P keep its rows of H.
 *
 * acino_ekf_marker_covariance maps states d_states [n_seq][n_frames][75] with covariances d_P [n_seq][n_frames][75][75]
 * (d_est with P_est from the workspace, or d_smooth with d_P_smooth) to the markers: with J_l the ANALYTIC Jacobian of
 * the forward kinematics of marker l at the given pose (not the filter's 1e-3 forward difference),
 *   d_cov_pos   [n_seq][n_frames][20][3][3]  J_l P[:25, :25] J_l^T
 *   d_std_pos   [n_seq][n_frames][20]        sqrt(trace of that)
 *   d_std_state [n_seq][n_frames][75]        sqrt(diag P)
 * Any output may be NULL; all three NULL is ACINO_ERR_INVALID_ARG.  Of prm only n_frames and n_seq are read.  The
 * covariances are the filter's belief under the reference's literal constants (R = 25^2 px^2 per coordinate, cam_width^2
 * under the likelihood threshold), not a calibrated detector noise. */
int acino_ekf_smoothed_covariance(const acino_ekf_params* prm, const void* d_ws, size_t ws_bytes, double* d_P_smooth,
                                  void* stream);
int acino_ekf_marker_covariance(const acino_ekf_params* prm, const double* d_states, const double* d_P, double* d_cov_pos,
                                double* d_std_pos, double* d_std_state, void* stream);

/* The same sharded iteration as FOUR fused phases with the three collectives between them; each phase is a fixed
 * launch sequence on caller-owned buffers and is captured into a hipGraph (acino_fte_enable_graph) per buffer set:
 *   reduce  : zero d_sep, local reduction, export separators            -> all_reduce(d_sep)
 *   solve   : separator solve, local back-substitution, trial iterate,
 *             export its 3+3 edge frames to d_edge_out[6][25]           -> all_gather -> d_all_edges[world][6][25]
 *   eval    : halo from the neighbours' rows of d_all_edges, residuals + Jacobians + assembly of iterate `which`,
 *             local sums to d_partial_out[8]                            -> all_gather -> d_all_partials[world][8]
 *   control : sums combined in rank order, accept/reject + lambda update (init=1: record the loaded iterate). */
/* Bit mask of instantiated graphs: bits 0..3 = the four sharded phases, bit 4 = the whole single-shard step. */
int acino_fte_graphs_active(acino_fte_ctx* ctx);
int acino_fte_shard_reduce(acino_fte_ctx* ctx, double* d_sep, int rank, int world, void* stream);
int acino_fte_shard_solve(acino_fte_ctx* ctx, const double* d_sep, double* d_sep_x, void* d_scratch, size_t scratch_bytes,
                          double* d_edge_out, int rank, int world, void* stream);
int acino_fte_shard_eval(acino_fte_ctx* ctx, int which, const double* d_all_edges, int rank, int world,
                         double* d_partial_out, void* stream);
int acino_fte_shard_control(acino_fte_ctx* ctx, const double* d_all_partials, int world, int init, void* stream);

/* Self-test of the fp64 MFMA tile layout used by the block solver: d_a[16][K], d_b[K][16] -> d_c[16][16]. */
/* Debug aid: n_blocks workgroups that fill 64 KB of LDS each with NaN (to be run on a second stream beside a solve:
 * any kernel that reads LDS it has not written itself then produces NaN). */
int acino_debug_poison_lds(int n_blocks, int spin, void* stream);
int acino_selftest_mfma(const double* d_a, const double* d_b, int k, double* d_c, void* stream);
/* Host only (tests): the table by which the fused narrow levels of the separator reduction (csrc/seplevel.hip) split an
 * eliminated node's work over T workgroups, 1 <= T <= 16.  out[T][64] ints per workgroup: bit mask of the strips of
 * [W_l | W_r] it computes (bit s < 5: columns 16 s .. of W_l, bit 5 + s: of W_r), bit mask of the strips it stores, number
 * of product tiles, then the tile codes (0 .. 24 P_l(a, b) = 5 a + b with a >= b; 25 .. 49 P_r; 50 .. 74 X(a, b)). */
int acino_debug_level_split(int T, int32_t* out);
/* Host only (tests): the right coupling table of chain node `node` (csrc/bcr_dev.hpp) for a window of n_frames frames at
 * n_offset of a sequence of n_global frames (clip_len > 0: clips of that many frames; pin_left: node 0 is a separator).
 * *interior: the value of the test by which the chunk sweep and its back-substitution take the constant table
 * 2 q {-1, 6, -15} in place of evaluating the band; coef[3 ii + jj]: the unscaled entry (frame jj of the node with frame ii of
 * node + 1) as the evaluation gives it, 0 for ii > jj and for a frame slot beyond the window.  The LEFT table of a node is
 * the right table of node - 1 (node = pin_left - 1 is valid). */
int acino_debug_coupling_table(int64_t n_global, int64_t n_frames, int64_t n_offset, int64_t clip_len, int pin_left, int node,
                               int32_t* interior, double* coef);

#ifdef __cplusplus
}
#endif
#endif /* ACINOSET_HIP_H */
