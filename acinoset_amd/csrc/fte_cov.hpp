// Posterior (Laplace) covariance of an FTE trajectory: launcher of the kernels in fte_cov.hip.
#pragma once
#include "fte_kernels.hpp"

namespace acino {

// Node grid of the covariance pass: every clip (clip_len > 0; otherwise the whole sequence is one clip) is cut into nodes
// of 3 frames of its own, a ragged last node padded with identity rows.
struct CovGrid {
  int n_clips, nodes_per_clip;
  int64_t clip;                                            // frames per clip
  int64_t n_nodes() const { return (int64_t)n_clips * nodes_per_clip; }
};
CovGrid cov_grid(int64_t n_frames, int64_t clip_len);

// one correction term of one sweep: the 15 lower 16 x 16 tiles of an 80 x 80 block, packed (bcr_dev.hpp: lower_item)
constexpr size_t COV_TERM_DOUBLES = 2 * 1920;
constexpr size_t COV_HEAD_BYTES = 256;                     // the error word
size_t cov_workspace_bytes(int64_t n_frames, int64_t clip_len);

// What every posterior launcher reads (fte_api.hip: post_in builds it from the context): the constants on the device and
// their host copy, the state word (st->cur selects the buffers on the device), the detections, the two x / H / g buffers.
struct PostIn {
  const FteConst* d_c;
  const FteConst* h_c;
  const acino_fte_state* d_st;
  const double* d_det;
  double* const* x;
  double* const* H;
  double* const* g;
};

// Sweeps + combine on stream s at the CURRENT iterate: cov_x [N][25][25], cov_pos [N][20][3][3], std_pos [N][20], and the
// covariances of dx / ddx [N][25][25] and of the marker velocities [N][20][3][3], [N][20] (k_fte_cov_rates: one more workgroup
// per node after the SAME sweeps).  ts: the frame period the rates are taken with.  d_ws: cov_workspace_bytes, 256-byte
// aligned; its first int is the error word (non-zero afterwards: a non-positive pivot).  Any output may be null.
int launch_fte_cov_rates(const PostIn& in, void* d_ws, double* d_cov_x, double* d_cov_pos, double* d_std_pos, double* d_cov_dx,
                         double* d_cov_ddx, double* d_cov_vel, double* d_std_vel, double ts, hipStream_t s);

// Joint samples of the trajectory: d_x_samples[S][N][25] = x_hat + L^-T z for d_z[S][N][25], A = L L^T the matrix the
// covariances invert (frame-major order; z of pinned variables counts as 0).  Forward sweep alone, the factors of all nodes
// in parallel, one backward substitution per clip and panel of 64 samples.  Workspace and error word as launch_fte_cov_rates.
int launch_fte_sample(const PostIn& in, void* d_ws, int64_t n_samples, const double* d_z, double* d_x_samples, hipStream_t s);

// A^-1 B for n_cols right-hand sides: d_b[n_cols][N][25] holds B on entry (column-major: one trajectory-shaped vector per
// column; entries of pinned variables count as 0) and A^-1 B on return (exactly 0 for pinned variables), d_y[n_cols][N][25]
// is scratch (L^-1 B).  The sampler's forward sweep and factors, one forward substitution (k_fte_sample_fwdsub) and the
// sampler's backward substitution per clip and panel of 64 columns.  Workspace and error word as launch_fte_cov_rates.
int launch_fte_solve_columns(const PostIn& in, void* d_ws, int64_t n_cols, double* d_b, double* d_y, hipStream_t s);

}  // namespace acino
