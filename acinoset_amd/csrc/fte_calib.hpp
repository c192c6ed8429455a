// Sensitivity of an FTE trajectory to the camera extrinsics (acino_fte_calibration_sensitivity): launcher of the kernels in
// fte_calib.hip.
#pragma once
#include "fte_cov.hpp"

namespace acino {

// the covariance workspace, then two column buffers [6C][N][25]: the right-hand side / solution and L^-1 of it
size_t calib_workspace_bytes(int64_t n_frames, int64_t clip_len, int n_cams);

// S = -A^-1 G on stream s at the CURRENT iterate (st->cur selects the buffers), then the products with d_cov_cams[6C][6C]
// (may be null: then only d_sens is written).  in.d_det[N][C][20][3] the context's detections.  Outputs as in acinoset_hip.h,
// any may be null.  d_ws: calib_workspace_bytes, 256-byte aligned; its first int is the error word of launch_fte_cov_rates.
int launch_fte_calib(const PostIn& in, void* d_ws, const double* d_cov_cams, double* d_sens, double* d_cov_x_cal,
                     double* d_cov_pos_cal, double* d_std_pos_cal, hipStream_t s);

}  // namespace acino
