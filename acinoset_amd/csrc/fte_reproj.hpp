// An FTE iterate seen in image space (acino_fte_reprojection): launcher of the kernel in fte_reproj.hip.
#pragma once
#include "fte_cov.hpp"

namespace acino {

// One launch on stream s at the CURRENT iterate (st->cur selects the x buffer on the device: no synchronisation).
// in.d_det[N][C][20][3] the context's detections, d_cov_pos[N][20][3][3] or null; outputs as in acinoset_hip.h, any may be null.
int launch_fte_reproj(const PostIn& in, const double* d_cov_pos, double* d_uv, double* d_cov_uv, double* d_res,
                      double* d_weight, double* d_mahal2, uint8_t* d_flags, hipStream_t s);

}  // namespace acino
