// The host layer that the two bundle-adjustment entries share (sba.hip: the solve, sba_cov.hip: the covariance at an iterate):
// the workspace carve and the check of an acino_sba_params problem.  No device code.
#pragma once
#include <cstdint>

#include "sba_dev.hpp"

namespace acino {

// ---- workspace layouts: consecutive regions, each starting on a 256-byte boundary.  An entry's layout function is the ONLY list
//      of its buffers: its ..._workspace_bytes export returns the layout's total and the entry carves at the layout's offsets.
inline size_t sba_align256(size_t v) { return (v + 255) / 256 * 256; }
struct SbaTake {
  size_t off = 0;                  // (after the last take: the bytes in use)
  size_t operator()(size_t bytes) {
    const size_t o = off;
    off += sba_align256(bytes);
    return o;
  }
};

// ---- the checks both entries make before the first device call, in this order.  buffers: the entry's own "every required
//      pointer is non-NULL"; need: the entry's ..._workspace_bytes export.  A workspace that is short or not aligned is answered
//      with the entry's own code and lead: ACINO_ERR_INVALID_ARG (the solve) or ACINO_ERR_WORKSPACE (the covariance).
inline int sba_check_problem(const acino_sba_params* prm, const void* info, bool buffers, const void* d_ws, size_t ws_bytes,
                             size_t (*need)(int, int64_t, int64_t), int ws_rc, const char* ws_lead) {
  ACINO_REQUIRE(prm && info, "params/info");
  ACINO_REQUIRE(prm->n_cams >= 1 && prm->n_cams <= SBA_MAXC, "n_cams in 1..16");
  ACINO_REQUIRE(prm->n_points >= 1 && prm->n_obs >= 1, "sizes (a rank without points cannot take part)");
  ACINO_REQUIRE(prm->n_points < (int64_t)1 << 31 && prm->n_obs < (int64_t)1 << 31, "sizes: n_points and n_obs below 2^31");
  ACINO_REQUIRE(prm->f_scale > 0, "f_scale");
  ACINO_REQUIRE(prm->camera_model == 0 || prm->camera_model == 1, "camera_model: 0 fisheye, 1 pinhole");
  ACINO_REQUIRE(buffers, "null buffer");
  if (((uintptr_t)d_ws & 255) != 0 || ws_bytes < need(prm->n_cams, prm->n_points, prm->n_obs)) {
    set_error("%sworkspace too small or not 256-byte aligned", ws_lead);
    return ws_rc;
  }
  return ACINO_OK;
}

}  // namespace acino
