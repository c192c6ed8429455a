// The host layer of the generic-skeleton entries (skel_fte.hip, skel_cov.hip, skel_sample.hip, skel_calib.hip, skel_links.hip,
// skel_reproj.hip): the argument checks, the workspace layout builder, the one writer of a SkelDev, the PT and camera-model
// dispatch and the status read-back.
// No device code.  skel_upload and skel_read_status are defined in skel_cov.hip, beside k_skel_dev_store.  What comes behind the
// checks of the two sensitivity entries (skel_calib.hip, skel_links.hip) is one function, skel_factor.hpp's skel_sens_run.
#pragma once
#include <cstdint>
#include <type_traits>
#include <vector>

#include "skel_dev.hpp"

namespace acino {

// ---- workspace layouts: consecutive regions, each starting on a 256-byte boundary
inline size_t skel_align256(size_t v) { return (v + 255) / 256 * 256; }
struct SkelTake {
  size_t off = 0;                  // (after the last take: the layout's total)
  size_t operator()(size_t bytes) {
    const size_t o = off;
    off = skel_align256(off + bytes);
    return o;
  }
};

// ---- the checks every batched entry makes, in this order.  clip_ceiling: n_clips is a grid dimension of the entry (one
//      workgroup per clip); buffers: the entry's own "all required pointers are non-NULL"
inline int skel_check_batch(const acino_skel_fte_params* p, int n_clips, bool clip_ceiling, int camera_model, bool buffers) {
  const int rc = skel_validate(p);
  if (rc) return rc;
  if (clip_ceiling) ACINO_REQUIRE(n_clips >= 1 && n_clips <= 65535, "n_clips in 1..65535");
  ACINO_REQUIRE(n_clips >= 1, "n_clips >= 1");
  ACINO_REQUIRE(camera_model == 0 || camera_model == 1, "camera_model: 0 fisheye, 1 pinhole");
  ACINO_REQUIRE(buffers, "null buffer");
  ACINO_REQUIRE((size_t)p->n_frames * n_clips < (size_t)1 << 31, "n_clips * n_frames < 2^31");
  return ACINO_OK;
}

// The workspace test, the last check before the first device call.  fail_rc: ACINO_ERR_INVALID_ARG (the solve) or
// ACINO_ERR_WORKSPACE (the entries at an iterate); query: the caller's own ..._workspace_bytes export.
inline int skel_check_workspace(const void* d_ws, size_t ws_bytes, size_t need, const char* query, int fail_rc) {
  const char* lead = fail_rc == ACINO_ERR_INVALID_ARG ? "invalid argument: " : "";
  if (((uintptr_t)d_ws & 255) != 0) {
    set_error("%sworkspace must be 256-byte aligned", lead);
    return fail_rc;
  }
  if (ws_bytes < need) {
    set_error("%sworkspace too small (%s)", lead, query);
    return fail_rc;
  }
  return ACINO_OK;
}

// ---- f(std::integral_constant<int, PT>) with PT = 16, 32, 48 or 64 at compile time (PT: n_active rounded up to 16, <= SK_MAXP).
//      A kernel template's dynamic-LDS attribute is set inside f, once per instantiation and device, where its launch is.
template <class F>
inline int skel_dispatch_pt(int PT, F&& f) {
  switch (PT) {
    case 16: return f(std::integral_constant<int, 16>{});
    case 32: return f(std::integral_constant<int, 32>{});
    case 48: return f(std::integral_constant<int, 48>{});
    default: return f(std::integral_constant<int, 64>{});
  }
}

// ---- the camera model's instantiation of a kernel template (0 fisheye: SkelDev::cams, 1 pinhole: SkelDev::pins); one launch line
template <class K>
inline K skel_camera_kernel(int camera_model, K fisheye, K pinhole) {
  return camera_model == 1 ? pinhole : fisheye;
}

// ---- The only writer of a SkelDev, all on stream s: the host half of h travels by value as the argument of k_skel_dev_store
//      (no host buffer has to outlive the call), the n_cams records of the camera model are copied device-to-device into cams or
//      pins (the other array is left as it is: no kernel reads it; d_cams NULL: neither is written), the clips' words are cleared.
int skel_upload(const SkelDev& h, const double* d_cams, int camera_model, SkelDev* d_dev, SkelClip* d_clip, int n_clips,
                hipStream_t s);

// ---- hc <- the clips' words: one copy, one synchronisation.  A clip that ended with status 5 makes the call fail with
//      ACINO_ERR_NUMERIC and numeric_text when it is the only clip (the failure is the call's) or when the caller has nowhere to
//      report it per clip; in a batch with per-clip output the other clips' results stand.  hc is filled in both cases.
int skel_read_status(const SkelClip* d_clip, int n_clips, hipStream_t s, bool per_clip_output, const char* numeric_text,
                     std::vector<SkelClip>& hc);

}  // namespace acino
