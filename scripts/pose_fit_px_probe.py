"""The per-frame pose fit from the detections (fte.pose_fit_pixels, k_pose_fit_px) beside the chain it competes with
(calib.triangulate_multiview_dense + fte.pose_fit), measured on the GPU in one session.

  timing      synth.make_sequence(10000) (6 cameras x 20 markers) resident on the device, the start x0 = the chain's fit with
              its unfitted frames filled; a host clock around the call ending in a synchronise, median of 5 after a warm-up,
              the variants alternating: acino_cheetah_pose_fit_px with every output and with x and status only, the Python
              entry with x0 given and with x0=None (the chain included), and the chain's two Python entries
  iterations  median, p99, max of ``iters``, the frames at max_iter, the shares of the four statuses, the detections per frame
  accuracy    the 120-frame sprint with and without 5 % of the valid detections pushed 9 to 30 px (tests/triangulate_mv_ref.py's
              push_detections), on 6 cameras and on cameras 0 and 1 alone: the median marker error against pos_true of the 3-D fit
              and of the pixel fit started from it (prior_sigma=1.0, max_iter=255 for both), over the frames both return, and
              the frames each returns

One JSON line per section.  ``--trace``: six calls of the kernel with every output and nothing else after the set-up, for one
rocprofv3 --kernel-trace run (the first call is the warm-up); ``--timing``: the first two sections only."""
import json
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
from acinoset_amd import _lib, calib, fte, synth
from acinoset_amd._lib import PoseFitPxParams, lib, ptr, stream_ptr

THRESH = 0.5
OPTS = dict(prior_sigma=1.0, max_iter=255)


def abi_call(det, cams, x0, full=True, max_iter=100, prior_sigma=np.pi):
    N, Cn, dev = det.shape[0], det.shape[1], det.device
    f64, u8 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.uint8, device=dev)
    out = dict(x=torch.empty((N, 25), **f64), status=torch.empty((N,), **u8))
    if full:
        out.update(cost=torch.empty((N,), **f64), n_detections=torch.empty((N,), dtype=torch.uint16, device=dev),
                   iters=torch.empty((N,), **u8), pinned=torch.empty((N, 25), **u8), cov_x=torch.empty((N, 25, 25), **f64),
                   pos=torch.empty((N, 20, 3), **f64), cov_pos=torch.empty((N, 20, 3, 3), **f64), std_pos=torch.empty((N, 20), **f64),
                   weight=torch.empty((N, Cn, 20, 2), **f64))
    prm = PoseFitPxParams(0, max_iter, 2, 0, 1e-3, 1e-10, 1e-10, prior_sigma, THRESH, 5.0, 5.0)
    g = out.get
    _lib.check(lib().acino_cheetah_pose_fit_px(prm, ptr(det), N, Cn, ptr(cams), ptr(x0), ptr(out["x"]), ptr(g("cost")),
                                               ptr(g("n_detections")), ptr(out["status"]), ptr(g("iters")), ptr(g("pinned")),
                                               ptr(g("cov_x")), ptr(g("pos")), ptr(g("cov_pos")), ptr(g("std_pos")), ptr(g("weight")),
                                               stream_ptr()))
    return out


def alternate(variants, rounds=5):
    """{name: fn} -> {name: [median, min, max] ms} and the last return values: a warm-up round, then the variants in turn."""
    times, last = {k: [] for k in variants}, {}
    for r in range(rounds + 1):
        for name, fn in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last[name] = fn()
            torch.cuda.synchronize()
            if r:
                times[name].append((time.perf_counter() - t0) * 1e3)
    return {k: [round(float(np.median(v)), 3), round(min(v), 3), round(max(v), 3)] for k, v in times.items()}, last


def staged(n_frames):
    """The detections, the rig, its records and the chain's start, on the device."""
    seq = synth.make_sequence(n_frames)
    rig = (seq["K"], seq["D"], seq["R"], seq["t"])
    det = torch.as_tensor(seq["det"], device="cuda")
    cams = torch.as_tensor(calib.camera_records("fisheye", *rig), device="cuda")
    fit = fte.pose_fit(calib.triangulate_multiview_dense(det, THRESH, *rig), return_cov=False)
    x0 = fte.fill_unfitted_frames(fit["x"].cpu().numpy(), fit["status"].cpu().numpy() < 2)
    return det, rig, cams, torch.as_tensor(x0, device="cuda")


def timing(n_frames=10000):
    det, rig, cams, x0 = staged(n_frames)
    tri = calib.triangulate_multiview_dense(det, THRESH, *rig)
    ms, last = alternate({"pixel_fit_all_outputs": lambda: abi_call(det, cams, x0),
                          "pixel_fit_x_and_status": lambda: abi_call(det, cams, x0, full=False),
                          "pixel_fit_python_entry_x0_given": lambda: fte.pose_fit_pixels(det, *rig, x0=x0),
                          "pixel_fit_python_entry_x0_none": lambda: fte.pose_fit_pixels(det, *rig),
                          "triangulate_multiview_python_entry": lambda: calib.triangulate_multiview_dense(det, THRESH, *rig),
                          "pose_fit_3d_python_entry": lambda: fte.pose_fit(tri)})
    out = last["pixel_fit_all_outputs"]
    st, it, nd = (out[k].cpu().numpy() for k in ("status", "iters", "n_detections"))
    print(json.dumps(dict(probe="pose_fit_px_timing", clock="host clock around a synchronised call, ms [median, min, max] of 5",
                          device=torch.cuda.get_device_name(0), n_frames=n_frames, n_cams=int(det.shape[1]), ms=ms)))
    has = nd >= 2
    it3 = last["pose_fit_3d_python_entry"]["iters"].cpu().numpy()
    print(json.dumps(dict(probe="pose_fit_px_iterations", max_iter=100, frames_with_detections=int(has.sum()),
                          median=float(np.median(it[has])), p99=float(np.percentile(it[has], 99)), max=int(it.max()),
                          mean=round(float(it[has].mean()), 2), at_max_iter=int((it[has] >= 100).sum()),
                          status_share={str(s): float((st == s).mean()) for s in range(4)},
                          detections_median=float(np.median(nd)), trials_3d_fit_median=float(np.median(it3)))))


def accuracy(n_frames=120):
    from triangulate_mv_ref import push_detections
    seq = synth.make_sequence(n_frames, "sprint")
    rig = (seq["K"], seq["D"], seq["R"], seq["t"])
    rows = {}
    for pushed in (False, True):
        det = push_detections(seq["det"], THRESH)[0] if pushed else seq["det"]
        for cams in (list(range(det.shape[1])), [0, 1]):
            sub = tuple(np.asarray(a)[cams] for a in rig)
            d = np.ascontiguousarray(det[:, cams])
            tri = calib.triangulate_multiview_dense(d, THRESH, *sub)
            fit3 = fte.pose_fit(tri, return_cov=False, **OPTS)
            x0 = fte.fill_unfitted_frames(fit3["x"], fit3["status"] < 2)
            px = fte.pose_fit_pixels(d, *sub, thresh=THRESH, x0=x0, return_cov=False, **OPTS)
            both = (fit3["status"] < 2) & (px["status"] < 2)
            err = lambda pos: np.linalg.norm(pos[both] - seq["pos_true"][both], axis=-1)
            e3, ep = err(fit3["positions"]), err(px["positions"])
            rows[f"{len(cams)} cameras, {'5 % pushed' if pushed else 'clean'}"] = dict(
                frames_3d_fit=int((fit3["status"] < 2).sum()), frames_pixel_fit=int((px["status"] < 2).sum()),
                median_mm_3d_fit=round(1e3 * float(np.median(e3)), 2), median_mm_pixel_fit=round(1e3 * float(np.median(ep)), 2),
                p90_mm_3d_fit=round(1e3 * float(np.percentile(e3, 90)), 2), p90_mm_pixel_fit=round(1e3 * float(np.percentile(ep, 90)), 2),
                markers_with_a_point_median=float(np.median(fit3["n_markers"])), detections_median=float(np.median(px["n_detections"])),
                pixel_fit_status_0=int((px["status"] == 0).sum()), pixel_fit_trials_max=int(px["iters"].max()))
    print(json.dumps(dict(probe="pose_fit_px_accuracy", clip=f"{n_frames}-frame sprint", options=OPTS,
                          error="marker error against pos_true over the frames both fits return", rows=rows)))


def trace(n_frames=10000):
    det, _rig, cams, x0 = staged(n_frames)
    for _ in range(6):
        abi_call(det, cams, x0)
        torch.cuda.synchronize()


if __name__ == "__main__":
    _lib.require_gpu()
    if "--trace" in sys.argv:
        trace()
    elif "--timing" in sys.argv:
        timing()
    else:
        timing()
        accuracy()
