"""The robust multi-view triangulation (calib.triangulate_multiview_dense, k_triangulate_multiview) measured on the GPU.

  timing      synth.make_sequence(10000) (6 cameras x 20 markers, 200 000 points), device-resident detections, a host clock
              around a call that ends in a synchronise, the variants alternating, median of 5 rounds after a warm-up round:
              acino_triangulate_multiview with points only / with cov, wssr, iters / with the sensitivities as well, the Python
              entry, triangulate_pairs_dense, and sba.bundle_adjust_points_only on the same observations (host lists, as that
              entry takes them) from the pair-mean start at the same f_scale - with the number of points each returns
  iterations  median, p99, max of ``iters`` and the share of status 1
  accuracy    the 60-frame sprint with 5 % of the valid detections pushed 9 to 30 px (tests/triangulate_mv_ref.py's
              push_detections): median error against pos_true over all markers and over the touched ones, for the pair mean and
              for f_scale 5 and 50
  bars        median std beside the median actual error at sigma_px = 2 (the synthetic noise), and the median std_calib / std on
              the two-camera subset with calib.extrinsic_cov(2, 0.05, 2e-3, fixed=(0,))

One JSON line per section.  ``--trace``: three calls of the kernel and nothing else, for one rocprofv3 --kernel-trace --stats run."""
import ctypes as C
import json
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
from acinoset_amd import _lib, calib, sba, synth
from acinoset_amd._lib import TriMvParams, lib, ptr, stream_ptr

THRESH = 0.5


def abi_call(det, cams, f_scale=5.0, cov=True, sens=False):
    N, Cn, L, _ = det.shape
    dev = det.device
    f64, u8 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.uint8, device=dev)
    out = dict(points=torch.empty((N, L, 3), **f64), n_views=torch.empty((N, L), **u8), status=torch.empty((N, L), **u8))
    if cov:
        out.update(cov=torch.empty((N, L, 3, 3), **f64), wssr=torch.empty((N, L), **f64), iters=torch.empty((N, L), **u8))
    if sens:
        out["sens"] = torch.empty((N, L, 3, 6 * Cn), **f64)
    prm = TriMvParams(0, 60, THRESH, f_scale, 5.0, 1e-10)
    _lib.check(lib().acino_triangulate_multiview(prm, ptr(det), N, Cn, L, ptr(cams), ptr(out["points"]), ptr(out.get("cov")),
                                                 ptr(out.get("wssr")), ptr(out["n_views"]), ptr(out["status"]), ptr(out.get("iters")),
                                                 ptr(out.get("sens")), stream_ptr()))
    return out


def alternate(variants, rounds=5):
    """{name: fn} -> {name: (median, min, max) ms}: one warm-up round, then ``rounds`` rounds with the variants in turn."""
    times = {k: [] for k in variants}
    for r in range(rounds + 1):
        for name, fn in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r:
                times[name].append((time.perf_counter() - t0) * 1e3)
    return {k: [round(float(np.median(v)), 3), round(min(v), 3), round(max(v), 3)] for k, v in times.items()}


def host_lists(det, start):
    """The observation lists of the points with two or more views and a finite start: keep [N, L], p2, pi, ci."""
    seen = det[..., 2].transpose(0, 2, 1) > THRESH
    keep = (seen.sum(-1) >= 2) & np.isfinite(start).all(-1)
    pi, ci = np.nonzero(seen[keep])
    return keep, det.transpose(0, 2, 1, 3)[keep][pi, ci, :2].copy(), pi, ci


def timing(n_frames=10000):
    seq = synth.make_sequence(n_frames)
    rig = (seq["K"], seq["D"], seq["R"], seq["t"])
    dev = torch.device("cuda")
    det = torch.as_tensor(seq["det"], device=dev)
    cams = torch.as_tensor(calib.camera_records("fisheye", *rig), device=dev)
    tri, npairs, _ = calib.triangulate_pairs_dense(seq["det"], THRESH, *rig)
    keep, p2, pi, ci = host_lists(seq["det"], tri)
    ba = {}

    def points_only():
        ba["X"] = sba.bundle_adjust_points_only(p2, tri[keep], pi, ci, *rig, f_scale=5.0)[0]

    ms = alternate({"mv_points_only": lambda: abi_call(det, cams, cov=False),
                    "mv_cov": lambda: abi_call(det, cams),
                    "mv_cov_sens": lambda: abi_call(det, cams, sens=True),
                    "mv_python_entry": lambda: calib.triangulate_multiview_dense(det, THRESH, *rig),
                    "pairs_dense": lambda: calib.triangulate_pairs_dense(det, THRESH, *rig),
                    "sba_points_only_host_lists": points_only})
    out = abi_call(det, cams)
    st, it = out["status"].cpu().numpy(), out["iters"].cpu().numpy()
    two = out["n_views"].cpu().numpy() >= 2
    print(json.dumps(dict(probe="triangulate_mv_timing", clock="host clock around a synchronised call, ms [median, min, max] of 5",
                          device=torch.cuda.get_device_name(0), n_frames=n_frames, n_points=int(st.size), ms=ms,
                          points_returned=dict(multiview=int((st < 2).sum()), pair_mean=int((npairs > 0).sum()),
                                               sba_points_only=int(np.isfinite(ba["X"]).all(-1).sum())),
                          sba_info={k: sba.last_info[k] for k in ("iterations", "status_name") if k in sba.last_info})))
    print(json.dumps(dict(probe="triangulate_mv_iterations", n_points_two_views=int(two.sum()), median=float(np.median(it[two])),
                          p99=float(np.percentile(it[two], 99)), max=int(it.max()), mean=round(float(it[two].mean()), 2),
                          share_status_1=float((st == 1).sum() / two.sum()), share_status_3=float((st == 3).sum() / two.sum()),
                          histogram=np.bincount(it[two], minlength=61).tolist())))


def accuracy(n_frames=60):
    from triangulate_mv_ref import push_detections
    seq = synth.make_sequence(n_frames, "sprint")
    rig = (seq["K"], seq["D"], seq["R"], seq["t"])
    det, touched = push_detections(seq["det"], THRESH)
    err = lambda X: np.linalg.norm(X - seq["pos_true"], axis=-1)
    rows = {"pair_mean": err(calib.triangulate_pairs_dense(det, THRESH, *rig)[0])}
    for f in (5.0, 50.0):
        rows[f"multiview_f{f:g}"] = err(calib.triangulate_multiview_dense(det, THRESH, *rig, f_scale=f)["points"])
    both = np.all([np.isfinite(e) for e in rows.values()], axis=0)
    print(json.dumps(dict(probe="triangulate_mv_accuracy", n_frames=n_frames, markers_compared=int(both.sum()),
                          markers_touched=int((both & touched).sum()),
                          median_error_mm_all={k: round(1e3 * float(np.median(e[both])), 2) for k, e in rows.items()},
                          median_error_mm_touched={k: round(1e3 * float(np.median(e[both & touched])), 2) for k, e in rows.items()},
                          points_returned={k: int(np.isfinite(e).sum()) for k, e in rows.items()})))
    out = calib.triangulate_multiview_dense(seq["det"], THRESH, *rig, sigma_px=2.0)
    ok = out["status"] < 2
    two = tuple(np.asarray(a)[:2] for a in rig)
    sub = calib.triangulate_multiview_dense(seq["det"][:, :2], THRESH, *two, sigma_px=2.0,
                                            cov_cams=calib.extrinsic_cov(2, 0.05, 2e-3, fixed=(0,)))
    oks = sub["status"] < 2
    print(json.dumps(dict(probe="triangulate_mv_bars", sigma_px=2.0, median_std_mm=round(1e3 * float(np.median(out["std"][ok])), 2),
                          median_error_mm=round(1e3 * float(np.median(err(out["points"])[ok])), 2),
                          sigma2_hat=round(out["sigma2_hat"], 3),
                          two_camera_median_std_calib_over_std=round(float(np.median((sub["std_calib"] / sub["std"])[oks])), 3),
                          two_camera_points=int(oks.sum()))))


def trace(n_frames=10000):
    seq = synth.make_sequence(n_frames)
    dev = torch.device("cuda")
    det = torch.as_tensor(seq["det"], device=dev)
    cams = torch.as_tensor(calib.camera_records("fisheye", seq["K"], seq["D"], seq["R"], seq["t"]), device=dev)
    for _ in range(3):
        abi_call(det, cams)
    torch.cuda.synchronize()


if __name__ == "__main__":
    _lib.require_gpu()
    if "--trace" in sys.argv:
        trace()
    else:
        timing()
        accuracy()
