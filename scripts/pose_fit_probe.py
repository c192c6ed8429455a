"""The per-frame pose fit (fte.pose_fit, k_pose_fit) and the FTE start made from it, measured on the GPU.

  timing      synth.make_sequence(10000) (6 cameras x 20 markers), its multi-view triangulation resident on the device, a host
              clock around acino_cheetah_pose_fit ending in a synchronise, median of 5 after a warm-up: with every output, with
              x and status only, and the Python entry; the multi-view triangulation that feeds it beside them
  iterations  median, p99, max and the histogram of ``iters``, the shares of the four statuses
  start       per clip (the 120-frame sprint, the 10 000-frame loop) and per ``init`` choice: the median marker error of the start
              against pos_true, the time the start takes, and fte_solve's iterations, cost, status and time to solution with the
              start's cost included - a host clock around fte_solve(..., reuse_context=True), the contexts warmed up by a first
              round, the three variants alternating, median of 5 rounds

One JSON line per section.  ``--trace``: six calls of the kernel with every output and nothing else after the set-up, for one
rocprofv3 --kernel-trace run (the first call is the warm-up); ``--timing``: the first two sections only."""
import json
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from acinoset_amd import _lib, calib, fte, synth
from acinoset_amd._lib import PoseFitParams, lib, ptr, stream_ptr

THRESH = 0.5
INITS = ("nose_line", "triangulation", "pose_fit")


def abi_call(points, cov, full=True):
    N, dev = points.shape[0], points.device
    f64, u8 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.uint8, device=dev)
    out = dict(x=torch.empty((N, 25), **f64), status=torch.empty((N,), **u8))
    if full:
        out.update(cost=torch.empty((N,), **f64), n_markers=torch.empty((N,), **u8), iters=torch.empty((N,), **u8),
                   pinned=torch.empty((N, 25), **u8), cov_x=torch.empty((N, 25, 25), **f64), pos=torch.empty((N, 20, 3), **f64),
                   cov_pos=torch.empty((N, 20, 3, 3), **f64), std_pos=torch.empty((N, 20), **f64))
    prm = PoseFitParams(100, 1, 1e-3, 1e-10, 1e-10, np.pi, 0.01)
    g = out.get
    _lib.check(lib().acino_cheetah_pose_fit(prm, ptr(points), ptr(cov), ptr(None), N, ptr(out["x"]), ptr(g("cost")), ptr(g("n_markers")),
                                            ptr(out["status"]), ptr(g("iters")), ptr(g("pinned")), ptr(g("cov_x")), ptr(g("pos")),
                                            ptr(g("cov_pos")), ptr(g("std_pos")), stream_ptr()))
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


def triangulated(n_frames):
    seq = synth.make_sequence(n_frames)
    rig = (seq["K"], seq["D"], seq["R"], seq["t"])
    det = torch.as_tensor(seq["det"], device="cuda")
    tri = calib.triangulate_multiview_dense(det, THRESH, *rig)
    return det, rig, tri["points"].contiguous(), tri["cov"].contiguous()


def timing(n_frames=10000):
    det, rig, pts, cov = triangulated(n_frames)
    ms, last = alternate({"pose_fit_all_outputs": lambda: abi_call(pts, cov),
                          "pose_fit_x_and_status": lambda: abi_call(pts, cov, full=False),
                          "pose_fit_python_entry": lambda: fte.pose_fit(pts, cov),
                          "triangulate_multiview_python_entry": lambda: calib.triangulate_multiview_dense(det, THRESH, *rig)})
    out = last["pose_fit_all_outputs"]
    st, it, nm = (out[k].cpu().numpy() for k in ("status", "iters", "n_markers"))
    print(json.dumps(dict(probe="pose_fit_timing", clock="host clock around a synchronised call, ms [median, min, max] of 5",
                          device=torch.cuda.get_device_name(0), n_frames=n_frames, ms=ms)))
    has = nm >= 1
    print(json.dumps(dict(probe="pose_fit_iterations", frames_with_a_marker=int(has.sum()), median=float(np.median(it[has])),
                          p99=float(np.percentile(it[has], 99)), max=int(it.max()), mean=round(float(it[has].mean()), 2),
                          status_share={str(s): float((st == s).mean()) for s in range(4)},
                          markers_entering_median=float(np.median(nm)), histogram=np.bincount(it[has], minlength=101).tolist())))


def start(n_frames, kind, max_iter=100):
    seq = synth.make_sequence(n_frames, kind)
    rig = (seq["K"], seq["D"], seq["R"], seq["t"])
    meas, lik = torch.as_tensor(seq["det"][..., :2], device="cuda"), torch.as_tensor(seq["det"][..., 2], device="cuda")
    det = torch.as_tensor(seq["det"], device="cuda")
    err = lambda pos: round(1e3 * float(np.median(np.linalg.norm(pos - seq["pos_true"], axis=-1))), 2)
    makers = {"nose_line": lambda: fte.nose_line_init(det, *rig, THRESH), "triangulation": lambda: fte.triangulation_init(det, *rig, THRESH),
              "pose_fit": lambda: fte.pose_fit_init(det, *rig, THRESH)}
    start_ms, x0 = alternate(makers)
    solve_ms, res = alternate({init: (lambda init=init: fte.fte_solve(meas, lik, *rig, seq["Ts"], init=init, max_iter=max_iter,
                                                                      reuse_context=True)) for init in INITS})
    rows = {}
    for init in INITS:
        out, info = res[init]
        rows[init] = dict(start_error_mm=err(fte.cheetah_fk(x0[init])), start_ms=start_ms[init], iterations=int(info["iter"]),
                          accepted=int(info["accepted"]), cost=float(info["cost"]), status=info["status_name"],
                          solve_with_start_ms=solve_ms[init], end_error_mm=err(out["positions"]))
    fte.clear_context_cache()
    print(json.dumps(dict(probe="pose_fit_start", clip=f"{n_frames}-frame {kind}", max_iter=max_iter,
                          clock="host clock around fte_solve(reuse_context=True), start included, ms [median, min, max] of 5", rows=rows)))


def trace(n_frames=10000):
    _det, _rig, pts, cov = triangulated(n_frames)
    for _ in range(6):
        abi_call(pts, cov)
        torch.cuda.synchronize()


if __name__ == "__main__":
    _lib.require_gpu()
    if "--trace" in sys.argv:
        trace()
    elif "--timing" in sys.argv:
        timing()
    else:
        timing()
        start(120, "sprint")
        start(10000, "loop")
