"""The per-frame skeleton pose fit (build.pose_fit, k_skel_pose_fit) and the solve start made from it, measured on the GPU on
the shipped video (6 240 frames, the shipped human skeleton, by-name pairing).

  --timing    the whole video as ONE model, its multi-view triangulation resident on the device: a host clock around
              acino_skel_pose_fit ending in a synchronise, median of 5 after a warm-up - with every output, with x and status
              only - and the Python entry; the triangulation that feeds it beside them.  Trials per frame (median, p99, frames at
              max_iter, the shares of the statuses) at the defaults, at prior_sigma = 1.0, and at prior_sigma = 1.0 with
              max_iter = 255.
  --trace     six calls of the kernel with every output and nothing else after the set-up, for one rocprofv3 --kernel-trace run
              (the first call is the warm-up).
  --start     build.solve_video from init="line" and from init="pose_fit" under the L1 and under the redescending loss, the
              four runs in one process from one binary after a warm-up: iterations, windows at max_iter, windows above 15 px,
              the final cost per window and the wall time with the start's cost included.

Without an option the three run one after the other, each as a child process under a time limit of its own (--trace under
rocprofv3 when it is installed, its files under $ACINO_PROBE_OUT, default build/); the first that fails, faults or runs out of time ends the run.  One JSON line per section."""
import json
import os
import shutil
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEPS = (("--timing", 300), ("--trace", 300), ("--start", 1100))      # seconds
MAX_ITER = 1500


def shipped():
    g = np.load(os.path.join(ROOT, "tests", "golden", "skel_fte_model.npz"))
    sk = json.loads(str(g["skeleton_json"]))
    full = np.load(os.path.join(ROOT, "tests", "golden", "human_dlc_full.npz"))
    tabs = [(list(full["parts"]), full[f"det{c}"].astype(np.float64)) for c in range(2)]
    return sk, (g["K"], g["D"], g["R"], g["t"]), tabs


def whole_video_model():
    from acinoset_amd import build
    sk, scene, tabs = shipped()
    n = min(len(t[1]) for t in tabs)
    return build.build_model(sk, scene=scene, dlc_tables=tabs, n_frames=n, start_frame=0, pairing="name", initial_line=False)[0]


def abi_call(model, tri, keep, full=True, **prm_kw):
    """acino_skel_pose_fit on device arrays (``keep``: the box, the link program and the workspace, made once)."""
    import torch
    from acinoset_amd import _lib
    from acinoset_amd._lib import lib, ptr, stream_ptr
    import ctypes as C
    N, Pa, Lp = model.N, len(model.active), len(model.names)
    dev = tri["points"].device
    f64, u8 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.uint8, device=dev)
    out = dict(x=torch.empty((N, Pa), **f64), status=torch.empty((N,), **u8), iters=torch.empty((N,), **u8))
    if full:
        out.update(cost=torch.empty((N,), **f64), n_markers=torch.empty((N,), **u8), pinned=torch.empty((N, Pa), **u8),
                   cov_x=torch.empty((N, Pa, Pa), **f64), pos=torch.empty((N, Lp, 3), **f64), cov_pos=torch.empty((N, Lp, 3, 3), **f64),
                   std_pos=torch.empty((N, Lp), **f64))
    o = dict(max_iter=100, min_markers=1, lam0=1e-3, ftol=1e-10, xtol=1e-10, prior_sigma=np.pi, sigma_iso=0.01)
    o.update(prm_kw)
    prm = _lib.PoseFitParams(o["max_iter"], o["min_markers"], o["lam0"], o["ftol"], o["xtol"], o["prior_sigma"], o["sigma_iso"])
    g = out.get
    _lib.check(lib().acino_skel_pose_fit(prm, C.byref(keep["p"]), keep["ops"], keep["act"], ptr(tri["points"]), ptr(tri["cov"]), ptr(None),
                                         ptr(keep["lo"]), ptr(keep["hi"]), N, ptr(out["x"]), ptr(g("cost")), ptr(g("n_markers")),
                                         ptr(out["status"]), ptr(out["iters"]), ptr(g("pinned")), ptr(g("cov_x")), ptr(g("pos")),
                                         ptr(g("cov_pos")), ptr(g("std_pos")), C.c_void_p((keep["ws"].data_ptr() + 255) // 256 * 256),
                                         keep["nbytes"], stream_ptr()))
    return out


def device_problem(model, dev):
    import ctypes as C
    import torch
    from acinoset_amd import build, calib
    from acinoset_amd._lib import lib
    act = np.asarray(model.active, dtype=np.int32)
    p = build._skel_params(model, len(act))
    nbytes = lib().acino_skel_pose_fit_workspace_bytes(C.byref(p))
    return dict(p=p, ops=build._ops_array(model.prog), act=(C.c_int32 * len(act))(*[int(a) for a in act]), nbytes=nbytes,
                lo=calib._to_dev(model.lo[:, act], dev), hi=calib._to_dev(model.hi[:, act], dev),
                ws=torch.empty(nbytes + 256, dtype=torch.uint8, device=dev))


def alternate(variants, rounds=5):
    """{name: fn} -> {name: [median, min, max] ms} and the last return values: a warm-up round, then the variants in turn."""
    import torch
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


def trials(out):
    it, st = out["iters"].cpu().numpy(), out["status"].cpu().numpy()
    has = st != 2
    return dict(frames_with_a_point=int(has.sum()), median=float(np.median(it[has])), p99=float(np.percentile(it[has], 99)),
                max=int(it.max()), status={str(s): int((st == s).sum()) for s in range(4)})


def timing():
    import torch
    from acinoset_amd import build
    model = whole_video_model()
    tri = build.model_triangulation(model)
    keep = device_problem(model, tri["points"].device)
    ms, last = alternate({"pose_fit_all_outputs": lambda: abi_call(model, tri, keep),
                          "pose_fit_x_and_status": lambda: abi_call(model, tri, keep, full=False),
                          "pose_fit_python_entry": lambda: build.pose_fit(model, tri),
                          "triangulate_multiview": lambda: build.model_triangulation(model)})
    print(json.dumps(dict(probe="skel_pose_fit_timing", frames=model.N, n_active=len(model.active), n_pose=len(model.names),
                          clock="host clock around a synchronised call, ms [median, min, max] of 5", ms=ms)), flush=True)
    out = {"defaults (prior_sigma pi, max_iter 100)": last["pose_fit_all_outputs"],
           "prior_sigma 1.0, max_iter 100": abi_call(model, tri, keep, prior_sigma=1.0),
           "prior_sigma 1.0, max_iter 255": abi_call(model, tri, keep, prior_sigma=1.0, max_iter=255)}
    torch.cuda.synchronize()
    print(json.dumps(dict(probe="skel_pose_fit_trials", trials={k: dict(trials(v), at_max_iter=int((v["iters"] == m).sum().item()))
                                                                 for (k, v), m in zip(out.items(), (100, 100, 255))})), flush=True)


def trace():
    import torch
    from acinoset_amd import build
    model = whole_video_model()
    tri = build.model_triangulation(model)
    keep = device_problem(model, tri["points"].device)
    torch.cuda.synchronize()
    for _ in range(6):
        abi_call(model, tri, keep)
        torch.cuda.synchronize()


def start():
    import torch
    from acinoset_amd import build
    sk, scene, tabs = shipped()
    n = min(len(t[1]) for t in tabs)
    video = dict(scene=scene, dlc_tables=tabs, first_frame=0, last_frame=n - 1, window=100, overlap=20, pairing="name", max_iter=MAX_ITER)
    build.solve_video(sk, **dict(video, max_iter=2, init="pose_fit"))                 # warm-up: library, kernels, allocator
    for loss in ("l1", "redescending"):
        row = {}
        for init in ("line", "pose_fit"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res, infos, starts = build.solve_video(sk, loss=loss, init=init, **video)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            stage = lambda i: [i] + ([i["l1"]] if "l1" in i else [])                   # noqa: E731  (the robust stage and its L1 stage)
            px = np.array([i["mean_abs_residual_px"] for i in infos])
            cost = np.array([i["cost_final"] for i in infos])
            row[init] = dict(wall_s=round(wall, 2), iterations=int(sum(s["iterations"] for i in infos for s in stage(i))),
                             iterations_last_stage=int(sum(i["iterations"] for i in infos)),
                             windows_at_max_iter=int(sum(i["status_name"] == "max_iter" for i in infos)),
                             windows_above_15px=int((px > 15.0).sum()), cost_per_window_median=float(np.median(cost)),
                             cost_sum=float(cost.sum()), warm_started=int(sum(i["warm_started_from"] is not None for i in infos)),
                             windows_started_from_pose_fit=int(sum(i.get("init") == "pose_fit" for i in infos)))
        print(json.dumps(dict(probe="skel_pose_fit_start", loss=loss, windows=len(starts), max_iter=MAX_ITER, runs=row,
                              note="iterations: of the kept end state's solve(s); retried windows' discarded solves are in wall_s only")),
              flush=True)


def drive():
    os.environ.setdefault("OMP_NUM_THREADS", "16")
    for step, limit in STEPS:
        cmd = [sys.executable, os.path.abspath(__file__), step]
        if step == "--trace":
            prof = shutil.which("rocprofv3")
            if prof is None:
                print(json.dumps(dict(probe="skel_pose_fit_trace", skipped="rocprofv3 not found")), flush=True)
                continue
            out_dir = os.path.join(os.environ.get("ACINO_PROBE_OUT", os.path.join(ROOT, "build")), "skel_pose_fit_trace")
            cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out_dir, "--"] + cmd
        rc = subprocess.run(cmd, timeout=limit, cwd=ROOT).returncode      # (TimeoutExpired ends the run as well)
        if rc != 0:
            sys.exit(f"{step} ended with status {rc}: nothing more is started")


if __name__ == "__main__":
    import torch
    torch.set_num_threads(min(16, torch.get_num_threads()))
    {"--timing": timing, "--trace": trace, "--start": start}.get(sys.argv[1] if len(sys.argv) > 1 else "", drive)()
