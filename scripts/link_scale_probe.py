"""The link-scale fit (build.fit_link_scales, k_skel_link_scale) measured on the GPU on the shipped video (6 240 frames, two
cameras, the shipped human skeleton, by-name pairing, the whole video as ONE model, its multi-view triangulation as points).

  --fit       build.fit_link_scales with one scale per link: the scales with their bars, which groups the clip observes, the
              frames used, the outer steps with cost, step and lam, the wall time.
  --timing    a host clock around acino_skel_link_scale ending in a synchronise, median of 5 after a warm-up - with and without
              the sensitivities - beside acino_skel_pose_fit through build.pose_fit (prior_sigma 1.0, max_iter 255, no
              covariances) on the same frames.
  --trace     six calls of the kernel (with the sensitivities) and of that pose fit for one rocprofv3 --kernel-trace run; the
              driver reads the trace and prints the median of the last five per kernel.

Without an option the three run one after the other, each as a child process under a time limit of its own (--trace under
rocprofv3 when it is installed, its files under $ACINO_PROBE_OUT, default build/); the first that fails, faults or runs out of
time ends the run.  One JSON line per section."""
import csv
import ctypes as C
import glob
import json
import os
import shutil
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
STEPS = (("--fit", 500), ("--timing", 300), ("--trace", 300))      # seconds
FIT = dict(prior_sigma=1.0, max_iter=255)


def setup():
    """The model, its triangulation, the pose fit at the scales 1 and the device arrays of one kernel call."""
    import torch
    from skel_pose_fit_probe import whole_video_model
    from acinoset_amd import build, calib
    from acinoset_amd._lib import lib
    model = whole_video_model()
    tri = build.model_triangulation(model)
    m = build._pose_fit_centre(model, tri["points"], tri["cov"], None, 0.01)
    fit = build.pose_fit(model, tri["points"], tri["cov"], x0=m, return_cov=False, **FIT)
    grp, K = build.link_groups(model.prog, "links")
    act = np.asarray(model.active, dtype=np.int32)
    dev = tri["points"].device
    p = build._skel_params(model, len(act))
    nbytes = lib().acino_skel_link_scale_workspace_bytes(C.byref(p))
    N, Pa = model.N, len(act)
    f64, u8 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.uint8, device=dev)
    keep = dict(p=p, ops=build._ops_array(model.prog), act=(C.c_int32 * Pa)(*[int(a) for a in act]), grp=(C.c_int32 * len(grp))(*[int(g) for g in grp]),
                K=K, nbytes=nbytes, ws=torch.empty(nbytes + 256, dtype=torch.uint8, device=dev), m=calib._to_dev(m, dev),
                S=torch.empty((N, K, K), **f64), r=torch.empty((N, K), **f64), F=torch.empty((N,), **f64), used=torch.empty((N,), **u8),
                fst=torch.empty((N,), **u8), sens=torch.empty((N, Pa, K), **f64), total=torch.empty((K * K + K + 2,), **f64))
    return model, tri, m, fit, keep


def abi_call(model, tri, fit, keep, sens=True):
    from acinoset_amd._lib import check, lib, ptr, stream_ptr
    k = keep
    check(lib().acino_skel_link_scale(C.byref(k["p"]), k["ops"], k["act"], k["grp"], k["K"], FIT["prior_sigma"], 0.01, ptr(tri["points"]),
                                      ptr(tri["cov"]), ptr(fit["x"]), ptr(k["m"]), ptr(fit["pinned"]), ptr(fit["status"]), model.N,
                                      ptr(k["S"]), ptr(k["r"]), ptr(k["F"]), ptr(k["used"]), ptr(k["fst"]), ptr(k["sens"] if sens else None),
                                      ptr(k["total"]), C.c_void_p((k["ws"].data_ptr() + 255) // 256 * 256), k["nbytes"], stream_ptr()))


def fit_scales():
    import torch
    from skel_pose_fit_probe import whole_video_model
    from acinoset_amd import build
    model = whole_video_model()
    tri = build.model_triangulation(model)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = build.fit_link_scales(model, tri["points"], tri["cov"])
    wall = time.perf_counter() - t0
    ops = model.prog["ops"]
    links = [f"{model.names[ops[k][1]]}->{model.names[ops[k][0]]}" for k in np.nonzero(out["groups"] >= 0)[0]]
    r5 = lambda a: [None if not np.isfinite(v) else round(float(v), 5) for v in a]                       # noqa: E731
    print(json.dumps(dict(probe="link_scale_fit", frames=model.N, frames_used=out["system"]["n_used"], groups=links, status=out["status"],
                          scales=r5(out["scales"]), std_scales=r5(out["std_scales"]), observed=[bool(o) for o in out["observed"]],
                          outer_steps=len(out["history"]), history=[{k: (round(float(v), 6) if k != "accepted" else bool(v)) for k, v in h.items()}
                                                                    for h in out["history"]], wall_s=round(wall, 2))), flush=True)


def timing():
    from skel_pose_fit_probe import alternate
    from acinoset_amd import build
    model, tri, m, fit, keep = setup()
    ms, _last = alternate({"link_scale_with_sens": lambda: abi_call(model, tri, fit, keep),
                           "link_scale_without_sens": lambda: abi_call(model, tri, fit, keep, sens=False),
                           "pose_fit_python_entry": lambda: build.pose_fit(model, tri["points"], tri["cov"], x0=m, return_cov=False, **FIT)})
    print(json.dumps(dict(probe="link_scale_timing", frames=model.N, n_active=len(model.active), n_pose=len(model.names), groups=keep["K"],
                          clock="host clock around a synchronised call, ms [median, min, max] of 5", ms=ms)), flush=True)


def trace():
    import torch
    from acinoset_amd import build
    model, tri, m, fit, keep = setup()
    torch.cuda.synchronize()
    for _ in range(6):
        abi_call(model, tri, fit, keep)
        build.pose_fit(model, tri["points"], tri["cov"], x0=m, return_cov=False, **FIT)
        torch.cuda.synchronize()


def read_trace(out_dir):
    """Median of the last five durations per kernel of interest, in ms, from the kernel trace under ``out_dir``."""
    rows = {}
    for path in glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                name = row.get("Kernel_Name", "")
                for key in ("k_skel_link_scale", "k_link_scale_total", "k_skel_pose_fit"):
                    if key in name:
                        rows.setdefault(key, []).append((int(row["Start_Timestamp"]), (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-6))
    return {k: dict(calls=len(v), median_of_last_5_ms=round(float(np.median([d for _s, d in sorted(v)][-5:])), 4)) for k, v in rows.items()}


def drive():
    os.environ.setdefault("OMP_NUM_THREADS", "16")
    for step, limit in STEPS:
        cmd = [sys.executable, os.path.abspath(__file__), step]
        out_dir = os.path.join(os.environ.get("ACINO_PROBE_OUT", os.path.join(ROOT, "build")), "link_scale_trace")
        if step == "--trace":
            prof = shutil.which("rocprofv3")
            if prof is None:
                print(json.dumps(dict(probe="link_scale_trace", skipped="rocprofv3 not found")), flush=True)
                continue
            cmd = [prof, "--kernel-trace", "--output-format", "csv", "-d", out_dir, "--"] + cmd
        rc = subprocess.run(cmd, timeout=limit, cwd=ROOT).returncode      # (TimeoutExpired ends the run as well)
        if rc != 0:
            sys.exit(f"{step} ended with status {rc}: nothing more is started")
        if step == "--trace":
            print(json.dumps(dict(probe="link_scale_trace", clock="rocprofv3 --kernel-trace, kernel durations", kernels=read_trace(out_dir))), flush=True)


if __name__ == "__main__":
    import torch
    torch.set_num_threads(min(16, torch.get_num_threads()))
    {"--fit": fit_scales, "--timing": timing, "--trace": trace}.get(sys.argv[1] if len(sys.argv) > 1 else "", drive)()
