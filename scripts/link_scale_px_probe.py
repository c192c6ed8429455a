"""The link-scale fit from the detections (build.fit_link_scales_pixels, k_skel_link_scale_px) measured on the GPU on the shipped
video (6 240 frames, two cameras, the shipped human skeleton, by-name pairing, the whole video as ONE model), beside the 3-D
form (build.fit_link_scales on the model's multi-view triangulation) in the same session.

  --fit       both fits with one scale per link: scales and bars of both, the groups either observes, frames used, outer steps,
              wall time, and per group the ratio of the pixel bar to the 3-D bar.
  --timing    a host clock around acino_skel_link_scale_px ending in a synchronise, median of 5 after a warm-up - with and
              without the sensitivities - beside acino_skel_pose_fit_px through build.pose_fit_pixels (prior_sigma 1.0, max_iter
              255, no covariances) on the same frames.
  --trace     six calls of the kernel (with the sensitivities) and of that pose fit for one rocprofv3 --kernel-trace run; the
              driver reads the trace and prints the median of the last five per kernel.

Without an option the three run one after the other, each as a child process under a time limit of its own (--trace under
rocprofv3 when it is installed, its files under $ACINO_PROBE_OUT, default build/); the first that fails, faults or runs out of
time ends the run.  One JSON line per section."""
import ctypes as C
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
STEPS = (("--fit", 600), ("--timing", 300), ("--trace", 300))      # seconds
FIT = dict(prior_sigma=1.0, max_iter=255)
KERNELS = ("k_skel_link_scale_px", "k_link_scale_total", "k_skel_pose_fit_px")


def setup():
    """The model, the ridge centre, the pixel pose fit at the scales 1 (device tensors) and the device arrays of one kernel call."""
    import torch
    from skel_pose_fit_probe import whole_video_model
    from acinoset_amd import _lib, build, calib
    from acinoset_amd._lib import lib
    model = whole_video_model()
    dev = calib._dev()
    m = build._pixel_start(model, None)
    det = torch.as_tensor(build._model_detections(model), device=dev)
    sigma_px = build._model_sigma_px(model)
    fit = build.pose_fit_pixels(model, x0=torch.as_tensor(m, device=dev), det=det, sigma_px=sigma_px, return_cov=False, **FIT)
    grp, K = build.link_groups(model.prog, "links")
    act = np.asarray(model.active, dtype=np.int32)
    p = build._skel_params(model, len(act))
    nbytes = lib().acino_skel_link_scale_px_workspace_bytes(C.byref(p))
    N, Pa, Cn = model.N, len(act), det.shape[1]
    camera_model = getattr(model, "camera_model", "fisheye")
    f64, u8 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.uint8, device=dev)
    keep = dict(p=p, ops=build._ops_array(model.prog), act=(C.c_int32 * Pa)(*[int(a) for a in act]), grp=(C.c_int32 * len(grp))(*[int(g) for g in grp]),
                K=K, Cn=Cn, nbytes=nbytes, ws=torch.empty(nbytes + 256, dtype=torch.uint8, device=dev), m=calib._to_dev(m, dev), det=det,
                cams=torch.as_tensor(calib.camera_records(camera_model, model.K, model.D, model.R, model.t), device=dev),
                prm=_lib.PoseFitPxParams(calib.CAMERAS[camera_model].code, 1, 1, 0, 1e-3, 1e-10, 1e-10, FIT["prior_sigma"], 0.5, 5.0, float(sigma_px)),
                S=torch.empty((N, K, K), **f64), r=torch.empty((N, K), **f64), F=torch.empty((N,), **f64), used=torch.empty((N,), **u8),
                fst=torch.empty((N,), **u8), sens=torch.empty((N, Pa, K), **f64), total=torch.empty((K * K + K + 2,), **f64))
    return model, m, sigma_px, fit, keep


def abi_call(model, fit, keep, sens=True):
    from acinoset_amd._lib import check, lib, ptr, stream_ptr
    k = keep
    check(lib().acino_skel_link_scale_px(C.byref(k["prm"]), C.byref(k["p"]), k["ops"], k["act"], k["grp"], k["K"], ptr(k["det"]), model.N,
                                         k["Cn"], ptr(k["cams"]), ptr(fit["x"]), ptr(k["m"]), ptr(fit["pinned"]), ptr(fit["status"]),
                                         ptr(k["S"]), ptr(k["r"]), ptr(k["F"]), ptr(k["used"]), ptr(k["fst"]),
                                         ptr(k["sens"] if sens else None), ptr(k["total"]),
                                         C.c_void_p((k["ws"].data_ptr() + 255) // 256 * 256), k["nbytes"], stream_ptr()))


def fit_scales():
    import torch
    from skel_pose_fit_probe import whole_video_model
    from acinoset_amd import build
    model = whole_video_model()
    tri = build.model_triangulation(model)
    torch.cuda.synchronize()
    out, wall = {}, {}
    for name, fn in (("points", lambda: build.fit_link_scales(model, tri["points"], tri["cov"])),
                     ("pixels", lambda: build.fit_link_scales_pixels(model))):
        t0 = time.perf_counter()
        out[name] = fn()
        wall[name] = round(time.perf_counter() - t0, 2)
    ops = model.prog["ops"]
    links = [f"{model.names[ops[k][1]]}->{model.names[ops[k][0]]}" for k in np.nonzero(out["pixels"]["groups"] >= 0)[0]]
    r5 = lambda a: [None if not np.isfinite(v) else round(float(v), 5) for v in a]                       # noqa: E731
    with np.errstate(all="ignore"):
        ratio = out["pixels"]["std_scales"] / out["points"]["std_scales"]
    side = lambda o: dict(status=o["status"], frames_used=o["system"]["n_used"], scales=r5(o["scales"]), std_scales=r5(o["std_scales"]),      # noqa: E731
                          observed=[bool(v) for v in o["observed"]], outer_steps=len(o["history"]),
                          cost=[round(float(o["history"][i]["cost"]), 3) for i in (0, -1)] if o["history"] else None)
    print(json.dumps(dict(probe="link_scale_px_fit", frames=model.N, groups=links, points=side(out["points"]), pixels=side(out["pixels"]),
                          std_ratio_pixels_over_points=r5(ratio), wall_s=wall)), flush=True)


def timing():
    from skel_pose_fit_probe import alternate
    from acinoset_amd import build
    import torch
    model, m, sigma_px, fit, keep = setup()
    x0 = torch.as_tensor(m, device=keep["det"].device)
    ms, _last = alternate({"link_scale_px_with_sens": lambda: abi_call(model, fit, keep),
                           "link_scale_px_without_sens": lambda: abi_call(model, fit, keep, sens=False),
                           "pose_fit_pixels_python_entry": lambda: build.pose_fit_pixels(model, x0=x0, det=keep["det"], sigma_px=sigma_px,
                                                                                         return_cov=False, **FIT)})
    st = fit["status"].cpu().numpy()
    print(json.dumps(dict(probe="link_scale_px_timing", frames=model.N, frames_with_a_pose=int((st < 2).sum()), n_active=len(model.active),
                          n_pose=len(model.names), n_cams=keep["Cn"], groups=keep["K"],
                          clock="host clock around a synchronised call, ms [median, min, max] of 5", ms=ms)), flush=True)


def trace():
    import torch
    from acinoset_amd import build
    model, m, sigma_px, fit, keep = setup()
    x0 = torch.as_tensor(m, device=keep["det"].device)
    torch.cuda.synchronize()
    for _ in range(6):
        abi_call(model, fit, keep)
        build.pose_fit_pixels(model, x0=x0, det=keep["det"], sigma_px=sigma_px, return_cov=False, **FIT)
        torch.cuda.synchronize()


def read_trace(out_dir):
    """Median of the last five durations per kernel of interest, in ms, from the kernel trace under ``out_dir``."""
    import csv
    import glob
    rows = {}
    for path in glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                name = row.get("Kernel_Name", "")
                key = next((k for k in KERNELS if any(k + end in name for end in "<(IE") or name.endswith(k)), None)
                if key:
                    rows.setdefault(key, []).append((int(row["Start_Timestamp"]), (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-6))
    return {k: dict(calls=len(v), median_of_last_5_ms=round(float(np.median([d for _s, d in sorted(v)][-5:])), 4)) for k, v in rows.items()}


def drive():
    os.environ.setdefault("OMP_NUM_THREADS", "16")
    for step, limit in STEPS:
        cmd = [sys.executable, os.path.abspath(__file__), step]
        out_dir = os.path.join(os.environ.get("ACINO_PROBE_OUT", os.path.join(ROOT, "build")), "link_scale_px_trace")
        if step == "--trace":
            prof = shutil.which("rocprofv3")
            if prof is None:
                print(json.dumps(dict(probe="link_scale_px_trace", skipped="rocprofv3 not found")), flush=True)
                continue
            cmd = [prof, "--kernel-trace", "--output-format", "csv", "-d", out_dir, "--"] + cmd
        rc = subprocess.run(cmd, timeout=limit, cwd=ROOT).returncode      # (TimeoutExpired ends the run as well)
        if rc != 0:
            sys.exit(f"{step} ended with status {rc}: nothing more is started")
        if step == "--trace":
            print(json.dumps(dict(probe="link_scale_px_trace", clock="rocprofv3 --kernel-trace, kernel durations", kernels=read_trace(out_dir))), flush=True)


if __name__ == "__main__":
    import torch
    torch.set_num_threads(min(16, torch.get_num_threads()))
    {"--fit": fit_scales, "--timing": timing, "--trace": trace}.get(sys.argv[1] if len(sys.argv) > 1 else "", drive)()
