"""The per-frame skeleton pose fit from the detections (build.pose_fit_pixels, k_skel_pose_fit_px) beside the fit from 3-D points
(build.pose_fit, k_skel_pose_fit), measured on the GPU in one session.

  --timing     the shipped video (6 240 frames, 2 cameras, the shipped human skeleton, by-name pairing) as ONE model: a host
               clock around the synchronised C call, median of 5 after a warm-up - the pixel fit with g from the Gram product's
               spare row, with g from the per-state loop (bit 0 of ``reserved``), the 3-D fit -, the Python entries (the pixel
               fit with x0 given and with the default chain); how many frames get a pose from either fit; the status and trial
               histogram of the pixel fit at the defaults and at prior_sigma = 1.0, max_iter = 255; detections per frame
               beside slots with a point.
  --trace      six calls of each of the three kernels and nothing else after the set-up, for one rocprofv3 --kernel-trace run
               (the first call of each is the warm-up); the driver reads the trace and prints the median of 5 per kernel.
  --synthetic  the shipped skeleton in front of cameras 0 and 1 of the unlike rig of the tests, 240 frames with a known truth
               (the recipe of tests/skel_pose_fit_px_ref.py: 2 px noise, a fifth of the detections dropped), clean and with
               5 % of the detections pushed by 9..30 px: median and 90th percentile of the slot error [mm] of both fits.

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

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
STEPS = (("--timing", 400), ("--trace", 300), ("--synthetic", 300))      # seconds
FIT = dict(prior_sigma=1.0, max_iter=255)


def px_problem(model, dev):
    """What the C call keeps between calls: the detections, the records, the box, the link program, the workspace."""
    import torch
    from acinoset_amd import build, calib
    from acinoset_amd._lib import lib
    act = np.asarray(model.active, dtype=np.int32)
    p = build._skel_params(model, len(act))
    nbytes = lib().acino_skel_pose_fit_px_workspace_bytes(C.byref(p))
    cam = getattr(model, "camera_model", "fisheye")
    return dict(p=p, ops=build._ops_array(model.prog), act=(C.c_int32 * len(act))(*[int(a) for a in act]), nbytes=nbytes,
                lo=calib._to_dev(model.lo[:, act], dev), hi=calib._to_dev(model.hi[:, act], dev), code=calib.CAMERAS[cam].code,
                det=torch.as_tensor(build._model_detections(model), device=dev),
                cams=torch.as_tensor(calib.camera_records(cam, model.K, model.D, model.R, model.t), device=dev),
                sigma_px=build._model_sigma_px(model), ws=torch.empty(nbytes + 256, dtype=torch.uint8, device=dev))


def px_call(model, keep, x0, loop_g=False, **prm_kw):
    """acino_skel_pose_fit_px on device arrays, every output."""
    import torch
    from acinoset_amd import _lib
    from acinoset_amd._lib import lib, ptr, stream_ptr
    N, Pa, Lp, Cn = model.N, len(model.active), len(model.names), keep["det"].shape[1]
    dev = keep["det"].device
    f64, u8 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.uint8, device=dev)
    out = dict(x=torch.empty((N, Pa), **f64), cost=torch.empty((N,), **f64), n_detections=torch.empty((N,), dtype=torch.uint16, device=dev),
               status=torch.empty((N,), **u8), iters=torch.empty((N,), **u8), pinned=torch.empty((N, Pa), **u8),
               cov_x=torch.empty((N, Pa, Pa), **f64), pos=torch.empty((N, Lp, 3), **f64), cov_pos=torch.empty((N, Lp, 3, 3), **f64),
               std_pos=torch.empty((N, Lp), **f64), weight=torch.empty((N, Cn, Lp, 2), **f64))
    o = dict(max_iter=100, min_detections=2, lam0=1e-3, ftol=1e-10, xtol=1e-10, prior_sigma=np.pi, thresh=0.5, f_scale=5.0)
    o.update(prm_kw)
    prm = _lib.PoseFitPxParams(keep["code"], o["max_iter"], o["min_detections"], 1 if loop_g else 0, o["lam0"], o["ftol"], o["xtol"],
                               o["prior_sigma"], o["thresh"], o["f_scale"], keep["sigma_px"])
    _lib.check(lib().acino_skel_pose_fit_px(prm, C.byref(keep["p"]), keep["ops"], keep["act"], ptr(keep["det"]), N, Cn, ptr(keep["cams"]),
                                            ptr(x0), ptr(keep["lo"]), ptr(keep["hi"]),
                                            *(ptr(out[k]) for k in ("x", "cost", "n_detections", "status", "iters", "pinned", "cov_x",
                                                                    "pos", "cov_pos", "std_pos", "weight")),
                                            C.c_void_p((keep["ws"].data_ptr() + 255) // 256 * 256), keep["nbytes"], stream_ptr()))
    return out


def histogram(out, max_iter):
    it, st = out["iters"].cpu().numpy(), out["status"].cpu().numpy()
    has = st != 2
    return dict(frames_with_a_pose=int((st < 2).sum()), status={str(s): int((st == s).sum()) for s in range(4)},
                trials=dict(median=float(np.median(it[has])), p90=float(np.percentile(it[has], 90)), p99=float(np.percentile(it[has], 99)),
                            max=int(it.max()), at_max_iter=int((it == max_iter).sum())))


def set_up():
    import torch
    import skel_pose_fit_probe as spf
    from acinoset_amd import build, calib
    model = spf.whole_video_model()
    tri = build.model_triangulation(model)
    dev = tri["points"].device
    keep3, keep = spf.device_problem(model, dev), px_problem(model, dev)
    act = np.asarray(model.active)
    x0 = calib._to_dev(build._pose_fit_start(model, {})[:, act], dev)
    torch.cuda.synchronize()
    return spf, model, tri, keep3, keep, x0


def timing():
    import torch
    from acinoset_amd import build
    spf, model, tri, keep3, keep, x0 = set_up()
    ms, last = spf.alternate({"pixel_fit_g_from_the_product": lambda: px_call(model, keep, x0),
                              "pixel_fit_g_by_the_loop": lambda: px_call(model, keep, x0, loop_g=True),
                              "fit_3d_all_outputs": lambda: spf.abi_call(model, tri, keep3),
                              "pixel_fit_python_entry_x0_given": lambda: build.pose_fit_pixels(model, x0),
                              "pixel_fit_python_entry_default_chain": lambda: build.pose_fit_pixels(model),
                              "fit_3d_python_entry": lambda: build.pose_fit(model, tri)})
    print(json.dumps(dict(probe="skel_pose_fit_px_timing", frames=model.N, cameras=int(keep["det"].shape[1]), n_active=len(model.active),
                          n_pose=len(model.names), clock="host clock around a synchronised call, ms [median, min, max] of 5", ms=ms)),
          flush=True)
    a, b = last["pixel_fit_g_from_the_product"], last["pixel_fit_g_by_the_loop"]
    same = {k: bool(torch.equal(a[k], b[k])) for k in ("status", "iters", "pinned")}
    dx = float(torch.nan_to_num(a["x"] - b["x"]).abs().max())
    fit3 = last["fit_3d_all_outputs"]
    runs = {"defaults (prior_sigma pi, max_iter 100)": histogram(a, 100),
            "prior_sigma 1.0, max_iter 255": histogram(px_call(model, keep, x0, **FIT), 255)}
    st3 = fit3["status"].cpu().numpy()
    det = a["n_detections"].cpu().numpy().astype(np.int64)
    slots = fit3["n_markers"].cpu().numpy().astype(np.int64)
    print(json.dumps(dict(probe="skel_pose_fit_px_poses", frames=model.N, frames_with_a_pose_3d=int((st3 < 2).sum()), pixel_fit=runs,
                          frames_without_a_detection=int((det == 0).sum()),
                          detections_per_frame=dict(median=float(np.median(det)), mean=round(float(det.mean()), 2)),
                          slots_with_a_point_per_frame=dict(median=float(np.median(slots)), mean=round(float(slots.mean()), 2)),
                          g_variants=dict(same_integers=same, x_max_abs_difference=dx))), flush=True)


def trace():
    import torch
    spf, model, tri, keep3, keep, x0 = set_up()
    for fn in (lambda: px_call(model, keep, x0), lambda: px_call(model, keep, x0, loop_g=True), lambda: spf.abi_call(model, tri, keep3)):
        for _ in range(6):
            fn()
            torch.cuda.synchronize()


def read_trace(out_dir):
    """Per kernel the durations [ms] of its launches in start order, from rocprofv3's kernel_trace.csv."""
    rows = {}
    for path in glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            for r in csv.DictReader(f):
                rows.setdefault(r["Kernel_Name"], []).append((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6))
    return {k: [d for _, d in sorted(v)] for k, v in rows.items() if "pose_fit" in k}


def synthetic():
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import skel_pose_fit_px_ref as ref
    import triangulate_mv_ref as tref
    import unlike_rig as ur
    from acinoset_amd import build
    from oracle import skel_fte as osf
    sk, N = ref.sref.skeleton("shipped"), 240
    rig = ur.subset(ur.unlike_rig(6, "fisheye", skew=True), [0, 1])
    act = osf.active_states(sk)
    blo, bhi = osf.bounds_table(sk, N)
    rng = np.random.default_rng(21)
    truth = np.concatenate([ref.root_centre(rig) + rng.uniform(-ref.ROOT_BOX, ref.ROOT_BOX, (N, 3)), 0.3 * rng.standard_normal((N, len(act) - 3))], 1)
    truth = np.clip(truth, blo[:, act], bhi[:, act])
    q = np.zeros((N, blo.shape[1]))
    q[:, act] = truth
    pos = osf.skeleton_fk_jac(sk, q)[0]
    L = pos.shape[1]
    clean = np.zeros((N, 2, L, 3))
    clean[..., :2] = ur.clean_pixels(pos, rig).transpose(1, 0, 2, 3) + rng.normal(0.0, ref.NOISE_PX, (N, 2, L, 2))
    clean[..., 2] = np.where(rng.random((N, 2, L)) >= ref.DROP, 0.9, 0.1)
    out = {}
    for label, det in (("clean", clean), ("pushed 5 %", tref.push_detections(clean, ref.THRESH)[0])):
        prog = build.skeleton.compile_skeleton(sk)
        valid = det[..., 2] > ref.THRESH
        model = build.SkeletonModel(skel=sk, prog=prog, names=prog["names"], active=act, lo=blo, hi=bhi, meas=det[..., :2].copy(),
                                    weights=np.where(valid, 1.0 / ref.NOISE_PX, 0.0), K=rig[0], D=rig[1], R=rig[2], t=rig[3], h=1.0 / 120.0,
                                    model_weight=0.002, camera_model="fisheye", loss="l1")
        fit3 = build.pose_fit(model, build.model_triangulation(model), **FIT)
        fitp = build.pose_fit_pixels(model, **FIT)
        row = {}
        for key, fit in (("fit_3d", fit3), ("pixel_fit", fitp)):
            p, st = (fit["positions"].cpu().numpy(), fit["status"].cpu().numpy()) if isinstance(fit["positions"], torch.Tensor) else (fit["positions"], fit["status"])
            err = 1e3 * np.linalg.norm(p - pos, axis=-1)[st < 2]
            row[key] = dict(frames_with_a_pose=int((st < 2).sum()), status_0=int((st == 0).sum()), slot_error_mm=dict(
                median=round(float(np.median(err)), 2), p90=round(float(np.percentile(err, 90)), 2)))
        out[label] = row
    print(json.dumps(dict(probe="skel_pose_fit_px_synthetic", frames=N, cameras=2, skeleton="shipped", noise_px=ref.NOISE_PX, drop=ref.DROP,
                          fit=FIT, runs=out)), flush=True)


def drive():
    os.environ.setdefault("OMP_NUM_THREADS", "16")
    for step, limit in STEPS:
        cmd = [sys.executable, os.path.abspath(__file__), step]
        out_dir = os.path.join(os.environ.get("ACINO_PROBE_OUT", os.path.join(ROOT, "build")), "skel_pose_fit_px_trace")
        if step == "--trace":
            prof = shutil.which("rocprofv3")
            if prof is None:
                print(json.dumps(dict(probe="skel_pose_fit_px_trace", skipped="rocprofv3 not found")), flush=True)
                continue
            cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out_dir, "--"] + cmd
        rc = subprocess.run(cmd, timeout=limit, cwd=ROOT).returncode      # (TimeoutExpired ends the run as well)
        if rc != 0:
            sys.exit(f"{step} ended with status {rc}: nothing more is started")
        if step == "--trace":
            five = lambda v: dict(median_of_5=round(float(np.median(v)), 3), min=round(min(v), 3), max=round(max(v), 3))      # noqa: E731
            ms = {}
            for k, v in read_trace(out_dir).items():
                if len(v) == 12:                             # the pixel kernel: six calls per way of summing g
                    ms[k] = dict(g_from_the_product=five(v[1:6]), g_by_the_loop=five(v[7:12]))
                elif len(v) >= 6:
                    ms[k] = five(v[1:6])
            print(json.dumps(dict(probe="skel_pose_fit_px_trace", clock="rocprofv3 kernel trace, ms, the first call of each dropped",
                                  kernels=ms)), flush=True)


if __name__ == "__main__":
    import torch
    torch.set_num_threads(min(16, torch.get_num_threads()))
    {"--timing": timing, "--trace": trace, "--synthetic": synthetic}.get(sys.argv[1] if len(sys.argv) > 1 else "", drive)()
