"""The joint fit of link lengths and FTE trajectory (build.link_fit_system, build.fit_link_scales_fte, csrc/skel_link_fit.hip)
measured on the GPU on the shipped video (tests/golden/human_dlc_full.npz, two cameras, the skeleton the reference ships with its
unobserved states pinned, by-name pairing, L1), as the windows of build.solve_video.

  --timing    one link_fit_system call (with and without sens_links / newton) beside one model_link_sensitivity call on the same
              windows of the video at the stitched trajectory's rows, in one process: host clock around calls that end in the copy
              of the outputs to the host, a warm-up round, then 5 alternating rounds; median, min, max.
  --trace     six link_fit_system calls on that batch for one rocprofv3 --kernel-trace run; the driver reads the trace and prints
              the median of the last five durations per kernel.
  --fit       fit_link_scales_fte on all windows of the video sharing one theta, started at the stitched trajectory of a solve at
              the scales 1: outer steps, cost before and after, wall time, the groups observed, the scales and bars beside those of
              fit_link_scales and fit_link_scales_pixels on the whole video, and the median std_pos_total of the joint posterior
              (solve_models(..., return_cov=True, cov_links=fit)) beside std_pos.

Without an option the three run one after the other, each as a child process under a time limit of its own (--trace under
rocprofv3 when it is installed, its files under $ACINO_PROBE_OUT, default build/); the first that fails, faults or runs out of
time ends the run.  One JSON line per section."""
import json
import os
import shutil
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
STEPS = (("--timing", 300), ("--trace", 300), ("--fit", 900))      # seconds
WINDOW, OVERLAP = 100, 20
MAX_OUTER, MAX_ITER = 12, 200
KERNELS = ("k_skel_link_fit_rhs", "k_skel_link_fit_reduce", "k_skel_fwdsub", "k_skel_sample_back", "k_skel_factor", "k_skel_cov_build",
           "k_skel_assemble", "k_skel_observability")


def timing():
    from skel_links_probe import batch
    from skel_pose_fit_probe import alternate
    from acinoset_amd import build
    models, xs, fit = batch()
    grp = fit["groups"]
    ms, _last = alternate({"model_link_sensitivity": lambda: build.model_link_sensitivity(models, xs, grp, pin_unobserved=True),
                           "link_fit_system": lambda: build.link_fit_system(models, xs, grp, pin_unobserved=True),
                           "link_fit_system_return_sens": lambda: build.link_fit_system(models, xs, grp, pin_unobserved=True,
                                                                                        return_sens=True)})
    print(json.dumps(dict(probe="link_fit_fte_timing", windows=len(models), window=WINDOW, n_active=len(models[0].active),
                          n_pose=len(models[0].names), groups=len(fit["scales"]),
                          clock="host clock around a call that ends in the copy of the outputs to the host, ms [median, min, max] of 5",
                          ms=ms)), flush=True)


def trace():
    import torch
    from skel_links_probe import batch
    from acinoset_amd import build
    models, xs, fit = batch()
    torch.cuda.synchronize()
    for _ in range(6):
        build.link_fit_system(models, xs, fit["groups"], pin_unobserved=True)
        torch.cuda.synchronize()


def _row(fit):
    return dict(status=fit["status"], outer_steps=len(fit["history"]), observed=[bool(v) for v in fit["observed"]],
                scales=[round(float(v), 4) for v in fit["scales"]],
                std_scales=[round(float(v), 4) if np.isfinite(v) else None for v in fit["std_scales"]])


def fit():
    import torch
    from skel_pose_fit_probe import shipped, whole_video_model
    from acinoset_amd import build
    sk, scene, tabs = shipped()
    res, _infos, starts = build.solve_video(sk, scene=scene, dlc_tables=tabs, window=WINDOW, overlap=OVERLAP, pairing="name")
    f0 = res["start_frame"]
    models = [build.build_model(sk, scene=scene, dlc_tables=tabs, n_frames=WINDOW, start_frame=st, pairing="name", initial_line=False)[0]
              for st in starts]
    xs = [res["x"][st - f0:st - f0 + WINDOW] for st in starts]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    joint = build.fit_link_scales_fte(models, x0=xs, pin_unobserved=True, max_outer=MAX_OUTER, max_iter=MAX_ITER)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    hist = joint["history"]
    row = dict(probe="link_fit_fte_fit", device=torch.cuda.get_device_name(0), windows=len(models), window=WINDOW,
               max_outer=MAX_OUTER, solve_max_iter=MAX_ITER, wall_s=round(wall, 2), n_used=int(joint["system"]["n_used"]),
               accepted_steps=int(sum(h["accepted"] for h in hist)),
               cost_first_accepted=float(hist[0]["cost"]) if hist else None, cost_end=float(hist[-1]["cost"]) if hist else None,
               max_dtheta_end=float(hist[-1]["max_dtheta"]) if hist else None, fit_link_scales_fte=_row(joint))
    whole = whole_video_model()
    row["fit_link_scales"] = _row(build.fit_link_scales(whole))
    row["fit_link_scales_pixels"] = _row(build.fit_link_scales_pixels(whole))
    out = build.solve_models(joint["models"], [r["x"] for r, _i in joint["results"]], max_iter=MAX_ITER, return_cov=True,
                             pin_unobserved=True, cov_links=joint)
    sp = np.concatenate([r["std_pos"].reshape(-1) for r, _i in out])
    st_ = np.concatenate([r["std_pos_total"].reshape(-1) for r, _i in out])
    ok = np.isfinite(sp) & np.isfinite(st_) & (sp > 0)
    row.update(finite_bars=int(ok.sum()), bars_below_an_unknown_group=int((np.isposinf(st_) & np.isfinite(sp)).sum()),
               median_std_pos_m=float(np.median(sp[ok])), median_std_pos_total_joint_m=float(np.median(st_[ok])),
               median_ratio_total_to_std_pos=float(np.median(st_[ok] / sp[ok])))
    print(json.dumps(row), flush=True)


def drive():
    from skel_links_probe import run_limited
    import skel_links_probe
    os.environ.setdefault("OMP_NUM_THREADS", "16")
    skel_links_probe.KERNELS = KERNELS
    for step, limit in STEPS:
        cmd = [sys.executable, os.path.abspath(__file__), step]
        out_dir = os.path.join(os.environ.get("ACINO_PROBE_OUT", os.path.join(ROOT, "build")), "link_fit_fte_trace")
        if step == "--trace":
            prof = shutil.which("rocprofv3")
            if prof is None:
                print(json.dumps(dict(probe="link_fit_fte_trace", skipped="rocprofv3 not found")), flush=True)
                continue
            cmd = [prof, "--kernel-trace", "--output-format", "csv", "-d", out_dir, "--"] + cmd
        rc = run_limited(cmd, limit)
        if rc != 0:
            sys.exit(f"{step} ended with status {rc}: nothing more is started")
        if step == "--trace":
            print(json.dumps(dict(probe="link_fit_fte_trace", clock="rocprofv3 --kernel-trace, kernel durations, all windows in one launch",
                                  kernels=skel_links_probe.read_trace(out_dir))), flush=True)


if __name__ == "__main__":
    import torch
    torch.set_num_threads(min(16, torch.get_num_threads()))
    {"--timing": timing, "--trace": trace, "--fit": fit}.get(sys.argv[1] if len(sys.argv) > 1 else "", drive)()
