"""The link lengths' share of the skeleton solve's error bars (build.model_link_sensitivity, csrc/skel_links.hip) measured on the
GPU on the shipped video (tests/golden/human_dlc_full.npz, two cameras, the skeleton the reference ships with its unobserved
states pinned, by-name pairing), as build.solve_video windows on the skeleton at the scales build.fit_link_scales_pixels finds.

  --ratios    solve_video(return_cov=True, pin_unobserved=True, cov_links=Sigma) for two Sigma: the dict of fit_link_scales_pixels
              on the whole video (its cov_log_scales; the groups it does not observe are flagged unknown) and a diagonal 10 % per
              link.  Per Sigma the median over frames and pose slots (finite entries) of std_pos_links / std_pos and of the bars.
              The fit's Sigma comes from the very video that is solved: the ratio shows the size of the term, the sum is not a
              valid total there.
  --timing    the batched call on every window of the video at the stitched trajectory's rows beside model_covariance and
              model_calibration_sensitivity on the same batch: host clock around calls that end in the copy of the outputs to the
              host, a warm-up round, then 5 alternating rounds; median, min, max.
  --trace     six model_link_sensitivity calls on that batch for one rocprofv3 --kernel-trace run; the driver reads the trace and
              prints the median of the last five durations per kernel.

Without an option the three run one after the other, each as a child process under a time limit of its own (--trace under
rocprofv3 when it is installed, its files under $ACINO_PROBE_OUT, default build/); the first that fails, faults or runs out of
time ends the run.  One JSON line per section."""
import json
import os
import shutil
import signal
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
STEPS = (("--ratios", 420), ("--timing", 300), ("--trace", 300))      # seconds
WINDOW, OVERLAP = 100, 20
KERNELS = ("k_skel_links_rhs", "k_skel_links_combine", "k_skel_fwdsub", "k_skel_sample_back", "k_skel_factor", "k_skel_cov_build",
           "k_skel_assemble", "k_skel_observability")


def fitted():
    """(sk, scene, tabs, fit): the shipped inputs and the length fit of the whole video from its detections."""
    from skel_pose_fit_probe import shipped, whole_video_model
    from acinoset_amd import build
    sk, scene, tabs = shipped()
    return sk, scene, tabs, build.fit_link_scales_pixels(whole_video_model())


def video(sk, scene, tabs, fit, cov_links):
    from acinoset_amd import build
    return build.solve_video(sk, scene=scene, dlc_tables=tabs, window=WINDOW, overlap=OVERLAP, pairing="name", return_cov=True,
                             pin_unobserved=True, link_scales=(fit["groups"], fit["scales"]), cov_links=cov_links,
                             link_groups=None if cov_links is None else fit["groups"])


def ratios():
    import torch
    sk, scene, tabs, fit = fitted()
    K = len(fit["scales"])
    row = dict(probe="skel_links_ratios", device=torch.cuda.get_device_name(0), window=WINDOW, groups=K,
               fit=dict(status=fit["status"], observed=[bool(v) for v in fit["observed"]],
                        scales=[round(float(v), 4) for v in fit["scales"]],
                        std_log_scales=[round(float(v), 5) for v in np.sqrt(np.diag(fit["cov_log_scales"]))]))
    for name, cov in (("fit_link_scales_pixels", fit), ("diagonal_10_percent", 0.01 * np.eye(K))):
        res, _infos, starts = video(sk, scene, tabs, fit, cov)
        ok = np.isfinite(res["std_pos"]) & np.isfinite(res["std_pos_links"]) & (res["std_pos"] > 0)
        inf = np.isposinf(res["std_pos_links"]) & np.isfinite(res["std_pos"])
        row.update(frames=int(res["x"].shape[0]), windows=len(starts), singular_windows=len(res["cov_singular_windows"]))
        row[name] = dict(finite_bars=int(ok.sum()), bars_below_an_unknown_group=int(inf.sum()),
                         median_ratio=float(np.median((res["std_pos_links"] / np.where(ok, res["std_pos"], 1.0))[ok])),
                         median_std_pos_m=float(np.median(res["std_pos"][ok])),
                         median_std_pos_links_m=float(np.median(res["std_pos_links"][ok])),
                         median_std_pos_total_m=float(np.median(res["std_pos_total"][ok])))
    print(json.dumps(row), flush=True)


def batch():
    """Every window of the video as one batch at the stitched trajectory's rows: (models, xs, fit)."""
    from acinoset_amd import build
    sk, scene, tabs, fit = fitted()
    res, _infos, starts = video(sk, scene, tabs, fit, None)
    f0 = res["start_frame"]
    models = [build.build_model(sk, scene=scene, dlc_tables=tabs, n_frames=WINDOW, start_frame=st, pairing="name", initial_line=False,
                                link_scales=(fit["groups"], fit["scales"]))[0] for st in starts]
    return models, [res["x"][st - f0:st - f0 + WINDOW] for st in starts], fit


def timing():
    from skel_pose_fit_probe import alternate
    from acinoset_amd import build, calib
    models, xs, fit = batch()
    sig_c = calib.extrinsic_cov(2, 0.05, 2e-3, fixed=(0,))
    ms, _last = alternate({"model_covariance": lambda: build.model_covariance(models, xs, pin_unobserved=True),
                           "model_calibration_sensitivity": lambda: build.model_calibration_sensitivity(models, xs, sig_c, pin_unobserved=True),
                           "model_link_sensitivity": lambda: build.model_link_sensitivity(models, xs, fit["groups"], fit, pin_unobserved=True)})
    print(json.dumps(dict(probe="skel_links_timing", windows=len(models), window=WINDOW, n_active=len(models[0].active),
                          n_pose=len(models[0].names), groups=len(fit["scales"]),
                          clock="host clock around a call that ends in the copy of the outputs to the host, ms [median, min, max] of 5",
                          ms=ms)), flush=True)


def trace():
    import torch
    from acinoset_amd import build
    models, xs, fit = batch()
    torch.cuda.synchronize()
    for _ in range(6):
        build.model_link_sensitivity(models, xs, fit["groups"], fit, pin_unobserved=True)
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


def run_limited(cmd, limit):
    """The exit status of ``cmd`` run as a child in a session of its own; at the time limit its whole process group is killed
    (under rocprofv3 the program that holds the GPU is a grandchild) and the status is 124."""
    child = subprocess.Popen(cmd, cwd=ROOT, start_new_session=True)
    try:
        return child.wait(timeout=limit)
    except subprocess.TimeoutExpired:
        os.killpg(child.pid, signal.SIGKILL)
        child.wait()
        return 124


def drive():
    os.environ.setdefault("OMP_NUM_THREADS", "16")
    for step, limit in STEPS:
        cmd = [sys.executable, os.path.abspath(__file__), step]
        out_dir = os.path.join(os.environ.get("ACINO_PROBE_OUT", os.path.join(ROOT, "build")), "skel_links_trace")
        if step == "--trace":
            prof = shutil.which("rocprofv3")
            if prof is None:
                print(json.dumps(dict(probe="skel_links_trace", skipped="rocprofv3 not found")), flush=True)
                continue
            cmd = [prof, "--kernel-trace", "--output-format", "csv", "-d", out_dir, "--"] + cmd
        rc = run_limited(cmd, limit)
        if rc != 0:
            sys.exit(f"{step} ended with status {rc}: nothing more is started")
        if step == "--trace":
            print(json.dumps(dict(probe="skel_links_trace", clock="rocprofv3 --kernel-trace, kernel durations, all windows in one launch",
                                  kernels=read_trace(out_dir))), flush=True)


if __name__ == "__main__":
    import torch
    torch.set_num_threads(min(16, torch.get_num_threads()))
    {"--ratios": ratios, "--timing": timing, "--trace": trace}.get(sys.argv[1] if len(sys.argv) > 1 else "", drive)()
