"""The redescending loss of the skeleton FTE beside L1 on the shipped video (6 240 frames, 78 windows x 100 frames, by-name
pairing, the shipped human skeleton): ms per Levenberg-Marquardt iteration of the whole-video batch under either loss - fixed
iteration count from the windows' L1 end states, (t(max_iter = K) - t(max_iter = 0)) / K, the losses alternating in one process,
median of REPS - and the wall time of build.solve_video with loss="l1" and with loss="redescending" (the two-stage solve: the L1
run plus one batched robust call), with what the robust stage did to the detections.  Measured, no bar.  Prints one JSON line.
usage: skel_loss_probe.py"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from acinoset_amd import build  # noqa: E402

REPS, ITERS, MAX_ITER = 5, 100, 1500


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    g = np.load(os.path.join(ROOT, "tests", "golden", "skel_fte_model.npz"))
    sk = json.loads(str(g["skeleton_json"]))
    full = np.load(os.path.join(ROOT, "tests", "golden", "human_dlc_full.npz"))
    tabs = [(list(full["parts"]), full[f"det{c}"].astype(np.float64)) for c in range(2)]
    scene = (g["K"], g["D"], g["R"], g["t"])
    video = dict(scene=scene, dlc_tables=tabs, first_frame=0, last_frame=6239, window=100, overlap=20, pairing="name", max_iter=MAX_ITER)
    out, total = {}, {}
    build.solve_video(sk, **dict(video, max_iter=2))                                  # warm-up: library, kernels, allocator
    for loss in ("l1", "redescending"):
        total[loss] = timed(lambda loss=loss: out.__setitem__(loss, build.solve_video(sk, loss=loss, return_reprojection=True, **video)))
    res, infos, starts = out["redescending"]
    rep = build.detection_report(res)
    px_l1 = [i["mean_abs_residual_px"] for i in out["l1"][1]]
    models = {loss: [build.build_model(sk, scene=scene, dlc_tables=tabs, n_frames=100, start_frame=st, pairing="name",
                                       initial_line=False, loss=loss)[0] for st in starts] for loss in ("l1", "redescending")}
    # the stitched L1 trajectory cut into the windows again: the start of both timed runs (the robust loss is saturated at a far start)
    l1_end = out["l1"][0]["x"]
    x0s = [l1_end[st:st + 100].copy() for st in starts]
    kw = dict(ftol=0.0, xtol=0.0, gtol=0.0, l1_start=False)
    ms = {loss: [] for loss in models}
    for _ in range(REPS):
        for loss in models:
            t0 = timed(lambda loss=loss: build.solve_models(models[loss], x0s, max_iter=0, **kw))
            tk = timed(lambda loss=loss: build.solve_models(models[loss], x0s, max_iter=ITERS, **kw))
            ms[loss].append(1e3 * (tk - t0) / ITERS)
    weighted = int(((res["flags"] & 1) != 0).sum())
    print(json.dumps(dict(
        windows=len(starts), frames=int(res["x"].shape[0]),
        ms_per_iteration={loss: sorted(v)[REPS // 2] for loss, v in ms.items()}, ms_all=ms,
        solve_video_s=total, robust_over_l1=total["redescending"] / total["l1"],
        l1_iterations=int(sum(i["iterations"] for i in out["l1"][1])),
        robust_stage_iterations=int(sum(i["iterations"] for i in infos if "l1" in i)),
        robust_failed_windows=res["robust_failed_windows"],
        robust_status={s: int(sum(i["status_name"] == s for i in infos)) for s in sorted({i["status_name"] for i in infos})},
        weighted_detections=weighted, rejected=int(rep["n_rejected"].sum()), mean_weight=float(np.nanmean(rep["mean_weight"])),
        median_window_px_l1=float(np.median(px_l1)))))


if __name__ == "__main__":
    main()
