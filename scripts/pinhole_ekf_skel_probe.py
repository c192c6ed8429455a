#!/usr/bin/env python3
"""Pinhole against fisheye for the EKF and the skeleton FTE: EKF us per frame (64 clips x 1 000 frames of the 2 m/s
circle through synth's ring rig, one ekf_batch launch, wall clock after a warm-up call) and skeleton solve ms per LM
iteration (the shipped video cut into 78 windows x 100 frames, the whole-video batch of solve_video, fixed iteration count:
(t(max_iter = K) - t(max_iter = 0)) / K), the models alternating in one process, median of REPS.  Prints one JSON line.
usage: pinhole_ekf_skel_probe.py"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pinhole_fte_ref as pref  # noqa: E402
from acinoset_amd import build, calib, ekf, fte, synth  # noqa: E402

REPS, EKF_CLIPS, EKF_FRAMES, SKEL_ITERS = 3, 64, 1000, 10


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def ekf_probe():
    q = synth.trajectory(EKF_FRAMES, "walk")          # (2 m/s: what the constant-acceleration model can follow)
    pos = fte.cheetah_fk(q)
    K, D, R, t = synth.make_rig()
    rigs = dict(fisheye=(K, D, R, t), pinhole=pref.pinhole_rig(pref.D12))
    dets = dict(fisheye=synth.detections_from_positions(pos, K, D, R, t),
                pinhole=pref.pinhole_detections(pos, *rigs["pinhole"]))
    s0 = {m: ekf.initial_state(dets[m], *rigs[m], 120.0, 0.5, camera_model=m) for m in rigs}
    numeric = {m: False for m in rigs}

    def run(m):
        # (through the pinhole rig - synth's fisheye focal length, a narrower view - the filter loses its target on this
        #  circle and reports it at the end of the call; the launch has done all frames by then, so the time stands)
        try:
            ekf.ekf_batch([dets[m]] * EKF_CLIPS, *rigs[m], 120.0, 0.5, (2704, 1520), states0=[s0[m]] * EKF_CLIPS,
                          with_positions=False, camera_model=m)
        except RuntimeError as e:
            if "positive definiteness" not in str(e):
                raise
            numeric[m] = True
    runs = {m: (lambda m=m: run(m)) for m in rigs}
    for m in rigs:
        runs[m]()
    us = {m: [] for m in rigs}
    for _ in range(REPS):
        for m in rigs:
            us[m].append(1e6 * timed(runs[m]) / EKF_FRAMES)
    return {m: dict(us_per_frame=sorted(us[m])[REPS // 2], us_all=us[m], lost_definiteness=numeric[m]) for m in rigs}


def skel_probe():
    g = np.load(os.path.join(ROOT, "tests", "golden", "skel_fte_model.npz"))
    sk = json.loads(str(g["skeleton_json"]))
    full = np.load(os.path.join(ROOT, "tests", "golden", "human_dlc_full.npz"))
    n = min(full["det0"].shape[0], full["det1"].shape[0])
    det = np.stack([full["det0"][:n], full["det1"][:n]], 1).astype(np.float64)        # [frames, 2, parts, 3]
    parts = [str(x) for x in full["parts"]]
    tabs = [(parts, det[:, c]) for c in range(det.shape[1])]
    scenes = dict(fisheye=(g["K"], g["D"], g["R"], g["t"]), pinhole=(g["K"], np.tile(pref.D5, (len(g["K"]), 1)), g["R"], g["t"]))
    starts = build.video_windows(0, det.shape[0] - 1, 100, 20)
    models = {m: [build.build_model(sk, scene=scenes[m], dlc_tables=tabs, n_frames=100, start_frame=st, pairing="name",
                                    initial_line=False, project_func=calib.project_points if m == "pinhole" else None)[0]
                  for st in starts] for m in scenes}
    x0s = {}
    for m in scenes:                         # root on the triangulated forehead of the window, angles 0
        head = calib.triangulate_pairs_dense(np.stack([det[:, c, parts.index("forehead")][:, None] for c in range(2)], 1),
                                             0.4, *scenes[m], return_masks=False, model=m)
        head = np.asarray(head.cpu().numpy() if isinstance(head, torch.Tensor) else head)[:, 0]
        ok = np.isfinite(head).all(1)
        fr = np.arange(det.shape[0], dtype=np.float64)
        head = np.stack([np.interp(fr, fr[ok], head[ok, j]) for j in range(3)], 1)
        x0s[m] = []
        for st, mod in zip(starts, models[m]):
            x0 = mod.init_x.copy()
            x0[:, :3] = head[st:st + 100]
            x0s[m].append(x0)
    kw = dict(ftol=0.0, xtol=0.0, gtol=0.0)
    for m in scenes:
        build.solve_models(models[m], x0s[m], max_iter=2, **kw)
    ms = {m: [] for m in scenes}
    iters = {}
    for _ in range(REPS):
        for m in scenes:
            t0 = timed(lambda m=m: build.solve_models(models[m], x0s[m], max_iter=0, **kw))
            out = []
            tk = timed(lambda m=m: out.append(build.solve_models(models[m], x0s[m], max_iter=SKEL_ITERS, **kw)))
            iters[m] = max(i["iterations"] for _r, i in out[0])
            ms[m].append(1e3 * (tk - t0) / max(iters[m], 1))
    return {m: dict(windows=len(starts), iterations=iters[m], ms_per_iteration=sorted(ms[m])[REPS // 2], ms_all=ms[m])
            for m in scenes}


def main():
    out = dict(what="EKF us per frame (%d clips x %d frames, one launch) and skeleton solve ms per LM iteration (78 windows x "
                    "100 frames), wall clock, median of %d alternating repetitions" % (EKF_CLIPS, EKF_FRAMES, REPS))
    out["ekf"] = ekf_probe()
    out["ekf"]["pinhole_over_fisheye"] = out["ekf"]["pinhole"]["us_per_frame"] / out["ekf"]["fisheye"]["us_per_frame"]
    out["skel"] = skel_probe()
    out["skel"]["pinhole_over_fisheye"] = out["skel"]["pinhole"]["ms_per_iteration"] / out["skel"]["fisheye"]["ms_per_iteration"]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
