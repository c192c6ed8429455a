#!/usr/bin/env python3
"""What the EKF's error bars say and what they cost: the 120-frame synthetic sprint through synth's six-camera ring rig, one
clip and a batch of 64 (seeds 20210313 + b).  Per size: the median of smoothed_std_positions / std_positions over the frames
1 .. N-2 (what smoothing is worth, in metres per marker), and the wall time of ``ekf_batch(..., return_cov="bars")`` beside
the plain call on the same inputs - host clock around the whole call, which ends with every output on the host; both
variants warmed up, then alternating, median of REPS.  Needs the GPU.  Prints one JSON line.
usage: ekf_cov_probe.py"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from acinoset_amd import ekf, synth  # noqa: E402

REPS, FRAMES, FPS, THRESH, RES = 5, 120, 120.0, 0.5, (2704, 1520)


def probe(n_clips):
    seqs = [synth.make_sequence(FRAMES, "sprint", seed=20210313 + b) for b in range(n_clips)]
    rig = tuple(seqs[0][k] for k in "KDRt")
    dets = [s["det"] for s in seqs]
    s0 = [ekf.initial_state(d, *rig, FPS, THRESH) for d in dets]

    def run(flag):
        t0 = time.perf_counter()
        out = ekf.ekf_batch(dets, *rig, FPS, THRESH, RES, states0=s0, with_positions=False, return_cov=flag)
        return time.perf_counter() - t0, out

    for flag in (False, "bars"):
        run(flag)
    times = {False: [], "bars": []}
    for _ in range(REPS):
        for flag in (False, "bars"):
            dt, out = run(flag)
            times[flag].append(dt)
    ratio = np.stack([r["smoothed_std_positions"][1:-1] / r["std_positions"][1:-1] for r in out])
    plain, bars = float(np.median(times[False])), float(np.median(times["bars"]))
    return dict(clips=n_clips, frames=FRAMES, std_ratio_median=float(np.median(ratio)),
                std_ratio_range=[float(ratio.min()), float(ratio.max())],
                smoothed_std_positions_median_m=float(np.median(np.stack([r["smoothed_std_positions"][1:-1] for r in out]))),
                plain_ms=plain * 1e3, bars_ms=bars * 1e3, bars_over_plain=bars / plain,
                plain_ms_all=[t * 1e3 for t in times[False]], bars_ms_all=[t * 1e3 for t in times["bars"]])


def main():
    out = dict(what="EKF + RTS smoother on the %d-frame sprint: median smoothed / filtered marker std over the frames 1 .. N-2, "
                    "and wall ms of ekf_batch with return_cov='bars' beside the plain call (outputs on the host, median of %d, "
                    "alternating)" % (FRAMES, REPS),
               one_clip=probe(1), batch_64=probe(64))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
