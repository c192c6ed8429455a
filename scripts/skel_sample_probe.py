"""Time of build.model_samples (acino_skel_fte_sample) beside build.model_covariance on the same clips: 8 windows of 100 frames
of the detection slice under tests/golden (36 active states: PT = 48), S = 64 and 1024.  Host clock around calls that end in
the entry's own synchronisation, median of 5 after 2 warm-ups, host copies of z and of the samples included; prints one JSON
line.  For the kernels alone run it under ``rocprofv3 --kernel-trace --stats -- python scripts/skel_sample_probe.py --trace``
(one pass of each call, S = 1024 alone, no repeats): k_skel_factor and k_skel_selinv are one workgroup per clip and walk 100 frames each,
k_skel_sample_back is (S / 64) x 8 workgroups that walk 100 frames each - divide their times by 100 for the time per frame (and
panel)."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import skel_cov_cases as cases  # noqa: E402
from acinoset_amd import build  # noqa: E402


def median_ms(fn, warm=2, reps=5):
    out = []
    for k in range(warm + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(out[warm:]))


def main():
    trace = "--trace" in sys.argv
    gd = os.path.join(ROOT, "tests", "golden")
    g, sk = cases.load(gd)
    sk = cases.generic_skeleton(sk)
    det = np.load(os.path.join(gd, "human_dlc_slice.npz"))["det"].astype(np.float64)
    models = [cases.make_model(g, sk, det, 100, 45 * k) for k in range(8)]
    xs = [cases.iterate(g, m, seed=k) for k, m in enumerate(models)]
    n_act = len(models[0].active)
    row = dict(probe="skel_fte_sample", device=torch.cuda.get_device_name(0), clips=8, frames=100, n_active=n_act, samples={})
    if trace:
        build.model_covariance(models, xs)
        build.model_samples(models, xs, n_samples=1024)
        return
    row["covariance_ms"] = round(median_ms(lambda: build.model_covariance(models, xs)), 3)
    for S in (64, 1024):
        z = np.random.default_rng(0).standard_normal((8, S, 100, n_act))
        full = median_ms(lambda: build.model_samples(models, xs, z=z))
        nofk = median_ms(lambda: build.model_samples(models, xs, z=z, positions=False))
        row["samples"][str(S)] = dict(sample_ms=round(full, 3), sample_no_fk_ms=round(nofk, 3))
    print(json.dumps(row))


if __name__ == "__main__":
    main()
