"""Time of build.model_covariance with and without the rate covariances (acino_skel_fte_covariance_rates), and against another
build of the project (the parent commit's): the skeleton the reference ships on the shipped video's detections
(tests/golden/human_dlc_full.npz), its unobserved states pinned, (a) the video's 78 windows of 100 frames (stride 80) in one
batched call and (b) one 100-frame clip; iterates from tests/skel_cov_cases.iterate, one seed per window.

    python scripts/skel_cov_rates_probe.py                         this tree: every request below, one JSON line
    python scripts/skel_cov_rates_probe.py --other DIR --pairs 4   alternating processes, this tree / the tree at DIR (a checkout of
                                                                   another commit with its library built), one JSON line each
    python scripts/skel_cov_rates_probe.py --trace                 one pass of the full rates call on (a), for
                                                                   rocprofv3 --kernel-trace --stats -- python ... --trace

Requests: ``plain`` (cov_x, cov_pos, std_pos: the call as it was), ``std_pos`` (std_only), ``rates`` (plain and the six rate
arrays), ``rates_std`` (std_only with rates: std_pos, std_dx, std_ddx, std_vel), ``std_pos_vel`` (std_pos and std_vel alone: no
[P, P] array leaves the device).  A tree whose model_covariance has no ``rates`` keyword runs the first two.  Host clock around
calls that end in the copy of the outputs to the host; after 2 warm-ups of every request, ``--reps`` rounds (default 5), every
round runs every request once and starts one request further down the list, so that no request always follows the same one;
reported: the median, the runs, and the spread (max - min) per request."""
import inspect
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def arg(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def child(root, label):
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tests"))
    import torch
    import skel_cov_cases as cases
    from acinoset_amd import build
    assert os.path.realpath(os.path.dirname(os.path.dirname(build.__file__))) == os.path.realpath(root), build.__file__
    reps = int(arg("--reps", 5))
    gd = os.path.join(root, "tests", "golden")
    g, sk = cases.load(gd)
    full = np.load(os.path.join(gd, "human_dlc_full.npz"))
    n_video = min(full["det0"].shape[0], full["det1"].shape[0])
    det = np.stack([full["det0"][:n_video], full["det1"][:n_video]], axis=1).astype(np.float64)
    starts = list(range(0, n_video - 100 + 1, 80))
    starts += [n_video - 100] if starts[-1] + 100 < n_video else []       # the last window ends with the video
    models = [cases.make_model(g, sk, det, 100, s, parts=list(full["parts"])) for s in starts]
    xs = [cases.iterate(g, m, seed=k) for k, m in enumerate(models)]
    has_rates = "rates" in inspect.signature(build.model_covariance).parameters
    row = dict(probe="skel_cov_rates", label=label, device=torch.cuda.get_device_name(0), windows=len(models), frames=100,
               n_active=len(models[0].active), has_rates=has_rates, reps=reps)

    def requests(ms, xm):
        r = [("plain", lambda: build.model_covariance(ms, xm, pin_unobserved=True)),
             ("std_pos", lambda: build.model_covariance(ms, xm, std_only=True, pin_unobserved=True))]
        if has_rates:
            r += [("rates", lambda: build.model_covariance(ms, xm, pin_unobserved=True, rates=True)),
                  ("rates_std", lambda: build.model_covariance(ms, xm, std_only=True, pin_unobserved=True, rates=True)),
                  ("std_pos_vel", lambda: build._covariance(ms, xm, 1e-2, ("std_pos", "std_vel"), pin_unobserved=True))]
        return r

    if "--trace" in sys.argv:
        fn = dict(requests(models, xs))["rates"]
        fn()
        torch.cuda.synchronize()
        out = fn()
        row["status_ok"] = int(sum(o["status"] == 0 for o in out))
        print(json.dumps(row))
        return
    ok = [k for k, o in enumerate(build.model_covariance(models, xs, std_only=True, pin_unobserved=True)) if o["status"] == 0]
    row["status_ok"] = len(ok)
    for case, ms, xm in ((f"{len(models)}x100", models, xs), ("1x100", [models[ok[0]]], [xs[ok[0]]])):
        req = requests(ms, xm)
        runs = {name: [] for name, _fn in req}
        for k in range(2 + reps):
            for j in range(len(req)):
                name, fn = req[(j + k) % len(req)]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if k >= 2:
                    runs[name].append(round(1e3 * (time.perf_counter() - t0), 3))
        row[case] = {name: dict(median_ms=float(np.median(v)), spread_ms=round(max(v) - min(v), 3), runs_ms=v) for name, v in runs.items()}
    print(json.dumps(row))


def main():
    if "--child" in sys.argv or "--trace" in sys.argv:
        child(os.path.abspath(arg("--root", HERE)), arg("--label", "this"))
        return
    other = arg("--other")
    trees = [("this", HERE)] + ([("other", os.path.abspath(other))] if other else [])
    for _pair in range(int(arg("--pairs", 4)) if other else 1):
        for label, root in trees:                              # a fresh process per line: each tree loads its own library
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--root", root, "--label", label, "--reps", arg("--reps", "5")]
            res = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=600)
            if res.returncode != 0:
                sys.stderr.write(res.stderr[-4000:])
                sys.exit(res.returncode)
            print(res.stdout.strip().splitlines()[-1], flush=True)


if __name__ == "__main__":
    main()
