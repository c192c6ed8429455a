"""The calibration's share of the skeleton solve's error bars on the shipped video (tests/golden/human_dlc_full.npz, the skeleton
the reference ships, its unobserved states pinned), for Sigma = calib.extrinsic_cov(2, 0.05, 2e-3, fixed=(0,)): camera 0 held,
camera 1 known to 0.05 degrees and 2 mm.

    python scripts/skel_calib_probe.py [--reps 5] [--window 100] [--overlap 20]

(1) build.solve_video(return_cov=True, pin_unobserved=True, cov_cams=Sigma) over the whole video: the median over frames and pose
    slots of std_pos_calib / std_pos (finite entries), and of both bars.
(2) the wall time of build.model_calibration_sensitivity next to build.model_covariance on the same batch - every window of the
    video in one call, at the stitched trajectory's rows: host clock around calls that end in the copy of the outputs to the
    host, 2 warm-ups, then ``--reps`` alternating runs; the median and the runs.
One JSON line."""
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def main():
    import torch
    from acinoset_amd import build, calib
    gd = os.path.join(HERE, "tests", "golden")
    g = np.load(os.path.join(gd, "skel_fte_model.npz"))
    sk = json.loads(str(g["skeleton_json"]))
    full = np.load(os.path.join(gd, "human_dlc_full.npz"))
    tabs = [(list(full["parts"]), full[f"det{c}"].astype(np.float64)) for c in range(2)]
    scene = (g["K"], g["D"], g["R"], g["t"])
    window, overlap, reps = arg("--window", 100), arg("--overlap", 20), arg("--reps", 5)
    sigma = calib.extrinsic_cov(2, 0.05, 2e-3, fixed=(0,))
    res, infos, starts = build.solve_video(sk, scene=scene, dlc_tables=tabs, window=window, overlap=overlap, pairing="name",
                                           return_cov=True, pin_unobserved=True, cov_cams=sigma)
    ok = np.isfinite(res["std_pos"]) & np.isfinite(res["std_pos_calib"]) & (res["std_pos"] > 0)
    row = dict(probe="skel_calib", device=torch.cuda.get_device_name(0), frames=int(res["x"].shape[0]), windows=len(starts),
               window=window, singular_windows=len(res["cov_singular_windows"]), finite_bars=int(ok.sum()),
               median_ratio=float(np.median((res["std_pos_calib"] / np.where(ok, res["std_pos"], 1.0))[ok])),
               median_std_pos_m=float(np.median(res["std_pos"][ok])), median_std_pos_calib_m=float(np.median(res["std_pos_calib"][ok])),
               median_std_pos_total_m=float(np.median(res["std_pos_total"][ok])))
    f0 = res["start_frame"]
    models = [build.build_model(sk, scene=scene, dlc_tables=tabs, n_frames=window, start_frame=st, pairing="name",
                                initial_line=False)[0] for st in starts]
    xs = [res["x"][st - f0:st - f0 + window] for st in starts]
    req = [("model_covariance", lambda: build.model_covariance(models, xs, pin_unobserved=True)),
           ("model_calibration_sensitivity", lambda: build.model_calibration_sensitivity(models, xs, sigma, pin_unobserved=True))]
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
    row["wall_ms"] = {name: dict(median=float(np.median(v)), runs=v) for name, v in runs.items()}
    print(json.dumps(row))


if __name__ == "__main__":
    main()
