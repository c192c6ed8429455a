"""build.model_observability on the skeleton the reference ships and on a clip that lost a limb, and the time of
build.model_covariance with ``pin_unobserved`` off and on beside build.model_observability alone: ``--clips`` windows (default 8;
a video is 78) of 100 frames of the detection slice under tests/golden, the covariance tests' generic skeleton (36 active states:
PT = 48; fully observed, so both settings factor the same matrix and the difference is the observability pass).  Host clock
around calls that end in the entry's own synchronisation or the copy of the outputs, median of 5 after 2 warm-ups, host copies
included; prints one JSON line."""
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
    return float(np.median(out[warm:])), [round(v, 3) for v in out[warm:]]


def main():
    clips = int(sys.argv[sys.argv.index("--clips") + 1]) if "--clips" in sys.argv else 8
    gd = os.path.join(ROOT, "tests", "golden")
    g, sk0 = cases.load(gd)
    det = np.load(os.path.join(gd, "human_dlc_slice.npz"))["det"].astype(np.float64)
    row = dict(probe="skel_unobs", device=torch.cuda.get_device_name(0), clips=clips, frames=100)
    # ---- what the rule says: the shipped skeleton, and the generic one with elbow1 / wrist1 undetected
    shipped = cases.make_model(g, sk0, det, 100, 60)
    xs = cases.iterate(g, shipped)
    ob = build.model_observability([shipped], [xs])[0]
    act = np.asarray(shipped.active)
    seen = ob["info"][act][ob["info"][act] > 0]
    row["shipped"] = dict(unobserved=ob["unobserved"], weakest_over_strongest=float(seen.min() / seen.max()),
                          info_at_unobserved=[float(ob["info"][u]) for u in ob["unobserved"]])
    cv = build.model_covariance([shipped], [xs], std_only=True, pin_unobserved=True)[0]
    row["shipped"].update(status=cv["status"], std_pos_m=[float(cv["std_pos"].min()), float(cv["std_pos"].max())])
    sk = cases.generic_skeleton(sk0)
    lost = cases.make_model(g, sk, det, 100, 60)
    names = list(lost.names)
    lost.weights = lost.weights.copy()
    lost.weights[:, :, [names.index("elbow1"), names.index("wrist1")]] = 0.0
    xl = cases.iterate(g, lost)
    ob = build.model_observability([lost], [xl])[0]
    cv = build.model_covariance([lost], [xl], std_only=True, pin_unobserved=True)[0]
    row["lost_limb"] = dict(unobserved=ob["unobserved"], status=cv["status"],
                            undetermined_poses=[names[l] for l in np.nonzero(np.isinf(cv["std_pos"]).any(0))[0]])
    # ---- time
    models = [cases.make_model(g, sk, det, 100, (4 * k) % 360) for k in range(clips)]
    xm = [cases.iterate(g, m, seed=k) for k, m in enumerate(models)]
    n_act = len(models[0].active)
    row["n_active"] = n_act
    for key, fn in (("covariance_ms", lambda: build.model_covariance(models, xm)),
                    ("covariance_pin_unobserved_ms", lambda: build.model_covariance(models, xm, pin_unobserved=True)),
                    ("observability_ms", lambda: build.model_observability(models, xm))):
        med, runs = median_ms(fn)
        row[key], row[key[:-3] + "_runs_ms"] = round(med, 3), runs
    print(json.dumps(row))


if __name__ == "__main__":
    main()
