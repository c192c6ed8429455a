"""Time of acino_skel_fte_reprojection beside build.model_covariance on the same input: the whole shipped video as 78 windows of
100 frames, and one 40-frame clip (the shipped human skeleton with its rest positions moved as in tests/skel_cov_cases.py, so
that the covariance beside it is regular; 36 active states, 15 pose slots, 2 cameras).  Three figures per input: the C call
alone on device-resident arrays (one kernel; device events, median of 20 after 3 warm-ups; with cov_pos and without), the Python
call build.model_reprojection(cov_pos=...) with its host copies (host clock, median of 5 after 2), and build.model_covariance
(host clock, the same way).  Prints one JSON line.  For the kernel's own line run it under ``rocprofv3 --kernel-trace --stats --
python scripts/skel_reproj_probe.py --trace`` (one pass of each call)."""
import ctypes as C
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
from acinoset_amd import _lib, build, calib  # noqa: E402


def median_ms(fn, warm=2, reps=5):
    out = []
    for k in range(warm + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(out[warm:]))


def call_ms(models, xs, cov_pos, warm=3, reps=20):
    """The C call alone, device arrays resident: (ms with cov_pos, ms without)."""
    m0 = models[0]
    dev = torch.device("cuda", torch.cuda.current_device())
    act = np.asarray(m0.active, dtype=np.int32)
    B, N, Cn, Lp = len(models), m0.N, int(m0.meas.shape[1]), len(m0.names)
    p = build._skel_params(m0, len(act))
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=dev)   # noqa: E731
    meas, w = t(np.stack([m.meas for m in models])), t(np.stack([m.weights for m in models]))
    cams = torch.as_tensor(calib.camera_records(m0.camera_model, m0.K, m0.D, m0.R, m0.t), device=dev)
    x, cp = t(np.stack([xf[:, act] for xf in xs])), t(np.stack(cov_pos))
    empty = lambda *shape: torch.empty((B, N, Cn, Lp) + shape, dtype=torch.float64, device=dev)   # noqa: E731
    uv, cuv, res, m2 = empty(2), empty(2, 2), empty(2), empty()
    flags = torch.empty((B, N, Cn, Lp), dtype=torch.uint8, device=dev)
    act_c = (C.c_int32 * len(act))(*[int(a) for a in act])
    ops = build._ops_array(m0.prog)
    gate_w = float(max(m.weights.max() for m in models))
    out = []
    for with_cov in (True, False):
        times = []
        for k in range(warm + reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _lib.check(_lib.lib().acino_skel_fte_reprojection(
                C.byref(p), B, 0, ops, act_c, _lib.ptr(meas), _lib.ptr(w), _lib.ptr(cams), _lib.ptr(x),
                _lib.ptr(cp if with_cov else None), gate_w, _lib.ptr(uv), _lib.ptr(cuv if with_cov else None), _lib.ptr(res),
                _lib.ptr(m2), _lib.ptr(flags), _lib.stream_ptr()))
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
        out.append(float(np.median(times[warm:])))
    return out


def main():
    trace = "--trace" in sys.argv
    gd = os.path.join(ROOT, "tests", "golden")
    g, sk = cases.load(gd)
    sk = cases.generic_skeleton(sk)
    full = np.load(os.path.join(gd, "human_dlc_full.npz"))
    tabs = [(list(full["parts"]), full[f"det{c}"].astype(np.float64)) for c in range(2)]
    scene = (g["K"], g["D"], g["R"], g["t"])

    def window(n, st):
        return build.build_model(sk, scene=scene, dlc_tables=tabs, n_frames=n, start_frame=st, pairing="name", initial_line=False,
                                 r_meas=cases.R_MEAS_TEST)[0]
    starts = build.video_windows(0, min(len(tb[1]) for tb in tabs) - 1, 100, 20)
    inputs = {"video": [window(100, st) for st in starts], "clip40": [window(40, cases.SLICE_STARTS[0])]}
    row = dict(probe="skel_fte_reprojection", device=torch.cuda.get_device_name(0), n_active=len(inputs["clip40"][0].active))
    for name, models in inputs.items():
        xs = [cases.iterate(g, m, seed=k) for k, m in enumerate(models)]
        covs = build._covariance(models, xs, 1e-2, ("cov_pos",), raise_numeric=False)
        cov_pos = [cv["cov_pos"] for cv in covs]
        if trace:
            build.model_reprojection(models, xs, cov_pos=cov_pos)
            continue
        with_cov, without = call_ms(models, xs, cov_pos)
        m0 = models[0]
        row[name] = dict(clips=len(models), frames=m0.N, entries=len(models) * m0.N * int(np.prod(m0.meas.shape[1:3])),
                         singular_clips=int(sum(cv["status"] == 5 for cv in covs)),
                         call_ms=round(with_cov, 4), call_no_cov_ms=round(without, 4),
                         model_reprojection_ms=round(median_ms(lambda: build.model_reprojection(models, xs, cov_pos=cov_pos)), 3),
                         model_covariance_ms=round(median_ms(lambda: build._covariance(models, xs, 1e-2, ("cov_pos", "std_pos"),
                                                                                    raise_numeric=False)), 3))
    if not trace:
        print(json.dumps(row))


if __name__ == "__main__":
    main()
