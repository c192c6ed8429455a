"""Time of FTEContext.calibration_sensitivity (acino_fte_calibration_sensitivity: the cross term, the sampler's forward sweep
and factors, one forward and one backward substitution per panel of 64 columns, the combine) beside FTEContext.covariance and
FTEContext.sample(36) of the same context: 10 000 frames of the loop as one sequence, 6 cameras, 60 LM iterations from the nose
line.  HIP events, median of 5 after 2 warm-ups.  Also the measured example of the README: on the solved 120-frame sprint the
median of std_pos_cal / std_pos for calib.extrinsic_cov(6, 0.05, 2e-3, fixed=(0,)).  Prints one JSON line."""
import json
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from acinoset_amd import calib, fte, synth


def median_ms(fn, warm=2, reps=5):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def solved(n, kind, max_iter):
    seq = synth.make_sequence(n, kind)
    rig = (seq["K"], seq["D"], seq["R"], seq["t"])
    ctx = fte.FTEContext(seq["det"], *rig, seq["Ts"])
    ctx.set_x(fte.nose_line_init(seq["det"], *rig, 0.5)[:, fte.ACTIVE])
    info = ctx.solve(max_iter)
    return ctx, info


def main():
    sigma = calib.extrinsic_cov(6, 0.05, 2e-3, fixed=(0,))
    out = dict(probe="fte_calibration", device=torch.cuda.get_device_name(0))
    ctx, info = solved(120, "sprint", 100)
    try:
        cal = ctx.calibration_sensitivity(sigma)
        std_pos = ctx.covariance(std_only=True)[2]
        out["sprint_120"] = dict(status=info["status_name"], median_std_pos_mm=float(std_pos.median()) * 1e3,
                                 median_std_pos_cal_mm=float(cal["std_pos_cal"].median()) * 1e3,
                                 median_ratio=float((cal["std_pos_cal"] / std_pos).median()),
                                 max_abs_sens=float(cal["sens"].abs().max()))
    finally:
        ctx.close()
    ctx, info = solved(10000, "loop", 60)
    try:
        z = torch.randn((36, ctx.N, 25), dtype=torch.float64, device=ctx.device)
        out["loop_10000"] = dict(status=info["status_name"], frames=int(ctx.N), cams=int(ctx.C),
                                 covariance_ms=round(median_ms(lambda: ctx.covariance()), 4),
                                 sample_36_no_fk_ms=round(median_ms(lambda: ctx.sample(36, z=z, positions=False)), 4),
                                 sensitivity_ms=round(median_ms(lambda: ctx.calibration_sensitivity()), 4),
                                 sensitivity_with_cov_ms=round(median_ms(lambda: ctx.calibration_sensitivity(sigma)), 4))
    finally:
        ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
