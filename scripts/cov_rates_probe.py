"""Time of FTEContext.covariance_rates (acino_fte_covariance_rates: the sweeps of acino_fte_covariance, once, plus one
workgroup per node for cov_dx / cov_ddx / cov_vel / std_vel) beside FTEContext.covariance in the same process: 999 and
10 000 frames as one sequence, 64 x 1 000 frames as clips.  HIP events, median of 5 after 2 warm-ups; prints one JSON line."""
import json
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from acinoset_amd import fte, synth


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


def case(name, det, rig, Ts, x0, **kw):
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ctx = fte.FTEContext(det, *rig, Ts, ftol=0.0, xtol=0.0, gtol=0.0, clamp_lambda=True, **kw)
        try:
            ctx.enable_graph(True)
            ctx.set_x(x0)
            for _ in range(12):
                ctx.step()
            old = median_ms(lambda: ctx.covariance())
            rates = median_ms(lambda: ctx.covariance_rates())
            both = median_ms(lambda: ctx.covariance_rates(with_cov=True))
            std = median_ms(lambda: ctx.covariance_rates(std_only=True))
            s = ctx.covariance_rates(std_only=True)[3]
            return dict(case=name, frames=int(ctx.N), clip_len=int(kw.get("clip_len", 0)), covariance_ms=round(old, 4),
                        rates_ms=round(rates, 4), rates_with_covariance_ms=round(both, 4), rates_std_only_ms=round(std, 4),
                        std_vel_median_m_s=float(s.median()), std_vel_max_m_s=float(s.max()))
        finally:
            ctx.close()


def main():
    out = []
    for n, kind in ((999, "trot"), (10000, "loop")):
        seq = synth.make_sequence(n, kind)
        rig = (seq["K"], seq["D"], seq["R"], seq["t"])
        x0 = fte.nose_line_init(seq["det"], *rig, 0.5)[:, fte.ACTIVE]
        out.append(case(f"{n} frames, one sequence", seq["det"], rig, seq["Ts"], x0))
    seq = synth.make_sequence(1000, "trot")
    rig = (seq["K"], seq["D"], seq["R"], seq["t"])
    det64 = torch.as_tensor(seq["det"], device="cuda").repeat(64, 1, 1, 1)
    x64 = np.tile(fte.nose_line_init(seq["det"], *rig, 0.5)[:, fte.ACTIVE], (64, 1))
    out.append(case("64 x 1000 frames, clips", det64, rig, seq["Ts"], x64, clip_len=1000))
    print(json.dumps(dict(probe="fte_covariance_rates", device=torch.cuda.get_device_name(0), cases=out)))


if __name__ == "__main__":
    main()
