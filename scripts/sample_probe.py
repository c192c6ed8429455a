"""Time of FTEContext.sample (acino_fte_sample: the forward pivot sweep of the covariance, the factors of all nodes in
parallel, one backward substitution per clip and panel of 64 samples, then the FK of every sample) beside
FTEContext.covariance of the same context: 999 and 10 000 frames as one sequence, 64 x 1 000 frames as clips, each at
S = 16, 64, 1024 (--quick: the 999-frame case alone).  HIP events, median of 5 after 2 warm-ups; prints one JSON line.
``sample_ms`` includes the FK, ``sample_no_fk_ms`` leaves it out (positions=False); z is drawn once, outside the timing."""
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


def case(name, det, rig, Ts, x0, sizes, **kw):
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ctx = fte.FTEContext(det, *rig, Ts, ftol=0.0, xtol=0.0, gtol=0.0, clamp_lambda=True, **kw)
        try:
            ctx.enable_graph(True)
            ctx.set_x(x0)
            for _ in range(12):                      # (a few iterations in: the iterate the samples are drawn at is a solved one)
                ctx.step()
            row = dict(case=name, frames=int(ctx.N), clip_len=int(kw.get("clip_len", 0)),
                       covariance_ms=round(median_ms(lambda: ctx.covariance()), 4), samples={})
            for S in sizes:
                if S * ctx.N * 25 * 8 * 4.4 > 120e9:  # z + x + positions of the samples: keep well inside the HBM
                    continue
                z = torch.randn((S, ctx.N, 25), dtype=torch.float64, device=ctx.device)
                full = median_ms(lambda: ctx.sample(S, z=z))
                nofk = median_ms(lambda: ctx.sample(S, z=z, positions=False))
                row["samples"][str(S)] = dict(sample_ms=round(full, 4), sample_no_fk_ms=round(nofk, 4))
                del z
            # one derived quantity with its interval: mean speed of the spine over the clip (first clip), 5 % / 95 %
            out = ctx.sample(256, seed=0)
            L = int(kw.get("clip_len", 0)) or ctx.N
            spine = out["positions"][:, :L, fte.MARKERS.index("spine")]
            speed = (spine[:, 1:] - spine[:, :-1]).norm(dim=-1).sum(dim=1) / ((L - 1) * ctx.Ts)
            q = torch.quantile(speed, torch.tensor([0.05, 0.5, 0.95], dtype=torch.float64, device=speed.device))
            row["spine_mean_speed_m_s"] = dict(q05=float(q[0]), q50=float(q[1]), q95=float(q[2]))
            return row
        finally:
            ctx.close()


def main():
    quick = "--quick" in sys.argv
    sizes = (16, 64, 1024)
    out = []
    for n, kind in ((999, "trot"),) if quick else ((999, "trot"), (10000, "loop")):
        seq = synth.make_sequence(n, kind)
        rig = (seq["K"], seq["D"], seq["R"], seq["t"])
        x0 = fte.nose_line_init(seq["det"], *rig, 0.5)[:, fte.ACTIVE]
        out.append(case(f"{n} frames, one sequence", seq["det"], rig, seq["Ts"], x0, sizes))
    if not quick:
        seq = synth.make_sequence(1000, "trot")
        rig = (seq["K"], seq["D"], seq["R"], seq["t"])
        det64 = torch.as_tensor(seq["det"], device="cuda").repeat(64, 1, 1, 1)
        x64 = np.tile(fte.nose_line_init(seq["det"], *rig, 0.5)[:, fte.ACTIVE], (64, 1))
        out.append(case("64 x 1000 frames, clips", det64, rig, seq["Ts"], x64, sizes, clip_len=1000))
    print(json.dumps(dict(probe="fte_sample", device=torch.cuda.get_device_name(0), cases=out)))


if __name__ == "__main__":
    main()
