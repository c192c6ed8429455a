"""Time of FTEContext.reprojection (acino_fte_reprojection: one streaming kernel) beside FTEContext.covariance of the same
context: 999 and 10 000 frames as one sequence, 64 x 1 000 frames as clips (--quick: the 999-frame case alone), with and
without cov_uv.  HIP events, median of 5 after 2 warm-ups; prints one JSON line.  ``reprojection_ms`` / ``..._no_cov_ms``
are the Python call (output tensors from torch's caching allocator, std_uv as torch arithmetic; cov_pos given, the covariance
sweeps not included), ``kernel_ms`` / ``kernel_no_cov_ms`` the library call alone into preallocated outputs; ``gbytes_per_s``
is the bytes the kernel must move (24 B detection + 72 / C B cov_pos in, 113 B or 81 B out per entry) over ``kernel_ms``."""
import json
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from acinoset_amd import _lib, fte, synth


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
            for _ in range(12):                      # (a few iterations in: the iterate reported on is a solved one)
                ctx.step()
            cov_pos = ctx.covariance()[1]
            rep = ctx.reprojection(cov_pos=cov_pos)
            lib, ptr, sp = _lib.lib(), _lib.ptr, _lib.stream_ptr

            def raw(with_cov):
                _lib.check(lib.acino_fte_reprojection(ctx._h, ptr(cov_pos if with_cov else None), ptr(rep["uv"]),
                                                      ptr(rep["cov_uv"] if with_cov else None), ptr(rep["res"]), ptr(rep["weight"]),
                                                      ptr(rep["mahal2"]), ptr(rep["flags"]), sp()))

            entries = ctx.N * ctx.C * 20
            row = dict(case=name, frames=int(ctx.N), clip_len=int(kw.get("clip_len", 0)), entries=entries,
                       covariance_ms=round(median_ms(lambda: ctx.covariance()), 4),
                       reprojection_ms=round(median_ms(lambda: ctx.reprojection(cov_pos=cov_pos)), 4),
                       reprojection_no_cov_ms=round(median_ms(lambda: ctx.reprojection(cov=False)), 4),
                       kernel_ms=round(median_ms(lambda: raw(True)), 4),
                       kernel_no_cov_ms=round(median_ms(lambda: raw(False)), 4))
            row["gbytes_per_s"] = round(entries * (24 + 72 / ctx.C + 113) / row["kernel_ms"] * 1e-6, 1)
            row["gbytes_per_s_no_cov"] = round(entries * (24 + 81) / row["kernel_no_cov_ms"] * 1e-6, 1)
            return row
        finally:
            ctx.close()


def main():
    quick = "--quick" in sys.argv
    out = []
    for n, kind in ((999, "trot"),) if quick else ((999, "trot"), (10000, "loop")):
        seq = synth.make_sequence(n, kind)
        rig = (seq["K"], seq["D"], seq["R"], seq["t"])
        x0 = fte.nose_line_init(seq["det"], *rig, 0.5)[:, fte.ACTIVE]
        out.append(case(f"{n} frames, one sequence", seq["det"], rig, seq["Ts"], x0))
    if not quick:
        seq = synth.make_sequence(1000, "trot")
        rig = (seq["K"], seq["D"], seq["R"], seq["t"])
        det64 = torch.as_tensor(seq["det"], device="cuda").repeat(64, 1, 1, 1)
        x64 = np.tile(fte.nose_line_init(seq["det"], *rig, 0.5)[:, fte.ACTIVE], (64, 1))
        out.append(case("64 x 1000 frames, clips", det64, rig, seq["Ts"], x64, clip_len=1000))
    print(json.dumps(dict(probe="fte_reprojection", device=torch.cuda.get_device_name(0), cases=out)))


if __name__ == "__main__":
    main()
