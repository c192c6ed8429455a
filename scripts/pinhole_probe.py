#!/usr/bin/env python3
"""Pinhole against fisheye FTE: ms per LM iteration (device events around 20 graph-replayed steps after warm-up) and the
assembly's share of it (the profiler's event time of the assemble class), at 999 and 10 000 frames of the same
trajectory seen through synth's ring rig with either camera model; the models alternate in one process.  Prints one JSON
line.  usage: pinhole_probe.py [frames ...]"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pinhole_fte_ref as pref  # noqa: E402
from acinoset_amd import fte, synth  # noqa: E402

STEPS, WARM, REPS = 20, 5, 3


def context(seq, model, s):
    rig = (seq["K"], seq["D"], seq["R"], seq["t"])
    x0 = fte.triangulation_init(seq["det"], *rig, 0.5, camera_model=model)[:, fte.ACTIVE]
    with torch.cuda.stream(s):
        ctx = fte.FTEContext(seq["det"], *rig, seq["Ts"], ftol=0.0, xtol=0.0, gtol=0.0, clamp_lambda=True, camera_model=model)
        ctx.enable_graph(True)
        ctx.set_x(x0)
    return ctx


def time_steps(ctx, s):
    with torch.cuda.stream(s):
        for _ in range(WARM):
            ctx.step()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        for _ in range(STEPS):
            ctx.step()
        b.record(s)
        b.synchronize()
        return a.elapsed_time(b) / STEPS


def assemble_us(ctx, s):
    with torch.cuda.stream(s):
        ctx.enable_graph(False)
        ctx.profile_begin()
        for _ in range(STEPS):
            ctx.step()
        torch.cuda.synchronize()
        prof = ctx.profile_end()
        ctx.enable_graph(True)
    return 1e3 * prof["assemble"]["ms"] / STEPS, prof["assemble"]["launches"] / STEPS


def main():
    sizes = [int(a) for a in sys.argv[1:]] or [999, 10000]
    out = dict(what="ms per LM iteration (graph replay, device events, %d steps after %d warm-up, median of %d alternating "
                    "repetitions) and assembly us per iteration (profiler events)" % (STEPS, WARM, REPS), sizes={})
    s = torch.cuda.Stream()
    for n in sizes:
        seqs = dict(fisheye=synth.make_sequence(n, "loop"), pinhole=pref.pinhole_sequence(n, "loop"))
        ctxs = {m: context(seqs[m], m, s) for m in seqs}
        ms = {m: [] for m in seqs}
        for _ in range(REPS):
            for m in ("fisheye", "pinhole"):
                ms[m].append(time_steps(ctxs[m], s))
        row = {}
        for m in ("fisheye", "pinhole"):
            asm, launches = assemble_us(ctxs[m], s)
            st = ctxs[m].state()
            row[m] = dict(ms_per_step=sorted(ms[m])[REPS // 2], ms_all=ms[m], assemble_us_per_step=asm,
                          assemble_launches_per_step=launches, status=st["status_name"], cost=st["cost"])
            ctxs[m].close()
        row["pinhole_over_fisheye_step"] = row["pinhole"]["ms_per_step"] / row["fisheye"]["ms_per_step"]
        row["pinhole_over_fisheye_assemble"] = row["pinhole"]["assemble_us_per_step"] / row["fisheye"]["assemble_us_per_step"]
        out["sizes"][str(n)] = row
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
