"""GPU (-m gpu): the ends of the chunk sweep (csrc/chunk.hip: k_chunk_sweep) - a run's first and last node, the run without a left
or a right separator, and the per-node choice between the constant coupling table and the evaluated one - against the block cyclic
reduction over the whole chain (chunk_nodes = -1), as tests/test_gpu_chunk.py::test_chunk_sweep_equals_block_cyclic_reduction does
for n >= 24: five LM steps from a perturbed start, status 0, equal accept decisions, 1e-9."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 1e-9
STEPS = 5


@pytest.fixture(scope="module")
def mods(gpu_lib):
    from acinoset_amd import fte, synth
    return fte, synth


def _start(fte, seq, n, seed, sigma=0.02):
    x0 = np.zeros((n, 45))
    x0[:, fte.ACTIVE] = seq["q_true"][:, fte.ACTIVE] + np.random.default_rng(seed).normal(0, sigma, (n, 25))
    lo, hi = fte.bounds45()
    return np.clip(x0, lo, hi)[:, fte.ACTIVE]


def _trial(ctx):
    from acinoset_amd._lib import check, lib, ptr, stream_ptr
    buf = torch.empty((ctx.N, 25), dtype=torch.float64, device=ctx.device)
    which = 0 if ctx.state()["last_accept"] else 1          # after an accepted step the trial became the current iterate
    check(lib().acino_fte_copy_frames(ctx._h, which, 0, 0, ctx.N, ptr(buf), stream_ptr()))
    return buf.cpu().numpy()


def _walk(fte, det, rig, Ts, xa, **kw):
    ctx = fte.FTEContext(det, *rig, Ts, ftol=0.0, xtol=0.0, gtol=0.0, clamp_lambda=True, **kw)
    ctx.set_x(xa)
    out = []
    for _ in range(STEPS):
        ctx.step()
        st = ctx.state()
        out.append((st["cost_trial"], st["last_accept"], st["pred"], st["status"], _trial(ctx)))
    ctx.close()
    return out


def _same_walk(ref, got):
    for it, (r, g) in enumerate(zip(ref, got)):
        assert g[3] == 0 and r[3] == 0, (it, g[3], r[3])
        assert g[1] == r[1], f"iteration {it}: accept decisions differ"
        assert abs(g[0] - r[0]) <= 0.1 * TOL * abs(r[0]), (it, g[0], r[0])
        assert abs(g[2] - r[2]) <= 10 * TOL * abs(r[2]) + 1e-14, (it, g[2], r[2])
        assert np.abs(g[4] - r[4]).max() < TOL, (it, float(np.abs(g[4] - r[4]).max()))


class _Refs:
    """One problem and one whole-chain walk per key, shared by the run lengths that are held against it."""

    def __init__(self):
        self.made = {}

    def get(self, key, make):
        if key not in self.made:
            self.made[key] = make()
        return self.made[key]


@pytest.fixture(scope="module")
def refs():
    return _Refs()


def _sequence_case(fte, synth, n):
    seq = synth.make_sequence(n, "sprint")
    rig = (seq["K"], seq["D"], seq["R"], seq["t"])
    xa = _start(fte, seq, n, n)
    return seq["det"], rig, seq["Ts"], xa, _walk(fte, seq["det"], rig, seq["Ts"], xa, chunk_nodes=-1)


# The end of the sequence at every offset from the last full run, one frame at a time: 24 .. 9 m + 9 frames are 8 .. 3 m + 3
# nodes, i.e. last runs of every length up to m + 1 nodes with a full, a two-frame and a one-frame last node; runs of one interior node (m = 2: the
# first node is the last); the first run (no left separator) and the last (no right separator).
@pytest.mark.parametrize("m,n", [(m, n) for m in (2, 3, 4) for n in range(24, 9 * m + 10)])
def test_sequence_end_against_run_boundary(mods, refs, m, n):
    fte, synth = mods
    det, rig, Ts, xa, ref = refs.get(("seq", n), lambda: _sequence_case(fte, synth, n))
    _same_walk(ref, _walk(fte, det, rig, Ts, xa, chunk_nodes=m))


def _clip_case(fte, synth, clip_len, n=60):
    seq = synth.make_sequence(clip_len, "sprint")
    rig = (seq["K"], seq["D"], seq["R"], seq["t"])
    reps = n // clip_len
    det = np.concatenate([seq["det"]] * reps, 0)
    xa = np.concatenate([_start(fte, seq, clip_len, 100 * clip_len + s) for s in range(reps)], 0)
    return det, rig, seq["Ts"], xa, _walk(fte, det, rig, seq["Ts"], xa, chunk_nodes=-1, clip_len=clip_len)


# Clip ends inside nodes (20), on node boundaries (12, 15, 30), inside runs and on run boundaries: nodes whose table is the constant
# one and nodes whose table is evaluated alternate within one run
@pytest.mark.parametrize("m", [2, 3, 5])
@pytest.mark.parametrize("clip_len", [12, 15, 20, 30])
def test_clips(mods, refs, clip_len, m):
    fte, synth = mods
    det, rig, Ts, xa, ref = refs.get(("clip", clip_len), lambda: _clip_case(fte, synth, clip_len))
    _same_walk(ref, _walk(fte, det, rig, Ts, xa, chunk_nodes=m, clip_len=clip_len))


def _window_case(fte, synth, n, kw):
    seq = synth.make_sequence(n, "sprint")
    rig = (seq["K"], seq["D"], seq["R"], seq["t"])
    xa = _start(fte, seq, n, 1000 + n)
    return seq["det"], rig, seq["Ts"], xa, _walk(fte, seq["det"], rig, seq["Ts"], xa, chunk_nodes=-1, **kw)


# A window inside a longer sequence: its end interior to the sequence with a full last node (60 frames), with one and with two
# live frames in the last node (61, 62), and a window that ends with the sequence
WINDOWS = {"interior-end": (60, dict(n_global=400, n_offset=120)),
           "one-live-frame": (61, dict(n_global=400, n_offset=120)),
           "two-live-frames": (62, dict(n_global=400, n_offset=121)),
           "sequence-end": (61, dict(n_global=400, n_offset=339))}


@pytest.mark.parametrize("m", [2, 3, 4])
@pytest.mark.parametrize("name", list(WINDOWS))
def test_window_inside_a_longer_sequence(mods, refs, name, m):
    fte, synth = mods
    n, kw = WINDOWS[name]
    det, rig, Ts, xa, ref = refs.get(("win", name), lambda: _window_case(fte, synth, n, kw))
    _same_walk(ref, _walk(fte, det, rig, Ts, xa, chunk_nodes=m, **kw))
