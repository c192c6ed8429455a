"""GPU (-m gpu): the chunk sweep (csrc/chunk.hip: k_chunk_sweep) where waves change roles at the ends of a run - the first node's
factorisation, whose helper U is a strip wave for that one call, and the last node of a run with a left separator, where two D
waves take a strip of the spike each and six tiles of the left separator's update change owner through memory - held to the
block cyclic reduction over the whole chain
(chunk_nodes = -1) with the walk of tests/test_gpu_sweep_ends.py (five LM steps from a perturbed "sprint" start: status 0, equal
accept decisions, cost to 1e-10 relative, trial iterate to 1e-9, `pred` as there), and to itself bit for bit over repeated walks
in fresh contexts: a role that changes waves changes no operand and no instruction, so a difference between two walks is a lost
hand-over between waves.

Pinned contexts (pin_left / pin_right) are the ranks of a sharded solve: a step of such a context needs its neighbours'
separators, and the whole-chain reference for them is the sharded driver of tests/test_gpu_parity.py, not a walk of one
context - no case of this file pins an end.  A last run of m + 1 nodes exists only under a right pin (ChunkPlan::build) and is
covered there for the same reason; without a pin the longest last run has m nodes, all interior, one more than any other run
eliminates - every length 1 .. m is here."""
import numpy as np
import pytest

from test_gpu_sweep_ends import _Refs, _same_walk, _sequence_case, _start, _trial, _walk, _clip_case, _window_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mods(gpu_lib):
    from acinoset_amd import fte, synth
    return fte, synth


@pytest.fixture(scope="module")
def refs():
    return _Refs()


def _run_end_cases(ms=(2, 3, 4, 5), lo=24, hi=48):
    """(m, n): per run length the first frame count in lo .. hi for every pair (nodes of the last run 1 .. m, live frames of the
    last node 1 .. 3).  m = 2: the first node of a run is its last; m = 3: a first and a last node only; a last run of one node
    is the run whose only node is first and last and has no right separator; the first run has only the right-hand side strip."""
    out = []
    for m in ms:
        seen = set()
        for n in range(lo, hi + 1):
            nodes = (n + 2) // 3
            key = (nodes - (-(-nodes // m) - 1) * m, n - 3 * (nodes - 1))
            if key not in seen:
                seen.add(key)
                out.append((m, n))
        assert len(seen) == 3 * m, (m, sorted(seen))
    return out


@pytest.mark.parametrize("m,n", _run_end_cases())
def test_every_combination_of_run_ends(mods, refs, m, n):
    fte, synth = mods
    det, rig, Ts, xa, ref = refs.get(("seq", n), lambda: _sequence_case(fte, synth, n))
    _same_walk(ref, _walk(fte, det, rig, Ts, xa, chunk_nodes=m))


# clip ends on node boundaries (15) and inside nodes (20): evaluated coupling tables at first and last nodes of runs
@pytest.mark.parametrize("m", [3, 4])
@pytest.mark.parametrize("clip_len", [15, 20])
def test_clips(mods, refs, clip_len, m):
    fte, synth = mods
    det, rig, Ts, xa, ref = refs.get(("clip", clip_len), lambda: _clip_case(fte, synth, clip_len))
    _same_walk(ref, _walk(fte, det, rig, Ts, xa, chunk_nodes=m, clip_len=clip_len))


# a window inside a longer sequence, one live frame in its last node
@pytest.mark.parametrize("m", [2, 3, 4, 5])
def test_window_inside_a_longer_sequence(mods, refs, m):
    fte, synth = mods
    kw = dict(n_global=400, n_offset=120)
    det, rig, Ts, xa, ref = refs.get("win", lambda: _window_case(fte, synth, 61, kw))
    _same_walk(ref, _walk(fte, det, rig, Ts, xa, chunk_nodes=m, **kw))


def _walk10(fte, det, rig, Ts, xa, graph, **kw):
    ctx = fte.FTEContext(det, *rig, Ts, ftol=0.0, xtol=0.0, gtol=0.0, clamp_lambda=True, **kw)
    if graph:
        ctx.enable_graph(True)
    ctx.set_x(xa)
    out = []
    for _ in range(10):
        ctx.step()
        st = ctx.state()
        assert st["status"] == 0, st
        out.append((st["cost_trial"], st["cost"], _trial(ctx)))
    ctx.close()
    return out


# 190 frames in automatic runs (64 nodes in runs of 4), 60 frames in runs of 3: 20 walks of 10 steps, each in a fresh context
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("n,m", [(190, 0), (60, 3)])
def test_walks_repeat_bit_for_bit(mods, n, m, graph):
    fte, synth = mods
    seq = synth.make_sequence(n, "sprint")
    rig = (seq["K"], seq["D"], seq["R"], seq["t"])
    xa = _start(fte, seq, n, n)
    first = _walk10(fte, seq["det"], rig, seq["Ts"], xa, graph, chunk_nodes=m)
    for rep in range(1, 20):
        got = _walk10(fte, seq["det"], rig, seq["Ts"], xa, graph, chunk_nodes=m)
        for it, (f, g) in enumerate(zip(first, got)):
            assert f[0] == g[0] and f[1] == g[1], (rep, it, f[0], g[0], f[1], g[1])
            assert np.array_equal(f[2], g[2]), (rep, it, float(np.abs(f[2] - g[2]).max()))
