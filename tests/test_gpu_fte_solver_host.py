"""GPU (-m gpu): the graph handling of the FTE solver's host layer (csrc/fte_api.hip: GraphSlot, replay, drop_graphs).  A
replayed LM step is the eager launch sequence, so a context that replays walks the trajectory of an eager twin bit for bit;
a capture belongs to one stream and is made again on another; whatever changes a captured kernel argument
(`acino_fte_set_precision`, `acino_fte_debug_stamps`) drops every capture and the next step captures again."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

STEP_GRAPH = 16          # bit of the single-shard step in acino_fte_graphs_active (bits 0..3: the four sharded phases)
STATE_KEYS = ("cost", "cost_trial", "lam", "iter", "accepted")
# the smallest shapes of test_gpu_chunk.py with several runs, a whole-chain reduction and the automatic plan
SHAPES = [(24, 2), (59, -1), (100, 0)]


@pytest.fixture(scope="module")
def mods(gpu_lib):
    from acinoset_amd import fte, synth
    return fte, synth


@pytest.fixture(scope="module")
def problems(mods):
    """Per shape: detections, rig, Ts and a perturbed start, built once and only read."""
    fte, synth = mods
    out = {}
    for n, m in SHAPES:
        seq = synth.make_sequence(n, "sprint")
        x0 = np.zeros((n, 45))
        x0[:, fte.ACTIVE] = seq["q_true"][:, fte.ACTIVE] + np.random.default_rng(n).normal(0, 0.02, (n, 25))
        lo, hi = fte.bounds45()
        out[n] = (seq["det"], (seq["K"], seq["D"], seq["R"], seq["t"]), seq["Ts"], np.clip(x0, lo, hi)[:, fte.ACTIVE], m)
    return out


def _pair(fte, problem, stream):
    """An eager context and one with the graph replay on, at the same start, both living on `stream`."""
    det, rig, Ts, xa, m = problem
    pair = []
    with torch.cuda.stream(stream):
        for graph in (False, True):
            ctx = fte.FTEContext(det, *rig, Ts, ftol=0.0, xtol=0.0, gtol=0.0, clamp_lambda=True, chunk_nodes=m)
            ctx.enable_graph(graph)
            ctx.set_x(xa)
            pair.append(ctx)
    return pair


def _snapshot(ctx):
    st = ctx.state()
    return ctx.result()[0].cpu().numpy(), tuple(st[k] for k in STATE_KEYS), st["status"]


def _step_both_and_compare(eager, replaying, stream, steps, tag):
    for it in range(steps):
        with torch.cuda.stream(stream):
            eager.step()
            replaying.step()
            assert replaying.graphs_active() == STEP_GRAPH and eager.graphs_active() == 0, (tag, it)
            (xe, se, status_e), (xr, sr, status_r) = _snapshot(eager), _snapshot(replaying)
        print(f"{tag} step {it}: max |x_replay - x_eager| = {float(np.abs(xr - xe).max()):.3e}, state eager {se}, replay {sr}")
        assert status_e == 0 and status_r == 0, (tag, it, status_e, status_r)
        assert sr == se, (tag, it, se, sr)
        assert np.array_equal(xr, xe), (tag, it, float(np.abs(xr - xe).max()))


@pytest.mark.parametrize("n", [n for n, _m in SHAPES])
def test_graph_replay_equals_eager(mods, problems, n):
    """Five steps from the same start on a side stream, eager against replayed: iterate and (cost, cost_trial, lam, iter,
    accepted) bit for bit after every step (equal bits on the commit before this layer, too: no tolerance)."""
    fte, _synth = mods
    side = torch.cuda.Stream()
    eager, replaying = _pair(fte, problems[n], side)
    _step_both_and_compare(eager, replaying, side, 5, f"n={n}")
    with torch.cuda.stream(side):
        assert replaying.state()["iter"] == 5
        eager.close()
        replaying.close()
    torch.cuda.synchronize()


def test_recapture_on_another_stream_and_invalidation(mods, problems):
    from acinoset_amd._lib import check, lib
    fte, _synth = mods
    first, second = torch.cuda.Stream(), torch.cuda.Stream()
    twin, ctx = _pair(fte, problems[24], first)
    _step_both_and_compare(twin, ctx, first, 2, "first stream")
    torch.cuda.synchronize()
    # a capture belongs to its stream: stepping on another one captures again and goes on where the twin goes
    _step_both_and_compare(twin, ctx, second, 2, "second stream")
    # the assembly kernel is chosen on the host and baked into the capture: set_precision drops it, even to the same precision
    check(lib().acino_fte_set_precision(ctx._h, fte.PRECISIONS["f64"]))
    assert ctx.graphs_active() == 0
    _step_both_and_compare(twin, ctx, second, 1, "after set_precision")
    # ... and so are the stamp pointers of the chains (this line does not hold before the host layer had ONE invalidation)
    check(lib().acino_fte_debug_stamps(ctx._h, None))
    assert ctx.graphs_active() == 0
    _step_both_and_compare(twin, ctx, second, 1, "after debug_stamps")
    with torch.cuda.stream(second):
        twin.close()
        ctx.close()
    torch.cuda.synchronize()


def test_no_capture_keeps_stamping_after_the_stamps_are_switched_off(mods, problems):
    """A step captured while the stamps were on wrote them on every replay; switching them off must reach the capture."""
    from acinoset_amd._lib import check, lib, ptr
    fte, _synth = mods
    side = torch.cuda.Stream()
    twin, ctx = _pair(fte, problems[24], side)
    with torch.cuda.stream(side):
        dbg = torch.zeros(72, dtype=torch.int64, device="cuda")       # ACINO_DEBUG_STAMP_ENTRIES; workgroup 0, node / level 0
        side.synchronize()
        check(lib().acino_fte_debug_stamps(ctx._h, ptr(dbg)))
        ctx.step()
        side.synchronize()
        assert ctx.graphs_active() == STEP_GRAPH
        stamped = int((dbg[:64] != 0).sum().item())
        print(f"stamps written by the captured step: {stamped}")
        assert stamped > 0
        check(lib().acino_fte_debug_stamps(ctx._h, None))
        dbg.zero_()
        ctx.step()
        side.synchronize()
        assert ctx.graphs_active() == STEP_GRAPH
        assert int((dbg != 0).sum().item()) == 0
        twin.close()
        ctx.close()
    torch.cuda.synchronize()
