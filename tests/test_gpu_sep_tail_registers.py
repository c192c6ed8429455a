"""GPU (-m gpu): k_sep_tail - the one-launch truncated solve, refinement sweeps and back-substitution of the separator chain,
its matrix parts held in registers and its row sums added across lanes - against the per-launch kernels of the same
iteration (k_bcr_backsub / k_bcr_refine, reached with ACINO_SEP_TAIL_CAPACITY=1: a device with room for one workgroup).

Both run the same block-Jacobi iteration on the same reduced chain, so a walk of LM steps must take the same decisions and
produce the same trial iterate to rounding; the tolerances are those of
test_gpu_chunk.py::test_separator_tail_falls_back_to_the_per_level_kernels_on_a_device_that_cannot_hold_it.

Sizes.  Runs of 14 nodes (42 frames) and one reduction level: the separators at even positions of the chain are level nodes,
those at odd positions stay isolated, and the schedule only truncates when MORE than one node is left (BcrSchedule::build:
R > 1) - a chain of 2 or 3 separators leaves one and is reduced completely, by the same kernels on both sides, so "one
isolated node without a neighbour" does not exist.  The smallest chains of each shape the kernel distinguishes:
  170 frames,  4 separators: isolated 1, 3 (each with ONE isolated neighbour); level nodes 0 (no left neighbour) and 2
  212 frames,  5 separators: isolated 1, 3; level nodes 0, 2, 4 - a level node without a neighbour on either end
  301 frames,  7 separators: isolated 1, 3, 5 (the middle one with both neighbours); level nodes 0, 2, 4, 6
  600 frames, 14 separators: isolated 1 .. 13 (seven: more than one interior node); level nodes 0 .. 12
Every case asserts that split (fte.solver_plan, the level count that was asked for) and that the two walks did run the two
sets of kernels (launch counts), so none can fall to the complete reduction unnoticed.

Sweeps 1, 2, 3, 4, 7: the norms that feed trunc_eps are different outputs for 1, 2, 3 and >= 4 sweeps.  trunc_tol = 1: the
bound k_totals forms from them is <= 1 by construction (rho / (1 - rho) |update| / |x| with rho <= 1/2, else 1), and one sweep
leaves far more than the default tolerance - with 1 no step is refused for the SIZE of the bound and every step is compared;
the reference must end every step with status 0 before anything is held against it."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CHUNK_NODES = 14
# frames -> (separators, isolated nodes)
SPLITS = {170: (4, 2), 212: (5, 2), 301: (7, 3), 600: (14, 7)}
STEPS = 4


@pytest.fixture(scope="module")
def mods(gpu_lib):
    from acinoset_amd import fte, synth
    return fte, synth


@functools.lru_cache(maxsize=None)
def _sequence(n):
    from acinoset_amd import fte, synth
    seq = synth.make_sequence(n, "loop")
    x0 = np.zeros((n, 45))
    x0[:, fte.ACTIVE] = seq["q_true"][:, fte.ACTIVE] + np.random.default_rng(5 * n).normal(0, 0.02, (n, 25))
    lo, hi = fte.bounds45()
    return seq, np.clip(x0, lo, hi)[:, fte.ACTIVE]


def _trial(ctx):
    """The trial iterate of the last step (frames x 25), through the C ABI."""
    from acinoset_amd._lib import check, lib, ptr, stream_ptr
    buf = torch.empty((ctx.N, 25), dtype=torch.float64, device=ctx.device)
    which = 0 if ctx.state()["last_accept"] else 1        # after an accepted step the trial became the current iterate
    check(lib().acino_fte_copy_frames(ctx._h, which, 0, 0, ctx.N, ptr(buf), stream_ptr()))
    return buf.cpu().numpy()


def _walk(fte, n, sweeps):
    """STEPS LM steps; per step (trial cost, accepted, status, trunc_eps, trial iterate), then the launches of one more step."""
    seq, xa = _sequence(n)
    ctx = fte.FTEContext(seq["det"], seq["K"], seq["D"], seq["R"], seq["t"], seq["Ts"], ftol=0.0, xtol=0.0, gtol=0.0,
                         clamp_lambda=True, chunk_nodes=CHUNK_NODES, bcr_levels=1, refine_sweeps=sweeps, trunc_tol=1.0)
    plan = fte.solver_plan(ctx.params)
    n_sep, n_iso = SPLITS[n]
    assert plan["m"] == CHUNK_NODES and plan["n_sep"] == n_sep and n_sep // 2 == n_iso > 1 and plan["levels"] > 1, plan
    assert ctx.params.bcr_levels == 1 and ctx.params.refine_sweeps == sweeps
    ctx.set_x(xa)
    out = []
    for _ in range(STEPS):
        ctx.step()
        st = ctx.state()
        out.append((st["cost_trial"], st["last_accept"], st["status"], st["trunc_eps"], _trial(ctx)))
    ctx.profile_begin()
    ctx.step()
    launches = {k: v["launches"] for k, v in ctx.profile_end().items()}
    ctx.close()
    return out, launches


def _compare(fte, monkeypatch, n, sweeps):
    monkeypatch.setenv("ACINO_SEP_TAIL_CAPACITY", "1")
    ref, l_ref = _walk(fte, n, sweeps)
    monkeypatch.delenv("ACINO_SEP_TAIL_CAPACITY")
    got, l_got = _walk(fte, n, sweeps)
    # the reference is the per-launch set (one refinement launch per sweep after the truncated solve's), the other the one launch
    assert l_ref.get("refine", 0) == sweeps and l_ref.get("backsub", 0) >= 1, l_ref
    assert l_got.get("refine", 0) == 1 and l_got.get("backsub", 0) < l_ref["backsub"], (l_got, l_ref)
    for it, r in enumerate(ref):
        assert r[2] == 0 and 0.0 <= r[3] <= 1.0, (it, r[2], r[3])
    for it, (r, g) in enumerate(zip(ref, got)):
        print(f"n={n} sweeps={sweeps} step {it}: cost {r[0]:.15e} / {g[0]:.15e}, accepted {r[1]} / {g[1]}, trunc_eps {r[3]:.3e} / "
              f"{g[3]:.3e}, max |d trial| {float(np.abs(g[4] - r[4]).max()):.3e}")
        assert g[2] == 0 and g[1] == r[1], (it, g[2], g[1], r[1])
        assert abs(g[0] - r[0]) <= 1e-11 * abs(r[0]), (it, g[0], r[0])
        assert np.abs(g[4] - r[4]).max() < 1e-10, (it, float(np.abs(g[4] - r[4]).max()))
        assert 0.0 <= g[3] <= 1.0, (it, g[3])


@pytest.mark.parametrize("sweeps", [1, 2, 3, 4, 7])
@pytest.mark.parametrize("n", sorted(SPLITS))
def test_sep_tail_equals_the_per_launch_kernels(mods, monkeypatch, n, sweeps):
    """Fused narrow levels (the default): the isolated nodes are factored inside k_sep_tail and solved with G = D^-1."""
    fte, _synth = mods
    _compare(fte, monkeypatch, n, sweeps)


def test_sep_tail_equals_the_per_launch_kernels_without_fused_levels(mods, monkeypatch):
    """ACINO_NO_FUSED_LEVELS=1: the per-phase reduction leaves the factor U, and a sweep is U (U^T t) - two triangular products."""
    fte, _synth = mods
    monkeypatch.setenv("ACINO_NO_FUSED_LEVELS", "1")
    _compare(fte, monkeypatch, 301, 7)
