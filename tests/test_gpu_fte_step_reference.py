"""GPU (-m gpu): the linear solve of the FTE step on EVERY solver path against a banded reference that is not a GPU kernel.

Before each LM step the device's own iterate, gradient, Gauss-Newton blocks and damping are read back; tests/fte_step_ref.py
solves that damped system on the CPU (fp64 banded Cholesky, then iterative refinement with a long-double residual) and the
step the device took - its solution vector, trial iterate, predicted reduction and step length - is held against it.  The
assembly is not part of the comparison (test_gpu_parity.py::test_fte_cost_gradient_hessian covers it); what is, is the chunk
sweep, k_sep_combine, the separator reduction (k_sep_level or the per-phase kernels of bcr.hip), k_sep_tail / k_bcr_refine with
the truncated solve and the block-Jacobi sweeps, and k_chunk_backsub with the folded trial, pred and step sums.

Every case asserts the path it is there for (fte.solver_plan, the reduction levels and sweeps the context resolved, the launch
counts of one profiled step), so a later scheduling change cannot move it onto another path unnoticed.

Tolerances.  The reference supplies the scale: e_lapack = |delta_lapack - delta_ref|_inf, what plain fp64 LAPACK is off by, and
eta_lapack, LAPACK's normwise backward error on the same system.  Asserted per step:
    e_gpu   <= K max(e_lapack, 2^-52 |delta_ref|_inf) + t
    eta_gpu <= K eta_lapack + t_eta
with t = trunc_eps |x_sep|_inf on truncated paths (the device's own bound times the max norm of the separators' solution; 0 on
complete reductions) and t_eta = |A|_inf t / (|A|_inf |delta|_inf + |rhs|_inf), the same allowance in backward-error form.
pred and step_inf use the same K on the reference's own sensitivity (the difference between the quantity at delta_lapack and at
delta_ref; floors: one rounding of the summed magnitudes / of the step).  The trial iterate is fl(x + delta): it is allowed one
rounding of x, 2^-52 |x|_inf, on top.

MEASURED (MI355X; the table of every case and step is in NOTES_perf.md, "FTE step against the banded reference").  Worst
e_gpu / max(e_lapack, 2^-52 |delta|) and eta_gpu / eta_lapack over the steps of each case:
    complete reductions                 e     eta        truncated + 7 sweeps                e     eta
    whole_chain_301                    3.6   18.2        default_999                       23.1  124.9
    chunked_short_190                 40.9   31.5        default_3331                      38.1  156.9
    fused_complete_999                23.1   22.9        default_10000                     18.4  162.4
    fused_complete_1000                7.3   23.4        per_level_3331                    38.1   39.1
    per_phase_complete_999            23.1   23.0        per_phase_999                     23.1   22.9
    one_wide_level_complete_1545      15.9   26.7        one_wide_level_1545               15.9   24.0
    two_wide_levels_complete_3096     15.9   10.0        two_wide_levels_3096              15.9   10.1
                                                         shared_gpu_400                    12.6   20.2
                                                         runs_of_3 / 5 / 9 _1000    6.2 / 106.9 / 8.5   75.3 / 119.3 / 87.3
                                                         clips_5x40 / 5x45               12.3 / 20.8  105.2 / 131.3
                                                         bound_active_400 / runs_of_2     11.0 / 9.0   19.4 / 15.0
K = 256: the next power of two at or above 4 x 40.9, the worst ratio of the complete reductions (fte_step_ref.K_GPU).
Two things stand out and are explained by the algorithm, not by a kernel:
  * k_sep_tail behind fused levels solves the isolated nodes with the explicit inverse G = D^-1: the same forward error as
    the complete reduction, a backward error 5 times larger at lam = 1e-6 (default_* against per_phase_999 / per_level_3331).
  * a chain whose last node holds one frame (190, 1000 frames) in a last run of more than two nodes: the error sits in the
    last two nodes, 10 to 50 times the median node's.  The marginal block of the lone last frame is what is left of a
    cancellation (smoothness weights ~1e9 against ~1e5 of its measurements) and inherits the error of the explicit inverse of
    its neighbour; a numpy elimination of the same system node by node with G = U U^T shows the same figures (1.8e-12 at the
    last node of 1000 frames, 2e-13 at 999 frames), with Cholesky solves in place of the inverses it does not (2e-14).
"""
import contextlib
import functools
import hashlib
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import fte as ofte

import fte_step_ref as ref

K_TOL = ref.K_GPU   # 256: see MEASURED in the module docstring
SWEEPS = 7          # FTEContext.REFINE_SWEEPS
EPS = 2.0 ** -52

# name -> frames, kind of sequence, start, context keywords, environment, and the path:
#   m / n_sep: fte.solver_plan;  levels: reduction levels the context resolved (0: complete);  launches (added below): launch
#   counts of one profiled step
CASES = {
    "whole_chain_301": dict(n=301, kw=dict(chunk_nodes=-1, bcr_levels=0), m=0, n_sep=0, levels=0),
    "chunked_short_190": dict(n=190, kw={}, m=4, n_sep=15, levels=0),
    "fused_complete_999": dict(n=999, kw=dict(bcr_levels=0), m=4, n_sep=83, levels=0),
    "fused_complete_1000": dict(n=1000, kw=dict(bcr_levels=0), m=4, n_sep=83, levels=0),
    "default_999": dict(n=999, kw={}, m=4, n_sep=83, levels=3),
    "default_3331": dict(n=3331, kw={}, m=5, n_sep=222, levels=3),
    "default_10000": dict(n=10000, kw={}, m=14, n_sep=238, levels=1),
    "per_level_3331": dict(n=3331, kw={}, env=dict(ACINO_SEP_TAIL_CAPACITY="1"), m=5, n_sep=222, levels=3),
    "per_phase_999": dict(n=999, kw={}, env=dict(ACINO_NO_FUSED_LEVELS="1"), m=4, n_sep=83, levels=3),
    "per_phase_complete_999": dict(n=999, kw=dict(bcr_levels=0), env=dict(ACINO_NO_FUSED_LEVELS="1"), m=4, n_sep=83, levels=0),
    "one_wide_level_1545": dict(n=1545, kw=dict(chunk_nodes=2), m=2, n_sep=257, levels=4),
    "one_wide_level_complete_1545": dict(n=1545, kw=dict(chunk_nodes=2, bcr_levels=0), m=2, n_sep=257, levels=0),
    "two_wide_levels_3096": dict(n=3096, kw=dict(chunk_nodes=2), m=2, n_sep=515, levels=4),
    "two_wide_levels_complete_3096": dict(n=3096, kw=dict(chunk_nodes=2, bcr_levels=0), m=2, n_sep=515, levels=0),
    "shared_gpu_400": dict(n=400, kw=dict(shared_gpu=True), m=4, n_sep=33, levels=3),
    "runs_of_3_1000": dict(n=1000, kw=dict(chunk_nodes=3), m=3, n_sep=111, levels=4),
    "runs_of_5_1000": dict(n=1000, kw=dict(chunk_nodes=5), m=5, n_sep=66, levels=3),
    "runs_of_9_1000": dict(n=1000, kw=dict(chunk_nodes=9), m=9, n_sep=37, levels=2),
    "clips_5x40": dict(n=200, clip=40, kw=dict(clip_len=40), m=4, n_sep=16, levels=3),
    "clips_5x45": dict(n=225, clip=45, kw=dict(clip_len=45), m=4, n_sep=18, levels=3),
    "bound_active_400": dict(n=400, kind="sprint", start="line", kw={}, m=4, n_sep=33, levels=3),
    "bound_active_runs_of_2_400": dict(n=400, kind="sprint", start="line", kw=dict(chunk_nodes=2), m=2, n_sep=66, levels=4),
}

# The launches of one step that tell the paths apart, (profiler class, low, high) - high None: no upper limit.
_CHUNKED = [("chunk_sweep", 1, 1), ("chunk_backsub", 1, 1), ("trial", 0, 0), ("backsub0", 0, 0)]
_FUSED = _CHUNKED + [("elim_deep", 1, None), ("elim", 0, 0), ("update", 0, 0), ("update_deep", 0, 0)]      # k_sep_level only
_TAIL = [("refine", 1, 1), ("backsub", 0, 0), ("backsub_tail", 0, 0)]                  # k_sep_tail: one launch
_PER_LEVEL = [("refine", SWEEPS, SWEEPS), ("backsub", 1, None)]                        # k_bcr_backsub, one k_bcr_refine per sweep
_COMPLETE = [("refine", 0, 0), ("backsub_tail", 1, 1)]
_PER_PHASE = _CHUNKED + [("update_deep", 1, None), ("elim", 0, 0), ("update", 0, 0)]   # k_bcr_elim_deep / k_bcr_update_deep
_WHOLE = [("chunk_sweep", 0, 0), ("chunk_backsub", 0, 0), ("elim", 1, 1), ("update0", 1, 1), ("elim_deep", 1, None),
          ("update_deep", 1, None), ("backsub0", 1, 1), ("backsub_tail", 1, 1), ("trial", 1, 1), ("refine", 0, 0)]
# wide levels (more than 128 picks) run k_bcr_elim after k_sep_combine has folded the runs' AL into D / b; two of them: the
# second's Schur products by k_bcr_update.  (Behind them the truncated cases take k_sep_tail or the per-level kernels,
# whichever the device holds: not asserted.)
_WIDE1 = _CHUNKED + [("elim", 1, 1), ("update", 0, 0), ("sep_combine", 1, None), ("elim_deep", 1, None)]
_WIDE2 = _CHUNKED + [("elim", 2, 2), ("update", 1, 1), ("sep_combine", 1, None), ("elim_deep", 1, None)]
for _name, _launches in {
        "whole_chain_301": _WHOLE, "chunked_short_190": _FUSED + _COMPLETE, "fused_complete_999": _FUSED + _COMPLETE,
        "fused_complete_1000": _FUSED + _COMPLETE, "default_999": _FUSED + _TAIL, "default_3331": _FUSED + _TAIL,
        "default_10000": _FUSED + _TAIL, "per_level_3331": _FUSED + _PER_LEVEL + [("sep_combine", 1, 1)],
        "per_phase_999": _PER_PHASE + _TAIL, "per_phase_complete_999": _PER_PHASE + _COMPLETE,
        "one_wide_level_1545": _WIDE1, "one_wide_level_complete_1545": _WIDE1 + _COMPLETE, "two_wide_levels_3096": _WIDE2,
        "two_wide_levels_complete_3096": _WIDE2 + _COMPLETE,
        "shared_gpu_400": _FUSED + _PER_LEVEL + [("backsub_tail", 0, 0), ("sep_combine", 1, 1)],
        "runs_of_3_1000": _FUSED + _TAIL, "runs_of_5_1000": _FUSED + _TAIL, "runs_of_9_1000": _FUSED + _TAIL,
        "clips_5x40": _FUSED + _TAIL, "clips_5x45": _FUSED + _TAIL, "bound_active_400": _FUSED + _TAIL,
        "bound_active_runs_of_2_400": _FUSED + _TAIL}.items():
    CASES[_name]["launches"] = _launches
assert all("launches" in c for c in CASES.values())


@pytest.fixture(scope="module")
def mods(gpu_lib):
    from acinoset_amd import fte, synth
    return fte, synth


@functools.lru_cache(maxsize=None)
def _sequence(n, kind, seed=None):
    from acinoset_amd import synth
    return synth.make_sequence(n, kind) if seed is None else synth.make_sequence(n, kind, seed=seed)


def _noisy(fte, q_true, seed, sigma=0.02):
    n = q_true.shape[0]
    x0 = np.zeros((n, 45))
    x0[:, fte.ACTIVE] = q_true[:, fte.ACTIVE] + np.random.default_rng(seed).normal(0, sigma, (n, 25))
    lo, hi = fte.bounds45()
    return np.clip(x0, lo, hi)[:, fte.ACTIVE]


@functools.lru_cache(maxsize=None)
def _inputs(n, kind, start, clip):
    """(det, rig, Ts, start iterate [n, 25], the oracle problem - one per clip in the clip form)."""
    from acinoset_amd import fte
    if clip:
        seqs = [_sequence(clip, ("sprint", "trot", "loop")[i % 3], 4242 + i) for i in range(n // clip)]
        det = np.concatenate([s["det"] for s in seqs])
        xa = np.concatenate([_noisy(fte, s["q_true"], 11 * clip + i) for i, s in enumerate(seqs)])
    else:
        seqs = [_sequence(n, kind)]
        det = seqs[0]["det"]
    s0 = seqs[0]
    rig = (s0["K"], s0["D"], s0["R"], s0["t"])
    if not clip:
        if start == "line":       # the reference's nose-line start: every angle 0, four of them ON their 0.0 bounds
            xa = fte.nose_line_init(det, *rig, 0.5)[:, fte.ACTIVE]
        else:
            xa = _noisy(fte, s0["q_true"], 7 * n)
    probs = [ofte.FTEProblem(s["det"][..., :2], s["det"][..., 2], *rig, s["Ts"]) for s in seqs]
    return det, rig, s0["Ts"], xa, (probs if clip else probs[0])


_REFS = {}


def _reference(prob, x, g, h, lam, share):
    """step_reference, computed once for the systems several cases share (step 0: the same start, the same assembly)."""
    if not share:
        return ref.step_reference(prob, x, g, h, lam)
    hh = hashlib.blake2b(digest_size=16)
    for a in (x, g, h, np.float64(lam)):
        hh.update(np.ascontiguousarray(a).tobytes())
    key = hh.digest()
    if key not in _REFS:
        _REFS[key] = ref.step_reference(prob, x, g, h, lam)
    return _REFS[key]


@contextlib.contextmanager
def _environment(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _frames(ctx, which):
    from acinoset_amd._lib import check, lib, ptr, stream_ptr
    buf = torch.empty((ctx.N, 25), dtype=torch.float64, device=ctx.device)
    check(lib().acino_fte_copy_frames(ctx._h, which, 0, 0, ctx.N, ptr(buf), stream_ptr()))
    return buf.cpu().numpy()


def _solution(ctx):
    """The solution vector of the step just taken (chain.b, node by node) as [frames, 25]."""
    from acinoset_amd._lib import check, lib, ptr, stream_ptr
    T = (ctx.N + 2) // 3
    buf = torch.zeros(T * 80, dtype=torch.float64, device=ctx.device)
    check(lib().acino_fte_debug_read(ctx._h, 0, ptr(buf), T * 80, stream_ptr()))
    torch.cuda.synchronize()
    return ref.nodes_to_frames(buf.cpu().numpy(), ctx.N)


def _context(fte, name, lam0, **over):
    case = CASES[name]
    det, rig, Ts, xa, prob = _inputs(case["n"], case.get("kind", "loop"), case.get("start", "noisy"), case.get("clip", 0))
    kw = dict(case["kw"], **over)
    ctx = fte.FTEContext(det, *rig, Ts, ftol=0.0, xtol=0.0, gtol=0.0, clamp_lambda=True, lam0=lam0, **kw)
    ctx.set_x(xa)
    return ctx, prob


def _one_step(ctx, prob, profile=False, share=False):
    """One LM step and everything that is compared, as a dict of figures."""
    x = _frames(ctx, 0)
    g, h = (a.cpu().numpy() for a in ctx.grad_hess())
    st0 = ctx.state()
    lam = st0["lam"]
    if profile:
        ctx.profile_begin()
    ctx.step()
    launches = {k: v["launches"] for k, v in ctx.profile_end().items()} if profile else None
    st = ctx.state()
    trial = _frames(ctx, 0 if st["last_accept"] else 1)      # (after an accepted step the trial became the current iterate)
    d_dev = _solution(ctx)
    r = _reference(prob, x, g, h, lam, share)
    p0 = prob[0] if isinstance(prob, list) else prob
    lo, hi = p0.lo, p0.hi
    d_gpu = np.where(r.fixed, 0.0, d_dev)                      # (k_trial / k_chunk_backsub: a bound-active step is 0, exactly)
    xt_ref = np.clip(x + r.delta_ref, lo, hi)
    xt_lap = np.clip(x + r.delta_lapack, lo, hi)
    dnorm = float(np.abs(r.delta_ref).max())
    e_lapack = float(np.abs(r.delta_lapack - r.delta_ref_ld).max())
    norm_a, rhs_n = r.band.norm_inf(), float(np.abs(r.rhs).max())
    step_ref, step_lap = float(np.abs(xt_ref - x).max()), float(np.abs(xt_lap - x).max())
    return dict(
        lam=lam, status=st["status"], accepted=int(st["last_accept"]), trunc_eps=st["trunc_eps"], launches=launches,
        cost_before=st0["cost"], cost_after=st["cost"], fixed=int(r.fixed.sum()), clipped=int((xt_ref != x + r.delta_ref).sum()),
        residual_ref=r.rel_residual, refine_steps=r.refine_steps, dnorm=dnorm, xnorm=float(np.abs(x).max()),
        e_lapack=e_lapack, e_scale=max(e_lapack, EPS * dnorm), e_gpu=float(np.abs(d_gpu - r.delta_ref_ld).max()),
        e_trial=float(np.abs(trial - xt_ref).max()), e_self=float(np.abs(np.clip(x + d_gpu, lo, hi) - trial).max()),
        eta_lapack=ref.backward_error(r.band, r.rhs, r.delta_lapack), eta_gpu=ref.backward_error(r.band, r.rhs, d_gpu),
        eta_ref=ref.backward_error(r.band, r.rhs, r.delta_ref_ld),
        eta_den=norm_a / (norm_a * float(np.abs(d_gpu).max()) + rhs_n),
        pred=st["pred"], pred_ref=r.pred_ref, pred_scale=max(abs(r.pred_lapack - r.pred_ref), EPS * r.pred_abs),
        pred_slope=r.pred_slope, step_inf=st["step_inf"], step_ref=step_ref, step_lapack=step_lap,
        d_gpu=d_gpu, ref=r, x=x)


def _sep_norm(fig, nodes, n):
    f = ref.node_frames(nodes, n)
    return float(np.abs(fig["d_gpu"][f]).max()) if len(f) else 0.0


def walk(fte, name, lam0, steps):
    """``steps`` LM steps of a case; the figures of every step, the plan and the launches of the first."""
    case = CASES[name]
    with _environment(case.get("env", {})):
        ctx, prob = _context(fte, name, lam0)
        try:
            plan = fte.solver_plan(ctx.params)
            levels, sweeps = int(ctx.params.bcr_levels), int(ctx.params.refine_sweeps)
            sep = ref.separator_nodes(plan)
            out = []
            for it in range(steps):
                fig = _one_step(ctx, prob, profile=it == 0, share=it == 0)
                fig["x_sep"] = _sep_norm(fig, sep, ctx.N)
                fig["t"] = fig["trunc_eps"] * fig["x_sep"] if levels > 0 else 0.0
                out.append(fig)
        finally:
            ctx.close()
    return dict(plan=plan, levels=levels, sweeps=sweeps, launches=out[0]["launches"], steps=out)


def describe(name, lam0, it, f):
    return (f"{name} lam0={lam0:g} step {it}: lam {f['lam']:.2e} status {f['status']} acc {f['accepted']} fixed {f['fixed']} "
            f"clipped {f['clipped']} | |d| {f['dnorm']:.2e} ref residual {f['residual_ref']:.1e} eta_ref {f['eta_ref']:.1e} | e_gpu {f['e_gpu']:.2e} e_lapack "
            f"{f['e_lapack']:.2e} ratio {f['e_gpu'] / f['e_scale']:.2f} | eta_gpu {f['eta_gpu']:.2e} eta_lapack {f['eta_lapack']:.2e} "
            f"ratio {f['eta_gpu'] / f['eta_lapack']:.2f} | e_trial {f['e_trial']:.2e} e_self {f['e_self']:.2e} | pred {f['pred']:.15e} "
            f"ref {f['pred_ref']:.15e} scale {f['pred_scale']:.1e} | step {f['step_inf']:.15e} ref {f['step_ref']:.15e} | trunc_eps "
            f"{f['trunc_eps']:.2e} x_sep {f['x_sep']:.2e}")


def check_path(name, res):
    case = CASES[name]
    plan, la = res["plan"], res["launches"]
    assert (plan["m"], plan["n_sep"]) == (case["m"], case["n_sep"]), (name, plan)
    assert res["levels"] == case["levels"] and res["sweeps"] == (SWEEPS if case["levels"] else 0), (name, res["levels"], res["sweeps"])
    for cls, low, high in case.get("launches", ()):
        assert low <= la[cls] and (high is None or la[cls] <= high), (name, cls, la)


def check_step(name, lam0, it, f):
    K = K_TOL
    t = f["t"]
    assert f["status"] == 0, (name, it, f["status"])
    assert f["eta_ref"] <= f["eta_lapack"] / 64, (name, it, f["eta_ref"], f["eta_lapack"])     # the reference is one
    assert f["e_gpu"] <= K * f["e_scale"] + t, (name, it, f["e_gpu"], f["e_scale"], t)
    assert f["eta_gpu"] <= K * f["eta_lapack"] + f["eta_den"] * t, (name, it, f["eta_gpu"], f["eta_lapack"], t)
    assert f["e_trial"] <= K * f["e_scale"] + t + EPS * f["xnorm"], (name, it, f["e_trial"], f["e_scale"], t)
    assert f["e_self"] <= EPS * f["xnorm"], (name, it, f["e_self"])                  # the vector read IS the step that was taken
    assert abs(f["pred"] - f["pred_ref"]) <= K * f["pred_scale"] + f["pred_slope"] * t, (name, it, f["pred"], f["pred_ref"])
    # (a step length moves by at most the max-norm error of the step: the reference's own sensitivity is e_lapack - the
    #  difference of the two maxima themselves vanishes whenever LAPACK happens to be exact in the one largest component)
    assert abs(f["step_lapack"] - f["step_ref"]) <= f["e_scale"] + EPS * f["xnorm"]
    assert abs(f["step_inf"] - f["step_ref"]) <= K * f["e_scale"] + t + EPS * f["xnorm"], (name, it, f["step_inf"], f["step_ref"])


@pytest.mark.parametrize("lam0,steps", [(1e-3, 3), (1e-6, 1)])
@pytest.mark.parametrize("name", sorted(CASES))
def test_step_equals_the_banded_reference(mods, name, lam0, steps):
    fte, _synth = mods
    res = walk(fte, name, lam0, steps)
    for it, f in enumerate(res["steps"]):
        print(describe(name, lam0, it, f))
    print(f"{name}: plan {res['plan']} levels {res['levels']} sweeps {res['sweeps']} launches "
          f"{ {k: v for k, v in res['launches'].items() if v} }")
    check_path(name, res)
    if CASES[name].get("start") == "line":
        assert res["steps"][0]["fixed"] > 0, "the nose-line start must have bound-active variables"
    for it, f in enumerate(res["steps"]):
        check_step(name, lam0, it, f)


# ---- the device's bound on the truncation is a bound -------------------------------------------------------------------
BOUND_CASES = {"default_3331": 3, "default_10000": 1, "default_999": 3}      # case -> reduction levels (asserted)
BOUND_SWEEPS = (2, 3, 7)
BOUND_LAM0 = 1e-6      # the smallest damping of this module: the dropped couplings are largest, two sweeps leave a measurable error


def bound_figures(fte, name):
    """One step at BOUND_LAM0 with 2, 3 and 7 sweeps and with the complete reduction (key 0: the floor): per variant the true
    error of the separators' solution against the reference, the bound the device reported and the norm it is relative to.

    The norm: k_bcr_refine / k_sep_tail record, per isolated node, max |update| and max |x| over its 80 rows; k_totals takes the
    maxima over the isolated nodes and reports rho / (1 - rho) max|update| / max|x| - a bound on the max-norm error of the ISOLATED
    separators' solution (those the incomplete reduction leaves) relative to its max norm.  (Without sweeps k_bcr_trunc_check
    would report Frobenius norms of the dropped, normalised couplings instead; no case here runs it.)"""
    case = CASES[name]
    levels = BOUND_CASES[name]
    out = {}
    for sweeps in BOUND_SWEEPS + (0,):
        over = dict(bcr_levels=levels, refine_sweeps=sweeps, trunc_tol=1.0) if sweeps else dict(bcr_levels=0)
        ctx, prob = _context(fte, name, BOUND_LAM0, **over)
        try:
            plan = fte.solver_plan(ctx.params)
            assert int(ctx.params.bcr_levels) == (levels if sweeps else 0) and int(ctx.params.refine_sweeps) == sweeps
            sep = ref.separator_nodes(plan)
            iso = sep[ref.isolated_positions(len(sep), levels)]
            assert len(sep) == case["n_sep"] and len(iso) > 1
            f = _one_step(ctx, prob, share=True)
        finally:
            ctx.close()
        fi, fs = ref.node_frames(iso, case["n"]), ref.node_frames(sep, case["n"])
        err = np.abs(f["d_gpu"] - f["ref"].delta_ref_ld)
        out[sweeps] = dict(status=f["status"], trunc_eps=f["trunc_eps"], err_iso=float(err[fi].max()), err_sep=float(err[fs].max()),
                           err_all=f["e_gpu"], x_iso=float(np.abs(f["d_gpu"][fi]).max()), x_sep=float(np.abs(f["d_gpu"][fs]).max()),
                           n_iso=len(iso), e_lapack=f["e_lapack"])
    return out


@pytest.mark.parametrize("name", sorted(BOUND_CASES))
def test_truncation_bound_is_a_bound_on_the_true_error(mods, name):
    """err_true <= trunc_eps |x|_inf + floor for 2, 3 and 7 sweeps, on the isolated separators (the nodes and the max norm the
    device's bound is about, see bound_figures) and on all separators (the level nodes are back-substituted from the isolated
    ones; max norm over all separators).  The floor is the error of the same case with the complete reduction against the same
    reference (e_gpu, the max over the whole step).  More sweeps must not leave a larger error: both errors carry rounding of
    the size of the floor, so err(more) <= err(fewer) + floor."""
    fte, _synth = mods
    figs = bound_figures(fte, name)
    floor = figs[0]["err_all"]
    print(f"{name}: complete reduction: err {floor:.3e} (separators {figs[0]['err_sep']:.3e}, isolated {figs[0]['err_iso']:.3e}), "
          f"LAPACK {figs[0]['e_lapack']:.3e}")
    for s in BOUND_SWEEPS:
        f = figs[s]
        print(f"{name} sweeps {s}: status {f['status']} trunc_eps {f['trunc_eps']:.3e} | isolated ({f['n_iso']}): err {f['err_iso']:.3e} "
              f"bound {f['trunc_eps'] * f['x_iso']:.3e} | all separators: err {f['err_sep']:.3e} bound {f['trunc_eps'] * f['x_sep']:.3e}")
    for s in BOUND_SWEEPS:
        f = figs[s]
        assert f["status"] == 0 and 0.0 <= f["trunc_eps"] <= 1.0, (name, s, f)
        assert f["err_iso"] <= f["trunc_eps"] * f["x_iso"] + floor, (name, s, f, floor)
        assert f["err_sep"] <= f["trunc_eps"] * f["x_sep"] + floor, (name, s, f, floor)
    for a, b in zip(BOUND_SWEEPS[:-1], BOUND_SWEEPS[1:]):
        assert figs[b]["err_iso"] <= figs[a]["err_iso"] + floor, (name, a, b, figs[a], figs[b])
        assert figs[b]["err_sep"] <= figs[a]["err_sep"] + floor, (name, a, b, figs[a], figs[b])


def test_refused_step_leaves_iterate_and_cost_unchanged(mods):
    """Status 7: two sweeps at a tolerance nothing meets.  The current iterate and ``cost`` must not change by a bit."""
    fte, _synth = mods
    ctx, _prob = _context(fte, "default_999", BOUND_LAM0, bcr_levels=3, refine_sweeps=2, trunc_tol=1e-300)
    try:
        x0, st0 = _frames(ctx, 0), ctx.state()
        ctx.step()
        st = ctx.state()
        x1 = _frames(ctx, 0)
    finally:
        ctx.close()
    assert st["status"] == 7 and st["trunc_eps"] > 1e-300, st
    assert st["cost"] == st0["cost"] and st["accepted"] == 0 and np.array_equal(x0, x1)
