"""Reference of ONE linear solve of the FTE Levenberg-Marquardt step (CPU, numpy / scipy only).  Test infrastructure.

The device hands out its own gradient and Gauss-Newton blocks of the current iterate (FTEContext.grad_hess) and its damping
(state()["lam"]); solving THAT system on the CPU isolates the linear solver - chunk sweep, separator reduction, truncated
solve, refinement sweeps, back-substitution - from the assembly.  The operator is exactly the one of
oracle.fte.FTEProblem.solve_banded: blockdiag(H_n) + 2 q (x) D3^T D3 plus lam times its diagonal, bound-active variables
(oracle.fte.FTEProblem.active_set) replaced by identity rows.

The reference solution is the fp64 banded Cholesky solution (LAPACK pbtrf / pbtrs) after iterative refinement with the
residual formed in np.longdouble (64-bit mantissa on x86): the factor only has to contract, the accuracy comes from the
residual.  What plain LAPACK differs from it by is the scale every GPU solver is held against.
"""
import types

import numpy as np
from scipy.linalg import cho_solve_banded, cholesky_banded

LD = np.longdouble

# How many times LAPACK's own error (forward: |delta_lapack - delta_ref|; backward: its normwise backward error) a GPU solve
# of the same system may be off by: the next power of two at or above 4 times the worst ratio measured on the MI355X over the
# complete-reduction paths (40.9; tests/test_gpu_fte_step_reference.py, NOTES_perf.md "FTE step against the banded reference").
K_GPU = 256.0


class Band:
    """A symmetric banded matrix from LAPACK's lower banded storage ab[i - j, j] = A[i, j], kept by its non-zero diagonals
    (the damped FTE system has 28 of 100: the 25 of the frame blocks and the three couplings at 25, 50, 75)."""

    def __init__(self, ab):
        ab = np.asarray(ab, dtype=np.float64)
        self.bw, self.n = ab.shape[0] - 1, ab.shape[1]
        self.ks = [k for k in range(ab.shape[0]) if k == 0 or ab[k].any()]
        self.rows = ab[self.ks].copy()

    def full(self):
        ab = np.zeros((self.bw + 1, self.n))
        ab[self.ks] = self.rows
        return ab

    def matvec(self, x, absolute=False):
        """A x (|A| x with ``absolute``) in np.longdouble."""
        x = np.asarray(x, dtype=LD).reshape(-1)
        n = self.n
        rows = np.abs(self.rows) if absolute else self.rows
        y = rows[0].astype(LD) * x
        for k, row in zip(self.ks[1:], rows[1:]):
            r = row[:n - k].astype(LD)
            y[k:] += r * x[:n - k]
            y[:n - k] += r * x[k:]
        return y

    def norm_inf(self):
        return float(self.matvec(np.ones(self.n), absolute=True).max())

    def dense(self):
        A = np.zeros((self.n, self.n))
        for k, row in zip(self.ks, self.rows):
            i = np.arange(self.n - k)
            A[i + k, i] = row[:self.n - k]
            A[i, i + k] = row[:self.n - k]
        return A


def _as_band(ab):
    return ab if isinstance(ab, Band) else Band(ab)


def backward_error(ab, rhs, delta):
    """Normwise backward error |rhs - A delta|_inf / (|A|_inf |delta|_inf + |rhs|_inf), formed in np.longdouble."""
    A = _as_band(ab)
    rhs = np.asarray(rhs, dtype=LD).reshape(-1)
    d = np.asarray(delta, dtype=LD).reshape(-1)
    r = rhs - A.matvec(d)
    den = LD(A.norm_inf()) * np.abs(d).max() + np.abs(rhs).max()
    return float(np.abs(r).max() / den) if den > 0 else 0.0


def smooth_diag(prob):
    """2 q_w band[0]: what the device's H carries on its diagonal beside the measurement blocks, [N, P]."""
    return 2.0 * prob.q_w[None, :] * prob.s_band()[0][:, None]


def damped_band(prob, h_dev, lam, fixed):
    """(ab, diag) of solve_banded's operator, lower banded, from blocks that ALREADY hold the smoothness diagonal: the
    statements of oracle.fte.FTEProblem.solve_banded behind its ``Hd[:, idx, idx] += 2 q band[0]``."""
    N, P = fixed.shape
    band = prob.s_band()
    n_tot = N * P
    ab = np.zeros((4 * P, n_tot))
    Hd = np.array(h_dev, dtype=np.float64, copy=True)
    idx = np.arange(P)
    diag = np.maximum(Hd[:, idx, idx], 1e-30)
    Hd[:, idx, idx] += lam * diag
    Hd = np.where(fixed[:, :, None] | fixed[:, None, :], 0.0, Hd)
    Hd[:, idx, idx] = np.where(fixed, 1.0, Hd[:, idx, idx])
    for r in range(P):
        for c in range(r + 1):
            ab[r - c, c::P][:N] = Hd[:, r, c]
    for k in range(1, 4):
        v = 2.0 * prob.q_w[None, :] * band[k][:, None]
        v[:N - k] = np.where(fixed[:N - k] | fixed[k:], 0.0, v[:N - k])
        flat = v.reshape(-1)
        ab[k * P, :n_tot - k * P] = flat[:n_tot - k * P]
    return ab, diag


def _rel(r, rhs):
    return float(np.abs(r).max() / max(float(np.abs(rhs).max()), np.finfo(np.float64).tiny))


def _solve_refined(ab, rhs, max_steps=10):
    """(delta_lapack fp64, delta_ref longdouble, relative residual of either, refinement steps taken)."""
    cb = cholesky_banded(ab, lower=True, check_finite=False)
    d0 = cho_solve_banded((cb, True), rhs, check_finite=False)
    A = Band(ab)
    b = rhs.astype(LD)
    d = d0.astype(LD)
    r = b - A.matvec(d)
    res0 = res = _rel(r, rhs)
    steps = 0
    while steps < max_steps:
        dn = d + cho_solve_banded((cb, True), np.asarray(r, dtype=np.float64), check_finite=False).astype(LD)
        rn = b - A.matvec(dn)
        resn = _rel(rn, rhs)
        steps += 1
        if resn < res:
            d, r, res, fell = dn, rn, resn, True
        else:
            fell = False
        if steps >= 2 and not fell:
            break
    return d0, d, res0, res, steps, A


def _step_one(prob, x, g, h_dev, lam):
    x, g, h_dev = (np.asarray(a, dtype=np.float64) for a in (x, g, h_dev))
    N, P = g.shape
    assert (N, P) == (prob.N, prob.P) and x.shape == (N, P) and h_dev.shape == (N, P, P)
    idx = np.arange(P)
    h_meas = h_dev.copy()
    h_meas[:, idx, idx] -= smooth_diag(prob)           # (active_set adds it again: it only scales the zero test of g)
    fixed = prob.active_set(x, g, h_meas)
    ab, diag = damped_band(prob, h_dev, lam, fixed)
    rhs = np.where(fixed, 0.0, -g).reshape(-1)
    d0, d, res0, res, steps, A = _solve_refined(ab, rhs)
    return dict(fixed=fixed, diag=diag, rhs=rhs, d0=d0, d=d, res0=res0, res=res, steps=steps, A=A, pg=np.where(fixed, 0.0, g))


def pred_terms(delta, lam, diag, pg):
    """The summands of oracle.fte.lm_solve's predicted reduction 0.5 sum delta (lam diag delta - pg), in np.longdouble."""
    d = np.asarray(delta, dtype=LD).reshape(diag.shape)
    return LD(0.5) * d * (LD(lam) * diag.astype(LD) * d - pg.astype(LD))


def step_reference(prob, x, g, h_dev, lam):
    """The damped step of the iterate ``x`` [N, 25] with the device's gradient ``g`` [N, 25], blocks ``h_dev`` [N, 25, 25]
    (smoothness diagonal included) and damping ``lam``.  ``prob``: an oracle.fte.FTEProblem, or a list of them for the clip
    form - one problem per clip, solved on its own from slices of the same arrays in the order given.

    Returns a namespace: ``delta_ref`` [N, 25] (fp64 rounding of the refined solution; ``delta_ref_ld`` keeps the long
    double), ``fixed``, ``diag``, ``delta_lapack``, ``pred_ref`` (and ``pred_lapack``, the same sum at ``delta_lapack``;
    ``pred_abs`` the sum of the |summands|, ``pred_slope`` the sum of |d summand / d delta|), ``rel_residual`` (max over the
    clips, after refinement) and ``rel_residual_lapack`` (before), ``refine_steps``, and the operator for
    ``backward_error``: ``band`` (a Band over all clips), ``rhs``."""
    probs = list(prob) if isinstance(prob, (list, tuple)) else [prob]
    x, g, h_dev = (np.asarray(a, dtype=np.float64) for a in (x, g, h_dev))
    parts, off = [], 0
    for p in probs:
        sl = slice(off, off + p.N)
        parts.append(_step_one(p, x[sl], g[sl], h_dev[sl], lam))
        off += p.N
    assert off == x.shape[0], "the clips must cover the frames"
    P = probs[0].P
    cat = lambda key: np.concatenate([q[key] for q in parts])
    fixed, diag, pg = cat("fixed"), cat("diag"), cat("pg")
    d_ld = cat("d").reshape(-1, P)
    d0 = cat("d0").reshape(-1, P)
    # (lower banded storage holds column j's entries below the diagonal: the clips' arrays side by side are the block
    #  diagonal matrix, no coupling reaching past a clip's last column)
    band = parts[0]["A"] if len(parts) == 1 else Band(np.concatenate([q["A"].full() for q in parts], axis=1))
    t_ref, t_lap = pred_terms(d_ld, lam, diag, pg), pred_terms(d0, lam, diag, pg)
    slope = np.abs(LD(lam) * diag.astype(LD) * d_ld - LD(0.5) * pg.astype(LD))
    return types.SimpleNamespace(
        delta_ref=np.asarray(d_ld, dtype=np.float64), delta_ref_ld=d_ld, fixed=fixed, diag=diag, delta_lapack=d0,
        pred_ref=float(t_ref.sum()), pred_lapack=float(t_lap.sum()), pred_abs=float(np.abs(t_ref).sum()),
        pred_slope=float(slope.sum()), rel_residual=max(q["res"] for q in parts),
        rel_residual_lapack=max(q["res0"] for q in parts), refine_steps=max(q["steps"] for q in parts), band=band,
        rhs=cat("rhs"), lam=float(lam))


# ---- the chain of 3-frame nodes ---------------------------------------------------------------------------------------
def separator_nodes(plan):
    """Chain nodes that are separators of a single-GPU context, from fte.solver_plan (acino_fte_plan's out[0..2]: nodes per
    run ``m``, runs ``n_chunks``, separators ``n_sep``) by ChunkPlan::build's rule: the LAST node of every run but the final
    one.  Whole-chain reduction (m = 0): none."""
    m, n_chunks, n_sep = int(plan["m"]), int(plan["n_chunks"]), int(plan["n_sep"])
    if m <= 0 or n_chunks <= 0:
        return np.zeros(0, dtype=np.int64)
    nodes = np.arange(n_chunks - 1, dtype=np.int64) * m + (m - 1)
    assert len(nodes) == n_sep, "pinned contexts have separators this rule does not list"
    return nodes


def isolated_positions(n_sep, levels):
    """Positions in the separator chain that an incomplete reduction of ``levels`` levels leaves isolated (BcrSchedule::build:
    a level eliminates the positions 0, 2, 4, ... of what is left, and the reduction is only cut while more than one node
    remains); empty when the chain is exhausted before - the complete reduction."""
    act = list(range(int(n_sep)))
    for _ in range(int(levels)):
        act = act[1::2]
    return np.asarray(act if int(levels) > 0 and len(act) > 1 else [], dtype=np.int64)


def node_frames(nodes, n_frames):
    """Frames held by the given chain nodes (node k: frames 3k .. 3k + 2, the last node possibly fewer)."""
    f = (np.asarray(nodes, dtype=np.int64)[:, None] * 3 + np.arange(3)[None, :]).reshape(-1)
    return f[f < n_frames]


def nodes_to_frames(buf, n_frames, P=25):
    """The solver's node vector [T * 80] (75 rows used per node, frame-major) as [n_frames, P]."""
    T = (n_frames + 2) // 3
    return np.asarray(buf).reshape(T, -1)[:, :3 * P].reshape(T * 3, P)[:n_frames]
