"""CPU: the reference the FTE linear solvers are held to (tests/fte_step_ref.py) against dense linear algebra on chains of
8 .. 14 frames - its banded operator entry by entry against a densely assembled matrix, its refined solution against a
refined dense solve, with bound-active variables, in the clip form, and the refinement shown to do its work."""
import numpy as np
import pytest

from oracle import fk as ofk
from oracle import fte as ofte

import fte_step_ref as ref

LD = np.longdouble
P = 25


def _problem(n, seed, Ts=1.0):
    """An FTEProblem of n frames: only its smoothness weights, stencil band and bounds matter here, so the detections and the
    rig are random (Ts = 1: couplings of the size of the blocks, a system of moderate condition)."""
    rng = np.random.default_rng(seed)
    C = 2
    meas = rng.normal(0, 100, (n, C, 20, 2))
    lik = rng.uniform(0, 1, (n, C, 20))
    K = np.tile(np.array([[1000.0, 0, 640], [0, 1000.0, 360], [0, 0, 1]]), (C, 1, 1))
    return ofte.FTEProblem(meas, lik, K, np.zeros((C, 4)), np.tile(np.eye(3), (C, 1, 1)), rng.normal(0, 1, (C, 3)), Ts)


def _system(prob, seed, n_fixed=0):
    """(x, g, h_meas, h_dev): random SPD blocks and gradient; n_fixed variables on a finite bound with the gradient pushing
    outward."""
    rng = np.random.default_rng(seed)
    n = prob.N
    B = rng.normal(0, 1, (n, P, P))
    h_meas = B @ B.transpose(0, 2, 1) / P + 0.05 * np.eye(P)
    g = rng.normal(0, 1, (n, P))
    u = rng.uniform(0.3, 0.7, (n, P))                          # strictly inside the box: some bounds are 0.0
    x = np.where(np.isfinite(prob.lo), np.where(np.isfinite(prob.lo), prob.lo, 0.0) * (1 - u) +
                 np.where(np.isfinite(prob.hi), prob.hi, 0.0) * u, u - 0.5)
    bounded = np.argwhere(np.isfinite(np.broadcast_to(prob.lo, (n, P))))
    for i in rng.permutation(len(bounded))[:n_fixed]:
        f, p = bounded[i]
        if i % 2:
            x[f, p], g[f, p] = prob.lo[p], abs(g[f, p]) + 0.1
        else:
            x[f, p], g[f, p] = prob.hi[p], -abs(g[f, p]) - 0.1
    h_dev = h_meas.copy()
    idx = np.arange(P)
    h_dev[:, idx, idx] += ref.smooth_diag(prob)
    return x, g, h_meas, h_dev


def _dense(prob, h_dev, lam, fixed):
    """The damped matrix assembled densely, entry by entry, without the banded code."""
    n = prob.N
    band = prob.s_band()
    A = np.zeros((n * P, n * P))
    for f in range(n):
        A[f * P:(f + 1) * P, f * P:(f + 1) * P] = h_dev[f]
        for k in range(1, 4):
            if f + k < n:
                for p in range(P):
                    A[(f + k) * P + p, f * P + p] = A[f * P + p, (f + k) * P + p] = 2.0 * prob.q_w[p] * band[k][f]
    d = np.maximum(np.diag(A), 1e-30).copy()
    A[np.arange(n * P), np.arange(n * P)] += lam * d
    fx = fixed.reshape(-1)
    A[fx, :] = 0.0
    A[:, fx] = 0.0
    A[fx, fx] = 1.0
    return A


def _dense_refined(A, rhs, steps=4):
    x = np.linalg.solve(A, rhs).astype(LD)
    A_ld = A.astype(LD)
    for _ in range(steps):
        r = rhs.astype(LD) - A_ld @ x
        x = x + np.linalg.solve(A, np.asarray(r, dtype=np.float64)).astype(LD)
    return x


def test_long_double_is_wider_than_double():
    assert np.finfo(LD).eps <= 2.0 ** -63, "the refinement's residual needs a format wider than fp64"


@pytest.mark.parametrize("n,lam,n_fixed", [(8, 1e-3, 0), (11, 1e-6, 0), (14, 1e-3, 9), (9, 1e-6, 5)])
def test_banded_operator_and_refined_solution_against_dense(n, lam, n_fixed):
    prob = _problem(n, 100 + n)
    x, g, h_meas, h_dev = _system(prob, 7 * n, n_fixed)
    out = ref.step_reference(prob, x, g, h_dev, lam)
    assert int(out.fixed.sum()) == n_fixed
    assert np.array_equal(out.fixed, prob.active_set(x, g, h_meas))
    A = _dense(prob, h_dev, lam, out.fixed)
    assert np.array_equal(out.band.dense(), A)                       # the operator, entry by entry
    assert np.array_equal(out.rhs, np.where(out.fixed, 0.0, -g).reshape(-1))
    # ... which is solve_banded's: same matrix, same LAPACK factorisation
    d_or, diag_or = prob.solve_banded(h_meas, g, lam, out.fixed)
    assert np.allclose(out.diag, diag_or, rtol=1e-15, atol=0)
    scale = float(np.abs(d_or).max())
    assert np.abs(out.delta_lapack - d_or).max() <= 1e-12 * scale
    assert np.all(out.delta_ref[out.fixed] == 0.0) and np.all(out.delta_lapack[out.fixed] == 0.0)
    # the banded mat-vec in long double against the dense one
    v = np.random.default_rng(n).normal(0, 1, n * P)
    assert np.abs(out.band.matvec(v) - A.astype(LD) @ v.astype(LD)).max() <= 2.0 ** -58 * np.abs(A).sum(1).max() * np.abs(v).max()
    assert abs(out.band.norm_inf() - np.abs(A).sum(1).max()) <= 1e-14 * np.abs(A).sum(1).max()
    # the refined solution: two refinements of different factorisations end within cond * (long double rounding) of each
    # other (both carry a backward error of a few units of 2^-64)
    cond = float(np.linalg.cond(A))
    xd = _dense_refined(A, out.rhs)
    err = float(np.abs(out.delta_ref_ld.reshape(-1) - xd).max())
    print(f"n={n} lam={lam:g} fixed={n_fixed}: cond {cond:.2e}, refined residual {out.rel_residual:.2e} "
          f"(LAPACK {out.rel_residual_lapack:.2e}, {out.refine_steps} steps), |ref - dense refined| {err:.2e}")
    assert cond < 1e9
    assert err <= 64 * cond * 2.0 ** -64 * scale
    assert out.refine_steps >= 2
    # the predicted reduction, as oracle.fte.lm_solve forms it
    pred = 0.5 * float((out.delta_ref * (lam * out.diag * out.delta_ref - np.where(out.fixed, 0.0, g))).sum())
    assert abs(out.pred_ref - pred) <= 1e-12 * out.pred_abs
    assert ref.backward_error(out.band, out.rhs, out.delta_ref_ld) <= 2.0 ** -60


@pytest.mark.parametrize("lam", [1e-3, 1e-6])
def test_refinement_lowers_the_residual_below_plain_lapack(lam):
    prob = _problem(14, 5)
    x, g, _h_meas, h_dev = _system(prob, 6, 4)
    out = ref.step_reference(prob, x, g, h_dev, lam)
    eta_lapack = ref.backward_error(out.band, out.rhs, out.delta_lapack)
    eta_ref = ref.backward_error(out.band, out.rhs, out.delta_ref_ld)
    print(f"lam={lam:g}: residual {out.rel_residual_lapack:.2e} -> {out.rel_residual:.2e}, backward error {eta_lapack:.2e} -> "
          f"{eta_ref:.2e}, |lapack - ref| {np.abs(out.delta_lapack - out.delta_ref).max():.2e}")
    assert 0.0 < out.rel_residual_lapack and out.rel_residual <= 2.0 ** -8 * out.rel_residual_lapack
    assert eta_ref <= 2.0 ** -8 * eta_lapack
    assert np.abs(out.delta_lapack - out.delta_ref).max() > 0.0           # fp64 LAPACK is measurably off the reference
    # fp64 rounding of the reference: its backward error is the rounding of delta, not the solver's
    assert ref.backward_error(out.band, out.rhs, out.delta_ref) <= 2.0 ** -52


def test_clip_form_solves_every_clip_on_its_own():
    probs = [_problem(9, 1), _problem(12, 2), _problem(8, 3)]
    sys_ = [_system(p, 10 + i, n_fixed=3 * i) for i, p in enumerate(probs)]
    x, g, _hm, h_dev = (np.concatenate([s[k] for s in sys_]) for k in range(4))
    lam = 1e-3
    out = ref.step_reference(probs, x, g, h_dev, lam)
    ones = [ref.step_reference(p, *(s[k] for k in (0, 1, 3)), lam) for p, s in zip(probs, sys_)]
    for key in ("delta_ref", "delta_lapack", "fixed", "diag"):
        assert np.array_equal(getattr(out, key), np.concatenate([getattr(o, key) for o in ones])), key
    assert int(out.fixed.sum()) == 9
    assert abs(out.pred_ref - sum(o.pred_ref for o in ones)) <= 1e-15 * out.pred_abs
    # the operator over all clips is block diagonal: nothing couples a clip's last frames to the next clip's first
    A = out.band.dense()
    off = 0
    for p, o in zip(probs, ones):
        n = p.N * P
        assert np.array_equal(A[off:off + n, off:off + n], o.band.dense())
        assert not A[off + n:, off:off + n].any()
        off += n
    assert ref.backward_error(out.band, out.rhs, out.delta_ref_ld) <= 2.0 ** -60
    with pytest.raises(AssertionError):
        ref.step_reference(probs[:2], x, g, h_dev, lam)


def test_chain_node_helpers():
    # 999 frames: 333 nodes in runs of 4 -> 84 runs, 83 separators, the last node of every run but the final one
    sep = ref.separator_nodes(dict(m=4, n_chunks=84, n_sep=83))
    assert len(sep) == 83 and sep[0] == 3 and sep[-1] == 331 and np.all(np.diff(sep) == 4)
    assert len(ref.separator_nodes(dict(m=0, n_chunks=0, n_sep=0))) == 0
    with pytest.raises(AssertionError):
        ref.separator_nodes(dict(m=4, n_chunks=84, n_sep=85))
    # one level leaves the odd positions, three levels every eighth; a chain that is exhausted first is reduced completely
    assert ref.isolated_positions(7, 1).tolist() == [1, 3, 5]
    assert ref.isolated_positions(83, 3).tolist() == list(range(7, 83, 8))
    assert ref.isolated_positions(3, 1).tolist() == [] and ref.isolated_positions(15, 0).tolist() == []
    assert ref.node_frames([0, 3], 11).tolist() == [0, 1, 2, 9, 10]
    buf = np.arange(4 * 80, dtype=np.float64)
    fr = ref.nodes_to_frames(buf, 11)
    assert fr.shape == (11, 25) and fr[3, 0] == 80.0 and fr[5, 24] == 80.0 + 74.0 and fr[10, 0] == 240.0 + 25.0
