"""Reference for the FTE posterior covariance (acino_fte_covariance): numpy / scipy on the CPU.  Test infrastructure.

    A = blockdiag(H_n) + 2 q (x) D3^T D3,   bound-active variables pinned (row and column zeroed, diagonal 1)

exactly the matrix of oracle.fte.FTEProblem.solve_banded with lam = 0.  The selected blocks of A^-1 come out of it in
independent ways:
  (a)  dense_blocks:  np.linalg.inv of the dense matrix (LU; N <= 160 frames)
  (b)  probe_blocks:  scipy.linalg.solveh_banded (banded Cholesky) on the 25 unit vectors of chosen frames (any N)
  (b') probe_blocks(lu=True):  scipy.linalg.solve_banded (banded LU with partial pivoting) - the second opinion where the
       dense inverse is out of reach (10 000 frames)
and, as a restatement of what the HIP kernels do, two_sweep_blocks: the forward / backward pivot recursions on nodes of 3
frames.  Rows / columns of pinned variables are 0 in every output (a variable held at its bound has no spread).
H / g come from FTEContext.grad_hess() (H then carries the smoothness diagonal: h_has_smooth_diag=True) or from the
oracle's evaluate (it does not) - never from the code under test.
"""
import numpy as np
from scipy.linalg import solve_banded, solveh_banded

from oracle import fk as ofk
from oracle import fte as ofte

P = 25
GRAD_ZERO_REL = 1e-14


def clip_band(n_frames, clip_len=0):
    """s_band() of a sequence of n_frames, or of n_frames / clip_len independent clips laid end to end."""
    S = int(clip_len) if clip_len else int(n_frames)
    assert n_frames % S == 0
    dummy = ofte.FTEProblem(np.zeros((S, 1, 20, 2)), np.zeros((S, 1, 20)), np.eye(3)[None], np.zeros((1, 4)), np.eye(3)[None],
                            np.zeros((1, 3)), 1.0)
    return np.tile(dummy.s_band(), (1, n_frames // S))          # (band[k, i] is 0 wherever frame i + k leaves the clip)


def with_smooth_diag(H, q_w, band):
    Hd = np.array(H, dtype=np.float64, copy=True)
    idx = np.arange(P)
    Hd[:, idx, idx] += 2 * q_w[None, :] * band[0][:, None]
    return Hd


def active_set(x, g, Hd, lo, hi):
    """oracle.fte.FTEProblem.active_set on blocks that already carry the smoothness diagonal."""
    idx = np.arange(P)
    tol = GRAD_ZERO_REL * Hd[:, idx, idx]
    return ((x <= lo) & (g > tol)) | ((x >= hi) & (g < -tol))


def banded(Hd, fixed, q_w, band):
    """LAPACK lower-banded storage of A, as solve_banded builds it with lam = 0.  Hd: blocks WITH the smoothness diagonal."""
    N = Hd.shape[0]
    n_tot = N * P
    bw = 4 * P - 1
    ab = np.zeros((bw + 1, n_tot))
    Hd = np.where(fixed[:, :, None] | fixed[:, None, :], 0.0, Hd)
    idx = np.arange(P)
    Hd[:, idx, idx] = np.where(fixed, 1.0, Hd[:, idx, idx])
    for r in range(P):
        for cc in range(r + 1):
            ab[r - cc, cc::P][:N] = Hd[:, r, cc]
    for k in range(1, 4):
        v = 2 * q_w[None, :] * band[k][:, None]
        v[:N - k] = np.where(fixed[:N - k] | fixed[k:], 0.0, v[:N - k])
        flat = v.reshape(-1)
        ab[k * P, :n_tot - k * P] = flat[:n_tot - k * P]
    return ab


def dense(ab):
    bw, n = ab.shape[0] - 1, ab.shape[1]
    A = np.zeros((n, n))
    for d in range(bw + 1):
        v = ab[d, :n - d]
        A[np.arange(d, n), np.arange(n - d)] = v
        A[np.arange(n - d), np.arange(d, n)] = v
    return A


def _unpin(blocks, fixed_rows):
    m = fixed_rows[:, :, None] | fixed_rows[:, None, :]
    return np.where(m, 0.0, blocks)


def dense_blocks(ab, fixed):
    """(a): every frame's diagonal block of inv(A)."""
    N = fixed.shape[0]
    assert N <= 160, "dense inverse: N <= 160 frames"
    Ai = np.linalg.inv(dense(ab))
    blocks = np.stack([Ai[n * P:(n + 1) * P, n * P:(n + 1) * P] for n in range(N)])
    return _unpin(blocks, fixed)


def probe_blocks(ab, fixed, frames, lu=False):
    """(b) / (b'): the diagonal blocks of the chosen frames from banded solves with their 25 unit vectors."""
    frames = np.asarray(frames, dtype=np.int64)
    n_tot = ab.shape[1]
    rhs = np.zeros((n_tot, len(frames) * P))
    for j, n in enumerate(frames):
        rhs[n * P + np.arange(P), j * P + np.arange(P)] = 1.0
    if lu:
        bw = ab.shape[0] - 1
        full = np.zeros((2 * bw + 1, n_tot))
        full[bw:] = ab
        for d in range(1, bw + 1):
            full[bw - d, d:] = ab[d, :n_tot - d]
        sol = solve_banded((bw, bw), full, rhs, check_finite=False)
    else:
        sol = solveh_banded(ab, rhs, lower=True, check_finite=False)
    blocks = np.stack([sol[n * P:(n + 1) * P, j * P:(j + 1) * P] for j, n in enumerate(frames)])
    return _unpin(blocks, fixed[frames])


def two_sweep_blocks(ab, fixed, clip_len=0):
    """The kernels' recursion in numpy: per clip, nodes of 3 frames (a ragged last node is simply smaller here; the kernels
    pad it with identity), F_k+1 = D_k+1 - E^T F_k^-1 E forwards, B_k-1 = D_k-1 - E B_k^-1 E^T backwards,
    Sigma_k = (F_k + B_k - D_k)^-1 formed as (D_k - CF_k - CB_k)^-1 from the subtracted corrections."""
    N = fixed.shape[0]
    S = int(clip_len) if clip_len else N
    A = None
    out = np.zeros((N, P, P))
    bw = ab.shape[0] - 1

    def block(r0, r1, c0, c1):                         # A[r0:r1, c0:c1], r >= c region or its mirror, from the band
        M = np.zeros((r1 - r0, c1 - c0))
        for r in range(r0, r1):
            for c in range(c0, c1):
                d = abs(r - c)
                if d <= bw:
                    M[r - r0, c - c0] = ab[d, min(r, c)]
        return M

    for c0 in range(0, N, S):
        edges = list(range(c0, c0 + S, 3)) + [c0 + S]
        M = len(edges) - 1
        D = [block(edges[k] * P, edges[k + 1] * P, edges[k] * P, edges[k + 1] * P) for k in range(M)]
        E = [block(edges[k] * P, edges[k + 1] * P, edges[k + 1] * P, edges[k + 2] * P) for k in range(M - 1)]
        CF = [np.zeros_like(D[k]) for k in range(M)]
        CB = [np.zeros_like(D[k]) for k in range(M)]
        for k in range(M - 1):
            CF[k + 1] = E[k].T @ np.linalg.solve(D[k] - CF[k], E[k])
        for k in range(M - 1, 0, -1):
            CB[k - 1] = E[k - 1] @ np.linalg.solve(D[k] - CB[k], E[k - 1].T)
        for k in range(M):
            Sg = np.linalg.inv(D[k] - CF[k] - CB[k])
            for j, n in enumerate(range(edges[k], edges[k + 1])):
                out[n] = Sg[j * P:(j + 1) * P, j * P:(j + 1) * P]
    return _unpin(out, fixed)


def fk_jacobian(x_active, h=1e-6):
    """J[n, l, 3, 25]: central differences of the oracle FK with respect to the active states (the inactive ones are 0, as
    in acino_fk_active)."""
    x = np.asarray(x_active, dtype=np.float64)
    N = x.shape[0]
    J = np.zeros((N, 20, 3, P))
    for p in range(P):
        qp = np.zeros((N, ofk.N_STATES))
        qm = np.zeros((N, ofk.N_STATES))
        qp[:, ofk.ACTIVE] = x
        qm[:, ofk.ACTIVE] = x
        qp[:, ofk.ACTIVE[p]] += h
        qm[:, ofk.ACTIVE[p]] -= h
        J[..., p] = (ofk.cheetah_fk(qp) - ofk.cheetah_fk(qm)) / (2 * h)
    return J


def fk_jacobian_exact(x_active):
    """The oracle's analytic FK Jacobian restricted to the active states."""
    q = np.zeros((x_active.shape[0], ofk.N_STATES))
    q[:, ofk.ACTIVE] = x_active
    _, Jq = ofk.cheetah_fk(q, with_jac=True)
    return Jq[..., ofk.ACTIVE]


def marker_cov(cov_x, J):
    cp = np.einsum("nlip,npq,nljq->nlij", J, cov_x, J)
    return cp, np.sqrt(np.maximum(np.einsum("nlii->nl", cp), 0.0))


def rel_err(S, S_ref):
    """e = max_n ||S[n] - S_ref[n]||_F / ||S_ref[n]||_F over the leading axis (blocks whose reference is all zero - every
    variable pinned - must be zero themselves)."""
    S = np.asarray(S).reshape(S.shape[0], -1)
    R = np.asarray(S_ref).reshape(S_ref.shape[0], -1)
    num = np.linalg.norm(S - R, axis=1)
    den = np.linalg.norm(R, axis=1)
    assert np.all(num[den == 0] == 0)
    return float(np.max(num[den > 0] / den[den > 0]))


def bar(d0):
    """The admissible error of the GPU path: 64 units of the references' own disagreement d0, at least 1e-13."""
    assert d0 <= 1e-8, f"input too ill-conditioned to test anything (d0 = {d0:.2e})"
    return max(64.0 * d0, 1e-13)
