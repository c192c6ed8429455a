"""Reference for the posterior samples of the FTE trajectory (acino_fte_sample): numpy / scipy on the CPU.  Test
infrastructure.

    delta = L^-T z,   A = L L^T,   A = fte_cov_ref.banded(...) (frame-major unknowns), z of pinned variables counted as 0

in three independent ways:
  (1) banded_map: scipy.linalg.cholesky_banded + a banded triangular solve (any N)
  (2) dense_map:  numpy.linalg.cholesky of the dense matrix + scipy.linalg.solve_triangular (N <= 160 frames)
  (2') block_map: the node-block recursion the kernels use, in numpy - per clip, nodes of 3 frames (a ragged last node is
       simply smaller here), F_0 = D_0, F_k = L_k L_k^T, W_k = L_k^-1 E_k, F_k+1 = D_k+1 - W_k^T W_k, and backwards
       delta_last = L_last^-T z_last, delta_k = L_k^-T (z_k - W_k delta_k+1) - the second opinion on long inputs.
z and delta are [S, N, 25].  Nothing here comes from the code under test.
"""
import numpy as np
from scipy.linalg import cholesky_banded, solve_banded, solve_triangular

import fte_cov_ref as ref

P = ref.P


def _rhs(z, fixed):
    z = np.where(fixed[None], 0.0, np.asarray(z, dtype=np.float64))
    S = z.shape[0]
    return z.reshape(S, -1).T.copy()                       # [N * 25, S]


def _back(sol, fixed, S):
    return sol.T.reshape(S, fixed.shape[0], P)


def banded_map(ab, fixed, z):
    """(1): banded Cholesky, then L^T delta = z as a banded upper-triangular solve."""
    n, bw = ab.shape[1], ab.shape[0] - 1
    cb = cholesky_banded(ab, lower=True, check_finite=False)             # cb[d, j] = L[j + d, j]
    up = np.zeros((bw + 1, n))                                            # up[bw - d, j] = L^T[j - d, j] = L[j, j - d]
    for d in range(bw + 1):
        up[bw - d, d:] = cb[d, :n - d]
    sol = solve_banded((0, bw), up, _rhs(z, fixed), check_finite=False)
    return _back(sol, fixed, z.shape[0])


def dense_map(ab, fixed, z):
    """(2): dense Cholesky and triangular solve."""
    assert fixed.shape[0] <= 160, "dense factor: N <= 160 frames"
    L = np.linalg.cholesky(ref.dense(ab))
    sol = solve_triangular(L.T, _rhs(z, fixed), lower=False, check_finite=False)
    return _back(sol, fixed, z.shape[0])


def _node_blocks(ab, o, m, m_next):
    """D = A[o : o + m, o : o + m] and E = A[o : o + m, o + m : o + m + m_next] out of the lower band."""
    bw = ab.shape[0] - 1
    i = np.arange(m)
    d = np.abs(i[:, None] - i[None, :])
    D = ab[d, o + np.minimum(i[:, None], i[None, :])]
    E = None
    if m_next:
        j = np.arange(m_next)
        d = m + j[None, :] - i[:, None]
        E = np.where(d <= bw, ab[np.minimum(d, bw), o + i[:, None] + 0 * j[None, :]], 0.0)
    return D, E


def block_map(ab, fixed, z, clip_len=0):
    """(2'): the block recursion on nodes of 3 frames, every clip on a node grid of its own."""
    N = fixed.shape[0]
    S_ = z.shape[0]
    L_clip = int(clip_len) if clip_len else N
    rhs = _rhs(z, fixed)
    out = np.zeros_like(rhs)
    for c0 in range(0, N, L_clip):
        edges = list(range(c0, c0 + L_clip, 3)) + [c0 + L_clip]
        M = len(edges) - 1
        Ls, Ws = [], []
        corr = None
        for k in range(M):
            o, m = edges[k] * P, (edges[k + 1] - edges[k]) * P
            m_next = (edges[k + 2] - edges[k + 1]) * P if k + 1 < M else 0
            D, E = _node_blocks(ab, o, m, m_next)
            Lk = np.linalg.cholesky(D if corr is None else D - corr)
            Ls.append(Lk)
            if m_next:
                W = solve_triangular(Lk, E, lower=True, check_finite=False)
                Ws.append(W)
                corr = W.T @ W
        nxt = None
        for k in range(M - 1, -1, -1):
            sl = slice(edges[k] * P, edges[k + 1] * P)
            r = rhs[sl] if nxt is None else rhs[sl] - Ws[k] @ nxt
            nxt = solve_triangular(Ls[k].T, r, lower=False, check_finite=False)
            out[sl] = nxt
    return _back(out, fixed, S_)


def map_err(delta, delta_ref):
    """e = max_s ( max_n ||delta[s, n] - delta_ref[s, n]||_2 / max_n ||delta_ref[s, n]||_2 ); a sample whose reference is all
    zero must be zero itself."""
    num = np.linalg.norm(np.asarray(delta) - delta_ref, axis=2).max(axis=1)
    den = np.linalg.norm(delta_ref, axis=2).max(axis=1)
    assert np.all(num[den == 0] == 0)
    return float(np.max(num[den > 0] / den[den > 0]))


def sample_matrix(ab, fixed, how="banded", clip_len=0):
    """M = L^-T with the columns of pinned variables zeroed, as rows of samples: delta[s] for z = the S = 25 N unit vectors,
    so that delta.reshape(S, -1).T @ delta.reshape(S, -1) ... = M M^T = inv(A) on the free variables."""
    N = fixed.shape[0]
    z = np.eye(N * P).reshape(N * P, N, P)
    if how == "dense":
        return dense_map(ab, fixed, z)
    if how == "block":
        return block_map(ab, fixed, z, clip_len)
    return banded_map(ab, fixed, z)


def cross_blocks(delta_identity, lag):
    """sum_s delta[s, n] delta[s, n + lag]^T for every n: the blocks (n, n + lag) of M M^T.  [N - lag, 25, 25]"""
    N = delta_identity.shape[1]
    a, b = delta_identity[:, :N - lag], delta_identity[:, lag:]
    return np.einsum("snp,snq->npq", a, b)


def inverse_blocks(Ai, fixed, lag):
    """Blocks (n, n + lag) of a dense inverse, rows / columns of pinned variables 0."""
    N = fixed.shape[0]
    out = np.stack([Ai[n * P:(n + 1) * P, (n + lag) * P:(n + lag + 1) * P] for n in range(N - lag)])
    return np.where(fixed[:N - lag, :, None] | fixed[lag:, None, :], 0.0, out)
