"""Reference for the posterior samples of the skeleton FTE trajectory (acino_skel_fte_sample): numpy / scipy on the CPU.  Test
infrastructure.

    delta = L^-T z,   A = L L^T,   A = skel_cov_ref.banded(prob, fisher_blocks, pin_set) (frame-major unknowns, P per frame),
    z of pinned variables counted as 0

in two independent ways (the functions of tests/fte_sample_ref.py, generalised to P states per frame):
  (1) banded_map: scipy.linalg.cholesky_banded + a banded triangular solve (any N)
  (2) dense_map:  numpy.linalg.cholesky of the dense matrix + scipy.linalg.solve_triangular (N <= 160 frames)
z and delta are [S, N, P]; ``fixed`` [N, P] is the pin set.  The bar is the project's: bar(d0) = max(64 d0, 1e-13) with
d0 = map_err(banded_map, dense_map) on the very input and z; an input with d0 > 1e-8 is refused (``reference``).
Nothing here comes from the code under test.
"""
import numpy as np
from scipy.linalg import cholesky_banded, solve_banded, solve_triangular

import skel_cov_ref as cref
from skel_cov_ref import bar  # noqa: F401  (re-exported: the project's bar)

D0_REFUSED = 1e-8


def _rhs(z, fixed):
    z = np.where(fixed[None], 0.0, np.asarray(z, dtype=np.float64))
    return z.reshape(z.shape[0], -1).T.copy()              # [N * P, S]


def _back(sol, fixed, S):
    return sol.T.reshape(S, *fixed.shape)


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
    L = np.linalg.cholesky(cref.dense(ab))
    sol = solve_triangular(L.T, _rhs(z, fixed), lower=False, check_finite=False)
    return _back(sol, fixed, z.shape[0])


def map_err(delta, delta_ref):
    """e = max_s ( max_n ||delta[s, n] - delta_ref[s, n]||_2 / max_n ||delta_ref[s, n]||_2 ); a sample whose reference is all
    zero must be zero itself."""
    num = np.linalg.norm(np.asarray(delta) - delta_ref, axis=2).max(axis=1)
    den = np.linalg.norm(delta_ref, axis=2).max(axis=1)
    assert np.all(num[den == 0] == 0)
    return float(np.max(num[den > 0] / den[den > 0]))


def identity_z(N, P):
    """The S = N P unit vectors as samples: delta = the rows of (L^-T)^T, so that sum_s delta delta^T = inv(A)."""
    return np.eye(N * P).reshape(N * P, N, P)


def cross_blocks(delta_identity, lag):
    """sum_s delta[s, n] delta[s, n + lag]^T for every n: the blocks (n, n + lag) of M M^T, M = L^-T.  [N - lag, P, P]"""
    N = delta_identity.shape[1]
    a, b = delta_identity[:, :N - lag], delta_identity[:, lag:]
    return np.einsum("snp,snq->npq", a, b)


def inverse_blocks(Ai, fixed, lag):
    """Blocks (n, n + lag) of a dense inverse, rows / columns of pinned variables 0."""
    N, P = fixed.shape
    out = np.stack([Ai[n * P:(n + 1) * P, (n + lag) * P:(n + lag + 1) * P] for n in range(N - lag)])
    return np.where(fixed[:N - lag, :, None] | fixed[lag:, None, :], 0.0, out)


def block_err(blocks, blocks_ref):
    """The covariance tests' error measure (fte_cov_ref.rel_err) on a stack of blocks."""
    return cref.rel_err(blocks, blocks_ref)


def system(prob, xa):
    """(ab, fixed) of the input: the oracle's pin set and the banded matrix, nothing from the code under test."""
    xa = np.asarray(xa, dtype=np.float64)
    fixed = cref.pin_set(prob, xa)
    return cref.banded(prob, cref.fisher_blocks(prob, xa), fixed), fixed


def reference(ab, fixed, z):
    """Both maps on (input, z), their disagreement d0 and the bar; d0 > 1e-8 refuses the input."""
    db, dd = banded_map(ab, fixed, z), dense_map(ab, fixed, z)
    d0 = map_err(db, dd)
    assert d0 <= D0_REFUSED, f"the two references disagree by {d0:.2e} on this input: refused"
    return dict(banded=db, dense=dd, d0=d0, bar=bar(d0))
