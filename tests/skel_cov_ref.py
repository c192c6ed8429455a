"""Reference for the skeleton-FTE covariance (acino_skel_fte_covariance): numpy / scipy on the CPU.  Test infrastructure.

    A = blockdiag_n( sum_{c,l,d} w_ncl^2 J_ncld^T J_ncld ) + 2 q D3^T D3,   bound-active variables pinned (row / column 0, diagonal 1)

H_F (the Fisher blocks) restates SkelFTEProblem.measurement_terms with hw = w**2 in place of the IRLS weight; the gradient,
the IRLS diagonal and the active set come from the oracle (oracle.skel_fte.SkelFTEProblem.evaluate, its inherited s_band and
active_set; the pinhole problem of tests/pinhole_skel_ref.py is the same class with the camera swapped) - never from the code
under test.  The selected blocks of A^-1 come out three ways:
  (a) dense_blocks:     np.linalg.inv of the dense matrix (N <= 100 frames)
  (b) probe_blocks:     scipy.linalg.solveh_banded on the unit vectors of chosen frames
  (c) takahashi_blocks: the recursion the HIP kernel walks, restated on numpy blocks of a dense Cholesky factor:
          Z_j = L_n+j,n L_nn^-1,   S_n+i,n = - sum_j S_n+i,n+j Z_j,   S_nn = L_nn^-T L_nn^-1 - sum_j Z_j^T S_n+j,n
G_l (3 x P) is oracle.skel_fte.skeleton_fk_jac restricted to the active states.  rel_err and bar are the project's
(tests/fte_cov_ref.py): bar(d0) = max(64 d0, 1e-13), d0 the disagreement of (a) and (b) on the input; d0 > 1e-8 is refused.
"""
import numpy as np
from scipy.linalg import solveh_banded

from oracle import camera
from oracle import skel_fte as osf

from fte_cov_ref import bar, rel_err  # noqa: F401  (re-exported: the project's bar and error measure)


def fisher_blocks(prob, xa):
    """H_F[n] = sum_{c,l,d} w^2 J^T J: measurement_terms with hw = w**2 (rows with w = 0, non-finite measurements - the
    problem has zeroed their weights - and the singular plane |z_cam| < 1e-9 contribute nothing)."""
    N, P = xa.shape
    H = np.zeros((N, P, P))
    pos, Jfk, _ = osf.skeleton_fk_jac(prob.skel, prob.full_state(xa))
    G = Jfk[..., prob.ACT]                                   # [n, L, 3, P]
    for ci in range(prob.C):
        if hasattr(prob, "D_pin"):
            import pinhole_fte_ref as pref
            with np.errstate(divide="ignore", invalid="ignore"):
                _uv, Jpi, zc = pref.project_with_jac(pos, prob.K[ci], prob.D_pin[ci], prob.R[ci], prob.t[ci])
        else:
            _uv, Jpi, zc = camera.pt3d_to_2d(pos, prob.K[ci], prob.D[ci], prob.R[ci], prob.t[ci], with_jac=True)
        sing = np.abs(zc) < 1e-9
        w = np.where(sing, 0.0, prob.w[:, ci])
        Jpi = np.where(sing[..., None, None], 0.0, Jpi)
        J = np.einsum("nlij,nljp->nlip", Jpi, G)
        hw = np.broadcast_to((w ** 2)[..., None], J.shape[:3])
        H += np.einsum("nlip,nli,nliq->npq", J, hw, J)
    return H


def pin_set(prob, xa):
    """The solver's bound-active set at xa: oracle gradient (L1 + smoothness), oracle IRLS blocks, oracle rule."""
    _F, g, H, _nb = prob.evaluate(xa)
    return prob.active_set(xa, g, H)


def banded(prob, HF, fixed):
    """LAPACK lower-banded storage of A (HF without the smoothness diagonal)."""
    N, P = fixed.shape
    band, q_w = prob.s_band(), prob.q_w
    n_tot, bw = N * P, 4 * P - 1
    ab = np.zeros((bw + 1, n_tot))
    idx = np.arange(P)
    Hd = np.array(HF, dtype=np.float64, copy=True)
    Hd[:, idx, idx] += 2 * q_w[None, :] * band[0][:, None]
    Hd = np.where(fixed[:, :, None] | fixed[:, None, :], 0.0, Hd)
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
    return np.where(fixed_rows[:, :, None] | fixed_rows[:, None, :], 0.0, blocks)


def dense_blocks(ab, fixed):
    """(a): every frame's diagonal block of inv(A)."""
    N, P = fixed.shape
    assert N <= 100, "dense inverse: N <= 100 frames"
    Ai = np.linalg.inv(dense(ab))
    return _unpin(np.stack([Ai[n * P:(n + 1) * P, n * P:(n + 1) * P] for n in range(N)]), fixed)


def probe_blocks(ab, fixed, frames):
    """(b): the diagonal blocks of the chosen frames from banded Cholesky solves with their unit vectors."""
    P = fixed.shape[1]
    frames = np.asarray(frames, dtype=np.int64)
    n_tot = ab.shape[1]
    rhs = np.zeros((n_tot, len(frames) * P))
    for j, n in enumerate(frames):
        rhs[n * P + np.arange(P), j * P + np.arange(P)] = 1.0
    sol = solveh_banded(ab, rhs, lower=True, check_finite=False)
    return _unpin(np.stack([sol[n * P:(n + 1) * P, j * P:(j + 1) * P] for j, n in enumerate(frames)]), fixed[frames])


def takahashi_blocks(ab, fixed):
    """(c): the kernel's recursion on the blocks of a dense Cholesky factor, right to left."""
    return _unpin(np.stack(_collect(ab, fixed)), fixed)


def _collect(ab, fixed):
    """The recursion of takahashi_blocks with every diagonal block kept."""
    N, P = fixed.shape
    Lf = np.linalg.cholesky(dense(ab))
    blk = lambda a, b: Lf[a * P:(a + 1) * P, b * P:(b + 1) * P]      # noqa: E731
    S, out = {}, [None] * N
    for n in range(N - 1, -1, -1):
        W = np.linalg.inv(blk(n, n))
        js = [j for j in (1, 2, 3) if n + j < N]
        Z = {j: blk(n + j, n) @ W for j in js}
        for i in js:
            acc = np.zeros((P, P))
            for j in js:
                acc -= (S[(n + i, n + j)] if i >= j else S[(n + j, n + i)].T) @ Z[j]
            S[(n + i, n)] = acc
        Snn = W.T @ W
        for j in js:
            Snn -= Z[j].T @ S[(n + j, n)]
        Snn = 0.5 * (Snn + Snn.T)        # as the kernel: the antisymmetric rounding error is the mode the recursion amplifies
        S[(n, n)] = out[n] = Snn
        for key in [k for k in S if k[0] > n + 2]:           # the next frame's window ends at n + 2
            del S[key]
    return out


def pose_jacobian(prob, xa):
    """G[n, l, 3, P]: the oracle's analytic pose Jacobian restricted to the active states."""
    return osf.skeleton_fk_jac(prob.skel, prob.full_state(xa))[1][..., prob.ACT]


def pose_cov(cov_x, G):
    cp = np.einsum("nlip,npq,nljq->nlij", G, cov_x, G)
    return cp, np.sqrt(np.maximum(np.einsum("nlii->nl", cp), 0.0))


def reference(prob, xa, probe_frames=None):
    """Everything a test needs on one input, computed once: the pin set, (a), (b) on ``probe_frames`` (default: all), their
    disagreement d0, the pose covariance of (a)."""
    xa = np.asarray(xa, dtype=np.float64)
    fixed = pin_set(prob, xa)
    ab = banded(prob, fisher_blocks(prob, xa), fixed)
    frames = np.arange(xa.shape[0]) if probe_frames is None else np.asarray(probe_frames)
    Sa = dense_blocks(ab, fixed)
    Sb = probe_blocks(ab, fixed, frames)
    d0 = rel_err(Sb, Sa[frames])
    G = pose_jacobian(prob, xa)
    cp, sp = pose_cov(Sa, G)
    return dict(fixed=fixed, ab=ab, Sa=Sa, Sb=Sb, frames=frames, d0=d0, G=G, cov_pos=cp, std_pos=sp)
