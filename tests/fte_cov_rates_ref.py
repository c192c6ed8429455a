"""Reference for the covariance of dx, ddx and of the marker velocities (acino_fte_covariance_rates): numpy / scipy on the
CPU.  Test infrastructure; the matrix A, its banded storage and the metric are those of fte_cov_ref.

dx_n, ddx_n are fixed linear maps of a window of consecutive frames of the frame's own clip (k_derivatives in
csrc/fte_api.hip, taken per clip):
    n >= 2   window (n-2, n-1, n):  dx_n = (x_n - x_n-1) / Ts,   ddx_n = (x_n - 2 x_n-1 + x_n-2) / Ts^2
    n = 1    window (0, 1, 2):      dx_1 = (x_1 - x_0) / Ts,     ddx_1 = ddx_2
    n = 0    window (0, 1, 2):      dx_0 = dx_1 - Ts ddx_2 = (-2 x_0 + 3 x_1 - x_2) / Ts,   ddx_0 = ddx_2
    clips of 2 frames: ddx = 0, dx_0 = dx_1 = (x_1 - x_0) / Ts;  of 1 frame: dx = ddx = 0
and the marker velocity of frame n is (p_l(x_n) - p_l(x_n-1)) / Ts, linearised with the FK Jacobians at x; frame 0 of a
clip repeats frame 1.  With Sigma_win the block of A^-1 over the window (rows / columns of pinned variables 0):
    cov_dx = C Sigma_win C^T, C = c (x) I_25;   cov_vel_l = G_l Sigma_win G_l^T, G_l = [-J_l(x_n-1) | J_l(x_n)] / Ts
Sigma_win comes out of A in independent ways:
  (a)  how="dense":  np.linalg.inv of the dense matrix (LU; N <= 160)
  (b)  how="chol":   scipy.linalg.solveh_banded on the 75 unit vectors of the window (any N)
  (b') how="lu":     scipy.linalg.solve_banded (banded LU, partial pivoting) on the same unit vectors
and factor_form restates what k_fte_cov_rates does: the joint precision of two neighbouring 3-frame nodes from the pivots
of the two sweeps, its Cholesky factors, the outputs as Y1^T Y1 + Y2^T Y2.
"""
import numpy as np
from scipy.linalg import cholesky, solve_banded, solve_triangular, solveh_banded

import fte_cov_ref as ref

P = ref.P
NL = 20


def coef_rows(n, L, Ts):
    """Frame n of a clip of L frames: (w0, c_dx[m], c_ddx[m], vel) - the window is frames w0 .. w0 + m - 1 of the clip,
    m = min(3, L); vel = (slot of frame n-1, slot of frame n) inside the window, None when there is no velocity."""
    if L >= 3:
        w0 = max(n - 2, 0)
        c_ddx = np.array([1.0, -2.0, 1.0]) / Ts ** 2
        c_dx = np.array([0.0, -1.0, 1.0] if n >= 2 else ([-1.0, 1.0, 0.0] if n == 1 else [-2.0, 3.0, -1.0])) / Ts
        nn = max(n, 1)
        return w0, c_dx, c_ddx, (nn - 1 - w0, nn - w0)
    if L == 2:
        return 0, np.array([-1.0, 1.0]) / Ts, np.zeros(2), (0, 1)
    return 0, np.zeros(1), np.zeros(1), None


def derivatives(x, Ts):
    """k_derivatives (csrc/fte_api.hip) of ONE clip, restated."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    dx, ddx = np.zeros_like(x), np.zeros_like(x)
    if n >= 2:
        dx[1:] = (x[1:] - x[:-1]) / Ts
        dx[0] = dx[1]
    if n >= 3:
        ddx[2:] = (dx[2:] - dx[1:-1]) / Ts
        ddx[0] = ddx[1] = ddx[2]
        dx[0] = dx[1] - Ts * ddx[2]
    return dx, ddx


def derivatives_from_rows(x, Ts):
    """dx, ddx of one clip from coef_rows: what the covariances below are the covariances OF."""
    L = x.shape[0]
    dx, ddx = np.zeros_like(x), np.zeros_like(x)
    for n in range(L):
        w0, c_dx, c_ddx, _ = coef_rows(n, L, Ts)
        win = x[w0:w0 + len(c_dx)]
        dx[n] = c_dx @ win
        ddx[n] = c_ddx @ win
    return dx, ddx


def _clip_of(n, N, clip_len):
    L = int(clip_len) if clip_len else int(N)
    return (n // L) * L, L


def window_sigma(ab, fixed, frames, clip_len=0, how="dense"):
    """[(global frames of the window, Sigma_win)] for the chosen frames; pinned rows / columns are 0."""
    N = fixed.shape[0]
    n_tot = ab.shape[1]
    wins = []
    for n in frames:
        c0, L = _clip_of(int(n), N, clip_len)
        w0 = coef_rows(int(n) - c0, L, 1.0)[0]
        wins.append(c0 + w0 + np.arange(min(3, L)))
    if how == "dense":
        assert N <= 160, "dense inverse: N <= 160 frames"
        Ai = np.linalg.inv(ref.dense(ab))
        pick = lambda cols, j: Ai[np.ix_(cols, cols)]
    else:
        width = sum(len(w) for w in wins) * P
        rhs = np.zeros((n_tot, width))
        offs, o = [], 0
        for w in wins:
            cols = (w[:, None] * P + np.arange(P)).reshape(-1)
            rhs[cols, o + np.arange(len(cols))] = 1.0
            offs.append(o)
            o += len(cols)
        if how == "lu":
            bw = ab.shape[0] - 1
            full = np.zeros((2 * bw + 1, n_tot))
            full[bw:] = ab
            for d in range(1, bw + 1):
                full[bw - d, d:] = ab[d, :n_tot - d]
            sol = solve_banded((bw, bw), full, rhs, check_finite=False)
        else:
            assert how == "chol"
            sol = solveh_banded(ab, rhs, lower=True, check_finite=False)
        pick = lambda cols, j: sol[cols, offs[j]:offs[j] + len(cols)]
    out = []
    for j, w in enumerate(wins):
        cols = (w[:, None] * P + np.arange(P)).reshape(-1)
        S = np.array(pick(cols, j))
        free = ~fixed[w].reshape(-1)
        out.append((w, S * free[:, None] * free[None, :]))
    return out


def rates_from_windows(wins, x, frames, Ts, clip_len=0):
    """cov_dx, cov_ddx [F,25,25], cov_vel [F,20,3,3], std_vel [F,20] of the chosen frames from their Sigma_win."""
    N = x.shape[0]
    F = len(frames)
    cov_dx, cov_ddx = np.zeros((F, P, P)), np.zeros((F, P, P))
    cov_vel = np.zeros((F, NL, 3, 3))
    for j, n in enumerate(frames):
        c0, L = _clip_of(int(n), N, clip_len)
        w, S = wins[j]
        m = len(w)
        _, c_dx, c_ddx, vel = coef_rows(int(n) - c0, L, Ts)
        S4 = S.reshape(m, P, m, P)
        cov_dx[j] = np.einsum("s,spuq,u->pq", c_dx, S4, c_dx)
        cov_ddx[j] = np.einsum("s,spuq,u->pq", c_ddx, S4, c_ddx)
        if vel is not None:
            J = ref.fk_jacobian_exact(x[[w[vel[0]], w[vel[1]]]])            # [2, 20, 3, 25]
            G = np.zeros((NL, 3, m, P))
            G[:, :, vel[0]] = -J[0] / Ts
            G[:, :, vel[1]] = J[1] / Ts
            G = G.reshape(NL, 3, m * P)
            cov_vel[j] = np.einsum("lia,ab,ljb->lij", G, S, G)
    std_vel = np.sqrt(np.maximum(np.einsum("nlii->nl", cov_vel), 0.0))
    return cov_dx, cov_ddx, cov_vel, std_vel


def reference(ab, fixed, x, Ts, frames=None, clip_len=0, how="dense"):
    frames = np.arange(fixed.shape[0]) if frames is None else np.asarray(frames, dtype=np.int64)
    return rates_from_windows(window_sigma(ab, fixed, frames, clip_len, how), x, frames, Ts, clip_len)


def factor_form(ab, fixed, x, Ts, clip_len=0):
    """The kernels' way, in numpy (dense A: N <= 160): per clip, nodes of 3 frames (a ragged last node simply smaller), the
    corrections CF, CB of the two sweeps as W^T W, and per node k with its predecessor
        F_k-1 = D_k-1 - CF_k-1 = L1 L1^T,   S_k = D_k - CF_k - CB_k = L2 L2^T,
        Y1 = L1^-1 c_a^T,   Y2 = L2^-1 (c_b^T - E^T L1^-T Y1),   cov = Y1^T Y1 + Y2^T Y2
    with the columns of c that belong to pinned variables zeroed.  Never a difference of blocks of A^-1."""
    N = fixed.shape[0]
    A = ref.dense(ab)
    Lc = int(clip_len) if clip_len else N
    cov_dx, cov_ddx = np.zeros((N, P, P)), np.zeros((N, P, P))
    cov_vel = np.zeros((N, NL, 3, 3))
    J = ref.fk_jacobian_exact(x)
    low = lambda Mx: cholesky(Mx, lower=True)
    for c0 in range(0, N, Lc):
        edges = list(range(c0, c0 + Lc, 3)) + [c0 + Lc]
        M = len(edges) - 1
        sl = [slice(edges[k] * P, edges[k + 1] * P) for k in range(M)]
        D = [A[sl[k], sl[k]] for k in range(M)]
        E = [A[sl[k], sl[k + 1]] for k in range(M - 1)]
        CF = [np.zeros_like(D[k]) for k in range(M)]
        CB = [np.zeros_like(D[k]) for k in range(M)]
        for k in range(M - 1):
            W = solve_triangular(low(D[k] - CF[k]), E[k], lower=True)
            CF[k + 1] = W.T @ W
        for k in range(M - 1, 0, -1):
            W = solve_triangular(low(D[k] - CB[k]), E[k - 1].T, lower=True)
            CB[k - 1] = W.T @ W
        for k in range(M):
            L2 = low(D[k] - CF[k] - CB[k])
            L1 = low(D[k - 1] - CF[k - 1]) if k > 0 else None
            lo_f = edges[k - 1] if k > 0 else edges[k]                      # first frame the pair of nodes covers
            na = (edges[k] - lo_f) * P
            free = ~fixed[lo_f:edges[k + 1]].reshape(-1)

            def quad(c):                                                   # c [rows, frames of the pair * 25]
                c = c * free[None, :]
                ca, cb = c[:, :na], c[:, na:]
                if k > 0:
                    Y1 = solve_triangular(L1, ca.T, lower=True)
                    Y2 = solve_triangular(L2, cb.T - E[k - 1].T @ solve_triangular(L1.T, Y1, lower=False), lower=True)
                    return Y1.T @ Y1 + Y2.T @ Y2
                Y2 = solve_triangular(L2, cb.T, lower=True)
                return Y2.T @ Y2

            nf = edges[k + 1] - lo_f
            for n in range(edges[k], edges[k + 1]):
                w0, c_dx, c_ddx, vel = coef_rows(n - c0, Lc, Ts)
                s0 = c0 + w0 - lo_f                                         # slot of the window's first frame in the pair
                assert s0 >= 0
                for coef, out in ((c_dx, cov_dx), (c_ddx, cov_ddx)):
                    c = np.zeros((P, nf, P))
                    for m, cm in enumerate(coef):
                        c[np.arange(P), s0 + m, np.arange(P)] = cm
                    out[n] = quad(c.reshape(P, nf * P))
                if vel is not None:
                    c = np.zeros((NL, 3, nf, P))
                    c[:, :, s0 + vel[0]] = -J[c0 + w0 + vel[0]] / Ts
                    c[:, :, s0 + vel[1]] = J[c0 + w0 + vel[1]] / Ts
                    full = quad(c.reshape(NL * 3, nf * P))
                    for l in range(NL):
                        cov_vel[n, l] = full[3 * l:3 * l + 3, 3 * l:3 * l + 3]
    std_vel = np.sqrt(np.maximum(np.einsum("nlii->nl", cov_vel), 0.0))
    return cov_dx, cov_ddx, cov_vel, std_vel


def errs(got, want):
    """fte_cov_ref.rel_err per output: cov_dx, cov_ddx, cov_vel (per marker block), std_vel (per frame)."""
    out = []
    for i, (g, w) in enumerate(zip(got, want)):
        g, w = np.asarray(g), np.asarray(w)
        if i == 2:
            g, w = g.reshape(-1, 9), w.reshape(-1, 9)
        out.append(ref.rel_err(g, w))
    return out
