"""Reference for the rate covariances of the skeleton FTE (acino_skel_fte_covariance_rates): numpy / scipy on the CPU, on top of
tests/skel_cov_ref.py (Fisher blocks, pin set, banded and dense A).  Test infrastructure; nothing here comes from the code
under test.

With e the estimation error of a clip, Cov(e) = A^-1 (rows / columns of pinned variables 0), the outputs are covariances of
linear maps of a window of at most three consecutive frames:

    dx_n, ddx_n    the rule of build._finite_diff_states (``coef_rows``): cov_dx[n] = C S_win C^T, C = c (x) I
    v_{n,l}        (G_l(x_n) e_n - G_l(x_{n-1}) e_{n-1}) / h, frame 0 repeats frame 1: cov_vel [N, L, 3, 3], std_vel = sqrt(trace)

A variable pinned in frame a contributes nothing from frame a (its row of C^T is 0).  Four ways to the same numbers:
  (a) ``by_dense_inverse``    blocks of np.linalg.inv(A), then differencing
  (b) ``by_banded_probes``    blocks from scipy.linalg.solveh_banded on unit vectors, then differencing
  (s) ``by_recursion``        blocks from the Takahashi recursion of skel_cov_ref._collect with the off-diagonal blocks of the
                              3-frame window kept (what k_skel_selinv leaves in the band), then differencing: the streaming route
  (c) ``by_factor``           cancellation-free: Y = solve_triangular(L, C^T), cov = Y^T Y, L the dense Cholesky factor of A;
      ``reverse=True``        (c'): the same from the factor of A with the frame order reversed
d0 is the disagreement of (c) and (c') on the outputs (rel_err, the largest over the four arrays); bar(d0) = max(64 d0, 1e-13)
is the project's, and refuses d0 > 1e-8.  The GPU is held to (c)."""
import numpy as np
from scipy.linalg import solve_triangular, solveh_banded

import skel_cov_ref as cref
from skel_cov_ref import bar, rel_err  # noqa: F401  (re-exported)

KEYS = ("cov_dx", "cov_ddx", "cov_vel", "std_vel")


def banded(prob, HF, fixed):
    """skel_cov_ref.banded for any N: a clip of fewer than four frames has fewer unknowns than the band is wide (and no row of
    D3 at all: the prior vanishes), so its matrix is stored with the bandwidth it has."""
    N, P = fixed.shape
    if N >= 4:
        return cref.banded(prob, HF, fixed)
    band, q_w = prob.s_band(), prob.q_w
    A = np.zeros((N * P, N * P))
    idx = np.arange(P)
    for n in range(N):
        Hn = np.array(HF[n], dtype=np.float64, copy=True)
        Hn[idx, idx] += 2 * q_w * band[0][n]
        Hn = np.where(fixed[n][:, None] | fixed[n][None, :], 0.0, Hn)
        Hn[idx, idx] = np.where(fixed[n], 1.0, Hn[idx, idx])
        A[n * P:(n + 1) * P, n * P:(n + 1) * P] = Hn
        for k in range(1, N - n):
            v = np.where(fixed[n] | fixed[n + k], 0.0, 2 * q_w * band[k][n])
            A[(n + k) * P + idx, n * P + idx] = v
            A[n * P + idx, (n + k) * P + idx] = v
    return np.stack([np.concatenate([np.diagonal(A, -d), np.zeros(d)]) for d in range(N * P)])


def coef_rows(N, n, h):
    """(frames, c_dx, c_ddx): dx_n = sum_k c_dx[k] x_frames[k], likewise ddx_n - the rule of build._finite_diff_states."""
    if N == 1:
        return (0,), np.zeros(1), np.zeros(1)
    if N == 2:
        return (0, 1), (np.array([-1.0, 1.0]) / h if n == 1 else np.zeros(2)), np.zeros(2)
    dd = np.array([1.0, -2.0, 1.0]) / h ** 2
    if n >= 2:
        return (n - 2, n - 1, n), np.array([0.0, -1.0, 1.0]) / h, dd
    return (0, 1, 2), (np.array([-1.0, 1.0, 0.0]) / h if n == 1 else np.array([-2.0, 3.0, -1.0]) / h), dd


def vel_frame(N, n):
    """The frame whose velocity frame n reports: frame 0 repeats frame 1; None: no velocity (N = 1)."""
    return None if N == 1 else max(n, 1)


def finite_diff(x, h):
    """dx, ddx of x [N, P] through ``coef_rows`` (what the host test compares with build._finite_diff_states)."""
    N = x.shape[0]
    dx, ddx = np.zeros_like(x), np.zeros_like(x)
    for n in range(N):
        fr, c1, c2 = coef_rows(N, n, h)
        dx[n] = sum(c * x[f] for c, f in zip(c1, fr))
        ddx[n] = sum(c * x[f] for c, f in zip(c2, fr))
    return dx, ddx


def _maps(fixed, G, h):
    """Per frame n: [(frame a, K_a)] with K_a [2 P + 3 L, P] the rows of (dx_n, ddx_n, v_n,:) acting on e_a, pins applied."""
    N, P = fixed.shape
    L = G.shape[1]
    out = []
    for n in range(N):
        fr, c1, c2 = coef_rows(N, n, h)
        K = {a: np.zeros((2 * P + 3 * L, P)) for a in fr}
        for a, u, v in zip(fr, c1, c2):
            K[a][:P] = u * np.eye(P)
            K[a][P:2 * P] = v * np.eye(P)
        m = vel_frame(N, n)
        if m is not None:
            K[m][2 * P:] += G[m].reshape(3 * L, P) / h
            K[m - 1][2 * P:] -= G[m - 1].reshape(3 * L, P) / h
        out.append([(a, np.where(fixed[a][None, :], 0.0, K[a])) for a in fr])
    return out


def _pack(full, N, P, L, dependent):
    """[N, 2P + 3L, 2P + 3L] -> the four arrays; ``dependent`` [N, L] (or None): slots whose G touches an unobserved state."""
    cov_dx, cov_ddx = full[:, :P, :P].copy(), full[:, P:2 * P, P:2 * P].copy()
    V = full[:, 2 * P:, 2 * P:].reshape(N, L, 3, L, 3)
    cov_vel = np.stack([V[:, l, :, l, :] for l in range(L)], axis=1)
    std_vel = np.sqrt(np.maximum(np.einsum("nlii->nl", cov_vel), 0.0))
    if dependent is not None and N > 1:
        dep = np.zeros((N, L), dtype=bool)
        for n in range(N):
            m = vel_frame(N, n)
            dep[n] = dependent[m] | dependent[m - 1]
        cov_vel = np.where(dep[:, :, None, None], np.nan, cov_vel)
        std_vel = np.where(dep, np.inf, std_vel)
    return dict(cov_dx=cov_dx, cov_ddx=cov_ddx, cov_vel=cov_vel, std_vel=std_vel)


def by_blocks(blk, fixed, G, h, dependent=None):
    """Differencing: sum_a sum_b K_a S_ab K_b^T with S_ab = blk(a, b) [P, P], |a - b| <= 2."""
    N, P = fixed.shape
    L = G.shape[1]
    full = np.zeros((N, 2 * P + 3 * L, 2 * P + 3 * L))
    for n, rows in enumerate(_maps(fixed, G, h)):
        for a, Ka in rows:
            for b, Kb in rows:
                full[n] += Ka @ blk(a, b) @ Kb.T
    return _pack(full, N, P, L, dependent)


def by_dense_inverse(ab, fixed, G, h, dependent=None):
    P = fixed.shape[1]
    Ai = np.linalg.inv(cref.dense(ab))
    return by_blocks(lambda a, b: Ai[a * P:(a + 1) * P, b * P:(b + 1) * P], fixed, G, h, dependent)


def by_banded_probes(ab, fixed, G, h, dependent=None):
    P = fixed.shape[1]
    Ai = solveh_banded(ab, np.eye(ab.shape[1]), lower=True, check_finite=False)
    return by_blocks(lambda a, b: Ai[a * P:(a + 1) * P, b * P:(b + 1) * P], fixed, G, h, dependent)


def window_blocks(ab, fixed):
    """skel_cov_ref._collect with the blocks S_{n+1,n}, S_{n+2,n} kept beside S_nn: {(a, b): S_ab, a >= b, a - b <= 2}."""
    N, P = fixed.shape
    Lf = np.linalg.cholesky(cref.dense(ab))
    blk = lambda a, b: Lf[a * P:(a + 1) * P, b * P:(b + 1) * P]      # noqa: E731
    S = {}
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
        S[(n, n)] = 0.5 * (Snn + Snn.T)
    return S


def by_recursion(ab, fixed, G, h, dependent=None):
    S = window_blocks(ab, fixed)
    return by_blocks(lambda a, b: S[(a, b)] if a >= b else S[(b, a)].T, fixed, G, h, dependent)


def by_factor(ab, fixed, G, h, dependent=None, reverse=False):
    """(c) / (c'): Y = L^-1 C^T, cov = Y^T Y.  ``reverse``: the factor of A with the frames in reverse order."""
    N, P = fixed.shape
    L = G.shape[1]
    R = 2 * P + 3 * L
    A = cref.dense(ab)
    order = np.arange(N * P)
    if reverse:
        order = order.reshape(N, P)[::-1].reshape(-1)
    Lf = np.linalg.cholesky(A[np.ix_(order, order)])
    Ct = np.zeros((N * P, N * R))
    for n, rows in enumerate(_maps(fixed, G, h)):
        for a, Ka in rows:
            Ct[a * P:(a + 1) * P, n * R:(n + 1) * R] = Ka.T
    Y = solve_triangular(Lf, Ct[order], lower=True, check_finite=False)
    full = np.stack([Y[:, n * R:(n + 1) * R].T @ Y[:, n * R:(n + 1) * R] for n in range(N)])
    return _pack(full, N, P, L, dependent)


def out_err(got, want):
    """{key: error}: rel_err per frame for the three covariances (NaN / inf entries must coincide and are left out), the
    largest relative difference for std_vel."""
    e = {}
    for k in KEYS:
        g, w = np.asarray(got[k], dtype=np.float64), np.asarray(want[k], dtype=np.float64)
        assert g.shape == w.shape, (k, g.shape, w.shape)
        odd = ~np.isfinite(w)
        assert np.array_equal(~np.isfinite(g), odd) and np.array_equal(g[odd], w[odd], equal_nan=True), f"{k}: NaN / inf pattern"
        g, w = np.where(odd, 0.0, g), np.where(odd, 0.0, w)
        N = w.shape[0]
        if k == "std_vel":
            assert np.all(g[w == 0] == 0)
            e[k] = float(np.max(np.abs(g - w)[w > 0] / w[w > 0])) if (w > 0).any() else 0.0
        else:
            gr, wr = g.reshape(N, -1), w.reshape(N, -1)
            e[k] = rel_err(gr, wr) if np.any(wr != 0) else float(np.abs(gr).max())
    return e


def reference(ab, fixed, G, h, dependent=None):
    """(c), (c'), their disagreement d0 on the outputs (per key and the largest), the bar.  d0 > 1e-8 is refused by ``bar``."""
    c = by_factor(ab, fixed, G, h, dependent)
    cr = by_factor(ab, fixed, G, h, dependent, reverse=True)
    d = out_err(cr, c)
    d0 = max(d.values())
    return dict(c=c, c_rev=cr, d0_by_key=d, d0=d0, bar=bar(d0), ab=ab, fixed=fixed, G=G, h=h, dependent=dependent)


def full_layout(cov, act, P_full):
    """[N, Pa, Pa] in the active layout -> [N, P, P] in the full-state layout (what build.model_covariance returns)."""
    out = np.zeros((cov.shape[0], P_full, P_full))
    out[:, np.asarray(act)[:, None], np.asarray(act)[None, :]] = cov
    return out
