"""References for the covariances of the EKF + RTS smoother (numpy, no GPU): csrc/ekf_cov.hip is held to the mathematics
of its OWN inputs, one smoothed frame at a time, as tests/ekf_step_ref.py holds the filter.

* ``smooth_cov_step``  one step P_est[i] + A_i (P_s[i+1] - P_pred[i+1]) A_i^T in extended precision with the entrywise
                       bound on what fp64 may lose in it in any order of summation;
* ``joint_marginals``  the marginal covariances of the dense joint Gaussian posterior of the linearised model - what the
                       recursion has to reproduce on the frames 1 .. N-1 if the formula is the right one;
* ``marker_cov``       J P[:25, :25] J^T per marker from the oracle's product-rule Jacobian, in extended precision;
* ``fp64_chain``       the filter (25 x 25 form, lower triangle mirrored as the kernel's is) and the smoothed covariances
                       of one clip in numpy fp64, with the pieces ``joint_marginals`` needs;
* ``loewner_min``      the smallest eigenvalue of the scaled P_est - P_s (smoothing may only shrink a covariance).

The marker tolerance of tests/test_gpu_ekf_cov.py is the named constant below: 100 x the deviation of numpy's fp64
J P J^T from the extended one, measured by tests/test_ekf_cov_host.py on every run (which asserts that it still lies
under constant / 100).  The factor 100 is the step tests' rule: the kernel forms J from cross products of rotation axes
and lever arms in its own order, the oracle by the product rule.
"""
import numpy as np

import ekf_step_ref as ref
from oracle import ekf as oekf
from oracle import fk as ofk

NS, N_POSE = 75, 25
LD = np.longdouble

# max |d cov_pos| / (|J| |P| |J|^T) entrywise.  Floor: numpy fp64 in three orders of evaluation ((J P) J^T, J (P J^T), one
# einsum) against ``marker_cov`` on every frame and both covariances of the host test's chains: measured 9.77e-16 (a
# double sum of 625 products: nine units of 2^-53 = 1.1e-16), recorded as 1.0e-15.  The MI355X's largest deviation is
# 1.3e-14 (tests/test_gpu_ekf_cov.py).
MARKER_FLOOR = 1.0e-15
MARKER_TOL = 100 * MARKER_FLOOR


def smooth_cov_step(P_est_i, A_i, P_s_next, sT):
    """(want, bound): the step in np.longdouble and, per entry,
    4 * (2 * 76 + 8) * 2^-53 * (|P_est| + |A| (|P_s_next| + |F| |P_est| |F|^T + Q) |A|^T): what two chained 76-term fp64
    sums of products and the rebuilt P_pred (8 more operations per entry) may lose in any order."""
    _, Q, F = oekf.model_matrices(sT)
    Pe, A, Pn = (np.asarray(v, dtype=np.float64).astype(LD) for v in (P_est_i, A_i, P_s_next))
    F, Q = F.astype(LD), Q.astype(LD)
    want = Pe + A @ (Pn - (F @ Pe @ F.T + Q)) @ A.T
    mag = np.abs(Pe) + np.abs(A) @ (np.abs(Pn) + np.abs(F) @ np.abs(Pe) @ np.abs(F).T + Q) @ np.abs(A).T
    return want, (4 * (2 * 76 + 8) * 2.0 ** -53 * mag).astype(np.float64)


def joint_marginals(Hs, Rds, P0, sT):
    """Marginal covariances [N, 75, 75] of the joint posterior of x_0 .. x_(N-1) under x_i = F x_(i-1) + w, w ~ N(0, Q), the
    state before the first prediction ~ N(., P0), and y_i = Hs[i] x_i + v, v ~ N(0, diag Rds[i]).  Q has rank 25, so the
    covariance form: the prior Cov(x_j, x_i) = F^(j-i) Pi_i for j >= i, Pi_i = F Pi_(i-1) F^T + Q (Pi_-1 = P0), then
    Sigma - Sigma H^T (H Sigma H^T + R)^-1 H Sigma."""
    _, Q, F = oekf.model_matrices(sT)
    n = len(Hs)
    Pi, prev = [], np.asarray(P0, dtype=np.float64)
    for _ in range(n):
        prev = F @ prev @ F.T + Q
        Pi.append(prev)
    Sigma = np.zeros((n * NS, n * NS))
    for i in range(n):
        blk = Pi[i]
        for j in range(i, n):
            Sigma[j * NS:(j + 1) * NS, i * NS:(i + 1) * NS] = blk
            Sigma[i * NS:(i + 1) * NS, j * NS:(j + 1) * NS] = blk.T
            blk = F @ blk
    rows = [h.shape[0] for h in Hs]
    H = np.zeros((sum(rows), n * NS))
    r0 = 0
    for i, h in enumerate(Hs):
        H[r0:r0 + rows[i], i * NS:(i + 1) * NS] = h
        r0 += rows[i]
    SH = Sigma @ H.T
    S = H @ SH + np.diag(np.concatenate(Rds))
    post = Sigma - SH @ np.linalg.solve(S, SH.T)
    return np.stack([post[i * NS:(i + 1) * NS, i * NS:(i + 1) * NS] for i in range(n)])


def marker_jacobian(state):
    """d marker positions / d pose parameters [20, 3, 25] (qb_list order) at state[:25]: the oracle's product-rule Jacobian."""
    q = np.zeros(ofk.N_STATES)
    q[oekf.EKF_ORDER] = np.asarray(state, dtype=np.float64)[:N_POSE]
    return ofk.cheetah_fk(q, with_jac=True)[1][:, :, oekf.EKF_ORDER]


def marker_cov(state, P):
    """(cov [20, 3, 3], scale [20, 3, 3]): J P[:25, :25] J^T in np.longdouble and |J| |P| |J|^T, the scale of its rounding."""
    J = marker_jacobian(state).astype(LD)
    Pq = np.asarray(P, dtype=np.float64)[:N_POSE, :N_POSE].astype(LD)
    cov = np.einsum("lip,pq,ljq->lij", J, Pq, J)
    scale = np.einsum("lip,pq,ljq->lij", np.abs(J), np.abs(Pq), np.abs(J))
    return cov, scale.astype(np.float64)


def marker_cov_fp64(state, P):
    """numpy's fp64 J P J^T in three orders of evaluation [3, 20, 3, 3]: what the floor is measured on."""
    J = marker_jacobian(state)
    Pq = np.asarray(P, dtype=np.float64)[:N_POSE, :N_POSE]
    return np.stack([np.stack([(Jl @ Pq) @ Jl.T for Jl in J]), np.stack([Jl @ (Pq @ Jl.T) for Jl in J]),
                     np.einsum("lip,pq,ljq->lij", J, Pq, J)])


def mirror_lower(P):
    """The lower triangle mirrored: how the forward kernel and the covariance kernel make their results symmetric."""
    return np.tril(P) + np.tril(P, -1).T


def fp64_chain(det, rig, s0, fps=120.0, thresh=0.5, width=2704):
    """The filter of one clip in numpy fp64 from ``ekf_step_ref.linearise`` + ``step_fp64(..., "push")`` and the smoothed
    covariances on top: dict of est [N, 75], P_est, P_s [N, 75, 75], gain [N, 75, 75] (NaN where there is none), and the H
    [rows, 75] and diag R of every frame."""
    n, sT = det.shape[0], 1.0 / fps
    P0, Q, F = oekf.model_matrices(sT)
    est, Pe, Hs, Rds = np.zeros((n, NS)), np.zeros((n, NS, NS)), [], []
    prev, P_prev = np.asarray(s0, dtype=np.float64), P0
    for i in range(n):
        lin = ref.linearise(det[i], rig, fps, thresh, width, prev, P_prev)
        x, P = ref.step_fp64(lin, "push")
        est[i], Pe[i] = x, mirror_lower(P)
        Hs.append(lin["H"])
        Rds.append(lin["Rd"])
        prev, P_prev = est[i], Pe[i]
    Ps, gain = Pe.copy(), np.full((n, NS, NS), np.nan)
    for i in range(n - 2, 0, -1):
        Pp = F @ Pe[i] @ F.T + Q
        gain[i] = Pe[i] @ F.T @ np.linalg.inv(Pp)
        Ps[i] = mirror_lower(Pe[i] + gain[i] @ (Ps[i + 1] - Pp) @ gain[i].T)
    return dict(est=est, P_est=Pe, P_s=Ps, gain=gain, H=Hs, Rd=Rds, P0=P0)


def loewner_min(P_est_i, P_s_i):
    """Smallest eigenvalue of d^-1 (P_est - P_s) d^-1, d = sqrt(diag P_est): >= 0 up to rounding when smoothing shrinks."""
    d = np.sqrt(np.diag(P_est_i))
    M = (np.asarray(P_est_i) - np.asarray(P_s_i)) / np.outer(d, d)
    return float(np.linalg.eigvalsh((M + M.T) / 2).min())
