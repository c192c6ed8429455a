"""CPU reference (numpy / scipy fp64) of acino_skel_fte_link_sensitivity: the sensitivity S = -A^-1 G of a skeleton-FTE trajectory
to the log-scales of its links, the poses' total derivative T_l = G_l S_n + D_l and the covariances a covariance Sigma of the
log-scales gives.  Test infrastructure.

Built only from pieces that are pinned elsewhere: link_scale_ref.oracle_fk / base_offsets (the oracle's FK on a skeleton whose
links carry other offsets: D_l[:, g] is the FK with only group g's offsets kept, minus the root), skel_calib_ref.project (the
projections with Jacobians of skel_cov_ref.fisher_blocks), skel_calib_ref.sens_banded / sens_dense (their right-hand side is
generic in the column count), skel_cov_ref.pose_jacobian and the project's col_err and bar.

theta_g: the log-scale of group g of the links (one group index per two-part link, in link order = the ops of the compiled
program; -1: fixed), theta = 0 the skeleton's own offsets.  Per kept row (n, c, l, d): J_x = J_pi G_l (2 x P),
J_theta = J_pi D_l (2 x K), weight w^2 (the Fisher weight: no residual, no l1_eps); G_n = sum J_x^T w^2 J_theta.
tests/test_skel_links_host.py pins G against central differences and the two solves against each other.  Nothing here comes
from the code under test."""
import numpy as np

import link_scale_ref as lref
import skel_calib_ref as kref
import skel_cov_ref as cref
from skel_calib_ref import D0_REFUSED, bar, col_err  # noqa: F401  (re-exported)
from oracle import skel_fte as osf


def groups_of(skel, groups):
    """int [n_ops] and K ("links", "global" or the array itself): link_scale_ref.groups_of."""
    return lref.groups_of(skel, groups)


def offsets(skel, grp, theta=None, only=None):
    """The links' offsets at the log-scales theta [K] (None: 0); ``only``: every group but that one set to 0."""
    off = lref.base_offsets(skel)
    s = np.ones(len(off))
    if theta is not None:
        s = np.where(grp >= 0, np.exp(np.asarray(theta, dtype=np.float64))[np.maximum(grp, 0)], 1.0)
    if only is not None:
        s = np.where(grp == only, s, 0.0)
    return off * s[:, None]


def positions(prob, xa, grp, theta=None):
    """pos [N, L, 3] of the skeleton at the log-scales theta."""
    return lref.oracle_fk(prob.skel, offsets(prob.skel, grp, theta), prob.full_state(xa))[0]


def direct_term(prob, xa, grp, K):
    """D [N, L, 3, K]: the FK with only group g's offsets kept, minus the root."""
    xa = np.asarray(xa, dtype=np.float64)
    q = prob.full_state(xa)
    return np.stack([lref.oracle_fk(prob.skel, offsets(prob.skel, grp, only=g), q)[0] - xa[:, None, :3] for g in range(K)], axis=-1)


def _kept(prob, pos, ci):
    """(uv, J_pi, w) of camera ci with the dropped rows' weight and Jacobian set to 0."""
    uv, Jpi, zc = kref.project(prob, pos, ci)
    sing = np.abs(zc) < 1e-9
    return uv, np.where(sing[..., None, None], 0.0, Jpi), np.where(sing, 0.0, prob.w[:, ci])


def cross_term(prob, xa, grp, K, D=None):
    """G [N, P, K] at xa, with the Fisher weights w^2 (prob.w, 0 on the singular plane)."""
    xa = np.asarray(xa, dtype=np.float64)
    pos, Jfk, _ = osf.skeleton_fk_jac(prob.skel, prob.full_state(xa))
    Gl = Jfk[..., prob.ACT]                                     # [n, L, 3, P]
    D = direct_term(prob, xa, grp, K) if D is None else D
    G = np.zeros(xa.shape + (K,))
    for ci in range(prob.C):
        _uv, Jpi, w = _kept(prob, pos, ci)
        Jx = np.einsum("nlij,nljp->nlip", Jpi, Gl)
        Jt = np.einsum("nlij,nljg->nlig", Jpi, D)
        G += np.einsum("nlip,nl,nlig->npg", Jx, w ** 2, Jt)
    return G


def cross_term_fd(prob, xa, grp, K, h=1e-6):
    """(G_fd, err): G with J_theta replaced by the central difference (uv(theta + h e_g) - uv(theta - h e_g)) / 2h of the
    projections through oracle_fk at the scaled offsets, and the error model's bound on |G_fd - G| entry by entry: per pixel
    component 8 eps max|uv| / h of rounding (a projection is a handful of operations on numbers of that size) plus
    h^2 max|J_theta| of truncation (theta is a log-scale: every derivative of a pixel in it is of the size of the first),
    carried through the same weighted sum with |J_x|."""
    xa = np.asarray(xa, dtype=np.float64)
    pos, Jfk, _ = osf.skeleton_fk_jac(prob.skel, prob.full_state(xa))
    Gl = Jfk[..., prob.ACT]
    D = direct_term(prob, xa, grp, K)
    side = []
    for sgn in (1.0, -1.0):
        side.append([positions(prob, xa, grp, sgn * h * np.eye(K)[g]) for g in range(K)])
    G, err = np.zeros(xa.shape + (K,)), np.zeros(xa.shape + (K,))
    eps = np.finfo(np.float64).eps
    for ci in range(prob.C):
        uv, Jpi, w = _kept(prob, pos, ci)
        Jx = np.einsum("nlij,nljp->nlip", Jpi, Gl)
        fd = np.stack([(kref.project(prob, side[0][g], ci)[0] - kref.project(prob, side[1][g], ci)[0]) / (2 * h) for g in range(K)], axis=-1)
        keep = w > 0
        fd = np.where(keep[..., None, None], fd, 0.0)
        Jt = np.einsum("nlij,nljg->nlig", Jpi, D)
        delta = 8 * eps * np.abs(uv[keep]).max() / h + h * h * np.abs(Jt[keep]).max()
        G += np.einsum("nlip,nl,nlig->npg", Jx, w ** 2, fd)
        err += np.einsum("nlip,nl->np", np.abs(Jx), w ** 2)[..., None] * delta
    return G, err


def total_derivative(prob, xa, S, D):
    """T [N, L, 3, K] = G_l S_n + D_l through the oracle pose Jacobian."""
    return np.einsum("nlip,npg->nlig", cref.pose_jacobian(prob, np.asarray(xa, dtype=np.float64)), S) + D


def link_cov(S, T, sigma):
    """(cov_x_links [N,P,P], cov_pos_links [N,L,3,3], std_pos_links [N,L]) = S Sigma S^T, T Sigma T^T, sqrt(trace)."""
    cov_x = np.einsum("npi,ij,nqj->npq", S, sigma, S)
    cov_pos = np.einsum("nlai,ij,nlbj->nlab", T, sigma, T)
    return cov_x, cov_pos, np.sqrt(np.maximum(np.einsum("nlii->nl", cov_pos), 0.0))


def random_psd(K, hold=0, seed=0, scale=0.05):
    """A random PSD [K, K] of log-scale covariances (sigmas of the order of ``scale``) with the row and column ``hold`` zero."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((K, K)) * scale
    A[hold, :] = 0.0
    return A @ A.T


def reference(prob, xa, ab, fixed, groups):
    """Both solves on one input, their disagreement d0 and the bar; d0 > 1e-8 refuses the input."""
    grp, K = groups_of(prob.skel, groups)
    xa = np.asarray(xa, dtype=np.float64)
    D = direct_term(prob, xa, grp, K)
    G = cross_term(prob, xa, grp, K, D)
    S1, S2 = kref.sens_banded(ab, fixed, G), kref.sens_dense(ab, fixed, G)
    d0 = col_err(S2, S1)
    assert d0 <= D0_REFUSED, f"the two references disagree by {d0:.2e} on this input: refused"
    return dict(grp=grp, K=K, D=D, G=G, S1=S1, S2=S2, T1=total_derivative(prob, xa, S1, D), T2=total_derivative(prob, xa, S2, D),
                d0=d0, bar=bar(d0))
