"""CPU reference (numpy / scipy fp64) of acino_skel_fte_calibration_sensitivity: the sensitivity S = -A^-1 G of a skeleton-FTE
trajectory to the camera extrinsics and the covariances S Sigma S^T a calibration covariance gives.  Test infrastructure.

Built only from pieces that are pinned elsewhere: oracle.skel_fte.skeleton_fk_jac, the projections with Jacobians that
skel_cov_ref.fisher_blocks uses (oracle.camera.pt3d_to_2d(with_jac=True); pinhole: pinhole_fte_ref.project_with_jac),
fte_calib_ref.skew, and the matrix and pin set of skel_sample_ref.system.

Camera parameters c = [dw_0, dt_0, ..., dw_C-1, dt_C-1], R_c <- exp([dw]x) R_c, t_c <- t_c + dt.  Per kept row (n, c, l, d):
J_x = J_pi G_l (2 x P), J_c = J_pi R_c^T [ -[R_c p]x | I ] (2 x 6), weight w^2 (the Fisher weight: no residual, no l1_eps);
G_n[:, 6c:6c+6] = sum_{l,d} J_x^T w^2 J_c;  S = -A^-1 G by scipy.linalg.solveh_banded (reference 1) or a dense LU solve
(reference 2, N <= 160), rows of pinned variables 0.  tests/test_skel_calib_host.py pins J_c, the two references and the
translation identity.  Nothing here comes from the code under test.
"""
import numpy as np
from scipy.linalg import solveh_banded

import skel_cov_ref as cref
from fte_calib_ref import col_err, skew  # noqa: F401  (re-exported: the project's column error)
from skel_cov_ref import bar  # noqa: F401
from oracle import camera
from oracle import skel_fte as osf

D0_REFUSED = 1e-8


def project(prob, pos, ci):
    """(uv, J_pi [..., 2, 3] in the world frame, z_cam) of camera ci: the calls of skel_cov_ref.fisher_blocks."""
    if hasattr(prob, "D_pin"):
        import pinhole_fte_ref as pref
        with np.errstate(divide="ignore", invalid="ignore"):
            return pref.project_with_jac(pos, prob.K[ci], prob.D_pin[ci], prob.R[ci], prob.t[ci])
    return camera.pt3d_to_2d(pos, prob.K[ci], prob.D[ci], prob.R[ci], prob.t[ci], with_jac=True)


def camera_jacobian(prob, pos, ci):
    """(uv [..., 2], J_pi [..., 2, 3], J_c [..., 2, 6], z_cam) of camera ci for world points pos[..., 3]."""
    uv, Jpi, zc = project(prob, pos, ci)
    R = np.asarray(prob.R[ci], dtype=np.float64)
    Jcam = Jpi @ R.T                                            # d uv / d (camera-frame point)
    q = pos @ R.T                                               # R_c p
    return uv, Jpi, np.concatenate([-Jcam @ skew(q), Jcam], axis=-1), zc


def cross_term(prob, xa):
    """G [N, P, 6C] at xa, with the Fisher weights w^2 (prob.w, 0 on the singular plane)."""
    xa = np.asarray(xa, dtype=np.float64)
    N, P = xa.shape
    pos, Jfk, _ = osf.skeleton_fk_jac(prob.skel, prob.full_state(xa))
    Gl = Jfk[..., prob.ACT]                                     # [n, L, 3, P]
    G = np.zeros((N, P, 6 * prob.C))
    for ci in range(prob.C):
        _uv, Jpi, Jc, zc = camera_jacobian(prob, pos, ci)
        sing = np.abs(zc) < 1e-9
        w = np.where(sing, 0.0, prob.w[:, ci])
        Jpi = np.where(sing[..., None, None], 0.0, Jpi)
        Jc = np.where(sing[..., None, None], 0.0, Jc)
        Jx = np.einsum("nlij,nljp->nlip", Jpi, Gl)
        G[:, :, 6 * ci:6 * ci + 6] = np.einsum("nlip,nl,nlij->npj", Jx, w ** 2, Jc)
    return G


def _rhs(G, fixed):
    N, P, W = G.shape
    return np.where(fixed[:, :, None], 0.0, -G).reshape(N * P, W)


def sens_banded(ab, fixed, G):
    """Reference 1: S [N, P, 6C] = -A^-1 G by the banded Cholesky solve; rows of pinned variables exactly 0."""
    sol = solveh_banded(ab, _rhs(G, fixed), lower=True, check_finite=False)
    return np.where(fixed[:, :, None], 0.0, sol.reshape(G.shape))


def sens_dense(ab, fixed, G):
    """Reference 2: the same by a dense LU solve (N <= 160 frames)."""
    assert fixed.shape[0] <= 160, "dense solve: N <= 160 frames"
    sol = np.linalg.solve(cref.dense(ab), _rhs(G, fixed))
    return np.where(fixed[:, :, None], 0.0, sol.reshape(G.shape))


def calib_cov(S, sigma, prob, xa):
    """(cov_x_cal [N,P,P], cov_pos_cal [N,L,3,3], std_pos_cal [N,L]) = S Sigma S^T through the oracle pose Jacobian."""
    cov_x = np.einsum("npi,ij,nqj->npq", S, sigma, S)
    cov_pos, std_pos = cref.pose_cov(cov_x, cref.pose_jacobian(prob, np.asarray(xa, dtype=np.float64)))
    return cov_x, cov_pos, std_pos


def translation_gen(R_arr, a):
    """gen = [0, -R_0 a, 0, -R_1 a, ...]: the change of the extrinsics that moves the whole rig by a in the world."""
    R_arr = np.asarray(R_arr, dtype=np.float64)
    gen = np.zeros(6 * R_arr.shape[0])
    for c in range(R_arr.shape[0]):
        gen[6 * c + 3:6 * c + 6] = -R_arr[c] @ np.asarray(a, dtype=np.float64)
    return gen


def identity_error(S, R_arr, a):
    """max |S_n gen - (a, 0, ..., 0)| over all frames and states (the caller asserts that no root state is pinned)."""
    want = np.zeros(S.shape[1])
    want[:3] = a
    return float(np.abs(S @ translation_gen(R_arr, a) - want).max())


def reference(prob, xa, ab, fixed):
    """Both solves on one input, their disagreement d0 and the bar; d0 > 1e-8 refuses the input."""
    G = cross_term(prob, xa)
    S1, S2 = sens_banded(ab, fixed, G), sens_dense(ab, fixed, G)
    d0 = col_err(S2, S1)
    assert d0 <= D0_REFUSED, f"the two references disagree by {d0:.2e} on this input: refused"
    return dict(G=G, S1=S1, S2=S2, d0=d0, bar=bar(d0))
