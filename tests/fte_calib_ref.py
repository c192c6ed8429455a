"""CPU reference (numpy / scipy fp64) of acino_fte_calibration_sensitivity: the sensitivity S = -A^-1 G of an FTE trajectory
to the camera extrinsics and the covariances S Sigma_c S^T a calibration covariance gives.  Test infrastructure.

Built from pieces that are pinned elsewhere: oracle.fk.cheetah_fk(with_jac=True), oracle.camera.pt3d_to_2d(with_jac=True)
(pinhole: tests/pinhole_fte_ref.project_with_jac), oracle.loss.redescending_dloss (third return value: the curvature weight
h), the binary weights oracle.fte.FTEProblem.w, and A = fte_cov_ref.banded(...) on blocks WITH the smoothness diagonal.

Camera parameters c = [dw_0, dt_0, ..., dw_C-1, dt_C-1], R_c <- exp([dw]x) R_c, t_c <- t_c + dt.  Per detection (n, c, l):
J_x = J_pi J_l (2 x 25), J_c = J_pi R_c^T [ -[R_c p]x | I ] (2 x 6), weight w^2 h per component;
G_n[:, 6c:6c+6] = sum_l J_x^T (w^2 h) J_c;  S = -A^-1 G by scipy.linalg.solveh_banded (reference 1) or a dense solve
(reference 2, N <= 160), rows of pinned variables 0.  tests/test_fte_calib_host.py pins J_c, the two references and the
translation identity.
"""
import numpy as np
from scipy.linalg import solveh_banded

import fte_cov_ref as cref
import fte_reproj_ref as rref
import fte_sample_ref as sref
import pinhole_fte_ref as pref
from oracle import fk as ofk
from oracle import fte as ofte
from oracle import loss as oloss

P = cref.P
REDESC = rref.REDESC


def skew(v):
    """[v]x for v[..., 3]."""
    v = np.asarray(v, dtype=np.float64)
    z = np.zeros(v.shape[:-1])
    return np.stack([np.stack([z, -v[..., 2], v[..., 1]], -1), np.stack([v[..., 2], z, -v[..., 0]], -1),
                     np.stack([-v[..., 1], v[..., 0], z], -1)], -2)


def rot_exp(w):
    """exp([w]x) (Rodrigues)."""
    w = np.asarray(w, dtype=np.float64)
    th = float(np.linalg.norm(w))
    if th == 0.0:
        return np.eye(3)
    Kx = skew(w / th)
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def problem(det, rig, Ts, model="fisheye"):
    K, D, R, t = rig
    cls = pref.PinholeFTEProblem if model == "pinhole" else ofte.FTEProblem
    return cls(det[..., :2], det[..., 2], K, D, R, t, Ts)


def camera_jacobian(pos, rig, c, model="fisheye"):
    """(uv [..., 2], J_pi [..., 2, 3], J_c [..., 2, 6], z_cam) of camera c for world points pos[..., 3]."""
    uv, Jpi, zc = rref.project(pos, rig, c, model)
    R = np.asarray(rig[2][c], dtype=np.float64)
    Jcam = Jpi @ R.T                                            # d uv / d (camera-frame point)
    q = pos @ R.T                                               # R_c p
    Jc = np.concatenate([-Jcam @ skew(q), Jcam], axis=-1)
    return uv, Jpi, Jc, zc


def cross_term(x_active, det, rig, Ts, model="fisheye"):
    """G [N, 25, 6C] at x, with the weights w (FTEProblem.w, 0 on the singular plane) and h of the solve."""
    x = np.asarray(x_active, dtype=np.float64)
    prob = problem(np.asarray(det, dtype=np.float64), rig, Ts, model)
    N, C = prob.N, prob.C
    pos, Jq = ofk.cheetah_fk(prob.full_state(x), with_jac=True)
    Jl = Jq[..., ofk.ACTIVE]                                    # [N, 20, 3, 25]
    G = np.zeros((N, P, 6 * C))
    for c in range(C):
        uv, Jpi, Jc, zc = camera_jacobian(pos, rig, c, model)
        sing = np.abs(zc) < 1e-9
        w = np.where(sing, 0.0, prob.w[:, c])
        res = np.where(sing[..., None], 0.0, uv - prob.meas[:, c])
        h = oloss.redescending_dloss(w[..., None] * res, *prob.redesc)[2]
        hw = (w[..., None] ** 2) * h
        Jpi = np.where(sing[..., None, None], 0.0, Jpi)
        Jc = np.where(sing[..., None, None], 0.0, Jc)
        Jx = np.einsum("nlij,nljp->nlip", Jpi, Jl)
        G[:, :, 6 * c:6 * c + 6] = np.einsum("nlip,nli,nlij->npj", Jx, hw, Jc)
    return G


def _rhs(G, fixed):
    N, _, W = G.shape
    return np.where(fixed[:, :, None], 0.0, -G).reshape(N * P, W)


def sens_banded(ab, fixed, G):
    """Reference 1: S [N, 25, 6C] = -A^-1 G by the banded Cholesky solve; rows of pinned variables exactly 0."""
    sol = solveh_banded(ab, _rhs(G, fixed), lower=True, check_finite=False)
    return np.where(fixed[:, :, None], 0.0, sol.reshape(G.shape))


def sens_dense(ab, fixed, G):
    """Reference 2: the same by a dense LU solve (N <= 160 frames)."""
    assert fixed.shape[0] <= 160, "dense solve: N <= 160 frames"
    sol = np.linalg.solve(cref.dense(ab), _rhs(G, fixed))
    return np.where(fixed[:, :, None], 0.0, sol.reshape(G.shape))


def col_err(S, S_ref):
    """fte_sample_ref.map_err with the 6C columns in the place of the samples: per column the max over frames of the 2-norm
    error over the max frame norm of the reference column; the worst column."""
    return sref.map_err(np.moveaxis(np.asarray(S), 2, 0), np.moveaxis(np.asarray(S_ref), 2, 0))


def calib_cov(S, sigma, x_active):
    """(cov_x_cal [N,25,25], cov_pos_cal [N,20,3,3], std_pos_cal [N,20]) = S Sigma S^T through the oracle FK Jacobian."""
    cov_x = np.einsum("npi,ij,nqj->npq", S, sigma, S)
    cov_pos, std_pos = cref.marker_cov(cov_x, cref.fk_jacobian_exact(np.asarray(x_active, dtype=np.float64)))
    return cov_x, cov_pos, std_pos


def translation_gen(R_arr, a):
    """gen = [0, -R_0 a, 0, -R_1 a, ...]: the change of the extrinsics that moves the whole rig by a in the world."""
    R_arr = np.asarray(R_arr, dtype=np.float64)
    gen = np.zeros(6 * R_arr.shape[0])
    for c in range(R_arr.shape[0]):
        gen[6 * c + 3:6 * c + 6] = -R_arr[c] @ np.asarray(a, dtype=np.float64)
    return gen


def identity_error(S, fixed, R_arr, a):
    """max over the frames whose head position is free of |S_n gen - (a, 0, ..., 0)|."""
    want = np.zeros(P)
    want[:3] = a
    free = ~fixed[:, :3].any(axis=1)
    assert free.any()
    return float(np.abs(S[free] @ translation_gen(R_arr, a) - want).max())


def random_psd(n_cams, seed=7, hold=(0,)):
    """A fixed-seed PSD [6C, 6C] matrix of the size of a calibration covariance (0.05 deg, 2 mm), full within and across the
    free cameras, with zero rows and columns for the cameras in hold."""
    W = 6 * n_cams
    rng = np.random.default_rng(seed)
    B = rng.normal(size=(W, W)) / np.sqrt(W)
    scale = np.tile(np.r_[np.full(3, np.deg2rad(0.05)), np.full(3, 2e-3)], n_cams)
    for c in hold:
        scale[6 * c:6 * c + 6] = 0.0
    M = (B @ B.T) * scale[:, None] * scale[None, :]
    return 0.5 * (M + M.T)
