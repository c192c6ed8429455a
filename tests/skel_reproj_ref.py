"""CPU reference (numpy fp64) of acino_skel_fte_reprojection: a skeleton-FTE iterate seen in image space.  Test infrastructure.

Built only from the oracle: the poses - and nothing else - of oracle.skel_fte.skeleton_fk_jac, oracle.camera.pt3d_to_2d(...,
with_jac=True) for the fisheye cameras, tests/pinhole_fte_ref.project_with_jac for the pinhole ones.  ``cov_uv`` is formed from
the cov_pos array the caller hands in - the SAME array that goes to the kernel - so that the kernel's error is seen apart from
the covariance's.  tests/test_skel_reproj_host.py pins this module to itself.

Per entry (frame n, camera c, pose slot l), with z, w the detection and its weight, finite = both components of z finite,
sing = |z_cam| < 1e-9 and wg = (w > 0 ? w : gate_w):
    uv      the projection; NaN where sing
    cov_uv  J_pi sym(cov_pos[n][l]) J_pi^T; NaN where sing
    res     uv - z where finite and not sing, else NaN
    mahal2  res^T (cov_uv + (2 / wg^2) I)^-1 res;  without cov_pos: res^T res wg^2 / 2
    flags   bit 0: w != 0, finite and not sing (the rows the assembly keeps); bit 1: z_cam < 1e-6; bit 2: sing
"""
import numpy as np

import pinhole_fte_ref as pref
from oracle import camera as ocam
from oracle import skel_fte as osf

BAR_UV = {"fisheye": 1e-9, "pinhole": 1e-8}     # px: tests/test_gpu_parity.py's bars for the two projections


def project(pos, scene, c, camera_model="fisheye"):
    """(uv [..., 2], J_pi = d uv / d p [..., 2, 3], z_cam [...]) of camera c for world points pos[..., 3]."""
    K, D, R, t = scene
    with np.errstate(divide="ignore", invalid="ignore"):
        if camera_model == "pinhole":
            return pref.project_with_jac(pos, K[c], pref.dist12(D[c]), R[c], np.asarray(t[c]).reshape(-1))
        return ocam.pt3d_to_2d(pos, K[c], np.asarray(D[c]).reshape(-1), R[c], np.asarray(t[c]).reshape(-1), with_jac=True)


def reprojection(skel, x_full, meas, weights, scene, camera_model="fisheye", cov_pos=None, gate_w=1.0):
    """Dict of uv [N,C,L,2], cov_uv [N,C,L,2,2] and std_uv [N,C,L] (None without cov_pos), res [N,C,L,2], mahal2 [N,C,L],
    flags [N,C,L] uint8, and J [N,C,L,2,3], z_cam, wg [N,C,L] for the tests.  ``x_full`` [N, 3 + 3 L_angles], ``meas`` raw."""
    meas = np.asarray(meas, dtype=np.float64)
    w = np.asarray(weights, dtype=np.float64)
    N, C, L, _ = meas.shape
    pos = osf.skeleton_fk_jac(skel, np.asarray(x_full, dtype=np.float64))[0]
    assert pos.shape == (N, L, 3)
    uv, J, zc = np.empty((N, C, L, 2)), np.empty((N, C, L, 2, 3)), np.empty((N, C, L))
    for c in range(C):
        uv[:, c], J[:, c], zc[:, c] = project(pos, scene, c, camera_model)
    finite = np.isfinite(meas).all(-1)
    sing = np.abs(zc) < 1e-9
    behind = zc < 1e-6
    uv = np.where(sing[..., None], np.nan, uv)
    with np.errstate(invalid="ignore"):
        res = np.where((finite & ~sing)[..., None], uv - np.where(finite[..., None], meas, 0.0), np.nan)
    wg = np.where(w > 0, w, float(gate_w))
    r2 = 2.0 / wg ** 2
    if cov_pos is not None:
        Cs = 0.5 * (cov_pos + np.swapaxes(cov_pos, -1, -2))
        S = np.einsum("nclij,nljk,nclmk->nclim", J, Cs, J)
        S = 0.5 * (S + np.swapaxes(S, -1, -2))
        S = np.where(sing[..., None, None], np.nan, S)
        a00, a11, a01 = S[..., 0, 0] + r2, S[..., 1, 1] + r2, S[..., 0, 1]
        with np.errstate(invalid="ignore"):
            mahal2 = (a11 * res[..., 0] ** 2 - 2 * a01 * res[..., 0] * res[..., 1] + a00 * res[..., 1] ** 2) / (a00 * a11 - a01 ** 2)
            std = np.sqrt(np.maximum(S[..., 0, 0] + S[..., 1, 1], 0.0))
    else:
        S = std = None
        mahal2 = (res ** 2).sum(-1) / r2
    on = (w != 0) & finite & ~sing
    flags = (on.astype(np.uint8) | (behind.astype(np.uint8) << 1) | (sing.astype(np.uint8) << 2)).astype(np.uint8)
    return dict(uv=uv, cov_uv=S, std_uv=std, res=res, mahal2=mahal2, flags=flags, J=J, z_cam=zc, wg=wg)


def measurement_cost(rep, weights):
    """The L1 measurement term of the objective from a report: sum over the entries with bit 0 of w (|res_u| + |res_v|)."""
    on = (rep["flags"] & 1) != 0
    return float((np.asarray(weights)[on][:, None] * np.abs(rep["res"][on])).sum())


def mahal2_bar(ref, camera_model):
    """The bar of tests/test_gpu_skel_reproj.py on |mahal2 - reference|, per entry (derived in that module's docstring)."""
    with np.errstate(invalid="ignore"):
        d = np.sqrt(ref["mahal2"])
    return np.sqrt(2.0) * ref["wg"] * d * BAR_UV[camera_model] + 1e-10 * d * d + 1e-18
