"""CPU reference (numpy fp64) of acino_fte_reprojection: an FTE iterate seen in image space.

Built from pieces that are pinned elsewhere: oracle.fk.cheetah_fk, oracle.camera.pt3d_to_2d(with_jac=True) (pinhole: the
projection + Jacobian of tests/pinhole_fte_ref.py), oracle.loss.redescending_dloss (its third return value is the
curvature weight h) and the binary weights of oracle.fte.FTEProblem.w.  tests/test_fte_reproj_host.py pins it to itself.
"""
import numpy as np

import pinhole_fte_ref as pref
from oracle import camera as ocam
from oracle import fk as ofk
from oracle import fte as ofte
from oracle import loss as oloss

REDESC = (3.0, 10.0, 20.0)


def positions(x_active):
    q = np.zeros((x_active.shape[0], ofk.N_STATES))
    q[:, ofk.ACTIVE] = x_active
    return ofk.cheetah_fk(q)


def project(pos, rig, c, model="fisheye"):
    """(uv [..., 2], J_pi = d uv / d p [..., 2, 3], z_cam [...]) of camera c for world points pos[..., 3]."""
    K, D, R, t = rig
    with np.errstate(divide="ignore", invalid="ignore"):
        if model == "pinhole":
            return pref.project_with_jac(pos, K[c], D[c], R[c], t[c])
        return ocam.pt3d_to_2d(pos, K[c], np.asarray(D[c]).reshape(-1), R[c], np.asarray(t[c]).reshape(-1), with_jac=True)


def weights(det, n_cams, dlc_thresh=0.5, r_meas=5.0):
    """oracle.fte.FTEProblem.w [N, C, 20]: 1 / r_meas where likelihood > dlc_thresh and the pixel is finite, else 0."""
    prob = ofte.FTEProblem(det[..., :2], det[..., 2], np.tile(np.eye(3), (n_cams, 1, 1)), np.zeros((n_cams, 4)),
                           np.tile(np.eye(3), (n_cams, 1, 1)), np.zeros((n_cams, 3)), 1.0, dlc_thresh=dlc_thresh, R_meas=r_meas)
    return prob.w


def reprojection(x_active, cov_pos, det, rig, model="fisheye", dlc_thresh=0.5, r_meas=5.0, redesc=REDESC):
    """Dict of uv [N,C,20,2], cov_uv [N,C,20,2,2] (None without cov_pos), res, weight [N,C,20,2], mahal2 [N,C,20],
    flags [N,C,20] uint8, and J [N,C,20,2,3], z_cam [N,C,20] for the tests."""
    x = np.asarray(x_active, dtype=np.float64)
    det = np.asarray(det, dtype=np.float64)
    N, C = det.shape[:2]
    pos = positions(x)
    w_all = weights(det, C, dlc_thresh, r_meas)
    meas = det[..., :2]
    finite = np.isfinite(meas).all(-1)
    uv = np.empty((N, C, 20, 2))
    J = np.empty((N, C, 20, 2, 3))
    zc = np.empty((N, C, 20))
    for c in range(C):
        uv[:, c], J[:, c], zc[:, c] = project(pos, rig, c, model)
    sing = np.abs(zc) < 1e-9
    behind = zc < 1e-6
    w = np.where(sing, 0.0, w_all)
    uv = np.where(sing[..., None], np.nan, uv)
    with np.errstate(invalid="ignore"):
        diff = uv - np.where(finite[..., None], meas, 0.0)
    res = np.where((finite & ~sing)[..., None], diff, np.nan)
    sres = w[..., None] * np.where(np.isfinite(diff), diff, 0.0)
    h = oloss.redescending_dloss(sres, *redesc)[2]
    weight = np.where((w > 0)[..., None], h, 0.0)
    R2 = float(r_meas) ** 2
    if cov_pos is not None:
        Cs = 0.5 * (cov_pos + np.swapaxes(cov_pos, -1, -2))
        S = np.einsum("nclij,nljk,nclmk->nclim", J, Cs, J)
        S = 0.5 * (S + np.swapaxes(S, -1, -2))
        S = np.where(sing[..., None, None], np.nan, S)
        a00, a11, a01 = S[..., 0, 0] + R2, S[..., 1, 1] + R2, S[..., 0, 1]
        with np.errstate(invalid="ignore"):
            mahal2 = (a11 * res[..., 0] ** 2 - 2 * a01 * res[..., 0] * res[..., 1] + a00 * res[..., 1] ** 2) / (a00 * a11 - a01 ** 2)
    else:
        S = None
        mahal2 = (res ** 2).sum(-1) / R2
    flags = ((w > 0).astype(np.uint8) | (behind.astype(np.uint8) << 1) | (sing.astype(np.uint8) << 2)).astype(np.uint8)
    return dict(uv=uv, cov_uv=S, res=res, weight=weight, mahal2=mahal2, flags=flags, J=J, z_cam=zc)


def measurement_cost(ref, r_meas=5.0, redesc=REDESC):
    """The measurement term of the objective from a report: sum of rho(res / r_meas) over the components of the weighted
    detections (bit 0), plus rho(0) for each component of the others - the objective counts a dropped detection as a
    residual of 0, and the redescending loss is not 0 there (rho(0) = -0.2034 for (3, 10, 20))."""
    on = (ref["flags"] & 1) != 0
    rho = oloss.redescending_loss(np.where(on[..., None], ref["res"], 0.0) / float(r_meas), *redesc)
    return float(rho.sum())


def small_component_share(ref, r_meas=5.0, e_min=1e-5):
    """Share of the weighted components whose scaled residual e = abs(res) / r_meas is below e_min (where the secant h
    loses its digits), and the mask of those components."""
    on = ((ref["flags"] & 1) != 0)[..., None] & np.ones(2, dtype=bool)
    e = np.abs(np.where(on, ref["res"], np.inf)) / float(r_meas)
    small = on & (e < e_min)
    return float(small.sum()) / max(int(on.sum()), 1), small
