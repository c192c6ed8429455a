"""Reference of the skeleton FTE under the redescending measurement loss (numpy fp64, CPU).  Test infrastructure.

``RobustSkelFTEProblem`` is oracle.skel_fte.SkelFTEProblem with ``measurement_terms`` overridden: with the scaled residual
e = w (pi_c(pose_l(x)) - z)_d of a row the assembly keeps (w != 0 after the problem has zeroed non-finite detections, off the
singular plane |z_cam| < 1e-9) and (rho, rho', h) = oracle.loss.redescending_dloss(e, 3, 10, 20) - the reference's only call,

    cost      sum rho(e)                     a dropped row contributes NOTHING (rho(0) is not 0: the logistic blend leaves a
                                             small constant there, and a row without a weight is not a row of the problem)
    gradient  J^T (w rho'(|e|) sign(e))
    curvature sum w^2 h J^T J,   h = clip((rho'(e) - rho'(0+)) / e, 0, 1)

``PinholeRobustSkelFTEProblem`` is the same on tests/pinhole_skel_ref.PinholeSkelFTEProblem.  Smoothness, bounds, the active
set and the Levenberg-Marquardt controller (oracle.fte.lm_solve) are the oracle's, unchanged.  ``curvature_blocks`` are the
blocks that replace skel_cov_ref.fisher_blocks in skel_cov_ref.banded / dense_blocks / probe_blocks; ``report`` is
tests/skel_reproj_ref.reprojection with the robust report's rule: ``weight`` = h(w res_d) for a row with bit 0 of the flags and
0 otherwise, and the noise variance 1 / wg^2 in ``mahal2`` in place of 2 / wg^2.  Nothing here comes from the code under test.
"""
import numpy as np

from oracle import loss as oloss
from oracle import skel_fte as osf

import pinhole_skel_ref as pskel
import skel_cov_ref as cref
import skel_reproj_ref as rref

ABC = (3.0, 10.0, 20.0)


def _camera(prob):
    return "pinhole" if hasattr(prob, "D_pin") else "fisheye"


def _scene(prob):
    return prob.K, (prob.D_pin if hasattr(prob, "D_pin") else prob.D), prob.R, prob.t


class _RobustTerms:
    """measurement_terms of the two problems: the projection of the camera model the problem carries, the robust loss."""

    def measurement_terms(self, xa, need_jac=True, chunk=2048, per_frame=False):
        N, P = xa.shape
        cost_n = np.zeros(N)
        g = np.zeros((N, P))
        H = np.zeros((N, P, P)) if need_jac else None
        pos, Jfk, _ = osf.skeleton_fk_jac(self.skel, self.full_state(xa))
        G = Jfk[..., self.ACT]                                   # [n, L, 3, P]
        cam, scene = _camera(self), _scene(self)
        n_behind = 0
        for ci in range(self.C):
            uv, Jpi, zc = rref.project(pos, scene, ci, cam)
            w = self.w[:, ci]
            n_behind += int(((zc < 1e-6) & (w > 0)).sum())
            sing = np.abs(zc) < 1e-9
            w = np.where(sing, 0.0, w)
            kept = (w != 0)[..., None]
            res = np.where(sing[..., None], 0.0, uv - self.meas[:, ci])
            e = w[..., None] * res
            rho, drho, h = oloss.redescending_dloss(e, *ABC)
            cost_n += np.where(kept, rho, 0.0).sum(axis=(1, 2))
            if need_jac:
                Jpi = np.where(sing[..., None, None], 0.0, Jpi)
                J = np.einsum("nlij,nljp->nlip", Jpi, G)
                g += np.einsum("nlip,nli->np", J, w[..., None] * drho * np.sign(e))
                H += np.einsum("nlip,nli,nliq->npq", J, (w[..., None] ** 2) * h, J)
        return (cost_n if per_frame else float(cost_n.sum())), g, H, n_behind


class RobustSkelFTEProblem(_RobustTerms, osf.SkelFTEProblem):
    pass


class PinholeRobustSkelFTEProblem(_RobustTerms, pskel.PinholeSkelFTEProblem):
    pass


def problem(sk, model, scene, camera_model="fisheye"):
    """The robust problem of a SkeletonModel (its measurements, weights, step and limits)."""
    cls = PinholeRobustSkelFTEProblem if camera_model == "pinhole" else RobustSkelFTEProblem
    return cls(sk, model.meas, model.weights, *scene, model.h, lo=model.lo, hi=model.hi, model_weight=model.model_weight)


def curvature_blocks(prob, xa):
    """sum w^2 h J^T J per frame at xa: what stands in for skel_cov_ref.fisher_blocks under the redescending loss."""
    return prob.measurement_terms(np.asarray(xa, dtype=np.float64))[2]


def cov_reference(prob, xa, probe_frames=None):
    """skel_cov_ref.reference with the robust blocks (the pin set is the robust problem's own: its gradient, its diagonal)."""
    xa = np.asarray(xa, dtype=np.float64)
    fixed = cref.pin_set(prob, xa)
    ab = cref.banded(prob, curvature_blocks(prob, xa), fixed)
    frames = np.arange(xa.shape[0]) if probe_frames is None else np.asarray(probe_frames)
    Sa = cref.dense_blocks(ab, fixed)
    Sb = cref.probe_blocks(ab, fixed, frames)
    G = cref.pose_jacobian(prob, xa)
    cp, sp = cref.pose_cov(Sa, G)
    return dict(fixed=fixed, ab=ab, Sa=Sa, Sb=Sb, frames=frames, d0=cref.rel_err(Sb, Sa[frames]), G=G, cov_pos=cp, std_pos=sp)


def scaled_residuals(rep, weights):
    """e = w res [N, C, L, 2] of a report, 0 where the row is not kept (bit 0 of the flags)."""
    on = (rep["flags"] & 1) != 0
    return np.where(on[..., None], np.asarray(weights)[..., None] * np.nan_to_num(rep["res"]), 0.0)


def report(skel, x_full, meas, weights, scene, camera_model="fisheye", cov_pos=None, gate_w=1.0):
    """skel_reproj_ref.reprojection under the robust report's rule: ``weight`` added, ``mahal2`` with the variance 1 / wg^2."""
    rep = rref.reprojection(skel, x_full, meas, weights, scene, camera_model, cov_pos=cov_pos, gate_w=gate_w)
    on = (rep["flags"] & 1) != 0
    e = scaled_residuals(rep, weights)
    rep["e"] = e
    rep["weight"] = np.where(on[..., None], oloss.redescending_dloss(e, *ABC)[2], 0.0)
    res, r2 = rep["res"], 1.0 / rep["wg"] ** 2
    if cov_pos is not None:
        S = rep["cov_uv"]
        a00, a11, a01 = S[..., 0, 0] + r2, S[..., 1, 1] + r2, S[..., 0, 1]
        with np.errstate(invalid="ignore"):
            rep["mahal2"] = (a11 * res[..., 0] ** 2 - 2 * a01 * res[..., 0] * res[..., 1] + a00 * res[..., 1] ** 2) / (a00 * a11 - a01 ** 2)
    else:
        rep["mahal2"] = (res ** 2).sum(-1) / r2
    return rep


def mahal2_bar(rep, camera_model):
    """tests/test_gpu_skel_reproj.py's bar with lambda_min(A) >= 1 / wg^2 in place of 2 / wg^2: the first term is 2 wg d bar_uv
    (|r^T A^-1 dr| <= d |dr| wg, twice that in m), the others are unchanged."""
    with np.errstate(invalid="ignore"):
        d = np.sqrt(rep["mahal2"])
    return 2.0 * rep["wg"] * d * rref.BAR_UV[camera_model] + 1e-10 * d * d + 1e-18
