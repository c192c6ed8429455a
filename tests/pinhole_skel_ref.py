"""Numpy reference of the skeleton FTE (oracle/skel_fte.py) on the OpenCV pinhole camera.

``PinholeSkelFTEProblem`` is oracle.skel_fte.SkelFTEProblem with the camera swapped: ``measurement_terms`` projects with
pinhole_fte_ref.project_with_jac (oracle.camera.project_points and its closed-form 2x3 Jacobian) in place of the
reference's fisheye ``pt3d_to_2d``; the L1 residual, the IRLS curvature w^2 / max(|e|, l1_eps), the singular-plane cut
|z_cam| < 1e-9 and everything outside the measurement terms (smoothness, bounds, the LM controller) are the oracle's.  The
``r^2 + 1e-12`` of pt3d_to_2d is a detail of the fisheye formula and has no counterpart here.
"""
import numpy as np

from oracle import skel_fte as osf

import pinhole_fte_ref as pref


class PinholeSkelFTEProblem(osf.SkelFTEProblem):
    """SkelFTEProblem on pinhole cameras: D[C] are OpenCV distortion vectors (4, 5, 8 or 12 entries)."""

    def __init__(self, skel, meas, weights, K, D, R, t, h, **kw):
        C = np.asarray(K).shape[0]
        self.D_pin = np.stack([pref.dist12(D[c]) for c in range(C)])
        super().__init__(skel, meas, weights, K, np.zeros((C, 4)), R, t, h, **kw)

    def measurement_terms(self, xa, need_jac=True, chunk=2048, per_frame=False):
        N, P = xa.shape
        cost, cost_n = 0.0, np.zeros(N)
        g = np.zeros((N, P))
        H = np.zeros((N, P, P)) if need_jac else None
        n_behind = 0
        for s in range(0, N, chunk):
            sl = slice(s, min(N, s + chunk))
            pos, Jfk, _ = osf.skeleton_fk_jac(self.skel, self.full_state(xa[sl]))
            G = Jfk[..., self.ACT]                                   # [n, L, 3, P]
            for ci in range(self.C):
                with np.errstate(divide="ignore", invalid="ignore"):
                    uv, Jpi, zc = pref.project_with_jac(pos, self.K[ci], self.D_pin[ci], self.R[ci], self.t[ci])
                w = self.w[sl, ci]
                n_behind += int(((zc < 1e-6) & (w > 0)).sum())
                sing = np.abs(zc) < 1e-9
                w = np.where(sing, 0.0, w)
                res = np.where(sing[..., None], 0.0, uv - self.meas[sl, ci])
                e = w[..., None] * res
                ae = np.abs(e)
                cost += float(ae.sum())
                if per_frame:
                    cost_n[sl] += ae.sum(axis=(1, 2))
                if need_jac:
                    Jpi = np.where(sing[..., None, None], 0.0, Jpi)
                    J = np.einsum("nlij,nljp->nlip", Jpi, G)
                    g[sl] += np.einsum("nlip,nli->np", J, w[..., None] * np.sign(e))
                    hw = (w[..., None] ** 2) / np.maximum(ae, self.l1_eps)
                    H[sl] += np.einsum("nlip,nli,nliq->npq", J, hw, J)
        return (cost_n if per_frame else cost), g, H, n_behind
