"""Reference of the per-frame cheetah pose fit from the detections (fte.pose_fit_pixels, csrc/pose_fit_px.hip), numpy only, on
top of the oracle's FK and the camera terms of the triangulation reference.

    F(x) = 1/sigma_px^2 sum_{(c,l) valid} sum_{k in (u,v)} 1/2 f^2 log1p(r_k^2 / f^2) + 1/2 sum_{p = 3..24} (x_p - m_p)^2 / prior_sigma^2
    r    = pi_c(FK_l(x)) - z_{n,c,l}

over the 25 active states inside the box of the FTE, m the start clipped to the box; a detection is valid when its likelihood is
above thresh and both pixel values are finite; F = inf where a valid detection's marker is behind its camera.  g and A carry the
IRLS weight w = 1 / (1 + r_k^2 / f^2).  All frames of an input are evaluated together: arrays are [N, ...].

    Problem(det, rig, model, x0, ...)  tests/pose_fit_ref_common.py's solver - active_set, solve, delta, free_block - with the
                                       constructor and the objective of this file; n_markers counts the valid detections
    inputs(name), solved(name, mutant), bound(name)   the inputs of the tests, the reference on them, the bound B

The detections and rigs are tests/triangulate_mv_ref.py's, the starts the 3-D fit reference's (tests/pose_fit_ref.py), so
nothing here depends on a kernel."""
import functools

import numpy as np

import pose_fit_ref as pref
import pose_fit_ref_common as common
import triangulate_mv_ref as tref
import unlike_rig as ur
from oracle import fk

NP_, NL = pref.NP_, pref.NL
LO, HI = pref.LO, pref.HI
THRESH, F_SCALE, SIGMA_PX = tref.THRESH, tref.F_SCALE, 5.0
OPTS = dict(prior_sigma=1.0, max_iter=255)       # of every test call (at the default prior_sigma two frames of sub520 run
#                                                  into max_iter)
PSI_COLUMNS = (20, 21, 22, 23, 24)               # the psi states among the active ones (fte.PSI_COLUMNS)


class Problem(common.Problem):
    """The cheetah seen by a rig: the oracle's FK, the constant box of the FTE, the Cauchy loss on every valid pixel coordinate."""
    P = NP_

    def __init__(self, det, rig, model, x0, thresh=THRESH, f_scale=F_SCALE, sigma_px=SIGMA_PX, min_detections=2, **kw):
        self.opt = dict(common.DEFAULTS, min_markers=min_detections, **kw)
        det = np.asarray(det, dtype=np.float64)
        self.N, self.C, self.L = det.shape[:3]
        self.rig, self.model = rig, "fisheye" if model == "fisheye" else "pinhole"
        self.fs, self.sigma_px = float(f_scale), float(sigma_px)
        self.valid = (det[..., 2] > thresh) & np.isfinite(det[..., 0]) & np.isfinite(det[..., 1])      # [N, C, L]
        self.obs = np.where(self.valid[..., None], det[..., :2], 0.0)
        self.n_markers = self.valid.sum((1, 2))
        self.lo, self.hi = np.broadcast_to(LO, (self.N, NP_)), np.broadcast_to(HI, (self.N, NP_))
        self.kappa = 1.0 / self.opt["prior_sigma"] ** 2
        self.x0 = np.clip(np.asarray(x0, dtype=np.float64), self.lo, self.hi)
        self.m = self.x0

    def objective(self, x, need_jac=True):
        """F, g, A, the positions and J_FK [N, L, 3, 25]; with the Jacobian also w [N, C, L, 2], r, and Jpx [N, C, L, 2, 25] =
        d r / d x, zero for an invalid detection."""
        N, C, L = self.N, self.C, self.L
        q = pref.full_state(x)
        if need_jac:
            pos, Jf = fk.cheetah_fk(q, with_jac=True)
            Jfk = Jf[..., pref.ACTIVE]
        else:
            pos, Jfk = fk.cheetah_fk(q), None
        fs2, s2 = self.fs ** 2, self.sigma_px ** 2
        F, behind = np.zeros(N), np.zeros(N, dtype=bool)
        w_all, r_all, Jpx = np.zeros((N, C, L, 2)), np.zeros((N, C, L, 2)), np.zeros((N, C, L, 2, NP_))
        for c in range(C):
            v = self.valid[:, c]
            uv, J, _, zc = tref.camera_terms(pos.reshape(-1, 3), self.rig[0][c], self.rig[1][c], self.rig[2][c], self.rig[3][c],
                                             self.model)
            with np.errstate(all="ignore"):
                r = np.where(v[..., None], uv.reshape(N, L, 2) - self.obs[:, c], 0.0)
                z = r * r / fs2
                F += 0.5 * fs2 * np.log1p(z).sum((1, 2)) / s2
            behind |= (v & ~(zc.reshape(N, L) > 0.0)).any(1)
            r_all[:, c] = r
            w_all[:, c] = np.where(v[..., None], 1.0 / (1.0 + z), 0.0)
            if need_jac:
                Jx = np.einsum("nlki,nlip->nlkp", J.reshape(N, L, 2, 3), Jfk)
                Jpx[:, c] = np.where(v[..., None, None], Jx, 0.0)
        e = (x - self.m)[:, 3:]
        F = F + 0.5 * self.kappa * (e * e).sum(1)
        out = dict(F=np.where(behind, np.inf, F), pos=pos, J=Jfk)
        if need_jac:
            g = np.einsum("nclkp,nclk->np", Jpx, w_all * r_all) / s2
            g[:, 3:] += self.kappa * e
            A = np.einsum("nclkp,nclk,nclkq->npq", Jpx, w_all, Jpx) / s2
            A[:, np.arange(3, NP_), np.arange(3, NP_)] += self.kappa
            out.update(g=g, A=A, w=w_all, r=r_all, Jpx=Jpx)
        return out


def fill_unfitted(x, fitted):
    """The frames without a fit interpolated over the frames that have one (held flat at the ends), the five psi columns
    unwrapped over the fitted frames first: the rule of fte.fill_unfitted_frames."""
    x = np.array(x, dtype=np.float64, copy=True)
    idx = np.arange(len(x))
    for p in range(x.shape[1]):
        col = np.unwrap(x[fitted, p]) if p in PSI_COLUMNS else x[fitted, p]
        x[:, p] = np.interp(idx, idx[fitted], col)
    return x


# ------------------------------------------------------------------------------------------------ inputs of the tests
NAMES = ("fisheye", "fisheye-pushed", "pinhole-pushed", "sub01", "sub520", "wide16", "mono", "mono-pushed")
MONO_CAMERA = 2
MONO_OFFSET = np.concatenate([[0.05, -0.05, 0.05], 0.05 * (-1.0) ** np.arange(NP_ - 3)])


@functools.lru_cache(maxsize=None)
def inputs(name):
    """name -> dict(det [N, C, 20, 3], rig, model, pushed, x0 [N, 25])."""
    kind, _, variant = name.partition("-")
    if kind == "mono":
        base = tref.inputs("fisheye-pushed" if variant == "pushed" else "fisheye")
        return dict(det=np.ascontiguousarray(base["det"][:, [MONO_CAMERA]]), rig=ur.subset(base["rig"], [MONO_CAMERA]),
                    model="fisheye", pushed=base["pushed"], x0=pref.solved("fisheye")["x"] + MONO_OFFSET)
    base, fit = tref.inputs(name), pref.solved(name)
    return dict(det=base["det"], rig=base["rig"], model=base["model"], pushed=base["pushed"],
                x0=fill_unfitted(fit["x"], fit["status"] < 2))


def problem(name, mutant=None, **kw):
    inp = inputs(name)
    rig = inp["rig"] if mutant is None else ur.MUTANTS[mutant](inp["rig"])
    return Problem(inp["det"], rig, inp["model"], inp["x0"], **dict(OPTS, **kw))


@functools.lru_cache(maxsize=None)
def solved(name, mutant=None):
    """The reference on an input (or on a mutant of its rig): the problem, x, status, iters, cost, the objective at x, delta,
    the active set at x."""
    return common.solved(problem(name, mutant))


def bound(name):
    """B of the comparisons on an input: 10 x the largest delta the reference solver reaches on its status-0 frames."""
    return common.bound(solved(name))
