"""Reference of the per-frame skeleton pose fit from the detections of every camera (build.pose_fit_pixels,
csrc/skel_pose_fit_px.hip), numpy only, on top of the oracle's skeleton FK (oracle.skel_fte.skeleton_fk_jac) and the camera terms
of the triangulation reference (tests/triangulate_mv_ref.py): the generic form of tests/pose_fit_px_ref.py.

    F(x) = 1/sigma_px^2 sum_{(c,l) valid} sum_{k in (u,v)} 1/2 f^2 log1p(r_k^2 / f^2) + 1/2 sum_{p >= 3} (x_p - m_p)^2 / prior_sigma^2
    r    = pi_c(FK_l(x)) - det[n, c, l, :2]

over the P active states inside the box lo[n] <= x <= hi[n], m the start clipped to the box; a detection is valid when its
likelihood is above thresh and both pixel values are finite; F = inf where a valid detection's slot is behind its camera.  g and A
carry the IRLS weight w = 1 / (1 + r_k^2 / f^2).  All frames of an input are evaluated together: arrays are [N, ...].

    Problem(skel, det, rig, model, lo, hi, x0, ...)  tests/pose_fit_ref_common.py's solver - active_set, solve, delta,
                                       free_block - with the constructor and the objective of this file; n_markers counts the
                                       valid detections
    inputs(name), solved(name, mutant), bound(name)   the inputs of the tests, the reference on them, the bound B

The inputs are synthetic - a truth state per frame, pixels = projection + noise - and depend on no kernel."""
import functools

import numpy as np

import pose_fit_ref_common as common
import skel_pose_fit_ref as sref
import triangulate_mv_ref as tref
import unlike_rig as ur
from oracle import skel_fte as osf
from oracle import synth as osynth

THRESH, F_SCALE, SIGMA_PX = 0.5, 5.0, 5.0        # sigma_px: pose_fit_px_ref's (fte.R_MEAS).  It sets cond(A_free), the detections'
#                                                  information over the ridge's: 1.5e5 on generic-fisheye, where the reference
#                                                  solved on a translated rig keeps inv(A_free) to 2.4e-12; at 2 px cond is 9.6e5
#                                                  and the reference itself misses the 1e-11 of the GPU test's identity (1.7e-11)
OPTS = dict(prior_sigma=1.0, max_iter=255)       # of every test call, as in the other fit tests
N_FRAMES = 24
NOISE_PX, DROP = 2.0, 0.2


class Problem(common.Problem):
    """A skeleton seen by a rig: the oracle's link program on the model's active states, a box per frame, the Cauchy loss on
    every valid pixel coordinate."""

    def __init__(self, skel, det, rig, model, lo, hi, x0, thresh=THRESH, f_scale=F_SCALE, sigma_px=SIGMA_PX, min_detections=2,
                 **kw):
        self.opt = dict(common.DEFAULTS, min_markers=min_detections, **kw)
        self.skel = skel
        self.ACT = osf.active_states(skel)
        self.P = len(self.ACT)
        self.P_full = 3 + 3 * len(skel["positions"])
        det = np.asarray(det, dtype=np.float64)
        self.N, self.C, self.L = det.shape[:3]
        self.rig, self.model = rig, "fisheye" if model == "fisheye" else "pinhole"
        self.fs, self.sigma_px = float(f_scale), float(sigma_px)
        self.valid = (det[..., 2] > thresh) & np.isfinite(det[..., 0]) & np.isfinite(det[..., 1])      # [N, C, L]
        self.obs = np.where(self.valid[..., None], det[..., :2], 0.0)
        self.n_markers = self.valid.sum((1, 2))
        self.lo, self.hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
        self.kappa = 1.0 / self.opt["prior_sigma"] ** 2
        self.x0 = np.clip(np.asarray(x0, dtype=np.float64), self.lo, self.hi)
        self.m = self.x0

    def fk(self, xa, with_jac=False):
        q = np.zeros(xa.shape[:-1] + (self.P_full,))
        q[..., self.ACT] = xa
        pos, J, _ = osf.skeleton_fk_jac(self.skel, q)
        return (pos, J[..., self.ACT]) if with_jac else pos

    def objective(self, x, need_jac=True):
        """F, g, A, the positions and G [N, L, 3, P]; with the Jacobian also w [N, C, L, 2], r, zc [N, C, L] and
        Jpx [N, C, L, 2, P] = d r / d x, zero for an invalid detection."""
        N, C, L, P = self.N, self.C, self.L, self.P
        if need_jac:
            pos, G = self.fk(x, with_jac=True)
        else:
            pos, G = self.fk(x), None
        fs2, s2 = self.fs ** 2, self.sigma_px ** 2
        F, behind = np.zeros(N), np.zeros(N, dtype=bool)
        w_all, r_all, z_all = np.zeros((N, C, L, 2)), np.zeros((N, C, L, 2)), np.zeros((N, C, L))
        Jpx = np.zeros((N, C, L, 2, P)) if need_jac else None
        for c in range(C):
            v = self.valid[:, c]
            uv, J, _, zc = tref.camera_terms(pos.reshape(-1, 3), self.rig[0][c], self.rig[1][c], self.rig[2][c], self.rig[3][c],
                                             self.model)
            with np.errstate(all="ignore"):
                r = np.where(v[..., None], uv.reshape(N, L, 2) - self.obs[:, c], 0.0)
                z = r * r / fs2
                F += 0.5 * fs2 * np.log1p(z).sum((1, 2)) / s2
            behind |= (v & ~(zc.reshape(N, L) > 0.0)).any(1)
            r_all[:, c], z_all[:, c] = r, zc.reshape(N, L)
            w_all[:, c] = np.where(v[..., None], 1.0 / (1.0 + z), 0.0)
            if need_jac:
                Jx = np.einsum("nlki,nlip->nlkp", J.reshape(N, L, 2, 3), G)
                Jpx[:, c] = np.where(v[..., None, None], Jx, 0.0)
        e = (x - self.m)[:, 3:]
        F = F + 0.5 * self.kappa * (e * e).sum(1)
        out = dict(F=np.where(behind, np.inf, F), pos=pos, J=G, zc=z_all)
        if need_jac:
            g = np.einsum("nclkp,nclk->np", Jpx, w_all * r_all) / s2
            g[:, 3:] += self.kappa * e
            A = np.einsum("nclkp,nclk,nclkq->npq", Jpx, w_all, Jpx) / s2
            A[:, np.arange(3, P), np.arange(3, P)] += self.kappa
            out.update(g=g, A=A, w=w_all, r=r_all, Jpx=Jpx)
        return out


# ------------------------------------------------------------------------------------------------ inputs of the tests
NAMES = ("generic-fisheye", "generic-pushed", "shipped-pinhole-pushed", "pt16-two", "pt32-three", "p51-wide16", "generic-mono",
         "generic-mono-pushed")
SKELETON = {"generic-fisheye": "generic", "generic-pushed": "generic", "shipped-pinhole-pushed": "shipped", "pt16-two": "pt16",
            "pt32-three": "pt32", "p51-wide16": "p51", "generic-mono": "generic", "generic-mono-pushed": "generic"}
PT = {name: sref.PT[sk] for name, sk in SKELETON.items()}
MONO_CAMERA = 2
EMPTY_FRAME = 5                                  # of the pushed inputs: no valid detection
ROOT_BOX = 0.4                                   # the root within this of the rig's centre of view, per axis [m]
ROOT_PULL = {1: 0.5, 2: 0.65}                  # by the number of cameras
MONO_NOISE_PX = 0.5
SEED = 11


def _rig(name):
    if name == "shipped-pinhole-pushed":
        return ur.unlike_rig(6, "pinhole"), "pinhole"
    full = ur.unlike_rig(6, "fisheye", skew=True)
    if name == "pt16-two":
        return ur.subset(full, [0, 1]), "fisheye"
    if name == "pt32-three":
        return ur.subset(full, ur.CAM_SUBSET), "fisheye"
    if name == "p51-wide16":
        return ur.moved(ur.unlike_rig(16, "fisheye", skew=True)), "fisheye"
    if name.startswith("generic-mono"):
        return ur.subset(full, [MONO_CAMERA]), "fisheye"
    return full, "fisheye"


def root_centre(rig):
    """Where the roots of an input lie: the point every camera looks at (oracle.synth.LOOK_AT); for a rig of one or two
    cameras, ROOT_PULL[C] of the way from it to the cameras' mean centre - there the angles show in the pixels above the noise."""
    centres = -np.einsum("cji,cj->ci", np.asarray(rig[2], dtype=np.float64), np.asarray(rig[3], dtype=np.float64).reshape(-1, 3))
    pull = ROOT_PULL.get(len(centres), 0.0)
    return osynth.LOOK_AT + pull * (centres.mean(0) - osynth.LOOK_AT)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """name -> dict(skel, det [N, C, L, 3], rig, model, pushed, lo, hi, x0 [N, P], truth, truth_pos).  A truth state per frame:
    the root within ROOT_BOX of the point every camera of the rig looks at (oracle.synth.LOOK_AT: the whole skeleton is in
    front of every camera; root_centre), the angles 0.3 N(0, 1), clipped to the box of bounds_table.  Pixels = projection +
    NOISE_PX noise - MONO_NOISE_PX on one camera: 36 states on at most 28 coordinates leave a flat valley, and at 2 px the
    reference finishes every frame but needs up to 192 of the 255 trials, so close to the limit that the last digits of an
    implementation decide on which side a frame ends; at 0.5 px it needs at most 65 -;
    a detection is dropped with probability DROP; the pushed inputs move 5 % of the detections by 9..30 px
    (tref.push_detections) and lose every detection of frame EMPTY_FRAME.  In pt16-two camera 1 has no valid detection in the
    frames n = 0 mod 3.  In pt32-three the box of state 5 ends 0.1 below the truth in the frames n = 1 mod 4 and the box of state 9
    begins 0.1 above it in the frames n = 2 mod 4.  The start is the truth off by 0.05 in every state, the sign alternating, clipped to the box."""
    sk = sref.skeleton(SKELETON[name])
    rig, model = _rig(name)
    pushed = name.endswith("pushed")
    act = osf.active_states(sk)
    P, N = len(act), 14 if name == "p51-wide16" else N_FRAMES
    blo, bhi = osf.bounds_table(sk, N)
    lo, hi = blo[:, act], bhi[:, act]
    rng = np.random.default_rng(SEED)
    truth = np.concatenate([root_centre(rig) + rng.uniform(-ROOT_BOX, ROOT_BOX, (N, 3)), 0.3 * rng.standard_normal((N, P - 3))], axis=1)
    truth = np.clip(truth, lo, hi)
    q = np.zeros((N, 3 + 3 * len(sk["positions"])))
    q[:, act] = truth
    pos = osf.skeleton_fk_jac(sk, q)[0]
    L, C = pos.shape[1], len(rig[0])
    uv = ur.clean_pixels(pos, rig, "fisheye" if model == "fisheye" else "pinhole")      # [C, N, L, 2]
    det = np.zeros((N, C, L, 3))
    det[..., :2] = uv.transpose(1, 0, 2, 3) + rng.normal(0.0, MONO_NOISE_PX if C == 1 else NOISE_PX, (N, C, L, 2))
    det[..., 2] = np.where(rng.random((N, C, L)) >= DROP, 0.9, 0.1)
    if pushed:
        det = tref.push_detections(det, THRESH)[0]
        det[EMPTY_FRAME, :, :, 2] = 0.0
    if name == "pt16-two":
        det[0::3, 1, :, 2] = 0.0
    if name == "pt32-three":                     # a box that cuts the truth off: states that end on a bound
        lo, hi = lo.copy(), hi.copy()
        hi[1::4, 5], lo[2::4, 9] = truth[1::4, 5] - 0.1, truth[2::4, 9] + 0.1
    x0 = np.clip(truth + 0.05 * (-1.0) ** np.arange(P), lo, hi)
    return dict(skel=sk, det=det, rig=rig, model=model, pushed=pushed, lo=lo, hi=hi, x0=x0, truth=truth, truth_pos=pos)


def problem(name, mutant=None, frames=None, **kw):
    inp = inputs(name)
    rig = inp["rig"] if mutant is None else ur.MUTANTS[mutant](inp["rig"])
    sl = slice(None) if frames is None else slice(0, frames)
    return Problem(inp["skel"], inp["det"][sl], rig, inp["model"], inp["lo"][sl], inp["hi"][sl], inp["x0"][sl], **dict(OPTS, **kw))


@functools.lru_cache(maxsize=None)
def solved(name, mutant=None, frames=None):
    """The reference on an input (on a mutant of its rig, on its first ``frames`` frames): the problem, x, status, iters,
    cost, the objective at x, delta, the active set at x."""
    return common.solved(problem(name, mutant, frames))


def bound(name):
    """B of the comparisons on an input: 10 x the largest delta the reference solver reaches on its status-0 frames."""
    return common.bound(solved(name))


def model_of(name):
    """The SkeletonModel of an input for build.pose_fit_pixels: the link program, the box, the rig and camera model, and the
    detections as a model holds them - meas [N, C, L, 2] and weights [N, C, L] = 1 / SIGMA_PX where the detection is valid, 0
    elsewhere, so that the model's own sigma_px is SIGMA_PX and its own detections are valid where the input's are."""
    from acinoset_amd import build
    inp = inputs(name)
    sk = inp["skel"]
    prog, act = build.skeleton.compile_skeleton(sk), build.active_states(sk)
    n, P = len(inp["lo"]), 3 + 3 * prog["n_angles"]
    lo, hi = np.full((n, P), -np.inf), np.full((n, P), np.inf)
    lo[:, act], hi[:, act] = inp["lo"], inp["hi"]
    det = inp["det"]
    valid = (det[..., 2] > THRESH) & np.isfinite(det[..., :2]).all(-1)
    K, D, R, t = inp["rig"]
    return build.SkeletonModel(skel=sk, prog=prog, names=prog["names"], active=act, lo=lo, hi=hi, meas=det[..., :2].copy(),
                               weights=np.where(valid, 1.0 / SIGMA_PX, 0.0), K=K, D=D, R=R, t=t, h=1.0 / 120.0, model_weight=0.002,
                               camera_model=inp["model"], loss="l1")
