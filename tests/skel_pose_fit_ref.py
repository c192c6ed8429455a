"""Reference of the per-frame skeleton pose fit (build.pose_fit, csrc/skel_pose_fit.hip), numpy only, on top of the oracle's
skeleton FK (oracle.skel_fte.skeleton_fk_jac): the generic form of tests/pose_fit_ref.py.

    F(x) = 1/2 sum_{l enters} (FK_l(x) - y_l)^T W_l (FK_l(x) - y_l) + 1/2 sum_{p >= 3} (x_p - m_p)^2 / prior_sigma^2

over the P active states inside the box lo[n] <= x <= hi[n], m the start clipped to the box.  All frames of an input are
evaluated together: arrays are [N, ...].

    Problem(skel, points, cov, lo, hi, x0, ...)   tests/pose_fit_ref_common.py's problem and solver - objective, active_set,
                                       solve, delta - with the model of this file: the link program's FK, the start rule
    inputs(name), solved(name), bound(name)   the inputs of the tests, the reference on them, the bound B

The named inputs are synthetic (a truth state per frame, points = FK(truth) + noise of the stated covariance), so nothing here
depends on another kernel."""
import functools
import os

import numpy as np

import pose_fit_ref_common as common
import skel_cov_cases as cases
from oracle import skel_fte as osf
from pose_fit_ref_common import DEFAULTS, GRAD_ZERO_REL  # noqa: F401  (names of this module)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIT = dict(prior_sigma=1.0, max_iter=255)           # what the tests run: the defaults leave the flat valleys unfinished
N_FRAMES = 24


class Problem(common.Problem):
    """A skeleton: the oracle's link program on the model's active states, a box per frame."""

    def __init__(self, skel, points, cov=None, lo=None, hi=None, x0=None, **kw):
        self.skel = skel
        self.ACT = osf.active_states(skel)
        self.P = len(self.ACT)
        self.P_full = 3 + 3 * len(skel["positions"])
        super().__init__(points, cov, lo, hi, x0, **kw)

    def full_state(self, xa):
        q = np.zeros(xa.shape[:-1] + (self.P_full,))
        q[..., self.ACT] = xa
        return q

    def fk(self, xa, with_jac=False):
        pos, J, _ = osf.skeleton_fk_jac(self.skel, self.full_state(xa))
        return (pos, J[..., self.ACT]) if with_jac else pos

    def default_start(self):
        """Every angle 0; x, y, z the mean over the entering slots of y_l - rest_l, rest the poses of the zero state, summed
        in slot order (the clip to the box is the caller's)."""
        rest = self.fk(np.zeros((1, self.P)))[0]
        x0 = np.zeros((self.N, self.P))
        for n in range(self.N):
            if self.enter[n].any():
                acc = np.zeros(3)
                for l in np.nonzero(self.enter[n])[0]:
                    acc = acc + (self.y0[n, l] - rest[l])
                x0[n, :3] = acc / self.enter[n].sum()
        return x0


# ------------------------------------------------------------------------------------------------ inputs of the tests
NAMES = ("shipped", "generic", "pt16", "pt32", "p51")
PT = {"shipped": 48, "generic": 48, "pt16": 16, "pt32": 32, "p51": 64}


@functools.lru_cache(maxsize=None)
def skeleton(name):
    _g, sk = cases.load(GOLDEN)
    if name == "shipped":
        return sk
    if name == "generic":
        return cases.generic_skeleton(sk)
    if name == "p51":
        return cases.generic_skeleton(sk, extra=5)
    return cases.sub_skeleton(cases.generic_skeleton(sk), cases.SUB_TREES[PT[name]])


@functools.lru_cache(maxsize=None)
def inputs(name):
    """name -> dict(skel, points [N, L, 3] (NaN where the slot has no point), cov [N, L, 3, 3], lo, hi [N, P], truth [N, P]).
    A truth state per frame - root uniform in [-2, 2]^3 + (0, 0, 1), angles 0.3 N(0, 1), clipped to the box of bounds_table -,
    y = FK(truth) + chol(S) z with S = 1e-4 (B B^T + I / 4), B standard normal (5 to 30 mm per axis).  Frame 0 has every slot,
    frame 1 slot 0 only, frame 2 the three slots L/2 .. L/2 + 2, frame 3 none, elsewhere a slot is dropped with probability 0.2."""
    sk = skeleton(name)
    act = osf.active_states(sk)
    P, N = len(act), N_FRAMES
    blo, bhi = osf.bounds_table(sk, N)
    lo, hi = blo[:, act], bhi[:, act]
    rng = np.random.default_rng(3)
    truth = np.concatenate([rng.uniform(-2.0, 2.0, (N, 3)) + np.array([0.0, 0.0, 1.0]), 0.3 * rng.standard_normal((N, P - 3))], axis=1)
    truth = np.clip(truth, lo, hi)
    q = np.zeros((N, 3 + 3 * len(sk["positions"])))
    q[:, act] = truth
    pos = osf.skeleton_fk_jac(sk, q)[0]
    L = pos.shape[1]
    B = rng.standard_normal((N, L, 3, 3))
    S = 1e-4 * (B @ np.swapaxes(B, -1, -2) + np.eye(3) / 4)
    z = rng.standard_normal((N, L, 3))
    y = pos + np.einsum("nlij,nlj->nli", np.linalg.cholesky(S), z)
    keep = rng.random((N, L)) >= 0.2
    keep[0] = True
    keep[1] = np.arange(L) == 0
    keep[2] = (np.arange(L) >= L // 2) & (np.arange(L) <= L // 2 + 2)
    keep[3] = False
    y[~keep] = np.nan
    return dict(skel=sk, points=y, cov=S, lo=lo, hi=hi, truth=truth, truth_pos=pos)


def problem(name, **kw):
    inp = inputs(name)
    return Problem(inp["skel"], inp["points"], inp["cov"], inp["lo"], inp["hi"], **dict(FIT, **kw))


@functools.lru_cache(maxsize=None)
def solved(name):
    """The reference on an input: the problem, x, status, iters, cost, the objective at x, delta, the active set at x."""
    return common.solved(problem(name))


def bound(name):
    """B of the comparisons on an input: 10 x the largest delta the reference solver reaches on its status-0 frames."""
    return common.bound(solved(name))
