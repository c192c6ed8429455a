"""Reference of the per-frame cheetah pose fit (fte.pose_fit, csrc/pose_fit.hip), numpy only, on top of the oracle's FK.

    F(x) = 1/2 sum_{l enters} (FK_l(x) - y_l)^T W_l (FK_l(x) - y_l) + 1/2 sum_{p = 3..24} (x_p - m_p)^2 / prior_sigma^2

over the 25 active states inside the box of the FTE, m the start clipped to the box.  All frames of an input are evaluated
together: arrays are [N, ...].

    Problem(points, cov, x0, ...)      tests/pose_fit_ref_common.py's problem and solver - objective, active_set, solve, delta -
                                       with the model of this file: the oracle's FK, the constant box, the start rule
    inputs(name), solved(name), bound(name)   the inputs of the tests, the reference on them, the bound B

The points and covariances of the named inputs are the CPU reference's of the multi-view triangulation (solved(name)["X"],
sigma_px^2 inv(obj["A"])), so nothing here depends on the triangulation kernel."""
import functools

import numpy as np

import pose_fit_ref_common as common
import triangulate_mv_ref as tref
from oracle import fk
from pose_fit_ref_common import DEFAULTS, GRAD_ZERO_REL  # noqa: F401  (names of this module)

ACTIVE = fk.ACTIVE
NP_, NL = len(ACTIVE), 20
LO, HI = (b[ACTIVE] for b in fk.bounds45())
PSI0 = 20                                # column of psi_0 among the active states
SIGMA_PX = 5.0


def full_state(xa):
    q = np.zeros(xa.shape[:-1] + (fk.N_STATES,))
    q[..., ACTIVE] = xa
    return q


def default_start(points, enter):
    """Columns 0..2 the mean of the entering markers among 0, 1, 2 (of all entering markers when none of them enters), psi_0
    the direction marker 3 -> marker 2 when both enter, everything else 0; clipped to the box.  Sums run in marker order."""
    N = len(points)
    x0 = np.zeros((N, NP_))
    for n in range(N):
        head = enter[n, :3] if enter[n, :3].any() else enter[n]
        if head.any():
            acc = np.zeros(3)
            for l in np.nonzero(head)[0]:
                acc = acc + points[n, l]
            x0[n, :3] = acc / head.sum()
        if enter[n, 2] and enter[n, 3]:
            d = points[n, 2] - points[n, 3]
            x0[n, PSI0] = np.arctan2(d[1], d[0])
    return np.clip(x0, LO, HI)


class Problem(common.Problem):
    """The cheetah: the oracle's FK on the 25 active states and, for every frame, the constant box of the FTE."""
    P = NP_

    def __init__(self, points, cov=None, x0=None, **kw):
        N = len(points)
        super().__init__(points, cov, np.broadcast_to(LO, (N, NP_)), np.broadcast_to(HI, (N, NP_)), x0, **kw)

    def fk(self, x, with_jac=False):
        if not with_jac:
            return fk.cheetah_fk(full_state(x))
        pos, Jf = fk.cheetah_fk(full_state(x), with_jac=True)
        return pos, Jf[..., ACTIVE]                                  # [N, L, 3, 25]

    def default_start(self):
        return default_start(self.y0, self.enter)


# ------------------------------------------------------------------------------------------------ inputs of the tests
NAMES = ("fisheye", "fisheye-pushed", "pinhole-pushed", "sub01", "sub520", "wide16", "sparse")
SPARSE_KEEP = {7: (9, 10), 8: (15,), 9: (0, 1, 2), 10: (0, 1, 2, 3)}
SPARSE_COV_MARKER = 5                     # the marker of frames 11 and 12 whose covariance is edited


@functools.lru_cache(maxsize=None)
def inputs(name):
    """name -> dict(points [N, 20, 3], cov [N, 20, 3, 3], pushed): NaN where the triangulation reference returned no point."""
    if name == "sparse":
        base = inputs("fisheye")
        pts, cov = base["points"].copy(), base["cov"].copy()
        pts[3:5, 0:4] = np.nan
        for n, keep in SPARSE_KEEP.items():
            gone = np.setdiff1d(np.arange(NL), keep)
            pts[n, gone] = np.nan
            cov[n, gone] = np.nan
        c = cov[11, SPARSE_COV_MARKER]
        cov[11, SPARSE_COV_MARKER] = c - 2.0 * c[1, 1] * np.outer([0.0, 1.0, 0.0], [0.0, 1.0, 0.0])     # the second pivot below zero
        cov[12, SPARSE_COV_MARKER, 0, 1] = np.nan
        return dict(points=pts, cov=cov, pushed=False)
    tri = tref.solved(name)
    n_frames = tref.inputs(name)["det"].shape[0]
    X = tri["X"].reshape(n_frames, NL, 3)
    ok = np.isfinite(tri["X"]).all(1)
    cov = np.full((len(ok), 3, 3), np.nan)
    cov[ok] = SIGMA_PX ** 2 * np.linalg.inv(tri["obj"]["A"][ok])
    return dict(points=X, cov=cov.reshape(n_frames, NL, 3, 3), pushed=tref.inputs(name)["pushed"])


@functools.lru_cache(maxsize=None)
def solved(name):
    """The reference on an input: the problem, x, status, iters, cost, the objective at x, delta, the active set at x."""
    inp = inputs(name)
    return common.solved(Problem(inp["points"], inp["cov"]))


def bound(name):
    """B of the comparisons on an input: 10 x the largest delta the reference solver reaches on its status-0 frames."""
    return common.bound(solved(name))
