"""Reference of the per-frame cheetah pose fit (fte.pose_fit, csrc/pose_fit.hip), numpy only, on top of the oracle's FK.

    F(x) = 1/2 sum_{l enters} (FK_l(x) - y_l)^T W_l (FK_l(x) - y_l) + 1/2 sum_{p = 3..24} (x_p - m_p)^2 / prior_sigma^2

over the 25 active states inside the box of the FTE, m the start clipped to the box.  All frames of an input are evaluated
together: arrays are [N, ...].

    Problem(points, cov, x0, ...)      the entering markers, their W = S^-1 (through L D L^T of the upper entries, the rule and
                                       the factorisation of tests/triangulate_mv_ref.py), the start
    Problem.objective(x)               F, g, A = sum J^T W J + ridge, positions, J
    Problem.active_set(x, g, A)        at a bound with the gradient pushing outward, |g_p| > 1e-14 A_pp
    Problem.solve()                    the controller of oracle.fte.lm_solve, per frame (without its gtol stop)
    Problem.delta(x)                   sqrt(g_free^T A_free^-1 g_free), free by the rule above: what a step could still gain
    inputs(name), solved(name), bound(name)   the inputs of the tests, the reference on them, the bound B

The points and covariances of the named inputs are the CPU reference's of the multi-view triangulation (solved(name)["X"],
sigma_px^2 inv(obj["A"])), so nothing here depends on the triangulation kernel."""
import functools

import numpy as np

import triangulate_mv_ref as tref
from oracle import fk

ACTIVE = fk.ACTIVE
NP_, NL = len(ACTIVE), 20
LO, HI = (b[ACTIVE] for b in fk.bounds45())
PSI0 = 20                                # column of psi_0 among the active states
SIGMA_PX = 5.0
DEFAULTS = dict(prior_sigma=np.pi, sigma_iso=0.01, min_markers=1, max_iter=100, ftol=1e-10, xtol=1e-10, lam0=1e-3)
GRAD_ZERO_REL = 1e-14


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


class Problem:
    def __init__(self, points, cov=None, x0=None, **kw):
        self.opt = dict(DEFAULTS, **kw)
        self.y = np.asarray(points, dtype=np.float64)
        self.N = len(self.y)
        enter = np.isfinite(self.y).all(-1)
        if cov is None:
            W = np.broadcast_to(np.eye(3) / self.opt["sigma_iso"] ** 2, (self.N, NL, 3, 3)).copy()
        else:
            S = np.asarray(cov, dtype=np.float64).reshape(-1, 3, 3)
            fin = np.isfinite(S).all((1, 2))
            Sz = np.where(fin[:, None, None], S, 0.0)
            ok, (l10, l20, l21, d0, d1, d2) = tref.ldl3(Sz, 1e-12 * np.trace(Sz, axis1=1, axis2=2))
            ok &= fin
            with np.errstate(all="ignore"):
                Li = np.zeros_like(S)                                # L^-1, unit lower
                Li[:, 0, 0] = Li[:, 1, 1] = Li[:, 2, 2] = 1.0
                Li[:, 1, 0], Li[:, 2, 1], Li[:, 2, 0] = -l10, -l21, l10 * l21 - l20
                W = np.einsum("pki,pk,pkj->pij", Li, 1.0 / np.stack([d0, d1, d2], -1), Li)
            enter &= ok.reshape(self.N, NL)
            W = W.reshape(self.N, NL, 3, 3)
        self.enter = enter
        self.W = np.where(enter[..., None, None], W, 0.0)
        self.y0 = np.where(enter[..., None], self.y, 0.0)
        self.n_markers = enter.sum(1)
        self.kappa = 1.0 / self.opt["prior_sigma"] ** 2
        self.x0 = np.clip(default_start(self.y0, enter) if x0 is None else np.asarray(x0, dtype=np.float64), LO, HI)
        self.m = self.x0

    def objective(self, x, need_jac=True):
        if need_jac:
            pos, Jf = fk.cheetah_fk(full_state(x), with_jac=True)
            J = Jf[..., ACTIVE]                                      # [N, L, 3, 25]
        else:
            pos, J = fk.cheetah_fk(full_state(x)), None
        r = np.where(self.enter[..., None], pos - self.y0, 0.0)
        Wr = np.einsum("nlij,nlj->nli", self.W, r)
        e = (x - self.m)[:, 3:]
        out = dict(F=0.5 * np.einsum("nli,nli->n", r, Wr) + 0.5 * self.kappa * (e * e).sum(1), pos=pos, J=J)
        if need_jac:
            g = np.einsum("nlip,nli->np", J, Wr)
            g[:, 3:] += self.kappa * e
            A = np.einsum("nlip,nlij,nljq->npq", J, self.W, J)
            A[:, np.arange(3, NP_), np.arange(3, NP_)] += self.kappa
            out.update(g=g, A=A)
        return out

    @staticmethod
    def active_set(x, g, A):
        tol = GRAD_ZERO_REL * np.einsum("npp->np", A)
        return ((x <= LO) & (g > tol)) | ((x >= HI) & (g < -tol))

    @staticmethod
    def free_block(A, fixed):
        """A with the rows and columns of the pinned states replaced by the identity's."""
        M = np.where(fixed[:, :, None] | fixed[:, None, :], 0.0, A)
        idx = np.arange(A.shape[-1])
        M[:, idx, idx] = np.where(fixed, 1.0, M[:, idx, idx])
        return M

    def solve(self):
        """Returns x [N, 25] (NaN for status 2, 3), status, iters, cost: oracle.fte.lm_solve's loop with one lam, nu per frame."""
        o = self.opt
        N = self.N
        live = self.n_markers >= o["min_markers"]
        status = np.where(live, 1, 2)
        x = self.x0.copy()
        with np.errstate(all="ignore"):
            cur = self.objective(x)
        F, g, A = cur["F"], cur["g"], cur["A"]
        bad = live & ~np.isfinite(F)
        status[bad] = 3
        run = live & ~bad
        lam, nu, iters = np.full(N, o["lam0"]), np.full(N, 2.0), np.zeros(N, dtype=np.int64)
        idx = np.arange(NP_)
        for _ in range(o["max_iter"]):
            if not run.any():
                break
            iters += run
            fixed = self.active_set(x, g, A)
            pg = np.where(fixed, 0.0, g)
            diag = np.maximum(A[:, idx, idx], 1e-30)
            M = self.free_block(A, fixed)
            M[:, idx, idx] += np.where(fixed, 0.0, lam[:, None] * diag)
            M = np.where(run[:, None, None], M, np.eye(NP_))
            d = np.linalg.solve(M, -pg[..., None])[..., 0]
            xt = np.clip(x + d, LO, HI)
            Ft = self.objective(xt, need_jac=False)["F"]
            pred = 0.5 * (d * (lam[:, None] * diag * d - pg)).sum(1)
            with np.errstate(all="ignore"):
                gain = np.where(pred > 0, (F - Ft) / pred, -1.0)
                acc = run & (Ft < F)
            step = np.abs(xt - x).max(1)
            dF = F - Ft
            rej = run & ~acc
            x = np.where(acc[:, None], xt, x)
            F = np.where(acc, Ft, F)
            if acc.any():
                new = self.objective(x)
                g, A = np.where(acc[:, None], new["g"], g), np.where(acc[:, None, None], new["A"], A)
            with np.errstate(all="ignore"):
                lam = np.where(acc, lam * np.maximum(1.0 / 3.0, 1.0 - (2.0 * gain - 1.0) ** 3), np.where(rej, lam * nu, lam))
                nu = np.where(acc, 2.0, np.where(rej, nu * 2.0, nu))
            done = acc & ((dF <= o["ftol"] * np.abs(F)) | (step <= o["xtol"]))
            status[done] = 0
            run &= ~done
            run &= ~(rej & (lam > 1e16))
        x = np.where((status < 2)[:, None], x, np.nan)
        return x, status, iters, np.where(status < 2, F, np.nan)

    def delta(self, x, o=None):
        ok = np.isfinite(x).all(1)
        xs = np.where(ok[:, None], x, self.x0)
        o = self.objective(xs) if o is None else o
        fixed = self.active_set(xs, o["g"], o["A"])
        pg = np.where(fixed, 0.0, o["g"])
        M = np.where(ok[:, None, None], self.free_block(o["A"], fixed), np.eye(NP_))
        sol = np.linalg.solve(M, pg[..., None])[..., 0]
        return np.where(ok, np.sqrt(np.maximum((pg * sol).sum(1), 0.0)), np.nan)


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
    prob = Problem(inp["points"], inp["cov"])
    x, status, iters, cost = prob.solve()
    xs = np.where(np.isfinite(x), x, prob.x0)
    obj = prob.objective(xs)
    return dict(prob=prob, x=x, status=status, iters=iters, cost=cost, obj=obj, delta=prob.delta(x, obj),
                pinned=prob.active_set(xs, obj["g"], obj["A"]))


def bound(name):
    """B of the comparisons on an input: 10 x the largest delta the reference solver reaches on its status-0 frames."""
    ref = solved(name)
    return 10.0 * float(np.nanmax(ref["delta"][ref["status"] == 0]))
