"""What the references of the two per-frame pose fits share (tests/pose_fit_ref.py: the cheetah; tests/skel_pose_fit_ref.py: a
skeleton), numpy only: the problem

    F(x) = 1/2 sum_{l enters} (FK_l(x) - y_l)^T W_l (FK_l(x) - y_l) + 1/2 sum_{p >= 3} (x_p - m_p)^2 / prior_sigma^2

over the P states of a model inside the box lo[n] <= x <= hi[n], m the start clipped to the box, and its projected
Levenberg-Marquardt.  All frames of an input are evaluated together: arrays are [N, ...].

    Problem(points, cov, lo, hi, x0, ...)   the entering slots, their W = S^-1 (through L D L^T of the upper entries, the rule
                                       and the factorisation of tests/triangulate_mv_ref.py), the start
    Problem.objective(x)               F, g, A = sum J^T W J + ridge, positions, J
    Problem.active_set(x, g, A)        at a bound with the gradient pushing outward, |g_p| > 1e-14 A_pp
    Problem.solve()                    the controller of oracle.fte.lm_solve, per frame (without its gtol stop)
    Problem.delta(x)                   sqrt(g_free^T A_free^-1 g_free), free by the rule above: what a step could still gain
    solved(prob), bound(ref)           the reference on a problem, the bound B of the comparisons

A model is a subclass that sets ``P`` before ``Problem.__init__`` and defines ``fk(x, with_jac)`` - positions [N, L, 3], with
the Jacobian [N, L, 3, P] on request - and ``default_start()`` [N, P]."""
import numpy as np

import triangulate_mv_ref as tref

DEFAULTS = dict(prior_sigma=np.pi, sigma_iso=0.01, min_markers=1, max_iter=100, ftol=1e-10, xtol=1e-10, lam0=1e-3)
GRAD_ZERO_REL = 1e-14


class Problem:
    def __init__(self, points, cov=None, lo=None, hi=None, x0=None, **kw):
        self.opt = dict(DEFAULTS, **kw)
        self.y = np.asarray(points, dtype=np.float64)
        self.N, self.L = self.y.shape[:2]
        self.lo = np.full((self.N, self.P), -np.inf) if lo is None else np.asarray(lo, dtype=np.float64)
        self.hi = np.full((self.N, self.P), np.inf) if hi is None else np.asarray(hi, dtype=np.float64)
        enter = np.isfinite(self.y).all(-1)
        if cov is None:
            W = np.broadcast_to(np.eye(3) / self.opt["sigma_iso"] ** 2, (self.N, self.L, 3, 3)).copy()
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
            enter &= ok.reshape(self.N, self.L)
            W = W.reshape(self.N, self.L, 3, 3)
        self.enter = enter
        self.W = np.where(enter[..., None, None], W, 0.0)
        self.y0 = np.where(enter[..., None], self.y, 0.0)
        self.n_markers = enter.sum(1)
        self.kappa = 1.0 / self.opt["prior_sigma"] ** 2
        start = self.default_start() if x0 is None else np.asarray(x0, dtype=np.float64)
        self.x0 = np.clip(start, self.lo, self.hi)
        self.m = self.x0

    def objective(self, x, need_jac=True):
        if need_jac:
            pos, J = self.fk(x, with_jac=True)                       # J [N, L, 3, P]
        else:
            pos, J = self.fk(x, with_jac=False), None
        r = np.where(self.enter[..., None], pos - self.y0, 0.0)
        Wr = np.einsum("nlij,nlj->nli", self.W, r)
        e = (x - self.m)[:, 3:]
        out = dict(F=0.5 * np.einsum("nli,nli->n", r, Wr) + 0.5 * self.kappa * (e * e).sum(1), pos=pos, J=J)
        if need_jac:
            g = np.einsum("nlip,nli->np", J, Wr)
            g[:, 3:] += self.kappa * e
            A = np.einsum("nlip,nlij,nljq->npq", J, self.W, J)
            A[:, np.arange(3, self.P), np.arange(3, self.P)] += self.kappa
            out.update(g=g, A=A)
        return out

    def active_set(self, x, g, A):
        tol = GRAD_ZERO_REL * np.einsum("npp->np", A)
        return ((x <= self.lo) & (g > tol)) | ((x >= self.hi) & (g < -tol))

    @staticmethod
    def free_block(A, fixed):
        """A with the rows and columns of the pinned states replaced by the identity's."""
        M = np.where(fixed[:, :, None] | fixed[:, None, :], 0.0, A)
        idx = np.arange(A.shape[-1])
        M[:, idx, idx] = np.where(fixed, 1.0, M[:, idx, idx])
        return M

    def solve(self):
        """Returns x [N, P] (NaN for status 2, 3), status, iters, cost: oracle.fte.lm_solve's loop with one lam, nu per frame."""
        o = self.opt
        N, P = self.N, self.P
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
        idx = np.arange(P)
        for _ in range(o["max_iter"]):
            if not run.any():
                break
            iters += run
            fixed = self.active_set(x, g, A)
            pg = np.where(fixed, 0.0, g)
            diag = np.maximum(A[:, idx, idx], 1e-30)
            M = self.free_block(A, fixed)
            M[:, idx, idx] += np.where(fixed, 0.0, lam[:, None] * diag)
            M = np.where(run[:, None, None], M, np.eye(P))
            d = np.linalg.solve(M, -pg[..., None])[..., 0]
            xt = np.clip(x + d, self.lo, self.hi)
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
        M = np.where(ok[:, None, None], self.free_block(o["A"], fixed), np.eye(self.P))
        sol = np.linalg.solve(M, pg[..., None])[..., 0]
        return np.where(ok, np.sqrt(np.maximum((pg * sol).sum(1), 0.0)), np.nan)


def solved(prob):
    """The reference on a problem: the problem, x, status, iters, cost, the objective at x, delta, the active set at x."""
    x, status, iters, cost = prob.solve()
    xs = np.where(np.isfinite(x), x, prob.x0)
    obj = prob.objective(xs)
    return dict(prob=prob, x=x, status=status, iters=iters, cost=cost, obj=obj, delta=prob.delta(x, obj),
                pinned=prob.active_set(xs, obj["g"], obj["A"]))


def bound(ref):
    """B of the comparisons on an input: 10 x the largest delta the reference solver reaches on its status-0 frames."""
    return 10.0 * float(np.nanmax(ref["delta"][ref["status"] == 0]))
