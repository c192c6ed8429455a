"""Reference of the robust multi-view triangulation (calib.triangulate_multiview_dense), numpy only.

Pixels come from the oracle's calibration-level projections (oracle.camera.project_points_fisheye, with the skew, and
project_points); the Jacobians are analytic and are held to central differences of those projections by
tests/test_triangulate_mv_host.py.  All points of a problem are evaluated together: arrays are [P, ...] with P = N * L in
(frame, marker) order and [P, C, ...] per camera.

    Problem(det, thresh, rig, model, f_scale)   the validity rule and the observations
    Problem.start()                              the N-view ray midpoint and its status
    Problem.objective(X)                         F, g, A (IRLS), wssr, G [P, C, 3, 6], and H (the step matrix), behind
    Problem.solve(xtol, max_iter)                the damped Gauss-Newton iteration with the stop rule of the kernel
    Problem.delta_px(X)                          sqrt(g^T A^-1 g): the pixels of weighted residual a move of the point can
                                                 still explain - independent of the conditioning of A
    inputs(name), solved(name, mutant), bound(name)   the inputs of the tests, the reference on them, the bound B
"""
import functools

import numpy as np

import unlike_rig as ur
from oracle import camera as ocam

XTOL, MAX_ITER = 1e-10, 60


def _dist14(d):
    k = np.zeros(14)
    d = np.asarray(d, dtype=np.float64).reshape(-1)
    k[:d.size] = d
    return k


def fisheye_jac(Xc, K, D):
    """d(uv)/d(Xc) [P, 2, 3] of project_points_fisheye (r > 1e-8 branch, skew alpha = K01 / K00) at camera-frame points."""
    fx, fy, al = K[0, 0], K[1, 1], K[0, 1] / K[0, 0]
    D = np.asarray(D, dtype=np.float64).reshape(-1)
    iz = 1.0 / Xc[:, 2]
    a, b = Xc[:, 0] * iz, Xc[:, 1] * iz
    r2 = a * a + b * b
    r = np.sqrt(r2)
    th = np.arctan(r)
    th2 = th * th
    thd = th * (1 + D[0] * th2 + D[1] * th2 ** 2 + D[2] * th2 ** 3 + D[3] * th2 ** 4)
    dthd = 1 + 3 * D[0] * th2 + 5 * D[1] * th2 ** 2 + 7 * D[2] * th2 ** 3 + 9 * D[3] * th2 ** 4
    m = thd / r
    dm_dr = (dthd / (1 + r2) * r - thd) / r2
    dm_da, dm_db = dm_dr * a / r, dm_dr * b / r
    dxd = np.stack([m + a * dm_da, a * dm_db], -1)                    # d xd / d(a, b)
    dyd = np.stack([b * dm_da, m + b * dm_db], -1)
    du, dv = fx * (dxd + al * dyd), fy * dyd
    return _chain(du, dv, a, b, iz)


def pinhole_jac(Xc, K, D):
    """d(uv)/d(Xc) [P, 2, 3] of project_points (rational + tangential + thin-prism model) at camera-frame points."""
    fx, fy, k = K[0, 0], K[1, 1], _dist14(D)
    iz = 1.0 / Xc[:, 2]
    a, b = Xc[:, 0] * iz, Xc[:, 1] * iz
    r2 = a * a + b * b
    num = 1 + k[0] * r2 + k[1] * r2 ** 2 + k[4] * r2 ** 3
    den = 1 + k[5] * r2 + k[6] * r2 ** 2 + k[7] * r2 ** 3
    rad = num / den
    drad = ((k[0] + 2 * k[1] * r2 + 3 * k[4] * r2 ** 2) - rad * (k[5] + 2 * k[6] * r2 + 3 * k[7] * r2 ** 2)) / den
    sx, sy = k[8] + 2 * k[9] * r2, k[10] + 2 * k[11] * r2
    du = fx * np.stack([rad + 2 * a * a * drad + 2 * k[2] * b + 6 * k[3] * a + 2 * a * sx,
                        2 * a * b * drad + 2 * k[2] * a + 2 * k[3] * b + 2 * b * sx], -1)
    dv = fy * np.stack([2 * a * b * drad + 2 * k[2] * a + 2 * k[3] * b + 2 * a * sy,
                        rad + 2 * b * b * drad + 6 * k[2] * b + 2 * k[3] * a + 2 * b * sy], -1)
    return _chain(du, dv, a, b, iz)


def _chain(du, dv, a, b, iz):
    """[d u / d(a, b), d v / d(a, b)] -> d(uv)/d(Xc) through a = x / z, b = y / z."""
    row = lambda d: np.stack([d[:, 0] * iz, d[:, 1] * iz, -(d[:, 0] * a + d[:, 1] * b) * iz], -1)
    return np.stack([row(du), row(dv)], 1)


def camera_terms(X, K, D, R, t, model):
    """One camera at the points X [P, 3]: uv [P, 2] (the oracle's), J = d uv / dX [P, 2, 3], Jc = d uv / d(dw, dt) [P, 2, 6]
    under R <- exp([dw]x) R, t <- t + dt, and the camera-frame depth z [P]."""
    R, t = np.asarray(R, dtype=np.float64), np.asarray(t, dtype=np.float64).reshape(3)
    RX = X @ R.T
    Xc = RX + t
    with np.errstate(all="ignore"):
        if model == "fisheye":
            uv, Jx = ocam.project_points_fisheye(X, K, D, R, t), fisheye_jac(Xc, K, D)
        else:
            uv, Jx = ocam.project_points(X, K, D, R, t), pinhole_jac(Xc, K, D)
    J = Jx @ R
    skew = np.zeros((len(X), 3, 3))                                    # -[R X]x
    skew[:, 0, 1], skew[:, 0, 2] = RX[:, 2], -RX[:, 1]
    skew[:, 1, 0], skew[:, 1, 2] = -RX[:, 2], RX[:, 0]
    skew[:, 2, 0], skew[:, 2, 1] = RX[:, 1], -RX[:, 0]
    return uv, J, np.concatenate([Jx @ skew, Jx], -1), Xc[:, 2]


def ldl3(M, tol):
    """L D L^T of symmetric 3 x 3 matrices [P, 3, 3]: ok [P] (every pivot d_i above tol [P]), and the factors."""
    with np.errstate(all="ignore"):
        d0 = M[:, 0, 0]
        l10, l20 = M[:, 0, 1] / d0, M[:, 0, 2] / d0
        d1 = M[:, 1, 1] - l10 * M[:, 0, 1]
        b21 = M[:, 1, 2] - l20 * M[:, 0, 1]
        l21 = b21 / d1
        d2 = M[:, 2, 2] - l20 * M[:, 0, 2] - l21 * b21
    ok = (d0 > tol) & (d1 > tol) & (d2 > tol)
    return ok, (l10, l20, l21, d0, d1, d2)


def ldl3_solve(f, b):
    l10, l20, l21, d0, d1, d2 = f
    with np.errstate(all="ignore"):
        z1 = b[:, 1] - l10 * b[:, 0]
        z2 = b[:, 2] - l20 * b[:, 0] - l21 * z1
        x2 = z2 / d2
        x1 = z1 / d1 - l21 * x2
        x0 = b[:, 0] / d0 - l10 * x1 - l20 * x2
    return np.stack([x0, x1, x2], -1)


class Problem:
    def __init__(self, det, thresh, rig, model="fisheye", f_scale=5.0):
        self.rig, self.model, self.fs = rig, "fisheye" if model == "fisheye" else "pinhole", float(f_scale)
        det = np.asarray(det, dtype=np.float64)
        self.N, self.C, self.L = det.shape[:3]
        d = det.transpose(0, 2, 1, 3).reshape(-1, self.C, 3)            # [P, C, 3]
        self.obs = d[..., :2]
        K, D = rig[0], rig[1]
        valid = (d[..., 2] > thresh) & np.isfinite(d[..., 0]) & np.isfinite(d[..., 1])
        self.xy = np.zeros(self.obs.shape)
        for c in range(self.C):
            px = np.where(valid[:, c, None], self.obs[:, c], np.array([K[c][0, 2], K[c][1, 2]]))
            if self.model == "fisheye":
                xy = ocam.undistort_points_fisheye(px, K[c], D[c], 10, 1e-8)
                valid[:, c] &= ~np.all(xy == -1000000.0, axis=1)
            else:
                xy = ocam.undistort_points(px, K[c], D[c])
            self.xy[:, c] = xy
        self.valid = valid
        self.n_views = valid.sum(1)
        self.P = len(valid)

    def start(self):
        """The ray midpoint X0 [P, 3] (NaN where there is none) and the status it leaves: 0 (go on), 2, 3."""
        R, t = np.asarray(self.rig[2], dtype=np.float64), np.asarray(self.rig[3], dtype=np.float64).reshape(self.C, 3)
        M, b = np.zeros((self.P, 3, 3)), np.zeros((self.P, 3))
        for c in range(self.C):
            ray = np.concatenate([self.xy[:, c], np.ones((self.P, 1))], -1)
            w = (ray / np.linalg.norm(ray, axis=1, keepdims=True)) @ R[c]          # R^T ray, row form
            o = -R[c].T @ t[c]
            Pj = np.eye(3)[None] - w[:, :, None] * w[:, None, :]
            v = self.valid[:, c]
            M += np.where(v[:, None, None], Pj, 0.0)
            b += np.where(v[:, None], Pj @ o, 0.0)
        status = np.where(self.n_views < 2, 2, 0)
        ok, f = ldl3(M, 1e-12 * np.trace(M, axis1=1, axis2=2))
        status[(status == 0) & ~ok] = 3
        X0 = np.where((status == 0)[:, None], ldl3_solve(f, b), np.nan)
        return X0, status

    def objective(self, X):
        """At X [P, 3]: F, g [P, 3], A = sum J^T W J [P, 3, 3], wssr, G [P, C, 3, 6] (zero outside V), H = sum J^T h J with
        h = max(rho'', 0.1 w), and behind (z_c <= 0 for a camera of V)."""
        valid = self.valid
        P, fs2 = len(X), self.fs ** 2
        F, g, A, H = np.zeros(P), np.zeros((P, 3)), np.zeros((P, 3, 3)), np.zeros((P, 3, 3))
        wssr, G, behind = np.zeros(P), np.zeros((P, self.C, 3, 6)), np.zeros(P, dtype=bool)
        for c in range(self.C):
            v = valid[:, c]
            uv, J, Jc, zc = camera_terms(X, self.rig[0][c], self.rig[1][c], self.rig[2][c], self.rig[3][c], self.model)
            with np.errstate(all="ignore"):
                r = uv - self.obs[:, c]
                z = r * r / fs2
                w = 1.0 / (1.0 + z)
                h = np.maximum((1.0 - z) * w * w, 0.1 * w)
                terms = dict(F=0.5 * fs2 * np.log1p(z).sum(1), wssr=(w * r * r).sum(1), g=np.einsum("pki,pk->pi", J, w * r),
                             A=np.einsum("pki,pk,pkj->pij", J, w, J), H=np.einsum("pki,pk,pkj->pij", J, h, J),
                             G=np.einsum("pki,pk,pkj->pij", J, w, Jc))
            F += np.where(v, terms["F"], 0.0)
            wssr += np.where(v, terms["wssr"], 0.0)
            g += np.where(v[:, None], terms["g"], 0.0)
            A += np.where(v[:, None, None], terms["A"], 0.0)
            H += np.where(v[:, None, None], terms["H"], 0.0)
            G[:, c] = np.where(v[:, None, None], terms["G"], 0.0)
            behind |= v & ~(zc > 0.0)
        return dict(F=F, g=g, A=A, wssr=wssr, G=G, H=H, behind=behind)

    def solve(self, xtol=XTOL, max_iter=MAX_ITER):
        """The iteration of the kernel: (H + lam diag H) d = -g, lam from 1e-3, / 10 on an accepted trial, x 10 on a rejected
        one (F raised, or behind a camera of V); ends on |d| < xtol (status 0) or after max_iter trials (1).  Returns
        X [P, 3] (NaN for status 2, 3), status, iters, X0."""
        X0, status = self.start()
        live = status == 0
        X = np.where(live[:, None], X0, 0.0)
        cur = self.objective(X)
        lam, iters = np.full(self.P, 1e-3), np.zeros(self.P, dtype=np.int64)
        run = live.copy()
        status = np.where(live, 1, status)
        eye = np.eye(3, dtype=bool)[None]
        for _ in range(max_iter):
            if not run.any():
                break
            iters += run
            Hd = np.where(eye, cur["H"] * (1.0 + lam[:, None, None]), cur["H"])
            pd, f = ldl3(Hd, np.zeros(self.P))
            d = np.where(pd[:, None], ldl3_solve(f, -cur["g"]), 0.0)
            T = X + d
            tr = self.objective(T)
            with np.errstate(invalid="ignore"):
                ok = run & pd & ~tr["behind"] & (tr["F"] <= cur["F"])
            X = np.where(ok[:, None], T, X)
            for k in cur:
                cur[k] = np.where(ok.reshape((-1,) + (1,) * (cur[k].ndim - 1)), tr[k], cur[k])
            lam = np.where(run, np.where(ok, np.maximum(lam * 0.1, 1e-12), np.minimum(lam * 10.0, 1e12)), lam)
            done = run & pd & ((d * d).sum(1) < xtol * xtol)
            status[done] = 0
            run &= ~done
        # the outputs' own test: A positive definite, everything finite
        okA, _ = ldl3(cur["A"], 1e-12 * np.trace(cur["A"], axis1=1, axis2=2))
        bad = live & ~(okA & np.isfinite(X).all(1) & np.isfinite(cur["wssr"]))
        status[bad] = 3
        X = np.where((status < 2)[:, None], X, np.nan)
        return X, status, iters, X0

    def delta_px(self, X, o=None):
        o = self.objective(np.where(np.isfinite(X), X, 0.0)) if o is None else o
        out = np.full(len(X), np.nan)
        ok = np.isfinite(X).all(1)
        out[ok] = np.sqrt(np.einsum("pi,pi->p", o["g"][ok], np.linalg.solve(o["A"][ok], o["g"][ok][..., None])[..., 0]))
        return out


def shaped(P, a):
    """[P, ...] -> [N, L, ...]."""
    return np.asarray(a).reshape((P.N, P.L) + np.asarray(a).shape[1:])


def push_detections(det, thresh=0.5, frac=0.05, lo=9.0, hi=30.0, seed=7):
    """``frac`` of the valid detections pushed ``lo``..``hi`` px in a random direction (seeded).  Returns the new detections and
    touched [N, L]: the markers with a pushed detection."""
    rng = np.random.default_rng(seed)
    det = det.copy()
    valid = det[..., 2] > thresh
    hit = valid & (rng.uniform(size=valid.shape) < frac)
    ang, mag = rng.uniform(0, 2 * np.pi, valid.shape), rng.uniform(lo, hi, valid.shape)
    det[..., 0] += np.where(hit, mag * np.cos(ang), 0.0)
    det[..., 1] += np.where(hit, mag * np.sin(ang), 0.0)
    return det, hit.any(axis=1)


# ------------------------------------------------------------------------------------------------ inputs of the tests
# Shared by tests/test_gpu_triangulate_mv.py and tests/test_triangulate_mv_host.py, made by the oracle alone, cached and never
# modified: name -> dict(det, rig, model, pushed).  ``model`` is the rig's ("fisheye", "pinhole", "pinhole12").
THRESH, F_SCALE = 0.5, 5.0
FISHEYE_FRAMES = 27            # 540 items: two full workgroup passes and one of 28, frames straddling the passes
WIDE_FRAMES = 14               # 16 cameras: 280 items, too wide to stage


def _base(model):
    rig = ur.unlike_rig(6, model, skew=(model == "fisheye"))
    frames = FISHEYE_FRAMES if model == "fisheye" else ur.PINHOLE_PAIR_FRAMES
    return rig, ur.sequence(frames, rig, "fisheye" if model == "fisheye" else "pinhole")["det"]


def _pushed(det):
    return ur.edit_detections(push_detections(det, THRESH)[0])


@functools.lru_cache(maxsize=None)
def inputs(name):
    kind, _, variant = name.partition("-")
    if kind in ur.MODELS:
        rig, det = _base(kind)
        return dict(rig=rig, model=kind, det=_pushed(det) if variant == "pushed" else det, pushed=variant == "pushed")
    rig, det = _base("fisheye")
    if kind == "sub01":
        return dict(rig=ur.subset(rig, [0, 1]), model="fisheye", det=np.ascontiguousarray(det[:, [0, 1]]), pushed=False)
    if kind == "sub520":
        return dict(rig=ur.subset(rig, ur.CAM_SUBSET), model="fisheye", det=np.ascontiguousarray(_pushed(det)[:, ur.CAM_SUBSET]),
                    pushed=True)
    if kind == "wide16":
        rig = ur.moved(ur.unlike_rig(16, "fisheye", skew=True))
        return dict(rig=rig, model="fisheye", det=ur.sequence(WIDE_FRAMES, rig)["det"], pushed=False)
    if kind == "single":
        return dict(rig=rig, model="fisheye", det=np.ascontiguousarray(det[3:4, :, 2:3]), pushed=False)
    raise KeyError(name)


INPUTS = ("fisheye", "fisheye-pushed", "pinhole", "pinhole-pushed", "pinhole12", "pinhole12-pushed", "sub01", "sub520", "wide16",
          "single")


@functools.lru_cache(maxsize=None)
def solved(name, mutant=None):
    """The reference on an input (or on a mutant of its rig): the problem, X, status, iters, X0, the objective at X, delta_px."""
    inp = inputs(name)
    rig = inp["rig"] if mutant is None else ur.MUTANTS[mutant](inp["rig"])
    prob = Problem(inp["det"], THRESH, rig, inp["model"], F_SCALE)
    X, status, iters, X0 = prob.solve()
    obj = prob.objective(np.where(np.isfinite(X), X, 0.0))
    return dict(prob=prob, X=X, status=status, iters=iters, X0=X0, obj=obj, delta=prob.delta_px(X, obj))


def bound(name):
    """B of the comparisons on an input: 10 x the largest delta_px the reference solver reaches on its status-0 points."""
    ref = solved(name)
    return 10.0 * float(np.nanmax(ref["delta"][ref["status"] == 0]))
