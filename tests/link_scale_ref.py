"""Reference of the link-scale fit (build.link_scale_system / build.fit_link_scales, csrc/skel_link_scale.hip), numpy only, on
top of skel_pose_fit_ref.Problem and the oracle's skeleton FK (oracle.skel_fte.skeleton_fk_jac).

One log-scale theta_g per group of links, off_k -> exp(theta_g(k)) off_k.  A pose is linear in the offsets, so the oracle's FK
on a skeleton whose links carry OTHER offsets gives everything: the scaled skeleton (every offset times its scale) and
d pos / d theta_g (only group g's scaled offsets kept, minus the root).  The oracle reads an offset as
``positions[child] - positions[parent]``, once per two-part link, in link order; ``LinkOffsets`` stands in for ``positions``
and answers those look-ups with the offset of the link they belong to - a part the skeleton defines twice has no positions that
would do (test_link_scale_host.py holds it to the plain skeleton at the scales 1).

    ScaledProblem(skel, points, cov, lo, hi, groups, scales)   the pose-fit problem of the scaled skeleton; with_scales(s)
    dpos_dtheta(prob, x)                 [N, L, 3, K]
    frame_system(prob, n, x, pinned, dtype)   S_n, r_n, F_n, sens_n and the magnitudes of the terms summed, in ``dtype``
    joint_matrix(prob, n, x, pinned)     the dense Gauss-Newton matrix and gradient of (free pose, theta) of one frame
    system(prob, x, pinned, status)      the per-frame arrays and their sums in frame order
    fit(prob, ...)                       the driver of build.fit_link_scales on the CPU
    inputs(name), scaled_inputs(name)    the inputs of the tests"""
import copy
import functools

import numpy as np

import skel_pose_fit_ref as pref
from oracle import skel_fte as osf

MAX_GROUPS = 16
SEED = 11                              # of the scaled-truth variant (test_link_scale_host.py: the CPU driver meets 4 bars on it)
GROUPS = {"shipped": "links", "pt16": "links", "pt32": "links", "p51": "mod8"}


class LinkOffsets:
    """``positions`` of a skeleton dictionary as skeleton_fk_jac reads it: len(), and per two-part link, in link order,
    positions[child] then positions[parent] - answered with the link's offset and with zero."""

    def __init__(self, n_parts, offsets):
        self.n_parts, self.offsets, self.calls = n_parts, offsets, 0

    def __len__(self):
        return self.n_parts

    def __getitem__(self, _part):
        link, second = divmod(self.calls, 2)
        self.calls += 1
        return np.zeros(3) if second else self.offsets[link]


def base_offsets(skel):
    """The offset of every two-part link, in link order: the ops of the compiled program."""
    pos = skel["positions"]
    return np.array([np.asarray(pos[l[1]], dtype=np.float64) - np.asarray(pos[l[0]], dtype=np.float64)
                     for l in skel["links"] if len(l) == 2])


def groups_of(skel, groups):
    """int [n_ops] and K: "links" one group per link with a non-zero offset, "global" one for all of them, "mod8" the op index
    mod 8, or the array itself."""
    off = base_offsets(skel)
    moving = (off != 0).any(1)
    if isinstance(groups, str) and groups == "links":
        grp = np.full(len(off), -1)
        grp[moving] = np.arange(moving.sum())
    elif isinstance(groups, str) and groups == "global":
        grp = np.where(moving, 0, -1)
    elif isinstance(groups, str) and groups == "mod8":
        grp = np.arange(len(off)) % 8
    else:
        grp = np.asarray(groups, dtype=np.int64)
    K = int(grp.max()) + 1
    assert grp.shape == (len(off),) and grp.min() >= -1 and 1 <= K <= MAX_GROUPS
    return grp.astype(np.int64), K


def oracle_fk(skel, offsets, q):
    sk = dict(skel, positions=LinkOffsets(len(skel["positions"]), offsets))
    return osf.skeleton_fk_jac(sk, q)


class ScaledProblem(pref.Problem):
    """The pose-fit problem of a skeleton whose links carry scales[group] * offset."""

    def __init__(self, skel, points, cov=None, lo=None, hi=None, x0=None, groups="links", scales=None, **kw):
        self.off0 = base_offsets(skel)
        self.grp, self.K = groups_of(skel, groups)
        self.scales = np.ones(self.K) if scales is None else np.asarray(scales, dtype=np.float64)
        super().__init__(skel, points, cov, lo, hi, x0, **kw)

    def offsets(self, only=None):
        s = np.where(self.grp >= 0, self.scales[np.maximum(self.grp, 0)], 1.0)
        if only is not None:
            s = np.where(self.grp == only, s, 0.0)
        return self.off0 * s[:, None]

    def fk(self, xa, with_jac=False):
        pos, J, _ = oracle_fk(self.skel, self.offsets(), self.full_state(xa))
        return (pos, J[..., self.ACT]) if with_jac else pos

    def with_scales(self, scales):
        """The same problem - points, box, start and ridge centre - at other scales."""
        p = copy.copy(self)
        p.scales = np.asarray(scales, dtype=np.float64)
        return p


def dpos_dtheta(prob, x):
    """[N, L, 3, K]: the FK with only group g's (scaled) offsets kept, minus the root."""
    q = prob.full_state(x)
    return np.stack([oracle_fk(prob.skel, prob.offsets(only=g), q)[0] - x[:, None, :3] for g in range(prob.K)], axis=-1)


# ------------------------------------------------------------------------------------------------ one frame
def _chol(A):
    n = len(A)
    L = np.zeros_like(A)
    for j in range(n):
        d = A[j, j] - L[j, :j] @ L[j, :j]
        if not d > 0:
            return None
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def _forward(L, B):
    Y = np.zeros_like(B)
    for i in range(len(L)):
        Y[i] = (B[i] - L[i, :i] @ Y[:i]) / L[i, i]
    return Y


def _backward(L, Y):
    X = np.zeros_like(Y)
    for i in range(len(L) - 1, -1, -1):
        X[i] = (Y[i] - L[i + 1:, i] @ X[i + 1:]) / L[i, i]
    return X


def frame_terms(prob, n, x, D=None, dtype=np.float64):
    """A, B, C, g, c, F of frame n at x [N, P] (FK, Jacobian and W from the fp64 oracle, the sums in ``dtype``), plus the
    whitened pieces |.| sums are taken from."""
    pos, J = prob.fk(x[n:n + 1], with_jac=True)
    D = dpos_dtheta(prob, x[n:n + 1])[0] if D is None else D[n]
    e = prob.enter[n]
    J, D, W = J[0][e].astype(dtype), D[e].astype(dtype), prob.W[n][e].astype(dtype)
    res = (pos[0][e] - prob.y0[n][e]).astype(dtype)
    kap = dtype(prob.kappa)
    ridge = np.zeros(prob.P, dtype=dtype)
    ridge[3:] = kap
    dx = (x[n].astype(dtype) - prob.m[n].astype(dtype)) * (ridge > 0)
    WJ, WD, Wr = np.einsum("lij,ljp->lip", W, J), np.einsum("lij,ljk->lik", W, D), np.einsum("lij,lj->li", W, res)
    A = np.einsum("lip,liq->pq", J, WJ) + np.diag(ridge)
    # magnitudes: a residual is a difference of a pose and a point of metres, so the rounding of either reaches everything that
    # is linear in it with |W| (|pose| + |point|) in place of W res
    Wm = np.einsum("lij,lj->li", np.abs(W), (np.abs(pos[0][e]) + np.abs(prob.y0[n][e])).astype(dtype))
    return dict(A=A, B=np.einsum("lip,lik->pk", J, WD), C=np.einsum("lik,lim->km", D, WD), g=np.einsum("lip,li->p", J, Wr) + kap * dx,
                c=np.einsum("lik,li->k", D, Wr), F=dtype(0.5) * np.einsum("li,li->", res, Wr) + dtype(0.5) * kap * (dx @ dx),
                magC=np.einsum("lik,lim->km", np.abs(D), np.abs(WD)), magc=np.einsum("lik,li->k", np.abs(D), Wm),
                magg=np.einsum("lip,li->p", np.abs(J), Wm) + kap * np.abs(dx),
                magA=np.einsum("lip,liq->pq", np.abs(J), np.abs(WJ)) + np.diag(ridge), magB=np.einsum("lip,lik->pk", np.abs(J), np.abs(WD)),
                magF=np.einsum("li,li->", np.abs(res), Wm) + dtype(0.5) * kap * (dx @ dx))


def frame_system(prob, n, x, pinned, D=None, dtype=np.float64):
    """S_n, r_n, F_n, sens_n [P, K] (pinned rows 0) of frame n in ``dtype``, and mag_S, mag_r, mag_F, mag_sens: the sums of the
    absolute values of the terms each entry adds up (sens, the solution of a linear system: the terms of its componentwise
    error bound).  None when A_FF has no factor."""
    t = frame_terms(prob, n, x, D, dtype)
    free = ~np.asarray(pinned[n], dtype=bool)
    L = _chol(t["A"][np.ix_(free, free)])
    if L is None:
        return None
    Y, v = _forward(L, t["B"][free]), _forward(L, t["g"][free])
    sens = np.zeros((prob.P, prob.K), dtype=dtype)
    sens[free] = -_backward(L, Y)
    Ainv = _backward(L, _forward(L, np.eye(int(free.sum()), dtype=dtype)))
    mag_sens = np.zeros((prob.P, prob.K), dtype=dtype)
    # (a solve: the componentwise bound |dX| <= eps |A^-1| (|A| |X| + |B|) of a linear system whose entries carry one rounding)
    mag_sens[free] = np.abs(Ainv) @ (t["magA"][np.ix_(free, free)] @ np.abs(sens[free]) + t["magB"][free])
    Linv = np.abs(_forward(L, np.eye(int(free.sum()), dtype=dtype)))
    return dict(S=t["C"] - Y.T @ Y, r=t["c"] - Y.T @ v, F=t["F"], sens=sens, mag_S=t["magC"] + np.abs(Y).T @ np.abs(Y),
                mag_r=t["magc"] + np.abs(Y).T @ (Linv @ t["magg"][free]), mag_F=t["magF"], mag_sens=mag_sens)


def joint_matrix(prob, n, x, pinned):
    """The dense Gauss-Newton matrix [[A_FF, B_F], [B_F^T, C]] and gradient [g_F, c] of frame n over (free pose states, theta)."""
    t = frame_terms(prob, n, x)
    free = ~np.asarray(pinned[n], dtype=bool)
    H = np.block([[t["A"][np.ix_(free, free)], t["B"][free]], [t["B"][free].T, t["C"]]])
    return H, np.concatenate([t["g"][free], t["c"]]), int(free.sum())


def system(prob, x, pinned, status, dtype=np.float64):
    """The per-frame arrays at x over the frames with status < 2 (zeros and used False elsewhere, NaN in sens) and the sums in
    frame order: S, r, cost, n_used; the magnitudes under mag_*."""
    N, P, K = prob.N, prob.P, prob.K
    xs = np.where(np.isfinite(x), x, prob.x0)
    D = dpos_dtheta(prob, xs)
    out = dict(S_frames=np.zeros((N, K, K), dtype), r_frames=np.zeros((N, K), dtype), cost_frames=np.zeros(N, dtype),
               sens=np.full((N, P, K), np.nan, dtype), used=np.zeros(N, bool), mag_S=np.zeros((N, K, K), dtype),
               mag_r=np.zeros((N, K), dtype), mag_F=np.zeros(N, dtype), mag_sens=np.zeros((N, P, K), dtype))
    for n in np.nonzero(np.asarray(status) < 2)[0]:
        f = frame_system(prob, n, xs, pinned, D, dtype)
        if f is None:
            continue
        out["used"][n] = True
        for key, src in (("S_frames", "S"), ("r_frames", "r"), ("cost_frames", "F"), ("sens", "sens"), ("mag_S", "mag_S"),
                         ("mag_r", "mag_r"), ("mag_F", "mag_F"), ("mag_sens", "mag_sens")):
            out[key][n] = f[src]
    S, r, cost = np.zeros((K, K), dtype), np.zeros(K, dtype), dtype(0)
    for n in range(N):
        S, r, cost = S + out["S_frames"][n], r + out["r_frames"][n], cost + out["cost_frames"][n]
    out.update(S=S, r=r, cost=cost, n_used=int(out["used"].sum()))
    return out


# ------------------------------------------------------------------------------------------------ the driver
def step(S, r, theta, lam, prec=0.0):
    obs = np.diag(S) > 0
    d = np.zeros(len(r))
    if obs.any():
        d[obs] = -np.linalg.solve(S[np.ix_(obs, obs)] + (lam + prec) * np.eye(int(obs.sum())), r[obs] + prec * theta[obs])
    return d, obs


def fit(prob, scale_prior_sigma=None, max_outer=30, tol=1e-6, fixed=()):
    """build.fit_link_scales on the CPU: the pose fits by the reference solver from the problem's start (its ridge centre), the
    same step, damping and stop.  ``fixed``: groups held at 1 (their rows and columns of S and r are set to 0)."""
    prec = 0.0 if scale_prior_sigma is None else 1.0 / scale_prior_sigma ** 2
    K = prob.K

    def evaluate(theta):
        p = prob.with_scales(np.exp(theta))
        x, status, _iters, _cost = p.solve()
        xs = np.where(np.isfinite(x), x, p.x0)
        o = p.objective(xs)
        sys_ = system(p, xs, p.active_set(xs, o["g"], o["A"]), status)
        for g in fixed:
            sys_["S"][g, :], sys_["S"][:, g], sys_["r"][g] = 0.0, 0.0, 0.0
        return p, x, sys_

    def cost_on(sys_, theta, frames):
        return float(np.add.reduce(sys_["cost_frames"][frames])) + 0.5 * prec * float(theta @ theta)

    theta = np.zeros(K)
    cur = evaluate(theta)
    lam, history, status = 0.0, [], "max_outer"
    for _ in range(max_outer if cur[2]["n_used"] else 0):
        sys_ = cur[2]
        top = float(np.diag(sys_["S"]).max())
        accepted = False
        while True:
            d, _obs = step(sys_["S"], sys_["r"], theta, lam, prec)
            size = float(np.abs(d).max())
            if size < tol:
                break
            trial = evaluate(theta + d)
            both = sys_["used"] & trial[2]["used"]
            if both.any() and cost_on(trial[2], theta + d, both) < cost_on(sys_, theta, both):
                theta, cur, accepted = theta + d, trial, True
                lam = lam / 10.0 if lam > 1e-12 * top else 0.0
                break
            lam = max(10.0 * lam, 1e-3 * top)
        history.append(dict(cost=cost_on(cur[2], theta, cur[2]["used"]), max_dtheta=size, lam=lam, n_used=cur[2]["n_used"]))
        if not accepted:
            status = "ok"
            break
    sys_ = cur[2]
    obs = np.diag(sys_["S"]) > 0
    cov_t = np.zeros((K, K))
    cov_t[np.ix_(obs, obs)] = np.linalg.inv(sys_["S"][np.ix_(obs, obs)] + prec * np.eye(int(obs.sum())))
    scales = np.exp(theta)
    return dict(scales=scales, cov_log_scales=cov_t, std_scales=np.where(obs, scales * np.sqrt(np.diag(cov_t)), np.inf),
                observed=obs, history=history, status=status if cur[2]["n_used"] else "no_frames", x=cur[1], system=sys_)


@functools.lru_cache(maxsize=None)
def fitted(name, drop_slot=None):
    """The CPU driver on the scaled-truth variant of an input, computed once; ``drop_slot``: that slot's points removed in every
    frame."""
    pts = scaled_inputs(name)["points"].copy()
    if drop_slot is not None:
        pts[:, drop_slot] = np.nan
    return fit(problem(name, points=pts))


# ------------------------------------------------------------------------------------------------ inputs of the tests
NAMES = ("shipped", "pt16", "pt32", "p51")


def problem(name, points=None, scales=None, **kw):
    inp = pref.inputs(name)
    return ScaledProblem(inp["skel"], inp["points"] if points is None else points, inp["cov"], inp["lo"], inp["hi"],
                         groups=GROUPS[name], scales=scales, **dict(pref.FIT, **kw))


@functools.lru_cache(maxsize=None)
def scaled_inputs(name, seed=SEED):
    """The input ``name`` of skel_pose_fit_ref with its points taken from a truth skeleton scaled per group by factors
    uniform in [0.85, 1.15] (seeded), the same truth states, noise and missing slots: dict(points, factors)."""
    inp = pref.inputs(name)
    grp, K = groups_of(inp["skel"], GROUPS[name])
    factors = 1.0 + np.random.default_rng(seed).uniform(-0.15, 0.15, K)
    truth = ScaledProblem(inp["skel"], inp["points"], inp["cov"], inp["lo"], inp["hi"], groups=GROUPS[name], scales=factors, **pref.FIT)
    pos = truth.fk(inp["truth"])
    return dict(points=pos + (inp["points"] - inp["truth_pos"]), factors=factors, groups=grp)
