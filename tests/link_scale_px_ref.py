"""Reference of the link-scale fit from the detections (build.link_scale_system_pixels / build.fit_link_scales_pixels,
csrc/skel_link_scale_px.hip), numpy only, on top of skel_pose_fit_px_ref.Problem (the pixel pose fit's objective and solver) and
link_scale_ref (LinkOffsets through ScaledProblem's methods, groups_of, dpos_dtheta, _chol / _forward / _backward, step).

One log-scale theta_g per group of links.  Per frame, at a pose x with the IRLS weights w = 1 / (1 + r^2 / f^2) at x:

    Jc  = sqrt(w) / sigma_px (d uv / dX) G_l,  Jsc = sqrt(w) / sigma_px (d uv / dX) d_gl,  u = sqrt(w) r / sigma_px
    A = sum Jc^T Jc + kappa, B = sum Jc^T Jsc, C = sum Jsc^T Jsc, g = sum Jc^T u + kappa (x - m), c = sum Jsc^T u
    S_n = C - Y^T Y, r_n = c - Y^T v, Y = L^-1 B_F, v = L^-1 g_F, A_FF = L L^T, sens_n = -A_FF^-1 B_F

    ScaledPxProblem(...)                  the pixel pose-fit problem of the scaled skeleton; with_scales(s)
    frame_terms / frame_system / system   in np.float64 or np.longdouble (projection, FK and Jacobians from the fp64 oracle, the
                                          weights and every sum in ``dtype``), with magnitudes
    joint_matrix(prob, n, x, pinned)      the dense joint Gauss-Newton matrix and gradient of one frame
    fit(prob, ...)                        the driver of build.fit_link_scales_pixels on the CPU
    problem(name, ...), scaled_inputs(name), model_of(name, det)

Magnitudes.  mag_* are the sums of the absolute values of the terms each entry adds up; a residual of pixels is a difference of
two values of order a thousand, so |uv| + |det| stands in place of |r| wherever a term is linear in it (as |pose| + |point|
does in link_scale_ref); mag_sens is the componentwise bound of a linear solve used there."""
import functools

import numpy as np

import link_scale_ref as lref
import skel_pose_fit_px_ref as ppx
import triangulate_mv_ref as tref
import unlike_rig as ur

SEED = 11                              # of the scaled-truth variant (test_link_scale_px_host.py: the CPU driver meets 4 bars on it)
GROUPS = {"generic": "mod8", "shipped": "links", "pt16": "links", "pt32": "links", "p51": "mod8"}
NAMES = ("generic-fisheye", "shipped-pinhole-pushed", "pt16-two", "pt32-three", "p51-wide16", "generic-mono")


def groups_for(name, groups=None):
    """The groups of an input: GROUPS of its skeleton; "mod16": the op index mod 16."""
    sk = ppx.inputs(name)["skel"]
    groups = GROUPS[ppx.SKELETON[name]] if groups is None else groups
    if isinstance(groups, str) and groups == "mod16":
        groups = np.arange(len(lref.base_offsets(sk))) % 16
    return lref.groups_of(sk, groups)


class ScaledPxProblem(ppx.Problem):
    """The pixel pose-fit problem of a skeleton whose links carry scales[group] * offset."""

    def __init__(self, skel, det, rig, model, lo, hi, x0, groups="links", scales=None, **kw):
        self.off0 = lref.base_offsets(skel)
        self.grp, self.K = lref.groups_of(skel, groups)
        self.scales = np.ones(self.K) if scales is None else np.asarray(scales, dtype=np.float64)
        super().__init__(skel, det, rig, model, lo, hi, x0, **kw)

    offsets = lref.ScaledProblem.offsets
    with_scales = lref.ScaledProblem.with_scales

    def full_state(self, xa):
        q = np.zeros(xa.shape[:-1] + (self.P_full,))
        q[..., self.ACT] = xa
        return q

    def fk(self, xa, with_jac=False):
        pos, J, _ = lref.oracle_fk(self.skel, self.offsets(), self.full_state(xa))
        return (pos, J[..., self.ACT]) if with_jac else pos


dpos_dtheta = lref.dpos_dtheta


# ------------------------------------------------------------------------------------------------ one frame
def frame_terms(prob, n, x, D=None, dtype=np.float64):
    """A, B, C, g, c, F of frame n at x [N, P] and the magnitudes of their terms."""
    pos, G = prob.fk(x[n:n + 1], with_jac=True)
    pos, G = pos[0], G[0].astype(dtype)                                      # [L, 3], [L, 3, P]
    D = (dpos_dtheta(prob, x[n:n + 1])[0] if D is None else D[n]).astype(dtype)      # [L, 3, K]
    fs2, s = dtype(prob.fs) ** 2, dtype(prob.sigma_px)
    rows_p, rows_s, us, ums, Fsum, Fmag = [], [], [], [], dtype(0), dtype(0)
    for c in range(prob.C):
        v = prob.valid[n, c]
        if not v.any():
            continue
        uv, J, _, _zc = tref.camera_terms(pos, prob.rig[0][c], prob.rig[1][c], prob.rig[2][c], prob.rig[3][c], prob.model)
        uv, J, obs = uv[v].astype(dtype), J.reshape(-1, 2, 3)[v].astype(dtype), prob.obs[n, c][v].astype(dtype)
        r = uv - obs                                                         # [V, 2]
        z = r * r / fs2
        w = 1 / (1 + z)
        sw = np.sqrt(w) / s
        px = np.abs(uv) + np.abs(obs)
        rows_p.append((sw[..., None] * np.einsum("vki,vip->vkp", J, G[v])).reshape(-1, prob.P))
        rows_s.append((sw[..., None] * np.einsum("vki,vig->vkg", J, D[v])).reshape(-1, prob.K))
        us.append((sw * r).reshape(-1))
        ums.append((sw * px).reshape(-1))
        Fsum = Fsum + (dtype(0.5) * fs2 * np.log1p(z)).sum() / (s * s)
        Fmag = Fmag + (dtype(0.5) * fs2 * np.log1p(z) + w * np.abs(r) * px).sum() / (s * s)
    Jp, Js = np.concatenate(rows_p), np.concatenate(rows_s)
    u, um = np.concatenate(us), np.concatenate(ums)
    kap = dtype(prob.kappa)
    ridge = np.zeros(prob.P, dtype=dtype)
    ridge[3:] = kap
    dx = (x[n].astype(dtype) - prob.m[n].astype(dtype)) * (ridge > 0)
    aJp, aJs = np.abs(Jp), np.abs(Js)
    return dict(A=Jp.T @ Jp + np.diag(ridge), B=Jp.T @ Js, C=Js.T @ Js, g=Jp.T @ u + kap * dx, c=Js.T @ u,
                F=Fsum + dtype(0.5) * kap * (dx @ dx),
                magA=aJp.T @ aJp + np.diag(ridge), magB=aJp.T @ aJs, magC=aJs.T @ aJs, magg=aJp.T @ um + kap * np.abs(dx),
                magc=aJs.T @ um, magF=Fmag + dtype(0.5) * kap * (dx @ dx))


def frame_system(prob, n, x, pinned, D=None, dtype=np.float64):
    """S_n, r_n, F_n, sens_n [P, K] (pinned rows 0) of frame n in ``dtype`` and mag_S, mag_r, mag_F, mag_sens.  None when A_FF
    has no factor."""
    t = frame_terms(prob, n, x, D, dtype)
    free = ~np.asarray(pinned[n], dtype=bool)
    ff = np.ix_(free, free)
    L = lref._chol(t["A"][ff])
    if L is None:
        return None
    eye = np.eye(int(free.sum()), dtype=dtype)
    Y, v = lref._forward(L, t["B"][free]), lref._forward(L, t["g"][free])
    sens = np.zeros((prob.P, prob.K), dtype=dtype)
    sens[free] = -lref._backward(L, Y)
    Linv = np.abs(lref._forward(L, eye))
    mag_sens = np.zeros_like(sens)
    # (a solve: the componentwise bound |dX| <= eps |A^-1| (|A| |X| + |B|) of a linear system whose entries carry one rounding)
    mag_sens[free] = np.abs(lref._backward(L, lref._forward(L, eye))) @ (t["magA"][ff] @ np.abs(sens[free]) + t["magB"][free])
    return dict(S=t["C"] - Y.T @ Y, r=t["c"] - Y.T @ v, F=t["F"], sens=sens, mag_S=t["magC"] + np.abs(Y).T @ np.abs(Y),
                mag_r=t["magc"] + np.abs(Y).T @ (Linv @ t["magg"][free]), mag_F=t["magF"], mag_sens=mag_sens)


def joint_matrix(prob, n, x, pinned):
    """The dense Gauss-Newton matrix [[A_FF, B_F], [B_F^T, C]] and gradient [g_F, c] of frame n over (free pose states, theta)."""
    t = frame_terms(prob, n, x)
    free = ~np.asarray(pinned[n], dtype=bool)
    H = np.block([[t["A"][np.ix_(free, free)], t["B"][free]], [t["B"][free].T, t["C"]]])
    return H, np.concatenate([t["g"][free], t["c"]]), int(free.sum())


KEYS = (("S_frames", "S"), ("r_frames", "r"), ("cost_frames", "F"), ("sens", "sens"))


def system(prob, x, pinned, status, dtype=np.float64):
    """The per-frame arrays at x over the frames with status < 2 (zeros and used False elsewhere, NaN in sens) and the sums in
    frame order: S, r, cost, n_used; the magnitudes under mag_S, mag_r, mag_F, mag_sens."""
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
        for key, src in KEYS:
            out[key][n], out[f"mag_{src}"][n] = f[src], f[f"mag_{src}"]
    S, r, cost = np.zeros((K, K), dtype), np.zeros(K, dtype), dtype(0)
    for n in range(N):
        S, r, cost = S + out["S_frames"][n], r + out["r_frames"][n], cost + out["cost_frames"][n]
    out.update(S=S, r=r, cost=cost, n_used=int(out["used"].sum()))
    return out


# ------------------------------------------------------------------------------------------------ the driver
def fit(prob, scale_prior_sigma=None, max_outer=30, tol=1e-6, fixed=()):
    """build.fit_link_scales_pixels on the CPU: the pose fits by the reference solver from the problem's start (its ridge
    centre), the step, damping and stop of link_scale_ref.fit.  ``fixed``: groups held at 1."""
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
            d, _obs = lref.step(sys_["S"], sys_["r"], theta, lam, prec)
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


# ------------------------------------------------------------------------------------------------ inputs of the tests
def problem(name, det=None, scales=None, groups=None, **kw):
    inp = ppx.inputs(name)
    grp, _K = groups_for(name, groups)
    return ScaledPxProblem(inp["skel"], inp["det"] if det is None else det, inp["rig"], inp["model"], inp["lo"], inp["hi"], inp["x0"],
                           groups=grp, scales=scales, **dict(ppx.OPTS, **kw))


@functools.lru_cache(maxsize=None)
def scaled_inputs(name, seed=SEED):
    """The input ``name`` of skel_pose_fit_px_ref with its detections re-projected from a truth skeleton scaled per group by
    factors uniform in [0.85, 1.15] (seeded): det + (project(scaled truth) - project(truth)), so the input's own noise, drops
    and pushes stay.  dict(det, factors, groups)."""
    inp = ppx.inputs(name)
    grp, K = groups_for(name)
    factors = 1.0 + np.random.default_rng(seed).uniform(-0.15, 0.15, K)
    pos = problem(name, scales=factors).fk(inp["truth"])
    model = "fisheye" if inp["model"] == "fisheye" else "pinhole"
    shift = ur.clean_pixels(pos, inp["rig"], model) - ur.clean_pixels(inp["truth_pos"], inp["rig"], model)      # [C, N, L, 2]
    det = inp["det"].copy()
    det[..., :2] += shift.transpose(1, 0, 2, 3)
    return dict(det=det, factors=factors, groups=grp)


@functools.lru_cache(maxsize=None)
def fitted(name, drop_slot=None):
    """The CPU driver on the scaled-truth variant of an input, computed once; ``drop_slot``: that slot's detections removed in
    every camera and frame."""
    return fit(problem(name, det=dropped(scaled_inputs(name)["det"], drop_slot)))


def dropped(det, slot):
    if slot is None:
        return det
    det = det.copy()
    det[:, :, slot, 2] = 0.0
    return det


def model_of(name, det=None):
    """skel_pose_fit_px_ref.model_of with other detections (the weights follow their validity)."""
    mdl = ppx.model_of(name)
    if det is None:
        return mdl
    from acinoset_amd import build
    valid = (det[..., 2] > ppx.THRESH) & np.isfinite(det[..., :2]).all(-1)
    return build.SkeletonModel(**{**mdl.__dict__, "meas": det[..., :2].copy(), "weights": np.where(valid, 1.0 / ppx.SIGMA_PX, 0.0)})


def camera_centre(rig, c=0):
    return -np.asarray(rig[2][c], dtype=np.float64).T @ np.asarray(rig[3][c], dtype=np.float64).reshape(3)
