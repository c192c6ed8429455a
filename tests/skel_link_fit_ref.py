"""CPU reference (numpy / scipy fp64) of acino_skel_fte_link_fit_system and of build.fit_link_scales_fte: the reduced system of
the links' log-scales theta with the skeleton-FTE trajectory eliminated, the joint posterior over (trajectory, theta) and the
joint fit's driver.  Test infrastructure.

Built only from pieces that are pinned elsewhere: skel_links_ref.cross_term / direct_term / reference (G, D_l and the two
solves), skel_calib_ref.sens_banded / sens_dense / project, skel_cov_ref.fisher_blocks (inside skel_sample_ref.system: the
matrix A and its pin set) and pose_jacobian, the oracle problem's own cost and gradient (prob.evaluate), oracle.fte.lm_solve,
link_scale_ref.LinkOffsets / base_offsets and the outer loop build._fit_link_scales, which the sibling fits' tests pin.

Per kept row (n, c, l, d), e = w (uv - meas), J_theta = J_pi D_l:
    c = sum w sign(e) J_theta          C = sum w^2 J_theta^T J_theta          cost = the oracle's F(x)
    S = C - G^T A^-1 G                 r = c - G^T A^-1 g_x        (g_x: the oracle gradient, 0 at pinned rows)
by the banded Cholesky (reference 1) and by a dense LU solve (reference 2).  tests/test_skel_link_fit_host.py pins c against
central differences of the cost, the two reductions against each other and the block-inverse identity against the dense
inverse of [[A, G], [G^T, C]].  Nothing here comes from the code under test."""
import copy

import numpy as np

import link_scale_ref as lref
import skel_calib_ref as kref
import skel_cov_cases as cases
import skel_cov_ref as cref
import skel_links_ref as lkref
import skel_sample_cases as scases
import skel_sample_ref as sref
from skel_calib_ref import D0_REFUSED, bar, col_err  # noqa: F401  (re-exported)
from oracle import camera
from oracle import fte as ofte
from oracle import skel_fte as osf

EPS = np.finfo(np.float64).eps
MIN_ABS_E = 1e-6                     # a kept residual nearer to 0 could change its sign between two implementations
SEED = 0                             # of the synthetic clip (test_skel_link_fit_host.py: the numpy driver meets 4 bars on it)


def rel(a, b):
    """max |a - b| relative to the reference's largest entry."""
    return float(np.abs(np.asarray(a) - b).max() / np.abs(b).max())


def theta_terms(prob, xa, grp, K, D=None, theta=None):
    """dict(c [K], C [K, K], c_mag, C_mag, data_cost, min_abs_e) at xa (and the log-scales theta; None: 0).  The magnitudes are
    the sums of the absolute values of the elementary products, w |J_pi| |D_l| per row for c and w^2 (|J_pi| |D_l|)_g (|J_pi| |D_l|)_h
    for C: what the rounding of any order of summation is bounded by."""
    xa = np.asarray(xa, dtype=np.float64)
    pos = lkref.positions(prob, xa, grp, theta) if theta is not None else osf.skeleton_fk_jac(prob.skel, prob.full_state(xa))[0]
    D = lkref.direct_term(prob, xa, grp, K) if D is None else D
    out = dict(c=np.zeros(K), C=np.zeros((K, K)), c_mag=np.zeros(K), C_mag=np.zeros((K, K)), data_cost=0.0, min_abs_e=np.inf)
    for ci in range(prob.C):
        uv, Jpi, zc = kref.project(prob, pos, ci)
        w = np.where(np.abs(zc) < 1e-9, 0.0, prob.w[:, ci])
        kept = w > 0
        e = np.where(kept[..., None], w[..., None] * (uv - prob.meas[:, ci]), 0.0)
        Jpi = np.where(kept[..., None, None], Jpi, 0.0)
        Jt = np.einsum("nlij,nljg->nlig", Jpi, D)
        Ja = np.einsum("nlij,nljg->nlig", np.abs(Jpi), np.abs(D))
        out["c"] += np.einsum("nli,nlig->g", w[..., None] * np.sign(e), Jt)
        out["c_mag"] += np.einsum("nl,nlig->g", w, Ja)
        out["C"] += np.einsum("nlig,nl,nlih->gh", Jt, w ** 2, Jt)
        out["C_mag"] += np.einsum("nlig,nl,nlih->gh", Ja, w ** 2, Ja)
        out["data_cost"] += float(np.abs(e).sum())
        if kept.any():
            out["min_abs_e"] = min(out["min_abs_e"], float(np.abs(e[kept]).min()))
    return out


def _gram(G, X, fixed):
    """G^T A^-1 [G | g] [K, K + 1] from X = -A^-1 [G | g] (rows of pinned variables 0)."""
    Gm = np.where(fixed[:, :, None], 0.0, G)
    return -np.einsum("npa,npb->ab", Gm, X)


def reference(prob, xa, ab, fixed, groups):
    """Both reductions on one input - S1, r1, sens1, newton1 by the banded Cholesky, S2, ... by the dense LU -, C, c, cost with their
    magnitudes, the references' own disagreement d0 on every output and the bars; d0 > 1e-8 refuses the input, and so does a kept
    residual below MIN_ABS_E."""
    xa = np.asarray(xa, dtype=np.float64)
    lk = lkref.reference(prob, xa, ab, fixed, groups)
    grp, K, G, D = lk["grp"], lk["K"], lk["G"], lk["D"]
    t = theta_terms(prob, xa, grp, K, D)
    assert t["min_abs_e"] > MIN_ABS_E, f"a kept residual of {t['min_abs_e']:.1e}: its sign is not safe, the input is refused"
    cost, g, _H, _nb = prob.evaluate(xa)
    gx = np.where(fixed, 0.0, g)
    GG = np.concatenate([G, gx[..., None]], axis=-1)
    out = dict(grp=grp, K=K, G=G, D=D, gx=gx, C=t["C"], c=t["c"], C_mag=t["C_mag"], c_mag=t["c_mag"], cost=float(cost), lk=lk)
    for tag, solve in (("1", kref.sens_banded), ("2", kref.sens_dense)):
        X = solve(ab, fixed, GG)
        M = _gram(GG[..., :K], X, fixed)
        out["S" + tag], out["r" + tag] = t["C"] - M[:, :K], t["c"] - M[:, K]
        out["sens" + tag], out["newton" + tag] = X[..., :K], X[..., K]
    out["d0"] = dict(S=rel(out["S2"], out["S1"]), r=rel(out["r2"], out["r1"]), newton=rel(out["newton2"], out["newton1"]))
    for key, d0 in out["d0"].items():
        assert d0 <= D0_REFUSED, f"the two references disagree by {d0:.2e} on {key} of this input: refused"
    out["bar"] = {key: bar(d0) for key, d0 in out["d0"].items()}
    return out


def joint_inverse(clips):
    """The dense inverse of the joint information of clips that share theta, [[A_1, 0, G_1], [0, A_2, G_2], [G_1^T, G_2^T, sum C]]
    (``clips``: dicts with ab, fixed, G, C): per clip cov_x [N, P, P] (rows and columns of pinned variables 0) and
    cross [N, P, K] = cov(x_n, theta), and Sigma [K, K]."""
    K = clips[0]["C"].shape[0]
    sizes = [c["fixed"].size for c in clips]
    n = sum(sizes)
    J = np.zeros((n + K, n + K))
    o = 0
    for c, sz in zip(clips, sizes):
        J[o:o + sz, o:o + sz] = cref.dense(c["ab"])
        Gm = np.where(c["fixed"][:, :, None], 0.0, c["G"]).reshape(sz, K)
        J[o:o + sz, n:], J[n:, o:o + sz] = Gm, Gm.T
        J[n:, n:] += c["C"]
        o += sz
    Ji = np.linalg.inv(J)
    out, o = [], 0
    for c, sz in zip(clips, sizes):
        N, P = c["fixed"].shape
        full = Ji[o:o + sz, o:o + sz].reshape(N, P, N, P)
        cov_x = np.stack([full[i, :, i, :] for i in range(N)])
        cov_x = np.where(c["fixed"][:, :, None] | c["fixed"][:, None, :], 0.0, cov_x)
        cross = np.where(c["fixed"][:, :, None], 0.0, Ji[o:o + sz, n:].reshape(N, P, K))
        out.append(dict(cov_x=cov_x, cross=cross))
        o += sz
    return out, Ji[n:, n:]


def pose_marginals(prob, xa, D, cov_x, cross, Sigma):
    """cov(pos_l) [N, L, 3, 3] of the joint posterior: [G_l D_l] cov(x_n, theta) [G_l D_l]^T."""
    Gl = cref.pose_jacobian(prob, np.asarray(xa, dtype=np.float64))
    a = np.einsum("nlip,npq,nljq->nlij", Gl, cov_x, Gl)
    b = np.einsum("nlip,npg,nljg->nlij", Gl, cross, D)
    return a + b + np.swapaxes(b, 2, 3) + np.einsum("nlig,gh,nljh->nlij", D, Sigma, D)


def block_inverse(prob, xa, ref_, ab, fixed, Sigma, which="1"):
    """(cov_x [N, P, P], cross [N, P, K], cov_pos [N, L, 3, 3]) of the block-inverse identity - cov(x) = A^-1 + S_x Sigma S_x^T,
    cov(x, theta) = S_x Sigma, cov(pos_l) = G_l A^-1 G_l^T + T_l Sigma T_l^T - from one reference's own pieces: "1" the banded
    solves (S_x, T_l, the blocks of A^-1 by skel_cov_ref.probe_blocks), "2" the dense ones (skel_cov_ref.dense_blocks)."""
    Sx, T = ref_["sens" + which], ref_["lk"]["T" + which]
    blocks = cref.probe_blocks(ab, fixed, np.arange(fixed.shape[0])) if which == "1" else cref.dense_blocks(ab, fixed)
    Gl = cref.pose_jacobian(prob, np.asarray(xa, dtype=np.float64))
    cov_pos = np.einsum("nlip,npq,nljq->nlij", Gl, blocks, Gl) + np.einsum("nlig,gh,nljh->nlij", T, Sigma, T)
    return blocks + np.einsum("npg,gh,nqh->npq", Sx, Sigma, Sx), np.einsum("npg,gh->nph", Sx, Sigma), cov_pos


# ---- the joint fit on the CPU ------------------------------------------------------------------------------------------------
class ScaledSkelProblem(osf.SkelFTEProblem):
    """The oracle problem of a skeleton whose links carry ``offsets`` [n_links, 3]: ``skel`` answers every look-up with a
    skeleton whose ``positions`` are a fresh link_scale_ref.LinkOffsets (one FK call reads it once, in link order)."""
    offsets = None

    @property
    def skel(self):
        if self.offsets is None:
            return self._skel
        return dict(self._skel, positions=lref.LinkOffsets(len(self._skel["positions"]), self.offsets))

    @skel.setter
    def skel(self, value):
        self._skel = value

    def with_offsets(self, offsets):
        p = copy.copy(self)
        p.offsets = np.asarray(offsets, dtype=np.float64)
        return p


def synthetic_clip(golden_dir, seed=SEED, n_frames=24):
    """The driver's input: the 5-link tree (cases.SUB_TREES[16], 15 active states) on the two cameras of the test rig, 24 frames.
    The root moves along the fixture's line, every angle follows a sinusoid of a quarter to half a period (0.15 rad; its third
    differences cost the smoothness prior about 10 against a data cost of 576, so the truth is a trajectory the model states)
    inside the box, the links are scaled by up to 15 %, and every pixel coordinate carries Laplace noise of the scale the model states, 1 / w = R_MEAS_TEST.
    Returns dict(sk, scene, det, parts, truth [K], x_true [N, P_full], grp, K)."""
    g, sk0, _det = scases.fixture(golden_dir)
    sk = cases.sub_skeleton(cases.generic_skeleton(sk0), cases.SUB_TREES[16])
    sc = scases.scene(g)
    rng = np.random.default_rng(seed)
    grp, K = lkref.groups_of(sk, "links")
    truth = 1.0 + 0.15 * rng.uniform(-1.0, 1.0, K)
    act = np.asarray(osf.active_states(sk))
    lo, hi = osf.bounds_table(sk, n_frames)
    P_full = lo.shape[1]
    tt = np.arange(n_frames) / n_frames
    x = np.zeros((n_frames, P_full))
    x0 = np.asarray(g["init_x"], dtype=np.float64)
    x[:, :3] = x0[0, :3][None, :] + np.arange(n_frames)[:, None] * (x0[1, :3] - x0[0, :3])[None, :]
    x[:, :3] += 0.05 * np.sin(2 * np.pi * tt[:, None] * rng.uniform(0.25, 0.5, 3)[None, :] + rng.uniform(0, 2 * np.pi, 3)[None, :])
    na = len(act) - 3
    ang = rng.uniform(-0.3, 0.3, na)[None, :] + 0.15 * np.sin(2 * np.pi * tt[:, None] * rng.uniform(0.25, 0.5, na)[None, :]
                                                             + rng.uniform(0, 2 * np.pi, na)[None, :])
    x[:, act[3:]] = ang
    x[:, act] = np.clip(x[:, act], lo[:, act] + 1e-3, hi[:, act] - 1e-3)
    off = lref.base_offsets(sk) * np.where(grp >= 0, truth[np.maximum(grp, 0)], 1.0)[:, None]
    pos = lref.oracle_fk(sk, off, x)[0]                         # [N, L, 3]
    names = osf.pose_names(sk)
    Cn = len(sc[0])
    det = np.zeros((n_frames, Cn, len(names), 3))
    for ci in range(Cn):
        uv = camera.pt3d_to_2d(pos, sc[0][ci], sc[1][ci], sc[2][ci], sc[3][ci])
        det[:, ci, :, :2] = uv + rng.laplace(0.0, cases.R_MEAS_TEST, uv.shape)
        det[:, ci, :, 2] = 1.0
    return dict(sk=sk, scene=sc, det=det, parts=list(names), truth=truth, x_true=x, grp=grp, K=K)


def clip_model(clip, first=0, n=None):
    """The SkeletonModel of frames first .. first + n of a synthetic clip, through build.build_model."""
    from acinoset_amd import build
    n = clip["det"].shape[0] - first if n is None else n
    model, _ = build.build_model(clip["sk"], scene=clip["scene"], dlc_tables=cases.tables(clip["det"], clip["parts"]), n_frames=n,
                                 start_frame=first, pairing="name", initial_line=False, r_meas=cases.R_MEAS_TEST)
    return model


def clip_problem(clip, model):
    return ScaledSkelProblem(clip["sk"], model.meas, model.weights, *clip["scene"], model.h, lo=model.lo, hi=model.hi)


def fit(prob, x0_active, groups="links", scale_prior_sigma=None, max_outer=30, tol=1e-6, max_iter=200):
    """build.fit_link_scales_fte on the CPU for ONE clip: build._fit_link_scales (the pinned outer loop) with a numpy evaluate -
    oracle.fte.lm_solve on the problem with the scaled offsets, started from the last solution, then the banded reduction."""
    from acinoset_amd import build
    grp, K = lkref.groups_of(prob._skel, groups)
    last = [np.asarray(x0_active, dtype=np.float64)]

    def evaluate(theta):
        p = prob.with_offsets(lkref.offsets(prob._skel, grp, theta))
        xa, info = ofte.lm_solve(p, last[0], max_iter=max_iter)
        last[0] = xa
        ab, fixed = sref.system(p, xa)
        D = lkref.direct_term(p, xa, grp, K)
        G = lkref.cross_term(p, xa, grp, K, D)
        t = theta_terms(p, xa, grp, K, D)
        cost, g, _H, _nb = p.evaluate(xa)
        GG = np.concatenate([G, np.where(fixed, 0.0, g)[..., None]], axis=-1)
        M = _gram(G, kref.sens_banded(ab, fixed, GG), fixed)
        sys_ = dict(S=t["C"] - M[:, :K], r=t["c"] - M[:, K], cost_frames=np.array([float(cost)]), used=np.array([True]), n_used=1)
        return p, (xa, info), sys_

    return build._fit_link_scales(evaluate, grp, K, scale_prior_sigma, max_outer, tol)


# ---- the inputs of the GPU tests, with their references, once per process ------------------------------------------------------
P51_GROUPS = np.arange(20) % 16
# name -> (input of skel_sample_cases / skel_unobs_cases, groups, every third variable pinned, pin_unobserved)
GPU_CASES = {"pt16": ("pt16", "links", False, False), "pt32": ("pt32", "links", False, False), "slice12": ("slice12", "links", False, False),
             "slice40global": ("slice40", "global", False, False), "slice40": ("slice40", "links", False, False),
             "p51": ("p51", P51_GROUPS, False, False), "pt16pin": ("pt16pin", "links", False, False),
             "pt16b": ("pt16b", "links", False, False),
             "slice40pins": ("slice40", "links", True, False), "shipped12": ("shipped12", "links", False, True)}
_CASES = {}


def tight(model, x, which):
    """A copy of ``model`` with the lower limits of the variables ``which`` [N, n_active] closed onto the iterate."""
    m = copy.copy(model)
    act = np.asarray(model.active)
    lo, hi = model.lo.copy(), model.hi.copy()
    la, ha = lo[:, act], hi[:, act]
    la[which], ha[which] = x[:, act][which], x[:, act][which] + 1.0
    lo[:, act], hi[:, act] = la, ha
    m.lo, m.hi = lo, hi
    return m


def gpu_case(golden_dir, name):
    """dict(model, x, prob, fixed, ab, groups, pin_unobserved, ref) of an input of the GPU tests; the reference asserts the
    condition on the kept residuals.  No case needed a perturbed iterate: every kept |e| of cases.iterate is above 1e-6."""
    if name in _CASES:
        return _CASES[name]
    base, groups, pins, unobs = GPU_CASES[name]
    if unobs:
        import skel_unobs_cases as ucases
        c = ucases.case(golden_dir, base)
        model, x, prob, ab, fixed = c["model"], c["x"], c["prob"], c["ref"]["ab"], c["ref"]["fixed"]
    else:
        c = scases.case(golden_dir, base)
        model, x, prob, ab, fixed = c["model"], c["x"], c["prob"], c["ab"], c["fixed"]
        if pins:
            which = np.zeros((model.N, prob.P), dtype=bool)
            which.reshape(-1)[::3] = True
            model = tight(model, x, which)
            prob = cases.problem(c["sk"], model, c["scene"])
            ab, fixed = sref.system(prob, x[:, prob.ACT])
            assert 0 < fixed.sum() < which.sum() and not (fixed & ~which).any()
    _CASES[name] = dict(model=model, x=x, prob=prob, ab=ab, fixed=fixed, groups=groups, pin_unobserved=unobs,
                        ref=reference(prob, x[:, prob.ACT], ab, fixed, groups))
    return _CASES[name]
