"""Host side of the joint link-length fit (no GPU): the reference of tests/skel_link_fit_ref.py held to itself - c against
central differences of the cost in theta, the banded reduction against the dense one, the block-inverse identity against the
dense inverse of [[A, G], [G^T, C]] for one clip and for two clips that share theta, the numpy driver on the synthetic clip -
and the ABI entries with the argument checks that come before any device call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import skel_link_fit_ref as fref
import skel_links_ref as lkref
import skel_sample_cases as scases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("acino_skel_fte_link_fit_workspace_bytes", "acino_skel_fte_link_fit_system")
CASES = list(fref.GPU_CASES)          # the GPU tests' inputs (and pt16b, the second clip of the two-clip identity)


def ref(golden_dir, name):
    return fref.gpu_case(golden_dir, name)["ref"]


def test_gradient_in_theta_against_central_differences(golden_dir):
    """c = dF/dtheta at fixed x on pt16 against (F(x, h e_g) - F(x, -h e_g)) / 2h of the reference's own data cost, h = 1e-6.  The
    error model is that of skel_links_ref.cross_term_fd, carried through the sum over the kept rows with their weights: per pixel
    component 8 eps max|uv| / h of rounding and h^2 max|J_theta| of truncation.  No kept residual crosses zero within the step:
    every |e| is above 1e-6 x max|w J_theta| (asserted).  Observed: 8.3e-11 of max|c| against a bar of 7.5e-8."""
    c = scases.case(golden_dir, "pt16")
    prob = c["prob"]
    xa = c["x"][:, prob.ACT]
    grp, K = lkref.groups_of(prob.skel, "links")
    D = lkref.direct_term(prob, xa, grp, K)
    t = fref.theta_terms(prob, xa, grp, K, D)
    h = 1e-6
    fd = np.array([(fref.theta_terms(prob, xa, grp, K, D, theta=h * np.eye(K)[g])["data_cost"]
                    - fref.theta_terms(prob, xa, grp, K, D, theta=-h * np.eye(K)[g])["data_cost"]) / (2 * h) for g in range(K)])
    pos = lkref.positions(prob, xa, grp)
    uv_max = max(np.abs(fref.kref.project(prob, pos, ci)[0][prob.w[:, ci] > 0]).max() for ci in range(prob.C))
    jt_max = max(np.abs(np.einsum("nlij,nljg->nlig", fref.kref.project(prob, pos, ci)[1], D)[prob.w[:, ci] > 0]).max()
                 for ci in range(prob.C))
    w_max = prob.w.max()
    assert t["min_abs_e"] > 2 * h * w_max * jt_max             # no sign changes inside the step
    rows = 2 * int((prob.w > 0).sum())
    bar = rows * w_max * (8 * fref.EPS * uv_max / h + h * h * jt_max)
    top = np.abs(t["c"]).max()
    e = np.abs(fd - t["c"]).max()
    print(f"pt16: max|c| {top:.3e}, |c_fd - c| / max|c| = {e / top:.2e}, the error model's bar {bar / top:.2e}")
    assert top > 0 and e <= bar
    assert bar / top <= 1e-5


@pytest.mark.parametrize("name", CASES)
def test_the_two_reductions_agree(golden_dir, name):
    """S, r and the Newton step by the banded Cholesky against the dense LU on every input of the GPU tests, which also meet the
    condition on the kept residuals (asserted inside the reference: every |e| above 1e-6); S is symmetric to rounding, and what C
    loses to the trajectory is not small (the Schur term is visible)."""
    r = ref(golden_dir, name)
    print(f"{name}: K {r['K']}, d0 " + ", ".join(f"{k} {v:.2e}" for k, v in r["d0"].items()) +
          f"; |S - C| / |C| {fref.rel(r['S1'], r['C']):.2e}; min |e| {fref.MIN_ABS_E:.0e} passed")
    assert all(v <= 1e-8 for v in r["d0"].values())
    assert fref.rel(r["S1"].T, r["S1"]) <= 1e-9
    assert fref.rel(r["S1"], r["C"]) > 1e-3


def test_group_nine_is_exactly_zero(golden_dir):
    r = ref(golden_dir, "slice12")
    for key in ("S1", "S2", "C"):
        assert np.all(r[key][9] == 0) and np.all(r[key][:, 9] == 0), key
    assert r["c"][9] == 0 and r["r1"][9] == 0 and r["r2"][9] == 0


def _clip_terms(golden_dir, name):
    c = fref.gpu_case(golden_dir, name)
    r = c["ref"]
    return dict(ab=c["ab"], fixed=c["fixed"], G=r["G"], C=r["C"], prob=c["prob"], xa=c["x"][:, c["prob"].ACT], D=r["D"], ref=r)


@pytest.mark.parametrize("names", [("pt16",), ("pt16", "pt16b")])
def test_block_inverse_identity(golden_dir, names):
    """cov(x) = A^-1 + S_x Sigma S_x^T and cov(pos_l) = G_l A^-1 G_l^T + T_l Sigma T_l^T with Sigma = (sum_b S_b)^-1 against the
    dense inverse of the joint information, for one clip and for two clips that share theta (pt16 at two start frames).  The bar
    is bar(d0) per output, d0 the disagreement of the identity evaluated from the reference's banded pieces and from its dense
    ones.  Observed (d0 -> worst e): Sigma 3.3e-12 -> 1.2e-11, cov_x 2.6e-9 -> 3.1e-9, cov(x, theta) 1.2e-9 -> 1.9e-9,
    cov_pos 6.1e-11 -> 6.9e-11, one clip and two alike."""
    clips = [_clip_terms(golden_dir, n) for n in names]
    per_clip, Sigma_dense = fref.joint_inverse(clips)
    Sig1 = np.linalg.inv(sum(c["ref"]["S1"] for c in clips))
    Sig2 = np.linalg.inv(sum(c["ref"]["S2"] for c in clips))
    d0 = fref.rel(Sig2, Sig1)
    bar = fref.bar(d0)
    e_sig = fref.rel(Sig1, Sigma_dense)
    print(f"{names}: Sigma: d0 {d0:.2e}, bar {bar:.2e}, against the dense inverse {e_sig:.2e}")
    assert d0 <= fref.D0_REFUSED and e_sig <= bar
    for c, dense in zip(clips, per_clip):
        v1 = fref.block_inverse(c["prob"], c["xa"], c["ref"], c["ab"], c["fixed"], Sig1, "1")
        v2 = fref.block_inverse(c["prob"], c["xa"], c["ref"], c["ab"], c["fixed"], Sig2, "2")
        want = (dense["cov_x"], dense["cross"], fref.pose_marginals(c["prob"], c["xa"], c["D"], dense["cov_x"], dense["cross"], Sigma_dense))
        for key, a1, a2, w_ in zip(("cov_x", "cov(x, theta)", "cov_pos"), v1, v2, want):
            d0k, e1, e2 = fref.rel(a2, a1), fref.rel(a1, w_), fref.rel(a2, w_)
            print(f"   {key}: d0 {d0k:.2e}, bar {fref.bar(d0k):.2e}; banded pieces {e1:.2e}, dense pieces {e2:.2e}")
            assert d0k <= fref.D0_REFUSED and e1 <= fref.bar(d0k) and e2 <= fref.bar(d0k)


def test_numpy_driver_recovers_the_truth(golden_dir):
    """The joint fit on the CPU on the synthetic clip (seed fref.SEED): status ok, the cost never rises over accepted steps, every
    group within 4 of its own bars of the truth.  This is where the seed of the GPU test is chosen."""
    clip = fref.synthetic_clip(golden_dir)
    model = fref.clip_model(clip)
    prob = fref.clip_problem(clip, model)
    x0 = clip["x_true"][:, prob.ACT]
    out = fref.fit(prob, x0, max_iter=60)
    z = (out["scales"] - clip["truth"]) / out["std_scales"]
    costs = [h["cost"] for h in out["history"] if h["accepted"]]
    print(f"seed {fref.SEED}: status {out['status']}, {len(out['history'])} outer steps, cost {costs[0] if costs else float('nan'):.4f} -> "
          f"{out['history'][-1]['cost']:.4f}; truth {np.round(clip['truth'], 4)}, scales {np.round(out['scales'], 4)}, "
          f"std {np.round(out['std_scales'], 4)}, z {np.round(z, 2)}")
    assert out["status"] == "ok" and out["observed"].all()
    assert all(b <= a for a, b in zip(costs, costs[1:]))
    assert (np.abs(z) < 4.0).all()


def test_header_library_and_binding_carry_the_two_entries():
    from acinoset_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "acinoset_hip.h")).read()
    handle = C.CDLL(_lib.SO_PATH)
    for name in SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert hasattr(handle, name) and name in _lib.SIGNATURES
    assert "skel_link_fit.hip" in _lib.SOURCES and callable(build.link_fit_system) and callable(build.fit_link_scales_fte)


def _params(n_active=36, n_cams=2, loss=0):
    from acinoset_amd import _lib
    p = _lib.SkelFteParams()
    p.n_frames, p.n_cams, p.n_pose, p.n_ops, p.n_angles, p.n_active = 100, n_cams, 7, 6, 15, n_active
    p.h, p.model_weight, p.l1_eps, p.lam0 = 1.0 / 120.0, 0.002, 1e-2, 1e-3
    p.loss = loss
    return p


def test_workspace_bytes():
    from acinoset_amd import _lib
    wsb, cov = _lib.lib().acino_skel_fte_link_fit_workspace_bytes, _lib.lib().acino_skel_fte_covariance_pinned_workspace_bytes
    p = _params()
    col = (8 * 17 * 100 * 36 + 255) // 256 * 256                # one column buffer [1][17][N][n_active]
    part = 8 * 100 * 16 * 16 + (8 * 100 * 16 + 255) // 256 * 256    # the frames' C_n and c_n
    assert wsb(C.byref(p), 1, 0) == cov(C.byref(p), 1, 0) + 2 * col + part
    assert wsb(C.byref(p), 1, 1) == cov(C.byref(p), 1, 1) + 2 * col + part
    assert wsb(C.byref(p), 1, 2) == 0 and wsb(C.byref(p), 0, 0) == 0 and wsb(None, 1, 0) == 0
    assert wsb(C.byref(_params(65)), 1, 0) == 0


def test_invalid_arguments_are_refused_without_a_device():
    from acinoset_amd import _lib
    fn = _lib.lib().acino_skel_fte_link_fit_system
    p = _params()
    ops, act = (_lib.SkelOp * 6)(), (C.c_int32 * 36)()
    status = (C.c_int32 * 2)()
    fake = C.c_void_p(1 << 20)
    I6 = C.c_int32 * 6

    def call(prm=p, group=I6(0, 1, 2, -1, 0, 1), K=3, outs=(fake,) * 7, pin=0, ws=fake, ws_bytes=0, n_clips=2):
        return fn(C.byref(prm), n_clips, 0, ops, act, fake, fake, fake, fake, fake, fake, group, K, *outs, status, ws, ws_bytes, None,
                  pin, None)

    err = _lib.lib().acino_last_error_string
    assert call() == -3 and b"too small" in err()               # (valid up to the workspace of 0 bytes: no device call)
    assert call(ws=C.c_void_p((1 << 20) + 8), ws_bytes=1 << 40) == -3 and b"aligned" in err()
    for kw, what in ((dict(outs=(None,) * 7), b"required"), (dict(outs=(fake, fake, fake, fake, None, fake, fake)), b"required"),
                     (dict(K=0), b"n_groups"), (dict(K=17), b"n_groups"), (dict(group=I6(0, 1, 3, -1, 0, 1)), b"h_group"),
                     (dict(group=I6(0, 1, -2, -1, 0, 1)), b"h_group"), (dict(group=None), b"h_group"),
                     (dict(prm=_params(loss=1)), b"L1 loss only"), (dict(pin=2), b"pin_unobserved"), (dict(n_clips=0), b"n_clips"),
                     (dict(prm=_params(65)), b"n_active")):
        assert call(**kw) == -1, kw
        assert what in err(), (kw, err())
    assert call(outs=(fake,) * 5 + (None, None)) == -3          # sens and newton are optional


def test_python_argument_checks_come_before_the_gpu(golden_dir, monkeypatch):
    """Robust loss, bad groups, a bad outer-loop parameter and one camera without a prior are ValueErrors of the host layer."""
    from acinoset_amd import build
    monkeypatch.setattr(build._lib, "require_gpu", lambda: (_ for _ in ()).throw(AssertionError("the device layer was asked")))
    c = scases.case(golden_dir, "pt16")
    model, x = c["model"], c["x"]
    robust = build._with_loss(model, "redescending")
    with pytest.raises(ValueError, match="l1 loss only"):
        build.link_fit_system([robust], [x])
    with pytest.raises(ValueError, match="l1 loss only"):
        build.fit_link_scales_fte(robust)
    with pytest.raises(ValueError, match="groups"):
        build.link_fit_system([model], [x], "limbs")
    with pytest.raises(ValueError, match="no models"):
        build.link_fit_system([], [])
    with pytest.raises(ValueError, match="max_outer"):
        build.fit_link_scales_fte([model], max_outer=0)
    one = build.SkeletonModel(**{**model.__dict__, "meas": model.meas[:, :1], "weights": model.weights[:, :1], "K": model.K[:1],
                                 "D": model.D[:1], "R": model.R[:1], "t": model.t[:1]})
    with pytest.raises(ValueError, match="a larger animal further away gives the same"):
        build.fit_link_scales_fte(one)
