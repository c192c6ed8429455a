"""Link-scale fit from the detections, host side (no GPU): the reference of tests/link_scale_px_ref.py against the derivative of
the minimised objective and against the dense joint Gauss-Newton system of a frame; the exact identity of a one-camera rig; the
argument handling of the Python wrappers and of the C ABI; build.fit_link_scales and build.fit_link_scales_pixels through their
shared outer loop with the reference standing in for the device; and the condition test_gpu_link_scale_px.py relies on - the CPU
driver alone recovers the scaled truth of pt16-two, seed link_scale_px_ref.SEED, within 4 of its own bars."""
import ctypes as C
import inspect

import numpy as np
import pytest

import __graft_entry__ as ge
import link_scale_px_ref as xref
import link_scale_ref as lref
import skel_pose_fit_px_ref as ppx
import skel_pose_fit_ref as pref
from acinoset_amd import _lib, build

# The longdouble reference's worst |S_n| / C_n over the frames of generic-mono with a free root, groups "global", at the
# reference's own minimisers: measured here on the CPU (test_mono_identity_of_the_reference prints it: 1.25e-18, 12 eps of the
# format).  S_n = 0 in exact arithmetic; the assertion on that reference gets a factor of 100 over the measured value, the rest
# being the rounding of the solve.  An fp64 evaluation - the reference's here, the device's in test_gpu_link_scale_px.py - is
# held to the bars of the per-frame outputs instead: 256 max(|ref64 - ref80|, eps * magnitude).
MONO_S_OVER_C = 1.3e-18
MONO_FACTOR = 100.0
EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def lib():
    ge.build()
    return _lib.lib()


def _solved(prob):
    x, status, _it, cost = prob.solve()
    xs = np.where(np.isfinite(x), x, prob.x0)
    o = prob.objective(xs)
    return xs, status, cost, prob.active_set(xs, o["g"], o["A"]), o


# ------------------------------------------------------------------------------------------------ reference self-checks
def test_r_is_the_derivative_of_the_minimised_objective():
    """pt16-two, the frames the reference solver finishes with no bound-active state: d/dtheta of min_x F_n(x; theta), by central
    differences through the CPU solver (h = 1e-4; the solver stops within 1e-10 F, hence the absolute term), against r_n at the
    minimiser - r_n carries w r, the exact gradient of the Cauchy cost."""
    base = np.full(5, 1.05)
    prob = xref.problem("pt16-two", scales=base)
    assert prob.K == 5
    xs, status, _cost, pinned, _o = _solved(prob)
    sys_ = xref.system(prob, xs, pinned, status)
    ok = (status == 0) & ~pinned.any(1) & sys_["used"]
    h = 1e-4
    worst = 0.0
    for g in range(prob.K):
        e = np.zeros(prob.K)
        e[g] = h
        Fp, Fm = (prob.with_scales(base * np.exp(s * e)).solve()[3] for s in (1.0, -1.0))
        fd = (Fp - Fm) / (2 * h)
        both = ok & np.isfinite(fd)
        err = np.abs(fd[both] - sys_["r_frames"][both, g])
        worst = max(worst, (err / (1e-3 * np.abs(sys_["r_frames"][both]).max(1) + 1e-3)).max())
    print(f"pt16-two: r_n against the finite difference of min F, error / bound {worst:.2e} on {ok.sum()} frames, "
          f"|r| max {np.abs(sys_['r_frames'][ok]).max():.2e}")
    assert ok.sum() >= 12 and worst <= 1.0 and np.abs(sys_["r_frames"][ok]).max() > 1.0


@pytest.mark.parametrize("name", ("shipped-pinhole-pushed", "pt32-three"))
def test_frame_system_is_the_schur_complement_of_the_dense_joint_system(name):
    K = xref.groups_for(name)[1]
    prob = xref.problem(name, scales=np.full(K, 1.07))
    xs, status, cost, pinned, o = _solved(prob)
    if name == "pt32-three":
        assert pinned.sum() >= 1
    worst = 0.0
    for n in np.nonzero(status < 2)[0]:
        f = xref.frame_system(prob, n, xs, pinned)
        H, grad, nf = xref.joint_matrix(prob, n, xs, pinned)
        fr = ~pinned[n]
        assert np.abs(H[:nf, :nf] - o["A"][n][np.ix_(fr, fr)]).max() <= 1e-9 * np.abs(H).max()
        assert np.allclose(grad[:nf], o["g"][n][fr], rtol=1e-9, atol=1e-9 * np.abs(grad).max())
        S = H[nf:, nf:] - H[nf:, :nf] @ np.linalg.solve(H[:nf, :nf], H[:nf, nf:])
        r = grad[nf:] - H[nf:, :nf] @ np.linalg.solve(H[:nf, :nf], grad[:nf])
        sens = -np.linalg.solve(H[:nf, :nf], H[:nf, nf:])
        worst = max(worst, np.abs(f["S"] - S).max() / np.abs(H[nf:, nf:]).max(), np.abs(f["r"] - r).max() / np.abs(grad[nf:]).max())
        assert np.abs(f["sens"][fr] - sens).max() <= 1e-7 * max(np.abs(sens).max(), 1.0) and (f["sens"][pinned[n]] == 0).all()
        assert np.isclose(f["F"], cost[n], rtol=1e-12, atol=0) and np.array_equal(f["S"], f["S"].T)
    print(f"{name}: S_n, r_n against the dense Schur complement, relative {worst:.2e}")
    assert worst < 1e-8


def mono_frames(prob, pinned, used):
    return np.nonzero(used & ~pinned[:, :3].any(1))[0]


def test_mono_identity_of_the_reference():
    """One camera, one scale for every link: scaling the animal about the camera centre leaves every pixel where it is, so
    (root - centre, 0, 1) is a null vector of [Jc Jsc]: S_n = 0, sens_n[:3, 0] = root - centre, sens_n[3:, 0] = 0."""
    prob = xref.problem("generic-mono", groups="global")
    assert prob.C == 1 and prob.K == 1
    xs, status, _cost, pinned, _o = _solved(prob)
    centre = xref.camera_centre(prob.rig)
    r64, r80 = (xref.system(prob, xs, pinned, status, dt) for dt in (np.float64, np.longdouble))
    frames = mono_frames(prob, pinned, r80["used"])
    assert len(frames) >= 12
    want = np.zeros((len(frames), prob.P))
    want[:, :3] = xs[frames, :3] - centre
    worst = {}
    for name, ref in (("float64", r64), ("longdouble", r80)):
        Cn = np.array([xref.frame_terms(prob, n, xs, dtype=np.longdouble)["C"][0, 0] for n in frames])
        sens = ref["sens"][frames, :, 0]
        worst[name] = (float(np.abs(ref["S_frames"][frames, 0, 0] / Cn).max()), float(np.abs(sens[:, :3] - want[:, :3]).max()),
                       float(np.abs(sens[:, 3:]).max()))
    print("generic-mono, global: worst |S_n| / C_n, |sens[:3] - (root - centre)| [m], |sens[3:]| [rad]: " +
          "; ".join(f"{k} {v[0]:.2e} {v[1]:.2e} {v[2]:.2e}" for k, v in worst.items()))
    assert worst["longdouble"][0] <= MONO_FACTOR * MONO_S_OVER_C
    # the fp64 evaluation against the exact values, within the bars of the per-frame outputs
    for key, mag, exact in (("S_frames", "mag_S", np.zeros((len(frames), 1, 1))), ("sens", "mag_sens", want[:, :, None])):
        bar = 256.0 * np.maximum(np.abs(r64[key][frames].astype(np.longdouble) - r80[key][frames]), EPS * r80[mag][frames])
        assert (np.abs(r64[key][frames] - exact) <= bar).all(), key


def test_the_cpu_driver_recovers_the_scaled_truth_within_four_bars():
    """Seed link_scale_px_ref.SEED on pt16-two: what test_gpu_link_scale_px.py asks of the GPU driver holds for the reference."""
    sc = xref.scaled_inputs("pt16-two")
    out = xref.fitted("pt16-two")
    z = (out["scales"] - sc["factors"]) / out["std_scales"]
    print(f"seed {xref.SEED}: factors {np.round(sc['factors'], 3)}, scales {np.round(out['scales'], 3)}, std {np.round(out['std_scales'], 4)}, "
          f"z {np.round(z, 2)}, {len(out['history'])} outer steps, status {out['status']}")
    assert out["status"] == "ok" and out["observed"].all() and np.abs(z).max() < 4.0
    costs = [h["cost"] for h in out["history"]]
    assert all(b <= a for a, b in zip(costs, costs[1:]))
    assert np.abs(sc["factors"] - 1).max() > 0.05 and np.abs(out["scales"] - sc["factors"]).max() < 0.5 * np.abs(sc["factors"] - 1).max()


# ------------------------------------------------------------------------------------------------ the shared outer loop
def _as_fit(x, status, pinned):
    return dict(x=x, status=status.astype(np.uint8), pinned=pinned.astype(np.uint8))


def test_fit_link_scales_is_unchanged_through_the_shared_driver(monkeypatch):
    """build.fit_link_scales with the numpy reference in place of the two device calls walks the path of link_scale_ref.fit:
    same scales, bars, history and status, the dict of before."""
    from test_gpu_link_scale import model_of
    inp, sc = pref.inputs("pt16"), lref.scaled_inputs("pt16")
    prob = lref.problem("pt16", points=sc["points"])

    def pose_fit(mdl, points, cov, x0=None, **kw):
        assert kw == dict(prior_sigma=1.0, max_iter=255, return_cov=False) and x0 is not None
        p = prob.with_scales(mdl.link_scales)
        x, status, _it, cost = p.solve()
        xs = np.where(np.isfinite(x), x, p.x0)
        o = p.objective(xs)
        return dict(_as_fit(x, status, p.active_set(xs, o["g"], o["A"])), cost=cost)

    def link_scale_system(mdl, points, cov, fit, groups, prior_sigma, sigma_iso, m):
        assert prior_sigma == 1.0 and sigma_iso == 0.01 and np.array_equal(m, prob.x0)
        return lref.system(prob.with_scales(mdl.link_scales), fit["x"], fit["pinned"].astype(bool), fit["status"])

    monkeypatch.setattr(build, "pose_fit", pose_fit)
    monkeypatch.setattr(build, "link_scale_system", link_scale_system)
    out = build.fit_link_scales(model_of(inp["skel"], inp["lo"], inp["hi"]), sc["points"], inp["cov"], x0=prob.x0)
    want = lref.fitted("pt16")
    assert set(out) == {"scales", "cov_log_scales", "std_scales", "observed", "groups", "model", "fit", "system", "history", "status"}
    assert out["status"] == want["status"] == "ok" and np.array_equal(out["observed"], want["observed"])
    assert np.array_equal(out["scales"], want["scales"]) and np.array_equal(out["std_scales"], want["std_scales"])
    assert np.array_equal(out["cov_log_scales"], want["cov_log_scales"])
    assert [{k: h[k] for k in ("cost", "max_dtheta", "lam", "n_used")} for h in out["history"]] == want["history"]
    assert [h["accepted"] for h in out["history"]] == [True] * (len(want["history"]) - 1) + [False]
    assert np.array_equal(out["model"].link_scales, out["scales"]) and np.array_equal(out["groups"], sc["groups"])


def test_fit_link_scales_pixels_walks_the_reference_drivers_path(monkeypatch):
    """The pixel form through the same outer loop, the numpy reference in place of the two device calls: link_scale_px_ref.fit."""
    sc = xref.scaled_inputs("pt16-two")
    prob = xref.problem("pt16-two", det=sc["det"])
    seen = []

    def pose_fit_pixels(mdl, x0=None, **kw):
        seen.append(kw)
        assert np.array_equal(x0, prob.x0)
        p = prob.with_scales(mdl.link_scales)
        xs, status, cost, pinned, _o = _solved(p)
        return dict(_as_fit(np.where((status < 2)[:, None], xs, np.nan), status, pinned), cost=cost)

    def link_scale_system_pixels(mdl, fit, groups, m, **kw):
        assert np.array_equal(m, prob.x0) and kw["prior_sigma"] == 1.0 and kw["sigma_px"] == ppx.SIGMA_PX
        return xref.system(prob.with_scales(mdl.link_scales), fit["x"], fit["pinned"].astype(bool), fit["status"])

    monkeypatch.setattr(build, "pose_fit_pixels", pose_fit_pixels)
    monkeypatch.setattr(build, "link_scale_system_pixels", link_scale_system_pixels)
    out = build.fit_link_scales_pixels(xref.model_of("pt16-two", sc["det"]), x0=ppx.inputs("pt16-two")["x0"])
    want = xref.fitted("pt16-two")
    assert seen[0]["max_iter"] == 255 and seen[0]["prior_sigma"] == 1.0 and seen[0]["thresh"] == 0.5 and seen[0]["return_cov"] is False
    assert np.array_equal(seen[0]["det"][..., :2], sc["det"][..., :2])
    assert out["status"] == want["status"] and np.array_equal(out["scales"], want["scales"])
    assert np.array_equal(out["std_scales"], want["std_scales"]) and len(out["history"]) == len(want["history"])


# ------------------------------------------------------------------------------------------------ the wrappers
def test_wrappers_check_their_arguments():
    mdl = ppx.model_of("pt16-two")
    N, P = mdl.N, len(mdl.active)
    fit = dict(x=np.zeros((N, P)), pinned=np.zeros((N, P), np.uint8), status=np.zeros(N, np.uint8))
    for kw, word in ((dict(fit=dict(fit, x=np.zeros((N, P + 1)))), r"fit\['x'\]"), (dict(fit=dict(fit, status=np.zeros(N + 1))), r"fit\['status'\]"),
                     (dict(fit=dict(fit, pinned=np.zeros((N, 1)))), r"fit\['pinned'\]"), (dict(m=np.zeros((N, P - 1))), "m must be"),
                     (dict(det=np.zeros((N, 3, 6, 3))), "det must be"), (dict(sigma_px=0.0), "sigma_px"), (dict(f_scale=np.inf), "f_scale"),
                     (dict(prior_sigma=-1.0), "prior_sigma"), (dict(thresh=np.nan), "thresh"), (dict(groups="parts"), "groups"),
                     (dict(groups=[0, 1, 2]), "groups")):
        with pytest.raises(ValueError, match=word):
            build.link_scale_system_pixels(mdl, **dict(dict(fit=fit), **kw))
    for kw, word in ((dict(scale_prior_sigma=0.0), "scale_prior_sigma"), (dict(max_outer=0), "max_outer"), (dict(tol=0.0), "tol"),
                     (dict(groups=[0] * 4), "groups")):
        with pytest.raises(ValueError, match=word):
            build.fit_link_scales_pixels(mdl, **kw)
    sig = inspect.signature(build.link_scale_system_pixels)
    assert {k: v.default for k, v in sig.parameters.items() if k not in ("model", "fit")} == dict(
        groups="links", det=None, thresh=0.5, f_scale=5.0, sigma_px=None, prior_sigma=np.pi, m=None, return_sens=True)
    sig = inspect.signature(build.fit_link_scales_pixels)
    assert {k: v.default for k, v in sig.parameters.items() if k not in ("model", "fit_kw")} == dict(
        groups="links", x0=None, det=None, thresh=0.5, f_scale=5.0, sigma_px=None, scale_prior_sigma=None, max_outer=30, tol=1e-6,
        prior_sigma=1.0, max_iter=255)
    assert "skel_link_scale_px.hip" in _lib.SOURCES and "link_scale_dev.hpp" in _lib.HEADERS


def test_one_camera_needs_a_prior_on_the_scales():
    mdl = ppx.model_of("generic-mono")
    with pytest.raises(ValueError, match="one camera"):
        build.fit_link_scales_pixels(mdl, groups="global", x0=ppx.inputs("generic-mono")["x0"])
    with pytest.raises(ValueError, match="scale_prior_sigma"):
        build.fit_link_scales_pixels(mdl, groups="global", scale_prior_sigma=np.inf)


# ------------------------------------------------------------------------------------------------ C ABI
BUFS = ("det", "cams", "x", "m", "pinned", "status", "S", "r", "F", "used", "fst", "ws")


def _skel_params_of(model):
    p = _lib.SkelFteParams()
    p.n_pose, p.n_ops = len(model.prog["names"]), len(model.prog["ops"])
    p.n_angles, p.n_active = model.prog["n_angles"], len(model.active)
    return p


def _prm(**kw):
    f = dict(camera_model=0, max_iter=1, min_detections=1, reserved=0, lam0=1e-3, ftol=1e-10, xtol=1e-10, prior_sigma=1.0, thresh=0.5,
             f_scale=5.0, sigma_px=5.0)
    f.update(kw)
    return _lib.PoseFitPxParams(*[f[name] for name, _t in _lib.PoseFitPxParams._fields_])


def _call(lib, p=None, prm=True, groups=(0, 1, 2, 3, 4), K=5, n_frames=10, n_cams=2, ops=True, active=True, ws_bytes=None, prm_kw=None,
          **bufs):
    model = ppx.model_of("pt16-two")
    p = _skel_params_of(model) if p is None else p
    b = dict(dict.fromkeys(BUFS, 256), **bufs)
    ptr, null = (lambda v: C.c_void_p(v)), C.c_void_p(0)
    act = np.asarray(model.active, dtype=np.int32)
    act_c = (C.c_int32 * len(act))(*[int(a) for a in act])
    grp_c = None if groups is None else (C.c_int32 * len(groups))(*groups)
    nbytes = lib.acino_skel_link_scale_px_workspace_bytes(C.byref(p)) if ws_bytes is None else ws_bytes
    return lib.acino_skel_link_scale_px(C.byref(_prm(**(prm_kw or {}))) if prm else None, C.byref(p),
                                        build._ops_array(model.prog) if ops else None, act_c if active else None, grp_c, K, ptr(b["det"]),
                                        n_frames, n_cams, ptr(b["cams"]), ptr(b["x"]), ptr(b["m"]), ptr(b["pinned"]), ptr(b["status"]),
                                        ptr(b["S"]), ptr(b["r"]), ptr(b["F"]), ptr(b["used"]), ptr(b["fst"]), null, null, ptr(b["ws"]),
                                        nbytes, null)


def test_abi_arguments_are_checked_before_any_device_call(lib):
    p0 = _skel_params_of(ppx.model_of("pt16-two"))
    assert lib.acino_skel_link_scale_px_workspace_bytes(C.byref(p0)) == lib.acino_skel_pose_fit_px_workspace_bytes(C.byref(p0)) > 0
    assert lib.acino_skel_link_scale_px_workspace_bytes(None) == 0
    assert lib.acino_sizeof_pose_fit_px_params() == C.sizeof(_lib.PoseFitPxParams)          # (no struct is added: prm is the pose fit's)
    for kw, word in ((dict(K=0), b"n_groups"), (dict(K=17), b"n_groups"), (dict(groups=(0, 1, 2, 3, 5)), b"h_group"),
                     (dict(groups=(0, 1, -2, 3, 4)), b"h_group"), (dict(groups=(0, 1, 2, 3, 4), K=4), b"h_group"),
                     (dict(groups=None), b"null buffer"), (dict(ops=False), b"null buffer"), (dict(active=False), b"null buffer"),
                     (dict(prm=False), b"prm"), (dict(n_frames=-1), b"n_frames"), (dict(n_cams=0), b"n_cams"), (dict(n_cams=17), b"n_cams"),
                     (dict(prm_kw=dict(camera_model=2)), b"camera_model"), (dict(prm_kw=dict(prior_sigma=0.0)), b"prior_sigma"),
                     (dict(prm_kw=dict(sigma_px=np.nan)), b"sigma_px"), (dict(prm_kw=dict(f_scale=0.0)), b"f_scale"),
                     (dict(prm_kw=dict(thresh=np.nan)), b"thresh"), (dict(prm_kw=dict(max_iter=0)), b"max_iter"),
                     *[(dict([(k, 0)]), b"null buffer") for k in BUFS]):
        assert _call(lib, **kw) == -1 and word in lib.acino_last_error_string(), kw
    assert _call(lib, groups=(0, -1, -1, 1, 1), K=2, n_frames=0) == 0
    assert _call(lib, ws=8) != 0 and b"aligned" in lib.acino_last_error_string()
    assert _call(lib, ws_bytes=16) != 0 and b"workspace too small" in lib.acino_last_error_string()
    bad = _skel_params_of(ppx.model_of("pt16-two"))
    bad.n_active = 65
    assert _call(lib, p=bad) == -1 and lib.acino_skel_link_scale_px_workspace_bytes(C.byref(bad)) == 0
    assert _call(lib, n_frames=0, **dict.fromkeys(BUFS, 0)) == 0              # empty input is a no-op


def test_a_shape_beyond_the_lds_is_refused_with_the_pixel_pose_fits_error(lib):
    """64 states and 64 slots seen by 16 cameras: G, Jc with the K columns and 16 cameras' detections pass 160 KB."""
    p = _lib.SkelFteParams()
    p.n_pose, p.n_ops, p.n_angles, p.n_active = 65, 64, 64, 64
    ops = (_lib.SkelOp * 64)()
    for k in range(64):
        ops[k].child, ops[k].parent, ops[k].angle, ops[k].flags = k + 1, k, k, 1 if k < 61 else 0
        ops[k].off[0] = 0.1
    act = (C.c_int32 * 64)(*([0, 1, 2] + [3 + k for k in range(61)]))
    grp = (C.c_int32 * 64)(*[k % 16 for k in range(64)])
    assert lib.acino_skel_link_scale_px_workspace_bytes(C.byref(p)) > 0
    a = C.c_void_p(256)
    rc = lib.acino_skel_link_scale_px(C.byref(_prm()), C.byref(p), ops, act, grp, 16, a, 10, 16, a, a, a, a, a, a, a, a, a, a, None, None,
                                      a, 1 << 20, None)
    assert rc == -1 and b"pixel pose fit's 160 KB" in lib.acino_last_error_string()
