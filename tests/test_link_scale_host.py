"""Link-scale fit, host side (no GPU): the reference of tests/link_scale_ref.py against central differences of the oracle's FK
on re-scaled offsets, against the dense joint Gauss-Newton system of a frame and against the derivative of the minimised
objective; the group rules of build.scale_links; build_model(link_scales=...); the argument handling of the C ABI; and the
condition test_gpu_link_scale.py relies on - the CPU driver alone recovers the scaled truth of seed link_scale_ref.SEED within 4
of its own bars."""
import ctypes as C
import inspect

import numpy as np
import pytest

import __graft_entry__ as ge
import link_scale_ref as lref
import skel_cov_cases as cases
import skel_pose_fit_ref as pref
from acinoset_amd import _lib, build


@pytest.fixture(scope="module")
def lib():
    ge.build()
    return _lib.lib()


def _point(prob, seed=5):
    rng = np.random.default_rng(seed)
    return np.clip(prob.x0 + rng.normal(0.0, 0.1, prob.x0.shape), prob.lo, prob.hi)


# ------------------------------------------------------------------------------------------------ reference self-checks
@pytest.mark.parametrize("name", ("shipped", "pt16", "p51"))
def test_link_offsets_at_the_scales_one_are_the_plain_skeleton(name):
    """The stand-in for ``positions`` gives the oracle's FK and Jacobian of the skeleton as it stands, bit for bit - the
    shipped skeleton, which defines a part twice, included - and the groups' shares add up to the pose."""
    prob = lref.problem(name)
    x = _point(prob)
    want = pref.problem(name).fk(x, with_jac=True)
    got = prob.fk(x, with_jac=True)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    D = lref.dpos_dtheta(prob, x)
    assert D.shape == (prob.N, prob.L, 3, prob.K)
    if (prob.grp >= 0).all():
        assert np.abs(D.sum(-1) - (want[0] - x[:, None, :3])).max() <= 1e-14


@pytest.mark.parametrize("name", ("shipped", "pt16"))
def test_dpos_dtheta_matches_central_differences_of_the_oracle_fk(name):
    """h = 1e-6 on theta at scales off 1: truncation ~1e-13 of a link of 0.5 m, rounding ~1e-10."""
    scales = 1.0 + np.random.default_rng(2).uniform(-0.1, 0.1, lref.groups_of(pref.inputs(name)["skel"], lref.GROUPS[name])[1])
    prob = lref.problem(name, scales=scales)
    x = _point(prob)
    D = lref.dpos_dtheta(prob, x)
    h = 1e-6
    worst = 0.0
    for g in range(prob.K):
        e = np.zeros(prob.K)
        e[g] = h
        fd = (prob.with_scales(scales * np.exp(e)).fk(x) - prob.with_scales(scales * np.exp(-e)).fk(x)) / (2 * h)
        worst = max(worst, np.abs(fd - D[..., g]).max())
    print(f"{name}: dpos/dtheta against central differences {worst:.2e}")
    assert worst < 1e-8 and np.abs(D).max() > 0.05


@pytest.mark.parametrize("name", ("shipped", "pt16"))
def test_frame_system_is_the_schur_complement_of_the_dense_joint_system(name):
    prob = lref.problem(name, scales=np.full(lref.groups_of(pref.inputs(name)["skel"], lref.GROUPS[name])[1], 1.07))
    x = _point(prob)
    o = prob.objective(x)
    pinned = prob.active_set(x, o["g"], o["A"])
    assert pinned.sum() >= 1
    worst = 0.0
    for n in np.nonzero(prob.n_markers >= 1)[0]:
        f = lref.frame_system(prob, n, x, pinned)
        H, grad, nf = lref.joint_matrix(prob, n, x, pinned)
        assert np.abs(H[:nf, :nf] - o["A"][n][np.ix_(~pinned[n], ~pinned[n])]).max() <= 1e-9 * np.abs(H).max()
        assert np.allclose(grad[:nf], o["g"][n][~pinned[n]], rtol=1e-9, atol=1e-9 * np.abs(grad).max())
        S = H[nf:, nf:] - H[nf:, :nf] @ np.linalg.solve(H[:nf, :nf], H[:nf, nf:])
        r = grad[nf:] - H[nf:, :nf] @ np.linalg.solve(H[:nf, :nf], grad[:nf])
        sens = -np.linalg.solve(H[:nf, :nf], H[:nf, nf:])
        scale = max(np.abs(H[nf:, nf:]).max(), 1e-300)                      # (frame 1 has the root's slot alone: C = 0)
        worst = max(worst, np.abs(f["S"] - S).max() / scale, np.abs(f["r"] - r).max() / max(np.abs(grad[nf:]).max(), 1e-300))
        assert np.abs(f["sens"][~pinned[n]] - sens).max() <= 1e-8 * max(np.abs(sens).max(), 1.0) and (f["sens"][pinned[n]] == 0).all()
        assert np.isclose(f["F"], o["F"][n], rtol=1e-12, atol=0)
    print(f"{name}: S_n, r_n against the dense Schur complement, relative {worst:.2e}")
    assert worst < 1e-9


def test_r_is_the_derivative_of_the_minimised_objective():
    """pt16, the frames the reference solver finishes: d/dtheta of min_x F_n(x; theta), by central differences through the
    CPU solver (h = 1e-4; the solver stops within 1e-10 F, hence the absolute term), against r_n at the minimiser."""
    base = np.full(5, 1.05)
    prob = lref.problem("pt16", scales=base)
    assert prob.K == 5
    x, status, _it, _cost = prob.solve()
    xs = np.where(np.isfinite(x), x, prob.x0)
    o = prob.objective(xs)
    sys_ = lref.system(prob, xs, prob.active_set(xs, o["g"], o["A"]), status)
    ok = status == 0
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
    print(f"pt16: r_n against the finite difference of min F, error / bound {worst:.2e} on {ok.sum()} frames")
    assert ok.sum() >= 15 and worst <= 1.0


def test_the_cpu_driver_recovers_the_scaled_truth_within_four_bars():
    """Seed link_scale_ref.SEED on pt16: what test_gpu_link_scale.py asks of the GPU driver holds for the reference alone."""
    sc = lref.scaled_inputs("pt16")
    out = lref.fitted("pt16")
    z = (out["scales"] - sc["factors"]) / out["std_scales"]
    print(f"seed {lref.SEED}: factors {np.round(sc['factors'], 3)}, scales {np.round(out['scales'], 3)}, std {np.round(out['std_scales'], 4)}, "
          f"z {np.round(z, 2)}, {len(out['history'])} outer steps, status {out['status']}")
    assert out["status"] == "ok" and out["observed"].all() and np.abs(z).max() < 4.0
    costs = [h["cost"] for h in out["history"]]
    assert all(b <= a for a, b in zip(costs, costs[1:]))
    assert np.abs(sc["factors"] - 1).max() > 0.05 and np.abs(out["scales"] - sc["factors"]).max() < 0.5 * np.abs(sc["factors"] - 1).max()


# ------------------------------------------------------------------------------------------------ scale_links
def _host_model(name="pt16", n=4):
    sk = pref.skeleton(name)
    lo, hi = build.bounds_table(sk, n)
    prog = build.skeleton.compile_skeleton(sk)
    Lp = len(prog["names"])
    return build.SkeletonModel(skel=sk, prog=prog, names=prog["names"], active=build.active_states(sk), lo=lo, hi=hi,
                               meas=np.zeros((n, 2, Lp, 2)), weights=np.zeros((n, 2, Lp)), h=1 / 120, model_weight=0.002, loss="l1")


def test_scale_links_group_rules():
    model = _host_model("pt16")
    before = [(op[:5], np.array(op[5])) for op in model.prog["ops"]]
    grp, K = build.link_groups(model.prog, "links")
    assert K == 5 and grp.tolist() == [0, 1, 2, 3, 4] and np.array_equal(grp, lref.groups_of(model.skel, "links")[0])
    s = np.array([1.1, 0.9, 1.0, 1.2, 0.8])
    out = build.scale_links(model, s)
    for (head, off), new, k in zip(before, out.prog["ops"], range(5)):
        assert new[:5] == head and np.array_equal(new[5], off * s[k])
    assert np.array_equal(out.link_scales, s) and np.array_equal(out.link_groups, grp) and out.names is model.names
    for (head, off), op in zip(before, model.prog["ops"]):                   # the input model is untouched
        assert op[:5] == head and np.array_equal(op[5], off)
    assert not hasattr(model, "link_scales")
    one = build.scale_links(model, [1.5], "global")
    assert all(np.array_equal(op[5], 1.5 * off) for op, (_h, off) in zip(one.prog["ops"], before))
    mixed = build.scale_links(model, [2.0, 3.0], [0, -1, 1, 1, -1])
    assert [float(op[5] @ off / (off @ off)) for op, (_h, off) in zip(mixed.prog["ops"], before)] == pytest.approx([2, 1, 3, 3, 1])
    assert build.link_groups(_host_model("p51").prog, np.arange(20) % 8)[1] == 8
    with pytest.raises(ValueError, match="explicit groups"):
        build.link_groups(_host_model("p51").prog, "links")                 # 20 links
    for bad in ("parts", [0, 1, 2], [0, 1, 2, 3, 16], [0, 0, 0, 0, -2], [-1] * 5, [0.0, 1.0, 2.0, 3.0, 4.0]):
        with pytest.raises(ValueError):
            build.link_groups(model.prog, bad)
    for bad in ([1.0] * 4, [1.0, 1.0, 1.0, 1.0, 0.0], [1.0, 1.0, 1.0, 1.0, np.nan], [1.0, -1.0, 1.0, 1.0, 1.0]):
        with pytest.raises(ValueError):
            build.scale_links(model, bad)
    # the compiled program of the scaled model is what the reference's scaled skeleton evaluates
    prob = lref.problem("pt16", scales=s)
    assert np.allclose(np.array([op[5] for op in out.prog["ops"]]), prob.offsets(), rtol=0, atol=1e-16)


def test_build_model_and_solve_video_take_link_scales(golden_dir):
    g, sk = cases.load(golden_dir)
    kw = dict(scene=(g["K"], g["D"], g["R"], g["t"]), dlc_tables=cases.tables(g["det"], g["parts"]), n_frames=int(g["n_frames"]),
              start_frame=int(g["start_frame"]), initial_line=False)
    plain, _ = build.build_model(sk, **kw)
    grp, K = build.link_groups(plain.prog, "links")
    s = 1.0 + 0.01 * np.arange(K)
    got, _ = build.build_model(sk, link_scales=("links", s), **kw)
    want = build.scale_links(plain, s)
    assert repr(got.prog["ops"]) == repr(want.prog["ops"]) and repr(got.prog["ops"]) != repr(plain.prog["ops"])
    assert np.array_equal(got.link_scales, s) and np.array_equal(got.link_groups, grp)
    same, _ = build.build_model(sk, link_scales=None, **kw)
    assert repr(same.prog["ops"]) == repr(plain.prog["ops"]) and not hasattr(same, "link_scales")
    for fn in (build.build_model, build.solve_video):
        assert inspect.signature(fn).parameters["link_scales"].default is None
    sig = inspect.signature(build.fit_link_scales)
    assert {k: v.default for k, v in sig.parameters.items() if k not in ("model", "fit_kw")} == dict(
        points=None, cov=None, groups="links", x0=None, scale_prior_sigma=None, max_outer=30, tol=1e-6, prior_sigma=1.0, max_iter=255)
    assert "skel_link_scale.hip" in _lib.SOURCES


# ------------------------------------------------------------------------------------------------ C ABI
def _skel_params_of(model):
    p = _lib.SkelFteParams()
    p.n_pose, p.n_ops = len(model.prog["names"]), len(model.prog["ops"])
    p.n_angles, p.n_active = model.prog["n_angles"], len(model.active)
    return p


def _call(lib, model=None, p=None, groups=(0, 1, 2, 3, 4), K=5, n_frames=10, prior_sigma=1.0, sigma_iso=0.01, ops=True, active=True,
          ws_bytes=None, **bufs):
    model = _host_model() if model is None else model
    p = _skel_params_of(model) if p is None else p
    b = dict(dict.fromkeys(("points", "x", "m", "pinned", "status", "S", "r", "F", "used", "fst", "ws"), 256), **bufs)
    ptr, null = (lambda v: C.c_void_p(v)), C.c_void_p(0)
    act = np.asarray(model.active, dtype=np.int32)
    act_c = (C.c_int32 * len(act))(*[int(a) for a in act])
    grp_c = None if groups is None else (C.c_int32 * len(groups))(*groups)
    nbytes = lib.acino_skel_link_scale_workspace_bytes(C.byref(p)) if ws_bytes is None else ws_bytes
    return lib.acino_skel_link_scale(C.byref(p), build._ops_array(model.prog) if ops else None, act_c if active else None, grp_c, K,
                                     prior_sigma, sigma_iso, ptr(b["points"]), null, ptr(b["x"]), ptr(b["m"]), ptr(b["pinned"]),
                                     ptr(b["status"]), n_frames, ptr(b["S"]), ptr(b["r"]), ptr(b["F"]), ptr(b["used"]), ptr(b["fst"]),
                                     null, null, ptr(b["ws"]), nbytes, null)


def test_abi_arguments_are_checked_before_any_device_call(lib):
    p0 = _skel_params_of(_host_model())
    assert lib.acino_skel_link_scale_workspace_bytes(C.byref(p0)) > 0 and lib.acino_skel_link_scale_workspace_bytes(None) == 0
    for kw, word in ((dict(K=0), b"n_groups"), (dict(K=17), b"n_groups"), (dict(groups=(0, 1, 2, 3, 5)), b"h_group"),
                     (dict(groups=(0, 1, -2, 3, 4)), b"h_group"), (dict(groups=(0, 1, 2, 3, 4), K=4), b"h_group"),
                     (dict(groups=None), b"null buffer"), (dict(ops=False), b"null buffer"), (dict(active=False), b"null buffer"),
                     (dict(n_frames=-1), b"n_frames"), (dict(prior_sigma=0.0), b"prior_sigma"), (dict(sigma_iso=np.nan), b"sigma_iso"),
                     *[(dict([(k, 0)]), b"null buffer") for k in ("points", "x", "m", "pinned", "status", "S", "r", "F", "used", "fst", "ws")]):
        assert _call(lib, **kw) == -1 and word in lib.acino_last_error_string(), kw
    assert _call(lib, groups=(0, -1, -1, 1, 1), K=2, n_frames=0) == 0
    assert _call(lib, ws=8) != 0 and b"aligned" in lib.acino_last_error_string()
    assert _call(lib, ws_bytes=16) != 0 and b"workspace too small" in lib.acino_last_error_string()
    bad = _skel_params_of(_host_model())
    bad.n_active = 65
    assert _call(lib, p=bad) == -1 and lib.acino_skel_link_scale_workspace_bytes(C.byref(bad)) == 0
    zeros = dict.fromkeys(("points", "x", "m", "pinned", "status", "S", "r", "F", "used", "fst", "ws"), 0)
    assert _call(lib, n_frames=0, **zeros) == 0                           # empty input is a no-op


def test_a_shape_beyond_the_lds_is_refused_with_the_pose_fits_error(lib):
    """64 states and 65 slots take 157 KB in the pose fit; the K columns of Js no longer fit beside them."""
    p = _lib.SkelFteParams()
    p.n_pose, p.n_ops, p.n_angles, p.n_active = 65, 64, 64, 64
    ops = (_lib.SkelOp * 64)()
    for k in range(64):
        ops[k].child, ops[k].parent, ops[k].angle, ops[k].flags = k + 1, k, k, 1 if k < 61 else 0
        ops[k].off[0] = 0.1
    act = (C.c_int32 * 64)(*([0, 1, 2] + [3 + k for k in range(61)]))
    grp = (C.c_int32 * 64)(*[k % 16 for k in range(64)])
    assert lib.acino_skel_link_scale_workspace_bytes(C.byref(p)) > 0
    a = C.c_void_p(256)
    rc = lib.acino_skel_link_scale(C.byref(p), ops, act, grp, 16, 1.0, 0.01, a, None, a, a, a, a, 10, a, a, a, a, a, None, None, a, 1 << 20, None)
    assert rc == -1 and b"160 KB" in lib.acino_last_error_string()
