"""Per-frame skeleton pose fit, host side (no GPU): the reference of tests/skel_pose_fit_ref.py against central differences of
the oracle's skeleton FK and against its own optimality conditions, the conditions tests/test_gpu_skel_pose_fit.py relies on
evaluated by the reference alone, and the argument handling of the C ABI and of the Python entries before any device work.

The reference on the named inputs (prior_sigma 1.0, max_iter 255; 23 of 24 frames with a point, frame 3 status 2): status 0 on
20 (shipped), 22 (generic, pt16, p51) and 21 (pt32) frames; 13 to 19 distinct trial counts, 7 to 255 trials; largest delta on
status-0 frames 4.0e-05 (pt16) to 1.3e-03 (p51); cond(A_free) at most 5.1e+05; 4 to 6 pinned entries; the fitted entering
slots a median 15 to 18 mm from the truth against 100 to 224 mm at the start."""
import ctypes as C
import inspect

import numpy as np
import pytest

import __graft_entry__ as ge
import skel_pose_fit_ref as ref
from acinoset_amd import _lib, build, fte


@pytest.fixture(scope="module")
def lib():
    ge.build()
    return _lib.lib()


# ------------------------------------------------------------------------------------------------ reference self-checks
@pytest.mark.parametrize("name", ("shipped", "pt16"))
def test_gradient_and_matrix_match_central_differences_of_the_oracle_fk(name):
    """G by central differences of oracle.skel_fte.skeleton_fk_jac's positions (h = 1e-6: truncation ~1e-12, rounding ~1e-10),
    then g = G^T W r + ridge and A = G^T W G + ridge from it, at a point off the start (so that the ridge term is not zero)."""
    prob = ref.problem(name)
    rng = np.random.default_rng(5)
    x = np.clip(prob.x0 + rng.normal(0.0, 0.1, prob.x0.shape), prob.lo, prob.hi)
    o = prob.objective(x)
    h = 1e-6
    Jfd = np.zeros_like(o["J"])
    for p in range(prob.P):
        e = np.zeros(prob.P)
        e[p] = h
        Jfd[..., p] = (prob.fk(x + e) - prob.fk(x - e)) / (2 * h)
    r = np.where(prob.enter[..., None], o["pos"] - prob.y0, 0.0)
    g = np.einsum("nlip,nlij,nlj->np", Jfd, prob.W, r)
    g[:, 3:] += prob.kappa * (x - prob.m)[:, 3:]
    A = np.einsum("nlip,nlij,nljq->npq", Jfd, prob.W, Jfd)
    A[:, np.arange(3, prob.P), np.arange(3, prob.P)] += prob.kappa
    eg, eA = np.abs(o["g"] - g).max() / np.abs(g).max(), np.abs(o["A"] - A).max() / np.abs(A).max()
    print(f"{name}: g {eg:.2e}  A {eA:.2e} (relative to the largest entry)")
    assert eg < 1e-7 and eA < 1e-7
    # and F is the function g differentiates: a central difference of F along a random direction
    d = rng.normal(0.0, 1.0, x.shape)
    d[(x <= prob.lo) | (x >= prob.hi)] = 0.0
    dF = (prob.objective(x + h * d, need_jac=False)["F"] - prob.objective(x - h * d, need_jac=False)["F"]) / (2 * h)
    assert np.allclose(dF, (o["g"] * d).sum(1), rtol=1e-6, atol=1e-6 * np.abs(dF).max())


@pytest.mark.parametrize("name", ref.NAMES)
def test_reference_end_points_satisfy_the_kkt_conditions(name):
    """At the reference's status-0 points: inside the box; a pinned state sits on its bound with the gradient pushing outward;
    and on the free states what a Newton step could still gain, delta^2 / 2, is below 1e-6 of a cost of order one or more (the
    solver stops on a decrease of 1e-10 F)."""
    r = ref.solved(name)
    prob, ok = r["prob"], r["status"] == 0
    x, g, pin = r["x"][ok], r["obj"]["g"][ok], r["pinned"][ok]
    lo, hi = prob.lo[ok], prob.hi[ok]
    assert ((x >= lo) & (x <= hi)).all()
    assert (((x == lo) & (g > 0)) | ((x == hi) & (g < 0)))[pin].all()
    print(f"{name}: delta max {r['delta'][ok].max():.2e}, cost median {np.median(r['cost'][ok]):.2f}")
    assert (r["delta"][ok] ** 2 / 2 <= 1e-6 * np.maximum(r["cost"][ok], 1.0)).all()
    assert (r["cost"][ok] <= prob.objective(prob.x0, need_jac=False)["F"][ok]).all()


# ------------------------------------------------------------------------------------------------ input conditions
@pytest.mark.parametrize("name", ref.NAMES)
def test_inputs_meet_the_conditions_of_the_gpu_tests(name):
    r, inp = ref.solved(name), ref.inputs(name)
    prob, st = r["prob"], r["status"]
    has = prob.n_markers >= 1
    L = prob.L
    assert prob.N == ref.N_FRAMES == 24 and (prob.P + 15) // 16 * 16 == ref.PT[name]
    assert prob.n_markers[:4].tolist() == [L, 1, 3, 0] and prob.enter[1, 0] and prob.enter[2, L // 2:L // 2 + 3].all()
    assert np.array_equal(prob.enter, np.isfinite(inp["points"]).all(-1))
    conds = [np.linalg.cond(r["obj"]["A"][n][np.ix_(~r["pinned"][n], ~r["pinned"][n])]) for n in np.nonzero(st < 2)[0]]
    trials = set(r["iters"][has].tolist())
    print(f"{name}: {has.sum()} of {len(st)} frames with a point, status 0 on {(st == 0).sum()}, 1 on {(st == 1).sum()}, 2 on "
          f"{(st == 2).sum()}, 3 on {(st == 3).sum()}; {len(trials)} distinct trial counts {min(trials)}..{max(trials)}; delta max "
          f"{np.nanmax(r['delta'][st == 0]):.2e}; cond(A_free) max {max(conds):.2e}; {r['pinned'].sum()} pinned entries")
    assert np.array_equal(np.nonzero(st == 2)[0], [3]) and (st == 3).sum() == 0
    assert (st == 0).sum() >= 0.8 * has.sum()
    assert len(trials) >= 4
    assert r["pinned"].sum() >= 1
    assert max(conds) <= 1e7
    assert np.array_equal(np.isnan(r["x"]).all(1), st >= 2) and np.array_equal(np.isnan(r["x"]).any(1), st >= 2)
    # the fit is worth something: the fitted entering slots are nearer to the truth than the start's
    back = (st < 2)[:, None] & prob.enter
    err = np.linalg.norm(r["obj"]["pos"] - inp["truth_pos"], axis=-1)[back]
    err0 = np.linalg.norm(prob.fk(prob.x0) - inp["truth_pos"], axis=-1)[back]
    print(f"{name}: entering slots from the truth, median: fitted {1e3 * np.median(err):.1f} mm, start {1e3 * np.median(err0):.1f} mm")
    assert np.median(err) < 0.5 * np.median(err0)


def test_frame_one_ends_by_lam_overflow_because_its_point_is_met_exactly():
    r = ref.solved("generic")
    assert r["status"][1] == 1 and r["iters"][1] < 255 and r["cost"][1] < 1e-20


def test_the_states_that_move_no_pose_rest_at_the_ridge_with_its_variance():
    """The shipped skeleton's psi angles of "chin" and "hip2": zero columns of G at every x, so the ridge alone holds them -
    x_p = m_p and cov_x[p, p] = prior_sigma^2, to 1e-12 relative."""
    r = ref.solved("shipped")
    prob = r["prob"]
    dead = np.nonzero(np.abs(r["obj"]["J"]).max(axis=(0, 1, 2)) == 0.0)[0]
    assert prob.ACT[dead].tolist() == [33, 43]               # (full-state indices: what model_observability reports)
    back = r["status"] < 2
    assert np.array_equal(r["x"][back][:, dead], prob.m[back][:, dead])
    for n in np.nonzero(back)[0]:
        free = ~r["pinned"][n]
        assert free[dead].all()
        cov = np.zeros((prob.P, prob.P))
        cov[np.ix_(free, free)] = np.linalg.inv(r["obj"]["A"][n][np.ix_(free, free)])
        assert np.abs(cov[dead, dead] - prob.opt["prior_sigma"] ** 2).max() <= 1e-12 * prob.opt["prior_sigma"] ** 2
    assert np.abs(ref.solved("generic")["obj"]["J"]).max(axis=(0, 1, 2)).min() > 0.0      # (the generic skeleton has none)


def test_default_start_is_the_mean_offset_from_the_rest_pose():
    prob = ref.problem("pt16")
    rest = prob.fk(np.zeros((1, prob.P)))[0]
    n = 5
    want = np.mean([prob.y0[n, l] - rest[l] for l in np.nonzero(prob.enter[n])[0]], axis=0)
    assert np.allclose(prob.default_start()[n, :3], want, rtol=0, atol=1e-14) and (prob.default_start()[:, 3:] == 0).all()
    assert (prob.x0[3] == np.clip(np.zeros(prob.P), prob.lo[3], prob.hi[3])).all()
    assert ((prob.x0 >= prob.lo) & (prob.x0 <= prob.hi)).all()


# ------------------------------------------------------------------------------------------------ the fill rule is shared
def test_the_fill_rule_is_the_cheetahs_with_the_skeletons_psi_columns():
    N = 7
    x = np.full((N, 6), np.nan)
    fitted = np.array([0, 1, 1, 0, 1, 0, 0], dtype=bool)
    rows = np.nonzero(fitted)[0]
    x[rows] = rows[:, None] * 0.1
    x[rows, 4] = x[rows, 2] = [3.1, -3.1, -3.0]
    got = fte.fill_unfitted_frames(x, fitted, psi_columns=[4])
    assert np.isfinite(got).all() and np.array_equal(got[0], got[1]) and np.array_equal(got[6], got[4])
    assert np.allclose(got[rows, 4], [3.1, -3.1 + 2 * np.pi, -3.0 + 2 * np.pi]) and np.array_equal(got[rows, 2], x[rows, 2])
    assert np.allclose(got[3, 4], 0.5 * (got[2, 4] + got[4, 4])) and np.allclose(got[3, 2], 0.5 * (-3.1 - 3.0))
    plain = fte.fill_unfitted_frames(np.pad(x, ((0, 0), (0, 19)), constant_values=1.0), fitted)      # (the default: the cheetah's columns)
    assert np.allclose(plain[3, 4], 0.5 * (-3.1 - 3.0))


# ------------------------------------------------------------------------------------------------ C ABI
def _params(n_pose=6, n_ops=5, n_angles=6, n_active=15):
    p = _lib.SkelFteParams()
    p.n_pose, p.n_ops, p.n_angles, p.n_active = n_pose, n_ops, n_angles, n_active
    return p


def _call(lib, prm, p=None, n_frames=10, ops=True, active=True, points=256, lo=256, hi=256, x=256, status=256, ws=256, ws_bytes=None):
    model = _pt16_model()
    p = _skel_params_of(model) if p is None else p
    null, ptr = C.c_void_p(0), lambda v: C.c_void_p(v)
    act = np.asarray(model.active, dtype=np.int32)
    act_c = (C.c_int32 * len(act))(*[int(a) for a in act])
    nbytes = lib.acino_skel_pose_fit_workspace_bytes(C.byref(p)) if ws_bytes is None else ws_bytes
    return lib.acino_skel_pose_fit(C.byref(prm), C.byref(p), build._ops_array(model.prog) if ops else None, act_c if active else None,
                                   ptr(points), null, null, ptr(lo), ptr(hi), n_frames, ptr(x), null, null, ptr(status), null, null,
                                   null, null, null, null, ptr(ws), nbytes, null)


def _pt16_model():
    return build.SkeletonModel(prog=build.skeleton.compile_skeleton(ref.skeleton("pt16")), active=build.active_states(ref.skeleton("pt16")))


def _skel_params_of(model):
    p = _lib.SkelFteParams()
    p.n_pose, p.n_ops = len(model.prog["names"]), len(model.prog["ops"])
    p.n_angles, p.n_active = model.prog["n_angles"], len(model.active)
    return p


def test_abi_arguments_are_checked_before_any_device_call(lib):
    good = lambda **kw: _lib.PoseFitParams(**dict(dict(max_iter=100, min_markers=1, lam0=1e-3, ftol=1e-10, xtol=1e-10,
                                                       prior_sigma=np.pi, sigma_iso=0.01), **kw))
    p0 = _skel_params_of(_pt16_model())
    assert (p0.n_pose, p0.n_active) == (6, 15)
    assert lib.acino_skel_pose_fit_workspace_bytes(C.byref(p0)) > 0 and lib.acino_skel_pose_fit_workspace_bytes(None) == 0
    for kw, shape, word in ((dict(max_iter=0), dict(), b"max_iter"), (dict(max_iter=256), dict(), b"max_iter"),
                            (dict(min_markers=0), dict(), b"min_markers"), (dict(min_markers=7), dict(), b"min_markers"),
                            (dict(lam0=0.0), dict(), b"lam0"), (dict(ftol=0.0), dict(), b"ftol"), (dict(xtol=-1.0), dict(), b"xtol"),
                            (dict(prior_sigma=0.0), dict(), b"prior_sigma"), (dict(sigma_iso=np.nan), dict(), b"sigma_iso"),
                            (dict(), dict(n_frames=-1), b"n_frames"), (dict(), dict(points=0), b"null buffer"),
                            (dict(), dict(lo=0), b"null buffer"), (dict(), dict(x=0), b"null buffer"),
                            (dict(), dict(status=0), b"null buffer"), (dict(), dict(ws=0), b"null buffer"),
                            (dict(), dict(ops=False), b"null buffer"), (dict(), dict(active=False), b"null buffer")):
        assert _call(lib, good(**kw), **shape) == -1 and word in lib.acino_last_error_string(), (kw, shape)
    assert _call(lib, good(), ws=8) != 0 and b"aligned" in lib.acino_last_error_string()
    assert _call(lib, good(), ws_bytes=16) != 0 and b"workspace too small" in lib.acino_last_error_string()
    bad = _skel_params_of(_pt16_model())
    bad.n_active = 65
    assert _call(lib, good(), p=bad) == -1 and lib.acino_skel_pose_fit_workspace_bytes(C.byref(bad)) == 0
    assert _call(lib, good(), n_frames=0, points=0, lo=0, hi=0, x=0, status=0, ws=0) == 0      # empty input is a no-op
    # only n_pose, n_ops, n_angles and n_active of the params block are read: the other fields may hold anything
    junk = _skel_params_of(_pt16_model())
    junk.n_frames, junk.n_cams, junk.h, junk.loss, junk.lam0 = -5, 99, -1.0, 7, -1.0
    assert _call(lib, good(), p=junk, n_frames=0) == 0


# ------------------------------------------------------------------------------------------------ Python entries
class Reached(Exception):
    pass


@pytest.fixture
def no_device(monkeypatch):
    def require_gpu():
        raise Reached()
    monkeypatch.setattr(_lib, "require_gpu", require_gpu)


def _host_model(name="pt16", n=4):
    sk = ref.skeleton(name)
    lo, hi = build.bounds_table(sk, n)
    prog = build.skeleton.compile_skeleton(sk)
    Lp = len(prog["names"])
    return build.SkeletonModel(skel=sk, prog=prog, names=prog["names"], active=build.active_states(sk), lo=lo, hi=hi,
                               meas=np.zeros((n, 2, Lp, 2)), weights=np.zeros((n, 2, Lp)), K=np.tile(np.eye(3), (2, 1, 1)),
                               D=np.zeros((2, 4)), R=np.tile(np.eye(3), (2, 1, 1)), t=np.zeros((2, 3, 1)), h=1 / 120,
                               model_weight=0.002, camera_model="fisheye", loss="l1", init_x=np.zeros((n, 3 + 3 * prog["n_angles"])))


def test_python_argument_errors_come_before_any_device_work(no_device):
    sig = inspect.signature(build.pose_fit)
    want = dict(cov=None, x0=None, prior_sigma=np.pi, sigma_iso=0.01, min_markers=1, max_iter=100, ftol=1e-10, xtol=1e-10,
                lam0=1e-3, return_cov=True)
    assert {k: v.default for k, v in sig.parameters.items() if k not in ("model", "points")} == want
    assert {k: v.default for k, v in inspect.signature(fte.pose_fit).parameters.items() if k != "points"} == want
    model = _host_model()
    assert np.array_equal(model.active, ref.problem("pt16").ACT) and len(model.names) == 6
    pts, cov = np.zeros((4, 6, 3)), np.tile(np.eye(3), (4, 6, 1, 1))
    with pytest.raises(Reached):
        build.pose_fit(model, pts, cov)
    with pytest.raises(Reached):
        build.pose_fit(model, dict(points=pts, cov=cov, status=None))
    for kw in (dict(prior_sigma=0.0), dict(sigma_iso=np.nan), dict(ftol=0.0), dict(xtol=-1.0), dict(lam0=0.0), dict(max_iter=0),
               dict(max_iter=256), dict(max_iter=2.5), dict(min_markers=0), dict(min_markers=7), dict(x0=np.zeros((4, 21))),
               dict(cov=cov[:3]), dict(cov=cov[..., 0])):
        with pytest.raises(ValueError):
            build.pose_fit(model, pts, **kw)
    with pytest.raises(ValueError):
        build.pose_fit(model, np.zeros((4, 5, 3)))
    with pytest.raises(ValueError):
        build.pose_fit(model, np.zeros((5, 6, 3)))            # (points must have model.N frames)
    with pytest.raises(ValueError):
        build.pose_fit(model, dict(points=pts, cov=cov), cov=cov)
    with pytest.raises(ValueError, match="sigma_px"):
        build.model_triangulation(model)                      # (no positive weight: the default sigma_px has no source)


def test_an_unknown_init_is_refused_and_line_stays_the_default(no_device):
    model = _host_model()
    for fn in (build.solve_models, build.solve_model, build.solve_video):
        assert inspect.signature(fn).parameters["init"].default == "line"
    with pytest.raises(ValueError, match="'line' or 'pose_fit'"):
        build.solve_models([model], init="bogus")
    with pytest.raises(ValueError, match="'line' or 'pose_fit'"):
        build.solve_model(model, init="triangulation")
    with pytest.raises(ValueError, match="'line' or 'pose_fit'"):
        build.solve_video(model.skel, scene=(model.K, model.D, model.R, model.t), dlc_tables=[], init="bogus")
    with pytest.raises(Reached):
        build.solve_models([model])
    assert "skel_pose_fit.hip" in _lib.SOURCES and "pose_fit_dev.hpp" in _lib.HEADERS
