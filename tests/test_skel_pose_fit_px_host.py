"""Per-frame skeleton pose fit from the detections, host side (no GPU): the reference of tests/skel_pose_fit_px_ref.py against
central differences of its own F and against the assembled Jacobian, its optimality conditions, the conditions
tests/test_gpu_skel_pose_fit_px.py relies on evaluated by the reference alone, its sensitivity to the camera records, the
rig-translation identity, and the argument handling of the C ABI and of the Python entry before any device work."""
import ctypes as C
import inspect

import numpy as np
import pytest

import __graft_entry__ as ge
import skel_pose_fit_px_ref as ref
import unlike_rig as ur
from acinoset_amd import _lib, build


@pytest.fixture(scope="module")
def lib():
    ge.build()
    return _lib.lib()


# ------------------------------------------------------------------------------------------------ reference self-checks
@pytest.mark.parametrize("name", ("generic-pushed", "shipped-pinhole-pushed", "pt16-two", "generic-mono"))
def test_gradient_and_matrix_match_central_differences(name):
    """g against central differences of F state by state (h = 1e-6), at a point off the start so that the ridge term is not zero;
    A = sum w J^T J / sigma^2 + ridge against the Jacobian of the residuals assembled by central differences of the pixels."""
    prob = ref.problem(name)
    P = prob.P
    rng = np.random.default_rng(5)
    x = np.clip(prob.x0 + rng.normal(0.0, 0.02, prob.x0.shape), prob.lo, prob.hi)
    o = prob.objective(x)
    assert np.isfinite(o["F"]).all()
    h = 1e-6
    gfd, Jfd = np.zeros_like(o["g"]), np.zeros_like(o["Jpx"])
    for p in range(P):
        e = np.zeros(P)
        e[p] = h
        up, dn = prob.objective(x + e), prob.objective(x - e)
        gfd[:, p] = (up["F"] - dn["F"]) / (2 * h)
        Jfd[..., p] = (up["r"] - dn["r"]) / (2 * h)
    A = np.einsum("nclkp,nclk,nclkq->npq", Jfd, o["w"], Jfd) / prob.sigma_px ** 2
    A[:, np.arange(3, P), np.arange(3, P)] += prob.kappa
    eg, eA = np.abs(o["g"] - gfd).max() / np.abs(gfd).max(), np.abs(o["A"] - A).max() / np.abs(A).max()
    print(f"{name}: g {eg:.2e}  A {eA:.2e} (relative to the largest entry)")
    assert eg < 1e-6 and eA < 1e-6
    assert (o["w"][~prob.valid] == 0.0).all() and (o["Jpx"][~prob.valid] == 0.0).all()
    w = 1.0 / (1.0 + (o["r"] / prob.fs) ** 2)
    assert np.allclose(o["w"][prob.valid], w[prob.valid], rtol=1e-14, atol=0.0)


def test_a_slot_behind_its_camera_makes_the_cost_infinite():
    prob = ref.problem("generic-mono")
    R, t = prob.rig[2][0], np.asarray(prob.rig[3][0], dtype=np.float64).reshape(3)
    x = prob.x0.copy()
    x[:, :3] = -R.T @ t - 5.0 * R[2]                        # the root five metres behind the camera centre
    F = prob.objective(x, need_jac=False)["F"]
    assert np.isinf(F).all() and (F > 0).all()
    inp = ref.inputs("generic-mono")
    blind = ref.Problem(inp["skel"], np.zeros((3, 1, prob.L, 3)), prob.rig, "fisheye", inp["lo"][:3], inp["hi"][:3], x[:3], **ref.OPTS)
    assert np.isfinite(blind.objective(x[:3], need_jac=False)["F"]).all()          # no valid detection: nothing is behind
    assert (blind.solve()[1] == 2).all()


@pytest.mark.parametrize("name", ref.NAMES)
def test_reference_end_points_satisfy_the_kkt_conditions(name):
    """First-order optimality on the free states at the reference's solution: inside the box; a pinned state sits on its bound
    with the gradient pushing outward; what a Newton step could still gain, delta^2 / 2, is below 1e-5 of a cost of order one or
    more (the solver stops on a decrease of 1e-10 F or a step of 1e-10)."""
    r = ref.solved(name)
    prob, ok = r["prob"], r["status"] == 0
    x, g, pin = r["x"][ok], r["obj"]["g"][ok], r["pinned"][ok]
    lo, hi = prob.lo[ok], prob.hi[ok]
    assert ((x >= lo) & (x <= hi)).all()
    assert (((x == lo) & (g > 0)) | ((x == hi) & (g < 0)))[pin].all()
    print(f"{name}: delta max {r['delta'][ok].max():.2e}, cost median {np.median(r['cost'][ok]):.2f}")
    assert (r["delta"][ok] ** 2 / 2 <= 1e-5 * np.maximum(r["cost"][ok], 1.0)).all()
    assert (r["cost"][ok] <= prob.objective(prob.x0, need_jac=False)["F"][ok]).all()


# ------------------------------------------------------------------------------------------------ input conditions
# name: (frames, frames with a detection, cameras, n_active, n_pose)
SHAPES = {"generic-fisheye": (24, 24, 6, 36, 15), "generic-pushed": (24, 23, 6, 36, 15), "shipped-pinhole-pushed": (24, 23, 6, 36, 15),
          "pt16-two": (24, 24, 2, 15, 6), "pt32-three": (24, 24, 3, 24, 9), "p51-wide16": (14, 14, 16, 51, 20),
          "generic-mono": (24, 24, 1, 36, 15), "generic-mono-pushed": (24, 23, 1, 36, 15)}


@pytest.mark.parametrize("name", ref.NAMES)
def test_inputs_meet_the_conditions_of_the_gpu_tests(name):
    """Every slot of every frame at least 0.5 m in front of every camera (at the truth, at the start and at the reference's end
    point); status 0 on every frame that has a detection and status 2 exactly on the others; 6 to 65 trials; the largest delta
    between 4e-6 and 4.2e-4 (shipped-pinhole-pushed: 4.2e-4, every other input below 3.1e-5); cond(A_free) at most 5.6e5: the
    GPU test's caps (0.9 of the frames, B = 10 delta, 1e-12 cond) rest on these."""
    r, inp = ref.solved(name), ref.inputs(name)
    prob, st = r["prob"], r["status"]
    has = prob.n_markers >= 1
    ok = st == 0
    conds = [np.linalg.cond(r["obj"]["A"][n][np.ix_(~r["pinned"][n], ~r["pinned"][n])]) for n in np.nonzero(ok)[0]]
    depth = min(prob.objective(p, need_jac=False)["zc"].min() for p in (inp["truth"], prob.x0, np.where(ok[:, None], r["x"], prob.x0)))
    print(f"{name}: {prob.C} cameras, {has.sum()} of {len(st)} frames with a detection, status 0 on {ok.sum()}; trials "
          f"{r['iters'][has].min()}..{r['iters'].max()}; delta max {r['delta'][ok].max():.2e}; cond(A_free) max {max(conds):.2e}; "
          f"least depth {depth:.2f} m")
    assert (prob.N, has.sum(), prob.C, prob.P, prob.L) == SHAPES[name] and ref.PT[name] == (prob.P + 15) // 16 * 16
    assert depth >= 0.5
    assert np.array_equal(st == 2, ~has) and np.array_equal(ok, has)
    assert r["iters"][has].min() >= 6 and r["iters"].max() <= 65
    assert 4e-6 <= r["delta"][ok].max() <= 4.2e-4 and max(conds) <= 5.6e5
    assert np.array_equal(np.isnan(r["x"]).all(1), st >= 2) and np.array_equal(np.isnan(r["x"]).any(1), st >= 2)


def test_inputs_hold_the_cases_the_gpu_tests_name():
    """Both camera models; every PT; a frame with no detection in every pushed input; pushed detections that end with w < 0.1
    (61 of 3 288 coordinates on generic-pushed and on shipped-pinhole-pushed, 1 of 546 on generic-mono-pushed); states pinned
    on a bound on pt32-three alone (11); two states of the shipped skeleton that move no pose; on pt16-two camera 1 blind in a
    third of the frames, where no slot has two views."""
    assert ref.inputs("shipped-pinhole-pushed")["model"] == "pinhole" and ref.inputs("generic-fisheye")["model"] == "fisheye"
    assert sorted(set(ref.PT.values())) == [16, 32, 48, 64]
    low = {}
    for name in ref.NAMES:
        r = ref.solved(name)
        ok = r["status"] == 0
        assert (r["status"] == 2).sum() == (1 if ref.inputs(name)["pushed"] else 0), name
        valid = r["prob"].valid[ok][..., None]
        low[name] = (int(((r["obj"]["w"][ok] < 0.1) & valid).sum()), int(2 * valid.sum()))
        assert int(r["pinned"][ok].sum()) == (11 if name == "pt32-three" else 0), name
    print(low)
    assert low["generic-pushed"] == (61, 3288) and low["shipped-pinhole-pushed"] == (61, 3288) and low["generic-mono-pushed"] == (1, 546)
    assert all(low[name][0] == 0 for name in ref.NAMES if not ref.inputs(name)["pushed"])
    G = ref.solved("shipped-pinhole-pushed")["obj"]["J"]
    assert (np.abs(G).max((0, 1, 2)) == 0.0).sum() == 2
    two = ref.solved("pt16-two")["prob"]
    blind = ~two.valid[:, 1].any(1)
    assert blind.sum() == 8 and np.array_equal(np.nonzero(blind)[0], np.arange(0, 24, 3)) and (two.n_markers[blind] >= 2).all()
    mono = ref.solved("generic-mono")["prob"]
    assert mono.C == 1 and (mono.n_markers >= 2).all()
    inp = ref.inputs("generic-fisheye")
    assert np.abs(inp["x0"] - inp["truth"]).max() == pytest.approx(0.05)


# ------------------------------------------------------------------------------------------------ sensitivity, invariance
MUTANT_FRAMES = 5          # (none of them the frame without a detection: that is frame 5)


@pytest.mark.parametrize("name,mutant", [("generic-fisheye", "rolled"), ("generic-fisheye", "no_skew"),
                                         ("shipped-pinhole-pushed", "rolled"), ("p51-wide16", "rolled"), ("pt32-three", "rolled"),
                                         ("pt16-two", "rolled")])
def test_a_wrong_camera_record_moves_the_solution_beyond_the_bound(name, mutant):
    """On the first frames of an input (a frame is a problem of its own): with a mutant of the rig the reference's minimiser
    leaves the neighbourhood the GPU test allows (A-norm distance 2 B to the reference's x, delta at most B at the right rig):
    a kernel that reads a camera record wrongly cannot pass."""
    right, B = ref.solved(name), ref.bound(name)
    n = MUTANT_FRAMES
    wrong_x, wrong_status = ref.problem(name, mutant, n).solve()[:2]
    both = (right["status"][:n] == 0) & (wrong_status < 2)
    dx = (wrong_x - right["x"][:n])[both]
    dist = np.sqrt(np.einsum("ni,nij,nj->n", dx, right["obj"]["A"][:n][both], dx))
    at = np.full_like(right["x"], np.nan)
    at[:n][both] = wrong_x[both]
    delta = right["prob"].delta(at)[:n][both]
    print(f"{name} / {mutant}: distance min {dist.min():.2e}, delta at the right rig min {delta.min():.2e} (B {B:.2e})")
    assert both.sum() >= 0.9 * n
    assert (dist > 2 * B).all() and (delta > B).all()


def _free_inverse(A, fixed):
    out = np.zeros_like(A)
    for n in range(len(A)):
        free = ~fixed[n]
        out[n][np.ix_(free, free)] = np.linalg.inv(A[n][np.ix_(free, free)])
    return out


def test_translating_the_rig_translates_the_root():
    """t_c -> t_c - R_c d with the start's root and the root's box + d, for the three translations of the GPU test: the root
    moves by d and nothing else to 1e-12, in the same number of trials - and inv(A_free) at the end points, which has cond(A_free)
    = 1.5e5 between the rounding of the translation and itself, stays within 0.5e-11 (measured 2.4e-12): the GPU test holds cov_x
    to 1e-11 under the same translations, which needs the problem itself to be that stable."""
    inp = ref.inputs("generic-fisheye")
    K, D, R, t = inp["rig"]
    base = ref.solved("generic-fisheye")
    cov = _free_inverse(base["obj"]["A"], base["pinned"])
    for d in (np.array([1.0, 0.0, 0.0]), np.array([0.0, -2.0, 0.5]), np.array([0.3, -0.5, 0.8])):
        td = (np.asarray(t, dtype=np.float64).reshape(len(K), 3) - np.einsum("cij,j->ci", R, d)).reshape(np.shape(t))
        x0, lo, hi = inp["x0"].copy(), inp["lo"].copy(), inp["hi"].copy()
        for a in (x0, lo, hi):                                  # (the root's box moves with the rig)
            a[:, :3] += d
        r = ref.common.solved(ref.Problem(inp["skel"], inp["det"], (K, D, R, td), inp["model"], lo, hi, x0, **ref.OPTS))
        x = r["x"]
        root, rest = np.abs(x[:, :3] - d - base["x"][:, :3]).max(), np.abs(x[:, 3:] - base["x"][:, 3:]).max()
        dcov = np.abs(_free_inverse(r["obj"]["A"], r["pinned"]) - cov).max()
        print(f"d = {d}: root {root:.1e}, angles {rest:.1e}, inv(A_free) {dcov:.1e}")
        assert root <= 1e-12 and rest <= 1e-12 and dcov <= 0.5e-11
        assert np.array_equal(r["status"], base["status"]) and np.array_equal(r["iters"], base["iters"])


# ------------------------------------------------------------------------------------------------ C ABI
def _skel_params_of(model):
    p = _lib.SkelFteParams()
    p.n_pose, p.n_ops = len(model.prog["names"]), len(model.prog["ops"])
    p.n_angles, p.n_active = model.prog["n_angles"], len(model.active)
    return p


def _pt16_model():
    sk = ref.sref.skeleton("pt16")
    return build.SkeletonModel(prog=build.skeleton.compile_skeleton(sk), active=build.active_states(sk))


def _call(lib, prm, p=None, n_frames=10, n_cams=2, det=256, cams=256, x0=256, lo=256, hi=256, x=256, status=256, ws=256, ws_bytes=None,
          ops=True, active=True):
    model = _pt16_model()
    p = _skel_params_of(model) if p is None else p
    null, ptr = C.c_void_p(0), lambda v: C.c_void_p(v)
    act = np.asarray(model.active, dtype=np.int32)
    act_c = (C.c_int32 * len(act))(*[int(a) for a in act])
    nbytes = lib.acino_skel_pose_fit_px_workspace_bytes(C.byref(p)) if ws_bytes is None else ws_bytes
    return lib.acino_skel_pose_fit_px(C.byref(prm) if prm is not None else None, C.byref(p), build._ops_array(model.prog) if ops else None,
                                      act_c if active else None, ptr(det), n_frames, n_cams, ptr(cams), ptr(x0), ptr(lo), ptr(hi),
                                      ptr(x), null, null, ptr(status), null, null, null, null, null, null, null, ptr(ws), nbytes, null)


def test_abi_arguments_are_checked_before_any_device_call(lib):
    """Every check of acino_cheetah_pose_fit_px and of acino_skel_pose_fit, with min_detections in 1 .. n_pose n_cams; every
    pointer handed over is a small integer no device call could take."""
    good = lambda **kw: _lib.PoseFitPxParams(**dict(dict(camera_model=0, max_iter=100, min_detections=2, reserved=0, lam0=1e-3,
                                                         ftol=1e-10, xtol=1e-10, prior_sigma=np.pi, thresh=0.5, f_scale=5.0,
                                                         sigma_px=5.0), **kw))
    p0 = _skel_params_of(_pt16_model())
    assert (p0.n_pose, p0.n_active) == (6, 15) and C.sizeof(_lib.PoseFitPxParams) == 72
    assert lib.acino_skel_pose_fit_px_workspace_bytes(C.byref(p0)) > 0 and lib.acino_skel_pose_fit_px_workspace_bytes(None) == 0
    for kw, shape, word in ((dict(max_iter=0), dict(), b"max_iter"), (dict(max_iter=256), dict(), b"max_iter"),
                            (dict(camera_model=2), dict(), b"camera_model"), (dict(camera_model=-1), dict(), b"camera_model"),
                            (dict(min_detections=0), dict(), b"min_detections"), (dict(min_detections=13), dict(), b"min_detections"),
                            (dict(min_detections=7), dict(n_cams=1), b"min_detections"),
                            (dict(lam0=0.0), dict(), b"lam0"), (dict(ftol=0.0), dict(), b"ftol"), (dict(xtol=-1.0), dict(), b"xtol"),
                            (dict(prior_sigma=0.0), dict(), b"prior_sigma"), (dict(thresh=np.nan), dict(), b"thresh"),
                            (dict(f_scale=0.0), dict(), b"f_scale"), (dict(f_scale=np.inf), dict(), b"f_scale"),
                            (dict(sigma_px=-5.0), dict(), b"sigma_px"), (dict(sigma_px=np.nan), dict(), b"sigma_px"),
                            (dict(), dict(n_frames=-1), b"n_frames"), (dict(), dict(n_cams=0), b"n_cams"),
                            (dict(), dict(n_cams=17), b"n_cams"), (dict(), dict(det=0), b"null buffer"),
                            (dict(), dict(cams=0), b"null buffer"), (dict(), dict(x0=0), b"null buffer"),
                            (dict(), dict(lo=0), b"null buffer"), (dict(), dict(hi=0), b"null buffer"),
                            (dict(), dict(x=0), b"null buffer"), (dict(), dict(status=0), b"null buffer"),
                            (dict(), dict(ws=0), b"null buffer"), (dict(), dict(ops=False), b"null buffer"),
                            (dict(), dict(active=False), b"null buffer")):
        assert _call(lib, good(**kw), **shape) == -1 and word in lib.acino_last_error_string(), (kw, shape)
    assert _call(lib, good(min_detections=12), ws=8) != 0 and b"aligned" in lib.acino_last_error_string()
    assert _call(lib, good(), ws_bytes=16) != 0 and b"workspace too small" in lib.acino_last_error_string()
    bad = _skel_params_of(_pt16_model())
    bad.n_active = 65
    assert _call(lib, good(), p=bad) == -1 and lib.acino_skel_pose_fit_px_workspace_bytes(C.byref(bad)) == 0
    assert _call(lib, None) == -1
    assert _call(lib, good(), n_frames=0, det=0, cams=0, x0=0, lo=0, hi=0, x=0, status=0, ws=0) == 0      # empty input is a no-op
    # only n_pose, n_ops, n_angles and n_active of the params block are read: the other fields may hold anything
    junk = _skel_params_of(_pt16_model())
    junk.n_frames, junk.n_cams, junk.h, junk.loss, junk.lam0 = -5, 99, -1.0, 7, -1.0
    assert _call(lib, good(), p=junk, n_frames=0) == 0


def test_a_shape_beyond_the_lds_is_refused_and_the_shipped_one_fits(lib):
    """A link program of 63 states and 60 slots with 16 pinhole cameras needs more than 160 KB (G alone 91 KB): refused
    with the limit named, before any device call; every shape of the tests and the shipped skeleton with 2 cameras pass the check
    (n_frames = 0 returns after it)."""
    good = _lib.PoseFitPxParams(camera_model=1, max_iter=100, min_detections=2, reserved=0, lam0=1e-3, ftol=1e-10, xtol=1e-10,
                                prior_sigma=np.pi, thresh=0.5, f_scale=5.0, sigma_px=5.0)
    null = C.c_void_p(0)

    def call(sk, n_cams):
        prog, act = build.skeleton.compile_skeleton(sk), np.asarray(build.active_states(sk), dtype=np.int32)
        p = _skel_params_of(build.SkeletonModel(prog=prog, active=act))
        act_c = (C.c_int32 * len(act))(*[int(a) for a in act])
        return lib.acino_skel_pose_fit_px(C.byref(good), C.byref(p), build._ops_array(prog), act_c, null, 0, n_cams, *([null] * 16),
                                          0, null)

    for name in ref.NAMES:
        assert call(ref.inputs(name)["skel"], len(ref.inputs(name)["rig"][0])) == 0, name
    assert call(ref.sref.skeleton("shipped"), 2) == 0
    big = ref.sref.cases.generic_skeleton(ref.sref.skeleton("shipped"), extra=9)
    for k in range(36):                                       # leaves without angles of their own: slots, no states
        big["positions"][f"leaf{k}"] = [0.1 * k, 0.2, 0.3]
        big["dofs"][f"leaf{k}"] = [0, 0, 0]
        big["markers"] = list(big["markers"]) + [f"leaf{k}"]
        big["links"] = list(big["links"]) + [["extra7", f"leaf{k}"]]
    P, L = len(build.active_states(big)), len(build.skeleton.compile_skeleton(big)["names"])
    assert (P, L) == (63, 60)
    assert call(big, 16) == -1 and b"160 KB" in lib.acino_last_error_string()


# ------------------------------------------------------------------------------------------------ Python entry
class Reached(Exception):
    pass


@pytest.fixture
def no_device(monkeypatch):
    def require_gpu():
        raise Reached()
    monkeypatch.setattr(_lib, "require_gpu", require_gpu)


def test_python_argument_errors_come_before_any_device_work(no_device):
    sig = inspect.signature(build.pose_fit_pixels)
    want = dict(x0=None, det=None, thresh=0.5, f_scale=5.0, sigma_px=None, prior_sigma=np.pi, min_detections=2, max_iter=100,
                ftol=1e-10, xtol=1e-10, lam0=1e-3, return_cov=True)
    assert {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty} == want
    assert list(sig.parameters)[:3] == ["model", "x0", "det"]
    model = ref.model_of("pt16-two")
    N, Cn, L, P = 24, 2, 6, 15
    det, x0 = np.zeros((N, Cn, L, 3)), np.zeros((N, P))
    with pytest.raises(Reached):
        build.pose_fit_pixels(model, x0)
    with pytest.raises(Reached):
        build.pose_fit_pixels(model, x0, det)
    with pytest.raises(Reached):
        build.pose_fit_pixels(model)
    for kw in (dict(prior_sigma=0.0), dict(f_scale=0.0), dict(sigma_px=np.nan), dict(sigma_px=0.0), dict(ftol=0.0), dict(xtol=-1.0),
               dict(lam0=0.0), dict(max_iter=0), dict(max_iter=256), dict(max_iter=2.5), dict(min_detections=0),
               dict(min_detections=13), dict(min_detections=1.5), dict(x0=np.zeros((N, 21))), dict(x0=np.zeros((N - 1, P))),
               dict(thresh=np.nan), dict(det=np.zeros((N, Cn, L, 2))), dict(det=np.zeros((N, 3, L, 3))),
               dict(det=np.zeros((N - 1, Cn, L, 3))), dict(det=np.zeros((N, Cn, L + 1, 3))), dict(det=np.zeros((Cn, L, 3)))):
        with pytest.raises(ValueError):
            build.pose_fit_pixels(model, **dict(dict(x0=x0), **kw))
    model.camera_model = "bogus"
    with pytest.raises(ValueError, match="camera_model"):
        build.pose_fit_pixels(model, x0)
    blank = ref.model_of("pt16-two")
    blank.weights = np.zeros_like(blank.weights)
    with pytest.raises(ValueError, match="sigma_px"):
        build.pose_fit_pixels(blank, x0)                      # (no positive weight: the default sigma_px has no source)
    with pytest.raises(Reached):
        build.pose_fit_pixels(blank, x0, sigma_px=2.0)


def test_the_sources_are_listed():
    assert "skel_pose_fit_px.hip" in _lib.SOURCES
    assert "pose_fit_skel.hpp" in _lib.HEADERS and "pose_fit_px_dev.hpp" in _lib.HEADERS
