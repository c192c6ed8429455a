"""Per-frame pose fit from the detections, host side (no GPU): the reference of tests/pose_fit_px_ref.py against central
differences of its own F and against the assembled Jacobian, its optimality conditions, the conditions
tests/test_gpu_pose_fit_px.py relies on evaluated by the reference alone, its sensitivity to the camera records, the
rig-translation identity, and the argument handling of the C ABI and of the Python entry before any device work."""
import ctypes as C
import inspect

import numpy as np
import pytest

import __graft_entry__ as ge
import pose_fit_px_ref as ref
import pose_fit_ref as pref
import unlike_rig as ur
from acinoset_amd import _lib, fte


@pytest.fixture(scope="module")
def lib():
    ge.build()
    return _lib.lib()


# ------------------------------------------------------------------------------------------------ reference self-checks
def test_constants_are_the_products():
    assert list(ref.PSI_COLUMNS) == fte.PSI_COLUMNS and ref.SIGMA_PX == fte.R_MEAS
    sig = inspect.signature(fte.pose_fit_pixels)
    assert sig.parameters["f_scale"].default == ref.F_SCALE and sig.parameters["sigma_px"].default == ref.SIGMA_PX
    assert sig.parameters["thresh"].default == ref.THRESH


@pytest.mark.parametrize("name", ("fisheye-pushed", "pinhole-pushed", "mono"))
def test_gradient_and_matrix_match_central_differences(name):
    """g against central differences of F state by state (h = 1e-6), at a point off the start so that the ridge term is not zero;
    A = sum w J^T J / sigma^2 + ridge against the Jacobian of the residuals assembled by central differences of the pixels."""
    prob = ref.problem(name)
    rng = np.random.default_rng(5)
    x = np.clip(prob.x0 + rng.normal(0.0, 0.02, prob.x0.shape), ref.LO, ref.HI)
    o = prob.objective(x)
    assert np.isfinite(o["F"]).all()
    h = 1e-6
    gfd, Jfd = np.zeros_like(o["g"]), np.zeros_like(o["Jpx"])
    for p in range(ref.NP_):
        e = np.zeros(ref.NP_)
        e[p] = h
        up, dn = prob.objective(x + e), prob.objective(x - e)
        gfd[:, p] = (up["F"] - dn["F"]) / (2 * h)
        Jfd[..., p] = (up["r"] - dn["r"]) / (2 * h)
    A = np.einsum("nclkp,nclk,nclkq->npq", Jfd, o["w"], Jfd) / prob.sigma_px ** 2
    A[:, np.arange(3, ref.NP_), np.arange(3, ref.NP_)] += prob.kappa
    eg, eA = np.abs(o["g"] - gfd).max() / np.abs(gfd).max(), np.abs(o["A"] - A).max() / np.abs(A).max()
    print(f"{name}: g {eg:.2e}  A {eA:.2e} (relative to the largest entry)")
    assert eg < 1e-6 and eA < 1e-6
    assert (o["w"][~prob.valid] == 0.0).all() and (o["Jpx"][~prob.valid] == 0.0).all()
    w = 1.0 / (1.0 + (o["r"] / prob.fs) ** 2)
    assert np.allclose(o["w"][prob.valid], w[prob.valid], rtol=1e-14, atol=0.0)


def test_a_marker_behind_its_camera_makes_the_cost_infinite():
    prob = ref.problem("mono")
    R, t = prob.rig[2][0], np.asarray(prob.rig[3][0], dtype=np.float64).reshape(3)
    x = prob.x0.copy()
    x[:, :3] = -R.T @ t - 5.0 * R[2]                        # the head five metres behind the camera centre
    F = prob.objective(x, need_jac=False)["F"]
    assert np.isinf(F).all() and (F > 0).all()
    blind = ref.Problem(np.zeros((3, 1, 20, 3)), prob.rig, "fisheye", x[:3], **ref.OPTS)
    assert np.isfinite(blind.objective(x[:3], need_jac=False)["F"]).all()          # no valid detection: nothing is behind
    assert (blind.solve()[1] == 2).all()


@pytest.mark.parametrize("name", ref.NAMES)
def test_reference_end_points_satisfy_the_kkt_conditions(name):
    """First-order optimality on the free states at the reference's solution: inside the box; a pinned state sits on its bound
    with the gradient pushing outward; what a Newton step could still gain, delta^2 / 2, is below 1e-6 of a cost of order one or
    more (the solver stops on a decrease of 1e-10 F)."""
    r = ref.solved(name)
    ok = r["status"] == 0
    x, g, pin = r["x"][ok], r["obj"]["g"][ok], r["pinned"][ok]
    assert ((x >= ref.LO) & (x <= ref.HI)).all()
    assert (((x == ref.LO) & (g > 0)) | ((x == ref.HI) & (g < 0)))[pin].all()
    print(f"{name}: delta max {r['delta'][ok].max():.2e}, cost median {np.median(r['cost'][ok]):.2f}")
    assert (r["delta"][ok] ** 2 / 2 <= 1e-6 * np.maximum(r["cost"][ok], 1.0)).all()
    assert (r["cost"][ok] <= r["prob"].objective(r["prob"].x0, need_jac=False)["F"][ok]).all()


# ------------------------------------------------------------------------------------------------ input conditions
FRAMES = {"fisheye": (27, 27), "fisheye-pushed": (27, 26), "pinhole-pushed": (16, 15), "sub01": (27, 27), "sub520": (27, 26),
          "wide16": (14, 14), "mono": (27, 27), "mono-pushed": (27, 26)}
CAMERAS = {"fisheye": 6, "fisheye-pushed": 6, "pinhole-pushed": 6, "sub01": 2, "sub520": 3, "wide16": 16, "mono": 1, "mono-pushed": 1}


@pytest.mark.parametrize("name", ref.NAMES)
def test_inputs_meet_the_conditions_of_the_gpu_tests(name):
    """Status 0 on every frame that has a detection, 7 to 96 trials, the largest delta between 0.8e-5 and 3.3e-5,
    cond(A_free) at most 1.6e5: the GPU test's caps (0.9 of the frames, B = 10 delta, 1e-12 cond) rest on these."""
    r = ref.solved(name)
    prob, st = r["prob"], r["status"]
    has = prob.n_markers >= 1
    ok = st == 0
    conds = [np.linalg.cond(r["obj"]["A"][n][np.ix_(~r["pinned"][n], ~r["pinned"][n])]) for n in np.nonzero(ok)[0]]
    print(f"{name}: {prob.C} cameras, {has.sum()} of {len(st)} frames with a detection, status 0 on {ok.sum()}; trials "
          f"{r['iters'][has].min()}..{r['iters'].max()}; delta max {r['delta'][ok].max():.2e}; cond(A_free) max {max(conds):.2e}")
    assert (prob.N, has.sum()) == FRAMES[name] and prob.C == CAMERAS[name]
    assert np.array_equal(st == 2, ~has) and np.array_equal(ok, has)
    assert r["iters"][has].min() >= 7 and r["iters"].max() <= 96
    assert 0.8e-5 <= r["delta"][ok].max() <= 3.3e-5 and max(conds) <= 1.6e5
    assert np.array_equal(np.isnan(r["x"]).all(1), st >= 2) and np.array_equal(np.isnan(r["x"]).any(1), st >= 2)


def test_inputs_hold_the_cases_the_gpu_tests_name():
    """Both camera models; a frame with no detection in every pushed input; pushed detections that end with w < 0.1 (84 of
    5 350 coordinates on fisheye-pushed); states pinned on a bound on sub01 and sub520; on sub01 more detections than twice the
    markers the 3-D fit can use; on the mono pair no marker with a point at all."""
    assert ref.inputs("pinhole-pushed")["model"] == "pinhole" and ref.inputs("fisheye")["model"] == "fisheye"
    for name in ref.NAMES:
        if ref.inputs(name)["pushed"]:
            assert (ref.solved(name)["status"] == 2).sum() == 1, name
    r = ref.solved("fisheye-pushed")
    ok = r["status"] == 0
    valid = r["prob"].valid[ok][..., None]
    assert ((r["obj"]["w"][ok] < 0.1) & valid).sum() == 84 and 2 * valid.sum() == 5350
    assert ref.solved("sub01")["pinned"].any() and ref.solved("sub520")["pinned"].any()
    n_det, n_markers = ref.solved("sub01")["prob"].n_markers, pref.solved("sub01")["prob"].n_markers
    print(f"sub01: detections per frame median {np.median(n_det):.0f}, markers with a point median {np.median(n_markers):.0f}")
    assert np.median(n_det) == 35 and np.median(n_markers) == 15 and (n_det > 2 * n_markers).all()
    mono = ref.solved("mono")["prob"]
    assert mono.C == 1 and (mono.n_markers >= 2).all()
    assert np.abs(ref.inputs("mono")["x0"] - pref.solved("fisheye")["x"]).max() == pytest.approx(0.05)


# ------------------------------------------------------------------------------------------------ sensitivity, invariance
MUTANT_FRAMES = 5          # (none of them the frame without a detection: that is frame 5)


@pytest.mark.parametrize("name,mutant", [("fisheye", "rolled"), ("fisheye", "no_skew"), ("pinhole-pushed", "rolled"),
                                         ("wide16", "rolled"), ("sub520", "rolled")])
def test_a_wrong_camera_record_moves_the_solution_beyond_the_bound(name, mutant):
    """On the first frames of an input (a frame is a problem of its own): with a mutant of the rig the reference's minimiser leaves the neighbourhood the GPU test allows (A-norm distance 2 B to
    the reference's x, delta at most B at the right rig): a kernel that reads a camera record wrongly cannot pass."""
    inp, right, B = ref.inputs(name), ref.solved(name), ref.bound(name)
    n = MUTANT_FRAMES
    wrong_x, wrong_status = ref.Problem(inp["det"][:n], ur.MUTANTS[mutant](inp["rig"]), inp["model"], inp["x0"][:n], **ref.OPTS).solve()[:2]
    both = (right["status"][:n] == 0) & (wrong_status < 2)
    dx = (wrong_x - right["x"][:n])[both]
    dist = np.sqrt(np.einsum("ni,nij,nj->n", dx, right["obj"]["A"][:n][both], dx))
    at = np.full_like(right["x"], np.nan)
    at[:n][both] = wrong_x[both]
    delta = right["prob"].delta(at)[:n][both]
    print(f"{name} / {mutant}: distance min {dist.min():.2e}, delta at the right rig min {delta.min():.2e} (B {B:.2e})")
    assert both.sum() >= 0.9 * n
    assert (dist > 2 * B).all() and (delta > B).all()


def test_translating_the_rig_translates_the_head():
    """t_c -> t_c - R_c d with the start's head + d: the head moves by d and nothing else, in the same number of trials."""
    inp = ref.inputs("fisheye")
    K, D, R, t = inp["rig"]
    base = ref.solved("fisheye")
    d = np.array([0.3, -0.5, 0.8])
    td = (np.asarray(t, dtype=np.float64).reshape(len(K), 3) - np.einsum("cij,j->ci", R, d)).reshape(np.shape(t))
    x0 = inp["x0"].copy()
    x0[:, :3] += d
    x, status, iters, cost = ref.Problem(inp["det"], (K, D, R, td), inp["model"], x0, **ref.OPTS).solve()
    head, rest = np.abs(x[:, :3] - d - base["x"][:, :3]).max(), np.abs(x[:, 3:] - base["x"][:, 3:]).max()
    print(f"head {head:.1e}, angles {rest:.1e}")
    assert head <= 1e-12 and rest <= 1e-12
    assert np.array_equal(status, base["status"]) and np.array_equal(iters, base["iters"])


# ------------------------------------------------------------------------------------------------ C ABI
def _call(lib, prm, n_frames=10, n_cams=6, det=8, cams=8, x0=8, x=8, status=8):
    null, p = C.c_void_p(0), lambda v: C.c_void_p(v)
    return lib.acino_cheetah_pose_fit_px(C.byref(prm), p(det), n_frames, n_cams, p(cams), p(x0), p(x), null, null, p(status),
                                         null, null, null, null, null, null, null, null)


def test_abi_arguments_are_checked_before_any_device_call(lib):
    good = lambda **kw: _lib.PoseFitPxParams(**dict(dict(camera_model=0, max_iter=100, min_detections=2, reserved=0, lam0=1e-3,
                                                         ftol=1e-10, xtol=1e-10, prior_sigma=np.pi, thresh=0.5, f_scale=5.0,
                                                         sigma_px=5.0), **kw))
    assert lib.acino_sizeof_pose_fit_px_params() == C.sizeof(_lib.PoseFitPxParams) == 72
    for kw, shape, word in ((dict(max_iter=0), dict(), b"max_iter"), (dict(max_iter=256), dict(), b"max_iter"),
                            (dict(camera_model=2), dict(), b"camera_model"), (dict(camera_model=-1), dict(), b"camera_model"),
                            (dict(min_detections=0), dict(), b"min_detections"), (dict(min_detections=121), dict(), b"min_detections"),
                            (dict(min_detections=21), dict(n_cams=1), b"min_detections"),
                            (dict(lam0=0.0), dict(), b"lam0"), (dict(ftol=0.0), dict(), b"ftol"), (dict(xtol=-1.0), dict(), b"xtol"),
                            (dict(prior_sigma=0.0), dict(), b"prior_sigma"), (dict(thresh=np.nan), dict(), b"thresh"),
                            (dict(f_scale=0.0), dict(), b"f_scale"), (dict(f_scale=np.inf), dict(), b"f_scale"),
                            (dict(sigma_px=-5.0), dict(), b"sigma_px"), (dict(sigma_px=np.nan), dict(), b"sigma_px"),
                            (dict(), dict(n_frames=-1), b"n_frames"), (dict(), dict(n_cams=0), b"n_cams"),
                            (dict(), dict(n_cams=17), b"n_cams"), (dict(), dict(det=0), b"null buffer"),
                            (dict(), dict(cams=0), b"null buffer"), (dict(), dict(x0=0), b"null buffer"),
                            (dict(), dict(x=0), b"null buffer"), (dict(), dict(status=0), b"null buffer")):
        assert _call(lib, good(**kw), **shape) == -1 and word in lib.acino_last_error_string(), (kw, shape)
    assert _call(lib, good(min_detections=120)) != -1 or b"min_detections" not in lib.acino_last_error_string()
    assert _call(lib, good(), n_frames=0, det=0, cams=0, x0=0, x=0, status=0) == 0          # empty input is a no-op
    null = C.c_void_p(0)
    assert lib.acino_cheetah_pose_fit_px(None, null, 0, 6, null, null, null, null, null, null, null, null, null, null, null,
                                         null, null, null) == -1


# ------------------------------------------------------------------------------------------------ Python entry
class Reached(Exception):
    pass


@pytest.fixture
def no_device(monkeypatch):
    def require_gpu():
        raise Reached()
    monkeypatch.setattr(_lib, "require_gpu", require_gpu)


def test_python_argument_errors_come_before_any_device_work(no_device):
    sig = inspect.signature(fte.pose_fit_pixels)
    want = dict(thresh=0.5, camera_model="fisheye", x0=None, f_scale=5.0, sigma_px=5.0, prior_sigma=np.pi, min_detections=2,
                max_iter=100, ftol=1e-10, xtol=1e-10, lam0=1e-3, return_cov=True)
    assert {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty} == want
    assert list(sig.parameters)[:5] == ["det", "k_arr", "d_arr", "r_arr", "t_arr"]
    rig = ur.unlike_rig(6, "fisheye", skew=True)
    det, x0 = np.zeros((4, 6, 20, 3)), np.zeros((4, 25))
    with pytest.raises(Reached):
        fte.pose_fit_pixels(det, *rig, x0=x0)
    with pytest.raises(Reached):
        fte.pose_fit_pixels(det, *rig)
    for kw in (dict(prior_sigma=0.0), dict(f_scale=0.0), dict(sigma_px=np.nan), dict(ftol=0.0), dict(xtol=-1.0), dict(lam0=0.0),
               dict(max_iter=0), dict(max_iter=256), dict(max_iter=2.5), dict(min_detections=0), dict(min_detections=121),
               dict(min_detections=1.5), dict(x0=np.zeros((4, 45))), dict(x0=np.zeros((3, 25))), dict(thresh=np.nan),
               dict(camera_model="bogus")):
        with pytest.raises(ValueError):
            fte.pose_fit_pixels(det, *rig, **dict(dict(x0=x0), **kw))
    for bad in (np.zeros((4, 6, 19, 3)), np.zeros((4, 6, 20, 2)), np.zeros((6, 20, 3)), np.zeros((4, 17, 20, 3)),
                np.zeros((4, 0, 20, 3)), np.zeros((4, 5, 20, 3))):
        with pytest.raises(ValueError):
            fte.pose_fit_pixels(bad, *rig, x0=x0)
