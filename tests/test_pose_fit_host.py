"""Per-frame pose fit, host side (no GPU): the reference of tests/pose_fit_ref.py against central differences of the oracle's
FK and against its own optimality conditions, the conditions tests/test_gpu_pose_fit.py relies on evaluated by the reference
alone, the fill rule of fte.pose_fit_init, and the argument handling of the C ABI and of the Python entry before any device
work."""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__ as ge
import pose_fit_ref as ref
from acinoset_amd import _lib, fte
from oracle import fk


@pytest.fixture(scope="module")
def lib():
    ge.build()
    return _lib.lib()


# ------------------------------------------------------------------------------------------------ reference self-checks
def test_the_box_and_the_state_order_are_the_products():
    lo, hi = fte.bounds45()
    assert np.array_equal(fte.ACTIVE, ref.ACTIVE) and np.array_equal(lo[fte.ACTIVE], ref.LO) and np.array_equal(hi[fte.ACTIVE], ref.HI)
    assert ref.ACTIVE[ref.PSI0] == fte.PSI and fte.PSI_COLUMNS == [20, 21, 22, 23, 24]


@pytest.mark.parametrize("name", ("fisheye", "sparse"))
def test_gradient_and_matrix_match_central_differences_of_the_oracle_fk(name):
    """J by central differences of oracle.fk.cheetah_fk (h = 1e-6 rad / m: truncation ~1e-12, rounding ~1e-10), then
    g = J^T W r + ridge and A = J^T W J + ridge from it, at a point off the start (so that the ridge term is not zero)."""
    inp = ref.inputs(name)
    prob = ref.Problem(inp["points"], inp["cov"])
    rng = np.random.default_rng(5)
    x = np.clip(prob.x0 + rng.normal(0.0, 0.1, prob.x0.shape), ref.LO, ref.HI)
    o = prob.objective(x)
    h = 1e-6
    Jfd = np.zeros_like(o["J"])
    for p in range(ref.NP_):
        e = np.zeros(ref.NP_)
        e[p] = h
        Jfd[..., p] = (fk.cheetah_fk(ref.full_state(x + e)) - fk.cheetah_fk(ref.full_state(x - e))) / (2 * h)
    r = np.where(prob.enter[..., None], o["pos"] - prob.y0, 0.0)
    g = np.einsum("nlip,nlij,nlj->np", Jfd, prob.W, r)
    g[:, 3:] += prob.kappa * (x - prob.m)[:, 3:]
    A = np.einsum("nlip,nlij,nljq->npq", Jfd, prob.W, Jfd)
    A[:, np.arange(3, ref.NP_), np.arange(3, ref.NP_)] += prob.kappa
    eg, eA = np.abs(o["g"] - g).max() / np.abs(g).max(), np.abs(o["A"] - A).max() / np.abs(A).max()
    print(f"{name}: g {eg:.2e}  A {eA:.2e} (relative to the largest entry)")
    assert eg < 1e-7 and eA < 1e-7
    # and F is the function g differentiates: a central difference of F along a random direction
    d = rng.normal(0.0, 1.0, x.shape)
    d[(x <= ref.LO) | (x >= ref.HI)] = 0.0
    dF = (prob.objective(x + h * d, need_jac=False)["F"] - prob.objective(x - h * d, need_jac=False)["F"]) / (2 * h)
    assert np.allclose(dF, (o["g"] * d).sum(1), rtol=1e-6, atol=1e-6 * np.abs(dF).max())


@pytest.mark.parametrize("name", ref.NAMES)
def test_reference_end_points_satisfy_the_kkt_conditions(name):
    """At the reference's status-0 points: inside the box; a pinned state sits on its bound with the gradient pushing outward;
    and on the free states what a Newton step could still gain, delta^2 / 2, is below 1e-6 of a cost of order one or more (the
    solver stops on a decrease of 1e-10 F)."""
    r = ref.solved(name)
    ok = r["status"] == 0
    x, g, pin = r["x"][ok], r["obj"]["g"][ok], r["pinned"][ok]
    assert ((x >= ref.LO) & (x <= ref.HI)).all()
    assert (((x == ref.LO) & (g > 0)) | ((x == ref.HI) & (g < 0)))[pin].all()
    print(f"{name}: delta max {r['delta'][ok].max():.2e}, cost median {np.median(r['cost'][ok]):.2f}")
    assert (r["delta"][ok] ** 2 / 2 <= 1e-6 * np.maximum(r["cost"][ok], 1.0)).all()
    assert (r["cost"][ok] <= r["prob"].objective(r["prob"].x0, need_jac=False)["F"][ok]).all()


# ------------------------------------------------------------------------------------------------ input conditions
@pytest.mark.parametrize("name", ref.NAMES)
def test_inputs_meet_the_conditions_of_the_gpu_tests(name):
    r = ref.solved(name)
    st, nm = r["status"], r["prob"].n_markers
    has = nm >= 1
    print(f"{name}: {has.sum()} of {len(st)} frames with a marker, status 0 on {(st == 0).sum()}, 1 on {(st == 1).sum()}, 2 on "
          f"{(st == 2).sum()}, 3 on {(st == 3).sum()}; trials {r['iters'][has].min()}..{r['iters'].max()}; delta max "
          f"{np.nanmax(r['delta'][st == 0]):.2e}")
    assert np.array_equal(st == 2, ~has) and (st == 3).sum() == 0
    assert (st == 0).sum() >= 0.9 * has.sum()
    assert np.array_equal(np.isnan(r["x"]).all(1), st >= 2) and np.array_equal(np.isnan(r["x"]).any(1), st >= 2)


def test_inputs_hold_the_cases_the_gpu_tests_name():
    """sub01: frames with a state on its bound and unlike trial counts; one frame without any marker in each of
    fisheye-pushed and sub520; the edited frames of sparse.  A state "on its bound" is counted as the issue's prototype
    counted it (18 of 27 frames here, as there): most are knee angles that start at their bound 0 with none of their markers
    entering, where the gradient is exactly 0 and the state is not pinned; the frames with a pinned state are counted too."""
    s01, s520 = ref.solved("sub01"), ref.solved("sub520")
    at_bound = lambda r: ((r["x"] <= ref.LO) | (r["x"] >= ref.HI))[r["status"] < 2]
    print(f"sub01: {at_bound(s01).any(1).sum()} frames with a state on its bound, {s01['pinned'].any(1).sum()} with a pinned one; "
          f"sub520: {at_bound(s520).any(1).sum()} and {s520['pinned'].any(1).sum()}")
    assert at_bound(s01).any(1).sum() >= 10
    assert s01["pinned"].any() and s520["pinned"].any(1).sum() >= 5
    assert s01["iters"].min() <= 7 and s01["iters"].max() >= 100
    assert (ref.solved("fisheye-pushed")["status"] == 2).sum() == 1 and (s520["status"] == 2).sum() == 1
    sp = ref.solved("sparse")
    assert sp["prob"].n_markers[[3, 4, 7, 8, 9, 10, 11, 12]].tolist() == [16, 16, 2, 1, 3, 4, 19, 19]
    assert not sp["prob"].enter[3:5, :4].any() and not sp["prob"].enter[11:13, ref.SPARSE_COV_MARKER].any()
    assert (sp["status"][[3, 4, 7, 8, 9, 10, 11, 12]] == 0).all()
    # the default start: no head marker -> the mean of all entering markers, no heading
    assert np.array_equal(sp["prob"].x0[8, :3], ref.inputs("sparse")["points"][8, 15]) and sp["prob"].x0[8, ref.PSI0] == 0.0
    assert sp["prob"].x0[9, ref.PSI0] == 0.0 and sp["prob"].x0[10, ref.PSI0] != 0.0


# ------------------------------------------------------------------------------------------------ the fill rule
def test_frames_without_a_fit_are_interpolated_with_the_psi_columns_unwrapped():
    N = 9
    x = np.full((N, 25), np.nan)
    fitted = np.array([0, 1, 1, 0, 0, 1, 0, 1, 0], dtype=bool)
    rows = np.nonzero(fitted)[0]
    x[rows] = rows[:, None] * 0.1 + np.arange(25)[None, :] * 0.01
    x[rows, 20] = [3.0, 3.1, -3.1, -3.0]                   # psi_0 crosses the cut between frames 2 and 5
    x[rows, 6] = [3.0, 3.1, -3.1, -3.0]                    # a theta column is NOT unwrapped
    got = fte.fill_unfitted_frames(x, fitted)
    assert np.isfinite(got).all() and np.array_equal(got[rows][:, :6], x[rows][:, :6])
    assert np.array_equal(got[0], got[1]) and np.array_equal(got[8], got[7])               # held flat at the ends
    assert np.allclose(got[3, 0], 0.2 + (0.5 - 0.2) / 3) and np.allclose(got[6, 1], 0.5 * (x[5, 1] + x[7, 1]))
    psi = np.array([3.0, 3.1, -3.1 + 2 * np.pi, -3.0 + 2 * np.pi])
    assert np.allclose(got[rows, 20], psi) and np.allclose(got[3, 20], 3.1 + (psi[2] - 3.1) / 3)
    assert np.allclose(got[3, 6], 3.1 + (-3.1 - 3.1) / 3)
    for p in fte.PSI_COLUMNS:
        assert fte.ACTIVE[p] >= fte.PSI
    with pytest.raises(ValueError):
        fte.fill_unfitted_frames(x, np.zeros(N, dtype=bool))
    keep = fte.fill_unfitted_frames(x[rows], np.ones(4, dtype=bool))
    assert np.array_equal(keep[:, :20], x[rows][:, :20])


# ------------------------------------------------------------------------------------------------ C ABI
def _call(lib, prm, n_frames=10, points=8, x=8, status=8):
    null, p = C.c_void_p(0), lambda v: C.c_void_p(v)
    return lib.acino_cheetah_pose_fit(C.byref(prm), p(points), null, null, n_frames, p(x), null, null, p(status), null, null, null,
                                      null, null, null, null)


def test_abi_arguments_are_checked_before_any_device_call(lib):
    good = lambda **kw: _lib.PoseFitParams(**dict(dict(max_iter=100, min_markers=1, lam0=1e-3, ftol=1e-10, xtol=1e-10,
                                                       prior_sigma=np.pi, sigma_iso=0.01), **kw))
    assert lib.acino_sizeof_pose_fit_params() == C.sizeof(_lib.PoseFitParams) == 48
    for kw, shape, word in ((dict(max_iter=0), dict(), b"max_iter"), (dict(max_iter=256), dict(), b"max_iter"),
                            (dict(min_markers=0), dict(), b"min_markers"), (dict(min_markers=21), dict(), b"min_markers"),
                            (dict(lam0=0.0), dict(), b"lam0"), (dict(ftol=0.0), dict(), b"ftol"), (dict(xtol=-1.0), dict(), b"xtol"),
                            (dict(prior_sigma=0.0), dict(), b"prior_sigma"), (dict(sigma_iso=-0.01), dict(), b"sigma_iso"),
                            (dict(sigma_iso=np.nan), dict(), b"sigma_iso"), (dict(), dict(n_frames=-1), b"n_frames"),
                            (dict(), dict(points=0), b"null buffer"), (dict(), dict(x=0), b"null buffer"),
                            (dict(), dict(status=0), b"null buffer")):
        assert _call(lib, good(**kw), **shape) == -1 and word in lib.acino_last_error_string(), (kw, shape)
    assert _call(lib, good(), n_frames=0, points=0, x=0, status=0) == 0                    # empty input is a no-op
    null = C.c_void_p(0)
    assert lib.acino_cheetah_pose_fit(None, null, null, null, 0, null, null, null, null, null, null, null, null, null, null,
                                      null) == -1


# ------------------------------------------------------------------------------------------------ Python entry
class Reached(Exception):
    pass


@pytest.fixture
def no_device(monkeypatch):
    def require_gpu():
        raise Reached()
    monkeypatch.setattr(_lib, "require_gpu", require_gpu)


def test_python_argument_errors_come_before_any_device_work(no_device):
    import inspect
    sig = inspect.signature(fte.pose_fit)
    want = dict(cov=None, x0=None, prior_sigma=np.pi, sigma_iso=0.01, min_markers=1, max_iter=100, ftol=1e-10, xtol=1e-10,
                lam0=1e-3, return_cov=True)
    assert {k: v.default for k, v in sig.parameters.items() if k != "points"} == want
    pts, cov = np.zeros((4, 20, 3)), np.tile(np.eye(3), (4, 20, 1, 1))
    with pytest.raises(Reached):
        fte.pose_fit(pts, cov)
    with pytest.raises(Reached):
        fte.pose_fit(dict(points=pts, cov=cov, status=None))
    for kw in (dict(prior_sigma=0.0), dict(sigma_iso=np.nan), dict(ftol=0.0), dict(xtol=-1.0), dict(lam0=0.0), dict(max_iter=0),
               dict(max_iter=256), dict(max_iter=2.5), dict(min_markers=0), dict(min_markers=21), dict(x0=np.zeros((4, 45))),
               dict(cov=cov[:3]), dict(cov=cov[..., 0])):
        with pytest.raises(ValueError):
            fte.pose_fit(pts, **kw)
    with pytest.raises(ValueError):
        fte.pose_fit(np.zeros((4, 19, 3)))
    with pytest.raises(ValueError):
        fte.pose_fit(dict(points=pts, cov=cov), cov=cov)


def test_an_unknown_init_names_the_three_choices():
    with pytest.raises(ValueError, match="'nose_line', 'triangulation' or 'pose_fit'"):
        fte._initial_x0(np.zeros((4, 6, 20, 3)), None, "bogus", (None,) * 4, 0.5, 0, "fisheye", "x0 must be [N, 45]")
