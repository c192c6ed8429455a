"""Per-frame pose fit on the GPU (fte.pose_fit, k_pose_fit) against the numpy reference of tests/pose_fit_ref.py, on the inputs
that file defines: points and covariances of the multi-view triangulation's CPU reference (tests/test_pose_fit_host.py holds the
reference to central differences and to its optimality conditions, and the inputs to the conditions relied on here).

The solution is held by delta(x) = sqrt(g_free^T A_free^-1 g_free) of the GPU's point, evaluated by the reference with its own
active-set rule: at most B = 10 x the largest delta the reference's solver reaches on its status-0 frames of the same input
(both stop on a relative decrease and may stop a step apart).  The definitions - cov_x, cov_positions - are held at the GPU's
own x to 1e-12 cond(A_free): the rounding of a Cholesky inverse times a margin of about 1e3 for the Jacobian arithmetic.

Measured on the MI355X (profiles/pose_fit/pytest_gpu_pose_fit.txt): delta of the GPU's points 5.96e-06 (fisheye, sparse), 5.59e-06
(fisheye-pushed), 4.21e-06 (pinhole-pushed), 7.76e-05 (sub01), 3.54e-04 (sub520), 4.05e-06 (wide16) - the reference's own figures
to three digits, B ten times that; the same number of trials as the reference on every frame; distance to the reference's
minimiser at most 2.8e-09 (sub01); cov_x and cov_positions within 2.0e-04 of their bounds; no marginal entry of the active set."""
import functools

import numpy as np
import pytest
import torch

import pose_fit_ref as ref
import triangulate_mv_ref as tref
from acinoset_amd import calib, fte
from oracle import fk as ofk
from oracle import synth as osynth

pytestmark = pytest.mark.gpu

FLOATS = ("x", "x_full", "positions", "cost", "cov_x", "cov_positions", "std_positions")
KEYS = FLOATS + ("n_markers", "status", "iters", "pinned")


@functools.lru_cache(maxsize=None)
def gpu(name):
    inp = ref.inputs(name)
    return fte.pose_fit(inp["points"], inp["cov"])


@functools.lru_cache(maxsize=None)
def at_gpu_point(name):
    """The reference's objective at the GPU's own x (the start where a frame was not returned)."""
    prob, x = ref.solved(name)["prob"], gpu(name)["x"]
    return prob.objective(np.where(np.isfinite(x), x, prob.x0))


def _free_inverse(A, fixed):
    """inv(A_free) with zero rows and columns for the pinned states, and cond(A_free)."""
    free = ~fixed
    out = np.zeros_like(A)
    sub = A[np.ix_(free, free)]
    out[np.ix_(free, free)] = np.linalg.inv(sub)
    return out, np.linalg.cond(sub)


@pytest.mark.parametrize("name", ref.NAMES)
def test_solution(gpu_lib, name):
    inp, want, got = ref.inputs(name), ref.solved(name), gpu(name)
    prob, x, st = want["prob"], got["x"], got["status"]
    assert got["n_markers"].dtype == st.dtype == got["iters"].dtype == got["pinned"].dtype == np.uint8
    assert x.shape == (prob.N, 25) and got["x_full"].shape == (prob.N, 45) and got["cov_x"].shape == (prob.N, 25, 25)
    assert np.array_equal(got["n_markers"], prob.n_markers)
    assert np.array_equal(st == 2, want["status"] == 2)
    gone = st >= 2
    for key in ("x", "positions", "cost", "cov_x", "cov_positions", "std_positions"):
        flat = np.isnan(got[key]).reshape(prob.N, -1)
        assert np.array_equal(flat.all(1), gone) and np.array_equal(flat.any(1), gone), key
    assert np.array_equal(got["x_full"][:, fte.ACTIVE], x, equal_nan=True)
    assert (np.delete(got["x_full"], fte.ACTIVE, axis=1)[~gone] == 0).all() and (got["pinned"][gone] == 0).all()
    has = prob.n_markers >= 1
    print(f"{name}: status 0 on {(st == 0).sum()} of {has.sum()}, 1 on {(st == 1).sum()}, 3 on {(st == 3).sum()}; trials "
          f"{got['iters'][has].min()}..{got['iters'].max()} (reference {want['iters'][has].min()}..{want['iters'].max()})")
    assert (st == 0).sum() >= 0.9 * has.sum()
    assert (got["iters"][st == 0] <= 100).all() and (got["iters"][gone & ~has] == 0).all()
    back = st < 2
    obj = at_gpu_point(name)
    F0 = prob.objective(prob.x0, need_jac=False)["F"]
    assert (obj["F"][back] <= F0[back]).all()
    # (a whitened residual carries the rounding of a position of metres over a sigma of centimetres, ~1e-13: a frame whose one
    #  or two markers are met exactly has a cost of that size squared, hence the absolute term)
    assert np.allclose(got["cost"][back], obj["F"][back], rtol=1e-10, atol=1e-12)
    assert ((x[back] >= ref.LO) & (x[back] <= ref.HI)).all()
    B = ref.bound(name)
    delta = prob.delta(x, obj)
    print(f"{name}: delta max {np.nanmax(delta[st == 0]):.2e} (reference {B / 10:.2e}, bound B {B:.2e})")
    assert (delta[st == 0] <= B).all()
    if not inp["pushed"]:
        both = (st == 0) & (want["status"] == 0)
        dx = (x - want["x"])[both]
        dist = np.sqrt(np.einsum("ni,nij,nj->n", dx, want["obj"]["A"][both], dx))
        print(f"{name}: A-norm distance to the reference's minimiser max {dist.max():.2e} (bound {2 * B:.2e})")
        assert (dist <= 2 * B).all()
    # the active set: the reference's rule at the GPU's x, wherever the gradient is not marginal (an exact zero - a state none
    # of whose markers enters, resting at the centre of the ridge - is not marginal: it is not pinned)
    g, diag = obj["g"], np.einsum("npp->np", obj["A"])
    rule = prob.active_set(np.where(back[:, None], x, prob.x0), g, obj["A"])
    clear = (np.abs(g) > 1e-9 * diag) | (g == 0.0)
    at_bound = back[:, None] & ((x <= ref.LO) | (x >= ref.HI))
    marginal = at_bound & ~clear
    print(f"{name}: {at_bound.sum()} entries on a bound, {rule[back].sum()} pinned, {marginal.sum()} marginal")
    assert np.array_equal(got["pinned"].astype(bool)[back[:, None] & clear], rule[back[:, None] & clear])
    assert marginal.sum() <= 0.01 * at_bound.sum()


@pytest.mark.parametrize("name", ref.NAMES)
def test_definitions_at_the_returned_point(gpu_lib, name):
    got, obj = gpu(name), at_gpu_point(name)
    back = np.nonzero(got["status"] < 2)[0]
    pin = got["pinned"].astype(bool)
    cov_x, cov_p = got["cov_x"], got["cov_positions"]
    worst_x = worst_p = 0.0
    for n in back:
        C_ref, cond = _free_inverse(obj["A"][n], pin[n])
        worst_x = max(worst_x, np.abs(cov_x[n] - C_ref).max() / (1e-12 * cond * np.abs(C_ref).max()))
        P_ref = np.einsum("lip,pq,ljq->lij", obj["J"][n], C_ref, obj["J"][n])
        worst_p = max(worst_p, np.abs(cov_p[n] - P_ref).max() / (1e-12 * cond * np.abs(P_ref).max()))
        assert (cov_x[n][pin[n]] == 0.0).all() and (cov_x[n][:, pin[n]] == 0.0).all()
    print(f"{name}: cov_x error / bound max {worst_x:.2e}, cov_positions error / bound max {worst_p:.2e}")
    assert worst_x <= 1.0 and worst_p <= 1.0
    assert np.array_equal(cov_x[back], cov_x[back].transpose(0, 2, 1)) and np.array_equal(cov_p[back], cov_p[back].transpose(0, 1, 3, 2))
    c = cov_p[back]
    assert np.array_equal(got["std_positions"][back], np.sqrt((c[..., 0, 0] + c[..., 1, 1]) + c[..., 2, 2]))
    assert np.abs(got["positions"][back] - obj["pos"][back]).max() <= 1e-13 * np.abs(obj["pos"][back]).max()
    assert (np.einsum("npp->np", cov_x[back])[~pin[back]] > 0).all()


def test_translating_the_points_translates_the_head(gpu_lib):
    inp = ref.inputs("fisheye")
    x0 = ref.solved("fisheye")["prob"].x0
    base = fte.pose_fit(inp["points"], inp["cov"], x0=x0)
    assert (base["status"] == 0).all()
    for d in (np.array([1.0, 0.0, 0.0]), np.array([0.0, -2.0, 0.5]), np.array([0.3, -0.5, 0.8])):
        x0d = x0.copy()
        x0d[:, :3] += d
        moved = fte.pose_fit(inp["points"] + d, inp["cov"], x0=x0d)
        err = {"head": np.abs(moved["x"][:, :3] - d - base["x"][:, :3]).max(), "x": np.abs(moved["x"][:, 3:] - base["x"][:, 3:]).max(),
               "positions": np.abs(moved["positions"] - d - base["positions"]).max()}
        for key in ("cost", "cov_x", "cov_positions", "std_positions"):
            err[key] = np.abs(moved[key] - base[key]).max()
        print(f"d = {d}: " + ", ".join(f"{k} {v:.1e}" for k, v in err.items()))
        assert max(err.values()) <= 1e-11
        for key in ("n_markers", "status", "iters", "pinned"):
            assert np.array_equal(moved[key], base[key]), key


def test_isotropic_form_is_a_covariance_of_sigma_iso_squared(gpu_lib):
    """cov=None, sigma_iso=s against cov = s^2 I: every output within 1e-12 of its largest entry.  The two differ by an ulp in
    the whitening factor (1 / s against the square root of 1 / s^2), which the solve amplifies by cond(A_free): the input is
    the fully observed one, where that is 1e3 to 1e4."""
    pts = ref.inputs("fisheye")["points"]
    s = 0.02
    iso = fte.pose_fit(pts, sigma_iso=s)
    full = fte.pose_fit(pts, np.broadcast_to(s * s * np.eye(3), pts.shape[:2] + (3, 3)).copy(), sigma_iso=123.0)
    assert np.array_equal(iso["n_markers"], np.isfinite(pts).all(-1).sum(1)) and (iso["status"] < 2).all()
    for key in FLOATS:
        err = np.abs(iso[key] - full[key]).max() / np.abs(full[key]).max()
        print(f"{key}: {err:.2e}")
        assert err <= 1e-12, key
    for key in ("n_markers", "status", "pinned"):
        assert np.array_equal(iso[key], full[key]), key


def test_a_callers_start_equal_to_the_default_start_changes_nothing(gpu_lib):
    """The kernel's own start is what a call whose single trial is refused returns (lam0 = 1e300: a step of 1e-300 leaves F
    where it is); handed back as x0 it gives the output of the default call bit for bit.  It is the reference's default start."""
    inp = ref.inputs("sparse")
    start = fte.pose_fit(inp["points"], inp["cov"], lam0=1e300, max_iter=1, return_cov=False)
    assert (start["status"] == 1).all() and (start["iters"] == 1).all()
    want = ref.solved("sparse")["prob"].x0
    assert np.abs(start["x"] - want).max() <= 1e-15 and np.array_equal(start["x"][:, :3], want[:, :3])
    given = fte.pose_fit(inp["points"], inp["cov"], x0=start["x"])
    for key in KEYS:
        assert np.array_equal(given[key], gpu("sparse")[key], equal_nan=True), key


def test_prior_sigma_sets_the_bars_of_the_unseen_markers(gpu_lib):
    inp = ref.inputs("sparse")
    wide, tight = gpu("sparse"), fte.pose_fit(inp["points"], inp["cov"], prior_sigma=0.3)
    assert np.array_equal(wide["n_markers"], tight["n_markers"]) and (tight["status"] < 2).all()
    unseen = ~ref.solved("sparse")["prob"].enter
    few = np.zeros_like(unseen)
    few[7:11] = unseen[7:11]                                # the frames with one to four markers
    assert few[7].sum() == 18 and few[8].sum() == 19
    print(f"std of the unseen markers of frames 7..10, median: prior_sigma pi {np.median(wide['std_positions'][few]):.3f} m, "
          f"0.3 {np.median(tight['std_positions'][few]):.3f} m")
    assert (tight["std_positions"][few] < wide["std_positions"][few]).all()
    beyond_the_neck = few[9, 4:]                            # frame 9 keeps eyes and nose: nothing but the ridge holds the rest
    assert beyond_the_neck.all() and (tight["std_positions"][9, 4:] < 0.5 * wide["std_positions"][9, 4:]).all()


def test_grid_stride_beyond_the_grid_cap(gpu_lib):
    """2048 + 300 frames, a tiled 64-frame block with a marker pattern of its own in every frame: frame i is frame i mod 64,
    bit for bit."""
    inp = ref.inputs("fisheye")
    pts, cov = np.tile(inp["points"], (3, 1, 1))[:64].copy(), np.tile(inp["cov"], (3, 1, 1, 1))[:64].copy()
    pts[np.random.default_rng(1).random((64, 20)) < 0.25] = np.nan                  # a quarter of the markers, seeded
    patterns = {tuple(np.isfinite(p).all(-1)) for p in pts}
    assert len(patterns) == 64
    n = 2048 + 300
    rep = lambda a: torch.as_tensor(np.tile(a, (n // 64 + 1,) + (1,) * (a.ndim - 1))[:n], device="cuda")
    out = fte.pose_fit(rep(pts), rep(cov))
    first = fte.pose_fit(pts, cov)
    assert (first["status"] == 0).sum() >= 0.9 * 64 and len(set(first["iters"].tolist())) >= 4
    idx = torch.arange(n, device="cuda") % 64
    for key in KEYS:
        a = out[key]
        assert a.shape[0] == n
        same = a.view(torch.int64) == a[:64][idx].view(torch.int64) if a.dtype == torch.float64 else a == a[:64][idx]
        assert bool(same.all()), key
        w = torch.as_tensor(first[key], device="cuda")
        assert bool((a[:64].view(torch.int64) == w.view(torch.int64)).all() if a.dtype == torch.float64 else (a[:64] == w).all()), key


def test_tensors_in_tensors_out(gpu_lib):
    """The dict of triangulate_multiview_dense in place of points and cov, on the device from the detections to the pose."""
    inp = tref.inputs("fisheye-pushed")
    dev = torch.device("cuda", torch.cuda.current_device())
    tri = calib.triangulate_multiview_dense(torch.as_tensor(inp["det"], device=dev), tref.THRESH, *inp["rig"], f_scale=tref.F_SCALE)
    out = fte.pose_fit(tri, return_cov=False)
    assert set(out) == {"x", "x_full", "positions", "cost", "n_markers", "status", "iters", "pinned"}
    for key, val in out.items():
        assert isinstance(val, torch.Tensor) and val.device == dev, key
    assert out["x"].shape == (tref.FISHEYE_FRAMES, 25) and out["positions"].shape == (tref.FISHEYE_FRAMES, 20, 3)
    host = fte.pose_fit(tri["points"].cpu().numpy(), tri["cov"].cpu().numpy())
    for key, val in out.items():
        assert isinstance(host[key], np.ndarray) and np.array_equal(val.cpu().numpy(), host[key], equal_nan=True), key
    assert np.array_equal(out["n_markers"].cpu().numpy(), (tri["status"] < 2).sum(1).cpu().numpy())
    assert (out["status"].cpu().numpy() == 2).sum() == 1
    with pytest.raises(ValueError):
        fte.pose_fit(tri, cov=tri["cov"])


def test_pose_fit_start_of_the_trajectory_solve(gpu_lib):
    """pose_fit_init on a turning clip: closer to the true markers than triangulation_init, and the FTE from it ends at the
    cost of the FTE from the triangulation start, or below it."""
    seq = osynth.make_sequence(60, "loop")
    rig = (seq["K"], seq["D"], seq["R"], seq["t"])
    err = lambda x0: np.median(np.linalg.norm(ofk.cheetah_fk(x0) - seq["pos_true"], axis=-1))
    x_fit, x_tri = fte.pose_fit_init(seq["det"], *rig, 0.5), fte.triangulation_init(seq["det"], *rig, 0.5)
    assert x_fit.shape == (60, 45) and (np.delete(x_fit, fte.ACTIVE, axis=1) == 0).all()
    lo, hi = fte.bounds45()
    assert ((x_fit >= lo) & (x_fit <= hi)).all()
    print(f"median marker error of the start: pose fit {1e3 * err(x_fit):.1f} mm, triangulation {1e3 * err(x_tri):.1f} mm")
    assert err(x_fit) < err(x_tri)
    info, res = {}, {}
    for init in ("pose_fit", "triangulation"):
        res[init], info[init] = fte.fte_solve(seq["det"][..., :2], seq["det"][..., 2], *rig, seq["Ts"], init=init, max_iter=60)
        print(f"init={init}: {info[init]['iter']} iterations, cost {info[init]['cost']:.6f}, status {info[init]['status_name']}, "
              f"median marker error {1e3 * np.median(np.linalg.norm(res[init]['positions'] - seq['pos_true'], axis=-1)):.2f} mm")
    a, b = info["pose_fit"]["cost"], info["triangulation"]["cost"]
    assert a <= b + 1e-6 * abs(b)
    res_x0, _ = fte.fte_solve(seq["det"][..., :2], seq["det"][..., 2], *rig, seq["Ts"], x0=x_fit, max_iter=60)
    assert np.array_equal(res_x0["x"], res["pose_fit"]["x"])               # init="pose_fit" is pose_fit_init, nothing else
    with pytest.raises(ValueError, match="'nose_line', 'triangulation' or 'pose_fit'"):
        fte.fte_solve(seq["det"][..., :2], seq["det"][..., 2], *rig, seq["Ts"], init="bogus")
    blank = seq["det"].copy()
    blank[..., 2] = 0.0
    with pytest.raises(ValueError):
        fte.pose_fit_init(blank, *rig, 0.5)
