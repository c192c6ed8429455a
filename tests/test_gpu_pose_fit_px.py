"""Per-frame pose fit from the detections on the GPU (fte.pose_fit_pixels, k_pose_fit_px) against the numpy reference of
tests/pose_fit_px_ref.py, on the inputs that file defines: the detections and rigs of the multi-view triangulation's tests, started
from the 3-D fit's reference (tests/test_pose_fit_px_host.py holds the reference to central differences and to its optimality
conditions, and the inputs to the conditions relied on here).  Every call runs with prior_sigma=1.0, max_iter=255.

The solution is held as tests/test_gpu_pose_fit.py holds the 3-D fit's: delta(x) = sqrt(g_free^T A_free^-1 g_free) of the GPU's
point, evaluated by the reference with its own active-set rule, at most B = 10 x the largest delta the reference's solver reaches
on its status-0 frames of the same input.  The definitions - cov_x, cov_positions - are held at the GPU's own x to
1e-12 cond(A_free) times the largest entry, the rule of the 3-D fit's test.

Measured on the MI355X (profiles/pose_fit_px/pytest_gpu_pose_fit_px.txt): status 0 on every frame with a detection and the
reference's range of trials on every input (7..11 fisheye, 8..88 sub520, 8..96 mono-pushed); delta of the GPU's
points 1.66e-05 (fisheye), 3.23e-05 (fisheye-pushed), 2.14e-05 (pinhole-pushed), 1.29e-05 (sub01), 2.71e-05 (sub520), 1.90e-05
(wide16), 8.47e-06 (mono), 1.76e-05 (mono-pushed) - the reference's own figures to three digits, B ten times that; distance to
the reference's minimiser at most 6.4e-13 (wide16); weights within 9.4e-14; cov_x within 3.0e-04 and cov_positions within
8.8e-05 of their bounds; no marginal entry of the active set; the rig-translation identity to 3.9e-13 (cov_x)."""
import functools

import numpy as np
import pytest
import torch

import pose_fit_px_ref as ref
import pose_fit_ref as pref
import triangulate_mv_ref as tref
from acinoset_amd import calib, fte

pytestmark = pytest.mark.gpu

FLOATS = ("x", "x_full", "positions", "cost", "cov_x", "cov_positions", "std_positions", "weight")
KEYS = FLOATS + ("n_detections", "status", "iters", "pinned")


def fit(inp, **kw):
    args = dict(thresh=ref.THRESH, camera_model=inp["model"], x0=inp["x0"], f_scale=ref.F_SCALE, sigma_px=ref.SIGMA_PX)
    return fte.pose_fit_pixels(inp["det"], *inp["rig"], **dict(args, **ref.OPTS, **kw))


@functools.lru_cache(maxsize=None)
def gpu(name):
    return fit(ref.inputs(name))


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
    assert st.dtype == got["iters"].dtype == got["pinned"].dtype == np.uint8 and got["n_detections"].dtype == np.uint16
    assert x.shape == (prob.N, 25) and got["x_full"].shape == (prob.N, 45) and got["cov_x"].shape == (prob.N, 25, 25)
    assert got["weight"].shape == (prob.N, prob.C, 20, 2) and got["positions"].shape == (prob.N, 20, 3)
    assert got["cov_positions"].shape == (prob.N, 20, 3, 3) and got["std_positions"].shape == (prob.N, 20)
    assert np.array_equal(got["n_detections"], prob.n_markers)
    assert np.array_equal(st == 2, want["status"] == 2)
    gone = st >= 2
    for key in ("x", "positions", "cost", "cov_x", "cov_positions", "std_positions", "weight"):
        flat = np.isnan(got[key]).reshape(prob.N, -1)
        assert np.array_equal(flat.all(1), gone) and np.array_equal(flat.any(1), gone), key
    assert np.array_equal(got["x_full"][:, fte.ACTIVE], x, equal_nan=True)
    assert (np.delete(got["x_full"], fte.ACTIVE, axis=1)[~gone] == 0).all() and (got["pinned"][gone] == 0).all()
    has = prob.n_markers >= 1
    print(f"{name}: status 0 on {(st == 0).sum()} of {has.sum()}, 1 on {(st == 1).sum()}, 3 on {(st == 3).sum()}; trials "
          f"{got['iters'][has].min()}..{got['iters'].max()} (reference {want['iters'][has].min()}..{want['iters'].max()})")
    assert (st == 0).sum() >= 0.9 * has.sum()
    assert (got["iters"][gone & ~has] == 0).all()
    back = st < 2
    obj = at_gpu_point(name)
    F0 = prob.objective(prob.x0, need_jac=False)["F"]
    assert (obj["F"][back] <= F0[back]).all()
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
    # the active set: the reference's rule at the GPU's x, wherever the gradient is not marginal
    g, diag = obj["g"], np.einsum("npp->np", obj["A"])
    rule = prob.active_set(np.where(back[:, None], x, prob.x0), g, obj["A"])
    clear = (np.abs(g) > 1e-9 * diag) | (g == 0.0)
    at_bound = back[:, None] & ((x <= ref.LO) | (x >= ref.HI))
    marginal = at_bound & ~clear
    print(f"{name}: {at_bound.sum()} entries on a bound, {rule[back].sum()} pinned, {marginal.sum()} marginal")
    assert np.array_equal(got["pinned"].astype(bool)[back[:, None] & clear], rule[back[:, None] & clear])
    assert marginal.sum() <= 0.01 * at_bound.sum()
    # the weights every coordinate ended with
    w_err = np.abs(got["weight"][back] - obj["w"][back]).max()
    low = (obj["w"][back] < 0.1) & prob.valid[back][..., None]
    print(f"{name}: weight error max {w_err:.2e}; {low.sum()} of {2 * prob.valid[back].sum()} coordinates end with w < 0.1")
    assert w_err <= 1e-9
    assert (got["weight"][back][~prob.valid[back]] == 0.0).all()


@pytest.mark.parametrize("name", ref.NAMES)
def test_definitions_at_the_returned_point(gpu_lib, name):
    """cov_x and cov_positions against inv(A_free) and J cov_x J^T of the reference at the GPU's x, to 1e-12 cond(A_free) times
    the largest entry.  Measured on the MI355X: the worst ratio error / bound this test prints is 3.0e-04 (cov_x, wide16)
    and 8.8e-05 (cov_positions, fisheye)."""
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


def test_one_camera_has_a_pose(gpu_lib):
    """The capability: on one camera the triangulation gives no point and the 3-D fit no pose; the pixel fit converges."""
    inp = ref.inputs("mono")
    tri = calib.triangulate_multiview_dense(inp["det"], ref.THRESH, *inp["rig"], f_scale=ref.F_SCALE)
    assert (tri["status"] == 2).all()
    assert (fte.pose_fit(tri, x0=inp["x0"])["status"] == 2).all()
    got = gpu("mono")
    assert (got["status"] == 0).all() and (got["n_detections"] >= 2).all()
    with pytest.raises(ValueError):
        fte.pose_fit_pixels(inp["det"], *inp["rig"], thresh=ref.THRESH)          # no start without a triangulated marker


def test_two_cameras_use_every_detection(gpu_lib):
    """On sub01 the pixel fit uses more detections per frame than twice the markers the 3-D fit could use."""
    n_det, n_markers = gpu("sub01")["n_detections"].astype(np.int64), pref.solved("sub01")["prob"].n_markers
    print(f"sub01: detections per frame median {np.median(n_det):.0f}, markers with a point median {np.median(n_markers):.0f}")
    assert (n_det > 2 * n_markers).all()


def test_translating_the_rig_translates_the_head(gpu_lib):
    """t_c -> t_c - R_c d and the start's head + d: the head moves by d and nothing else does."""
    inp = ref.inputs("fisheye")
    K, D, R, t = inp["rig"]
    base = gpu("fisheye")
    assert (base["status"] == 0).all()
    for d in (np.array([1.0, 0.0, 0.0]), np.array([0.0, -2.0, 0.5]), np.array([0.3, -0.5, 0.8])):
        x0d = inp["x0"].copy()
        x0d[:, :3] += d
        td = np.asarray(t, dtype=np.float64).reshape(len(K), 3) - np.einsum("cij,j->ci", R, d)
        moved = fit(dict(inp, rig=(K, D, R, td.reshape(np.shape(t))), x0=x0d))
        err = {"head": np.abs(moved["x"][:, :3] - d - base["x"][:, :3]).max(), "x": np.abs(moved["x"][:, 3:] - base["x"][:, 3:]).max(),
               "positions": np.abs(moved["positions"] - d - base["positions"]).max()}
        for key in ("cost", "cov_x", "cov_positions", "std_positions", "weight"):
            err[key] = np.abs(moved[key] - base[key]).max()
        print(f"d = {d}: " + ", ".join(f"{k} {v:.1e}" for k, v in err.items()))
        assert max(err.values()) <= 1e-11
        for key in ("n_detections", "status", "iters", "pinned"):
            assert np.array_equal(moved[key], base[key]), key


def test_default_start_is_the_chain_of_triangulation_and_3d_fit(gpu_lib):
    """x0=None: triangulate_multiview_dense, pose_fit without covariances, fill_unfitted_frames - bit for bit."""
    inp = tref.inputs("fisheye-pushed")
    tri = calib.triangulate_multiview_dense(inp["det"], ref.THRESH, *inp["rig"], model=inp["model"])
    first = fte.pose_fit(tri, return_cov=False)
    assert (first["status"] == 2).sum() == 1
    x0 = fte.fill_unfitted_frames(first["x"], first["status"] < 2)
    chain = fte.pose_fit_pixels(inp["det"], *inp["rig"], thresh=ref.THRESH, camera_model=inp["model"], x0=x0, **ref.OPTS)
    default = fte.pose_fit_pixels(inp["det"], *inp["rig"], thresh=ref.THRESH, camera_model=inp["model"], **ref.OPTS)
    for key in KEYS:
        assert np.array_equal(default[key], chain[key], equal_nan=True), key
    assert (default["status"] == 2).sum() == 1 and (default["status"] == 0).sum() >= 0.9 * (len(x0) - 1)


def test_grid_stride_beyond_the_grid_cap(gpu_lib):
    """2048 + 300 frames, a tiled 64-frame block with a validity pattern of its own in every frame: frame i is frame i mod 64,
    bit for bit."""
    inp = ref.inputs("fisheye")
    det, x0 = np.tile(inp["det"], (3, 1, 1, 1))[:64].copy(), np.tile(inp["x0"], (3, 1))[:64].copy()
    det[..., 2][np.random.default_rng(1).random(det.shape[:3]) < 0.25] = 0.0          # a quarter of the detections, seeded
    patterns = {tuple((p[..., 2] > ref.THRESH).ravel()) for p in det}
    assert len(patterns) == 64
    n = 2048 + 300
    rep = lambda a: torch.as_tensor(np.tile(a, (n // 64 + 1,) + (1,) * (a.ndim - 1))[:n], device="cuda")
    out = fit(dict(inp, det=rep(det), x0=rep(x0)))
    first = fit(dict(inp, det=det, x0=x0))
    assert (first["status"] == 0).sum() >= 0.9 * 64 and len(set(first["iters"].tolist())) >= 4
    idx = torch.arange(n, device="cuda") % 64
    bits = lambda a: a.view(torch.int64) if a.dtype == torch.float64 else a.to(torch.int32)
    for key in KEYS:
        a = bits(out[key])
        assert a.shape[0] == n
        assert bool((a == a[:64][idx]).all()), key
        assert bool((a[:64] == bits(torch.as_tensor(first[key], device="cuda"))).all()), key


def test_tensors_in_tensors_out(gpu_lib):
    """Tensors on the device from the detections to the pose, on the pinhole rig: the second camera model."""
    inp = ref.inputs("pinhole-pushed")
    assert inp["model"] == "pinhole"
    dev = torch.device("cuda", torch.cuda.current_device())
    out = fit(dict(inp, det=torch.as_tensor(inp["det"], device=dev), x0=torch.as_tensor(inp["x0"], device=dev)), return_cov=False)
    assert set(out) == {"x", "x_full", "positions", "cost", "n_detections", "status", "iters", "pinned", "weight"}
    for key, val in out.items():
        assert isinstance(val, torch.Tensor) and val.device == dev, key
    host = gpu("pinhole-pushed")
    for key, val in out.items():
        assert isinstance(host[key], np.ndarray) and np.array_equal(val.cpu().numpy(), host[key], equal_nan=True), key
