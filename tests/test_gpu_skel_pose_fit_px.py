"""Per-frame skeleton pose fit from the detections on the GPU (build.pose_fit_pixels, k_skel_pose_fit_px) against the numpy
reference of tests/skel_pose_fit_px_ref.py, on the inputs that file defines (tests/test_skel_pose_fit_px_host.py holds the
reference to central differences and to its optimality conditions, and the inputs to the conditions relied on here).  Every call
runs with prior_sigma=1.0, max_iter=255.

The solution is held as tests/test_gpu_pose_fit_px.py holds the cheetah's: delta(x) = sqrt(g_free^T A_free^-1 g_free) of the
GPU's point, evaluated by the reference with its own active-set rule, at most B = 10 x the largest delta the reference's solver
reaches on its status-0 frames of the same input.  The definitions - cov_x, cov_positions - are held at the GPU's own x to
1e-12 cond(A_free) times the largest entry."""
import functools

import numpy as np
import pytest
import torch

import skel_pose_fit_px_ref as ref
from acinoset_amd import build

pytestmark = pytest.mark.gpu

FLOATS = ("x", "x_full", "positions", "cost", "cov_x", "cov_positions", "std_positions", "weight")
KEYS = FLOATS + ("n_detections", "status", "iters", "pinned")


def fit(name, model=None, **kw):
    inp = ref.inputs(name)
    args = dict(x0=inp["x0"], det=inp["det"], thresh=ref.THRESH, f_scale=ref.F_SCALE, sigma_px=ref.SIGMA_PX)
    return build.pose_fit_pixels(ref.model_of(name) if model is None else model, **dict(args, **ref.OPTS, **kw))


@functools.lru_cache(maxsize=None)
def gpu(name):
    return fit(name)


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
    N, P, L, Cn = prob.N, prob.P, prob.L, prob.C
    act = np.asarray(prob.ACT)
    assert st.dtype == got["iters"].dtype == got["pinned"].dtype == np.uint8 and got["n_detections"].dtype == np.uint16
    assert x.shape == (N, P) and got["x_full"].shape == (N, prob.P_full) and got["cov_x"].shape == (N, P, P)
    assert got["weight"].shape == (N, Cn, L, 2) and got["positions"].shape == (N, L, 3)
    assert got["cov_positions"].shape == (N, L, 3, 3) and got["std_positions"].shape == (N, L)
    assert np.array_equal(got["n_detections"], prob.n_markers)
    assert np.array_equal(st == 2, want["status"] == 2)
    gone = st >= 2
    for key in ("x", "positions", "cost", "cov_x", "cov_positions", "std_positions", "weight"):
        flat = np.isnan(got[key]).reshape(N, -1)
        assert np.array_equal(flat.all(1), gone) and np.array_equal(flat.any(1), gone), key
    assert np.array_equal(got["x_full"][:, act], x, equal_nan=True)
    assert (np.delete(got["x_full"], act, axis=1)[~gone] == 0).all() and (got["pinned"][gone] == 0).all()
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
    assert ((x[back] >= prob.lo[back]) & (x[back] <= prob.hi[back])).all()
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
    xs = np.where(back[:, None], x, prob.x0)
    rule = prob.active_set(xs, g, obj["A"])
    clear = (np.abs(g) > 1e-9 * diag) | (g == 0.0)
    at_bound = back[:, None] & ((xs <= prob.lo) | (xs >= prob.hi))
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
    """cov_x and cov_positions against inv(A_free) and G cov_x G^T of the reference at the GPU's x, to 1e-12 cond(A_free) times
    the largest entry; symmetric bit for bit; pinned rows and columns exactly 0; std_positions by the trace rule; positions."""
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


def test_a_frame_one_camera_sees_has_a_pose(gpu_lib):
    """The capability on pt16-two: in the frames where camera 1 is blind the triangulation gives no point and the 3-D fit no
    pose; the pixel fit converges."""
    model, prob = ref.model_of("pt16-two"), ref.solved("pt16-two")["prob"]
    blind = ~prob.valid[:, 1].any(1)
    assert blind.sum() == 8
    tri = build.model_triangulation(model)
    assert not np.isfinite(tri["points"].cpu().numpy()[blind]).any()
    first = build.pose_fit(model, tri, return_cov=False)
    assert (first["status"].cpu().numpy()[blind] == 2).all()
    got = gpu("pt16-two")
    assert (got["status"][blind] == 0).all() and (got["n_detections"][blind] >= 2).all()


def test_one_camera_has_a_pose(gpu_lib):
    got = gpu("generic-mono")
    assert (got["status"] == 0).all() and (got["n_detections"] >= 2).all()
    with pytest.raises(ValueError, match="x0"):
        build.pose_fit_pixels(ref.model_of("generic-mono"), **ref.OPTS)          # no start without a triangulated slot


def test_translating_the_rig_translates_the_root(gpu_lib):
    """t_c -> t_c - R_c d with the start's root and the root's box + d: the root moves by d and nothing else does, every
    floating-point output to 1e-11 (absolute, the measure of tests/test_gpu_pose_fit_px.py) and every integer output exactly.
    cov_x is the tight one: cond(A_free) = 1.5e5 stands between the rounding of the translation and it;
    tests/test_skel_pose_fit_px_host.py holds the reference's own inv(A_free) to 0.5e-11 under the same translations."""
    name = "generic-fisheye"
    inp, base = ref.inputs(name), gpu(name)
    K, D, R, t = inp["rig"]
    assert (base["status"] == 0).all()
    worst = {}
    for d in (np.array([1.0, 0.0, 0.0]), np.array([0.0, -2.0, 0.5]), np.array([0.3, -0.5, 0.8])):
        model = ref.model_of(name)
        model.t = (np.asarray(t, dtype=np.float64).reshape(len(K), 3) - np.einsum("cij,j->ci", R, d)).reshape(np.shape(t))
        model.lo, model.hi, x0d = model.lo.copy(), model.hi.copy(), inp["x0"].copy()
        for a in (model.lo, model.hi, x0d):
            a[:, :3] += d
        moved = fit(name, model, x0=x0d)
        err = {"root": np.abs(moved["x"][:, :3] - d - base["x"][:, :3]).max(), "x": np.abs(moved["x"][:, 3:] - base["x"][:, 3:]).max(),
               "positions": np.abs(moved["positions"] - d - base["positions"]).max()}
        for key in ("cost", "cov_x", "cov_positions", "std_positions", "weight"):
            err[key] = np.abs(moved[key] - base[key]).max()
        print(f"d = {d}: " + ", ".join(f"{k} {v:.2e}" for k, v in err.items()))
        for key in ("n_detections", "status", "iters", "pinned"):
            assert np.array_equal(moved[key], base[key]), key
        worst = {k: max(v, worst.get(k, 0.0)) for k, v in err.items()}
    assert {k: v for k, v in worst.items() if not v <= 1e-11} == {}


def test_default_detections_are_the_models_own(gpu_lib):
    """det=None reads [model.meas, model.weights > 0] and sigma_px=None 1 / max(model.weights): the explicit call, bit for bit."""
    name = "generic-pushed"
    inp = ref.inputs(name)
    own = build.pose_fit_pixels(ref.model_of(name), inp["x0"], **ref.OPTS)
    explicit = gpu(name)
    for key in KEYS:
        assert np.array_equal(own[key], explicit[key], equal_nan=True), key


def test_default_start_is_the_chain_of_triangulation_and_3d_fit(gpu_lib):
    """x0=None: model_triangulation, pose_fit without covariances, fill_unfitted_frames with the psi columns, the clip - bit
    for bit."""
    name = "generic-pushed"
    model = ref.model_of(name)
    act = np.asarray(model.active)
    first = build.pose_fit(model, build.model_triangulation(model), return_cov=False)
    fitted = first["status"].cpu().numpy() < 2
    assert (~fitted).sum() == 1
    psi = [int(c) for c in np.nonzero(act >= 3 + 2 * model.prog["n_angles"])[0]]
    x0 = np.clip(build.fte.fill_unfitted_frames(first["x"].cpu().numpy(), fitted, psi_columns=psi), model.lo[:, act], model.hi[:, act])
    chain = build.pose_fit_pixels(model, x0, **ref.OPTS)
    default = build.pose_fit_pixels(model, **ref.OPTS)
    for key in KEYS:
        assert np.array_equal(default[key], chain[key], equal_nan=True), key
    assert (default["status"] == 2).sum() == 1 and (default["status"] == 0).sum() >= 0.9 * (len(x0) - 1)


def test_grid_stride_beyond_the_grid_cap(gpu_lib):
    """2048 + 300 frames, a tiled 64-frame block with a validity pattern of its own in every frame: frame i is frame i mod 64,
    bit for bit on every output - and the same bits from a second launch of other dimensions."""
    name = "pt32-three"
    inp = ref.inputs(name)
    tile = lambda a, n: np.tile(a, (n // len(a) + 1,) + (1,) * (a.ndim - 1))[:n].copy()
    det = tile(inp["det"], 64)
    det[..., 2][np.random.default_rng(1).random(det.shape[:3]) < 0.25] = 0.0          # a quarter of the detections, seeded
    patterns = {tuple((p[..., 2] > ref.THRESH).ravel()) for p in det}
    assert len(patterns) == 64
    base = ref.model_of(name)

    def run(n, tensors):
        model = ref.model_of(name)
        model.lo, model.hi = tile(tile(base.lo, 64), n), tile(tile(base.hi, 64), n)
        model.meas, model.weights = np.zeros((n,) + base.meas.shape[1:]), np.zeros((n,) + base.weights.shape[1:])
        d, x0 = tile(det, n), tile(tile(inp["x0"], 64), n)
        if tensors:
            d, x0 = torch.as_tensor(d, device="cuda"), torch.as_tensor(x0, device="cuda")
        return build.pose_fit_pixels(model, x0, d, thresh=ref.THRESH, f_scale=ref.F_SCALE, sigma_px=ref.SIGMA_PX, **ref.OPTS)

    n = 2048 + 300
    out, first = run(n, True), run(64, False)
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
    name = "shipped-pinhole-pushed"
    inp = ref.inputs(name)
    assert inp["model"] == "pinhole"
    dev = torch.device("cuda", torch.cuda.current_device())
    out = fit(name, det=torch.as_tensor(inp["det"], device=dev), x0=torch.as_tensor(inp["x0"], device=dev), return_cov=False)
    assert set(out) == {"x", "x_full", "positions", "cost", "n_detections", "status", "iters", "pinned", "weight"}
    for key, val in out.items():
        assert isinstance(val, torch.Tensor) and val.device == dev, key
    host = gpu(name)
    for key, val in out.items():
        assert isinstance(host[key], np.ndarray) and np.array_equal(val.cpu().numpy(), host[key], equal_nan=True), key
