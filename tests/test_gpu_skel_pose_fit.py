"""Per-frame skeleton pose fit on the GPU (build.pose_fit, k_skel_pose_fit) against the numpy reference of
tests/skel_pose_fit_ref.py, on the synthetic inputs that file defines (tests/test_skel_pose_fit_host.py holds the reference to
central differences and to its optimality conditions, and the inputs to the conditions relied on here).  The fits run at
prior_sigma = 1.0, max_iter = 255 (ref.FIT): under the defaults the flat valleys of poorly observed angles leave a quarter of the
frames on status 1.

The solution is held by delta(x) = sqrt(g_free^T A_free^-1 g_free) of the GPU's point, evaluated by the reference with its own
active-set rule: at most B = 10 x the largest delta the reference's solver reaches on its status-0 frames of the same input
(both stop on a relative decrease and may stop a step apart).  The definitions - cov_x, cov_positions - are held at the GPU's
own x to 1e-12 cond(A_free): the rounding of a Cholesky inverse times a margin of about 1e3 for the Jacobian arithmetic.

Measured on the MI355X (profiles/skel_pose_fit/pytest_gpu_skel_pose_fit.txt): delta of the GPU's points 3.22e-04 (shipped),
3.51e-04 (generic), 3.98e-05 (pt16), 3.35e-04 (pt32), 1.96e-04 (p51) - the reference's own figures to three digits but on shipped
(3.36e-04) and p51 (1.33e-03), B ten times the reference's; status 0 on 20, 22, 22, 21, 22 of 23 frames, as the reference; the
reference's trial count on every frame but two of shipped and one of p51 (205 trials for 175); distance to the reference's
minimiser at most 3.2e-04 (p51); cov_x and cov_positions within 1.4e-04 of their bounds; no marginal entry of the active set; the
translation moves x by at most 9.2e-14 and cov_x by 9.9e-13; the isotropic form equals cov = s^2 I bit for bit."""
import functools

import numpy as np
import pytest
import torch

import skel_pose_fit_ref as ref
import skel_sample_cases as scases
from acinoset_amd import build

pytestmark = pytest.mark.gpu

FLOATS = ("x", "x_full", "positions", "cost", "cov_x", "cov_positions", "std_positions")
KEYS = FLOATS + ("n_markers", "status", "iters", "pinned")


def model_of(sk, lo, hi):
    """A SkeletonModel for the pose fit alone: the link program, the active states and the box [N, n_active] of an input."""
    prog = build.skeleton.compile_skeleton(sk)
    act = build.active_states(sk)
    n, P = len(lo), 3 + 3 * prog["n_angles"]
    lo_f, hi_f = np.full((n, P), -np.inf), np.full((n, P), np.inf)
    lo_f[:, act], hi_f[:, act] = lo, hi
    return build.SkeletonModel(skel=sk, prog=prog, names=prog["names"], active=act, lo=lo_f, hi=hi_f, meas=np.zeros((n, 1, len(prog["names"]), 2)),
                               weights=np.zeros((n, 1, len(prog["names"]))), h=1.0 / 120.0, model_weight=0.002, loss="l1")


@functools.lru_cache(maxsize=None)
def model(name):
    inp = ref.inputs(name)
    return model_of(inp["skel"], inp["lo"], inp["hi"])


def fit(name, points=None, cov="input", **kw):
    inp = ref.inputs(name)
    return build.pose_fit(model(name), inp["points"] if points is None else points, inp["cov"] if isinstance(cov, str) else cov,
                          **dict(ref.FIT, **kw))


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
    want, got = ref.solved(name), gpu(name)
    prob, x, st = want["prob"], got["x"], got["status"]
    N, P, L, act = prob.N, prob.P, prob.L, prob.ACT
    assert got["n_markers"].dtype == st.dtype == got["iters"].dtype == got["pinned"].dtype == np.uint8
    assert all(got[k].dtype == np.float64 for k in FLOATS)
    assert x.shape == (N, P) and got["x_full"].shape == (N, prob.P_full) and got["cov_x"].shape == (N, P, P)
    assert got["positions"].shape == (N, L, 3) and got["cov_positions"].shape == (N, L, 3, 3) and got["std_positions"].shape == (N, L)
    assert got["cost"].shape == st.shape == got["iters"].shape == (N,) and got["pinned"].shape == (N, P)
    assert np.array_equal(got["n_markers"], prob.n_markers)
    assert np.array_equal(st == 2, want["status"] == 2) and np.array_equal(np.nonzero(st == 2)[0], [3])
    gone = st >= 2
    for key in ("x", "positions", "cost", "cov_x", "cov_positions", "std_positions"):
        flat = np.isnan(got[key]).reshape(N, -1)
        assert np.array_equal(flat.all(1), gone) and np.array_equal(flat.any(1), gone), key
    assert np.array_equal(got["x_full"][:, act], x, equal_nan=True)
    assert (np.delete(got["x_full"], act, axis=1)[~gone] == 0).all() and (got["pinned"][gone] == 0).all()
    has = prob.n_markers >= 1
    print(f"{name}: status 0 on {(st == 0).sum()} of {has.sum()}, 1 on {(st == 1).sum()}, 3 on {(st == 3).sum()}; trials "
          f"{got['iters'][has].min()}..{got['iters'].max()} (reference {want['iters'][has].min()}..{want['iters'].max()}); "
          f"{(got['iters'] == want['iters']).sum()} of {N} frames with the reference's trial count")
    assert (st == 0).sum() >= 0.8 * has.sum()
    assert (got["iters"][gone & ~has] == 0).all()
    back = st < 2
    obj = at_gpu_point(name)
    F0 = prob.objective(prob.x0, need_jac=False)["F"]
    assert (obj["F"][back] <= F0[back]).all()
    # (a whitened residual carries the rounding of a position of metres over a sigma of centimetres, ~1e-13: a frame whose one
    #  point is met exactly has a cost of that size squared, hence the absolute term)
    assert np.allclose(got["cost"][back], obj["F"][back], rtol=1e-10, atol=1e-12)
    assert ((x[back] >= prob.lo[back]) & (x[back] <= prob.hi[back])).all()
    B = ref.bound(name)
    delta = prob.delta(x, obj)
    print(f"{name}: delta max {np.nanmax(delta[st == 0]):.2e} (reference {B / 10:.2e}, bound B {B:.2e})")
    assert (delta[st == 0] <= B).all()
    both = (st == 0) & (want["status"] == 0)
    dx = (x - want["x"])[both]
    dist = np.sqrt(np.einsum("ni,nij,nj->n", dx, want["obj"]["A"][both], dx))
    print(f"{name}: A-norm distance to the reference's minimiser max {dist.max():.2e} (bound {2 * B:.2e})")
    assert (dist <= 2 * B).all()
    # the active set: the reference's rule at the GPU's x, wherever the gradient is not marginal (an exact zero - a state none
    # of whose slots enters, resting at the centre of the ridge - is not marginal: it is not pinned)
    g, diag = obj["g"], np.einsum("npp->np", obj["A"])
    xs = np.where(back[:, None], x, prob.x0)
    rule = prob.active_set(xs, g, obj["A"])
    clear = (np.abs(g) > 1e-9 * diag) | (g == 0.0)
    at_bound = back[:, None] & ((xs <= prob.lo) | (xs >= prob.hi))
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


def test_the_states_that_move_no_pose_get_the_ridges_value_and_variance(gpu_lib):
    """The shipped skeleton as it stands: the psi angles of "chin" and "hip2" end at m with cov_x[p, p] = prior_sigma^2."""
    got, prob = gpu("shipped"), ref.solved("shipped")["prob"]
    dead = [int(np.nonzero(prob.ACT == s)[0][0]) for s in (33, 43)]
    back = got["status"] < 2
    assert np.array_equal(got["x"][back][:, dead], prob.m[back][:, dead]) and (got["pinned"][back][:, dead] == 0).all()
    var = got["cov_x"][back][:, dead, dead]
    print(f"variance of the two states that move no pose: {var.min():.15f} .. {var.max():.15f} (prior_sigma^2 = 1)")
    assert np.abs(var - ref.FIT["prior_sigma"] ** 2).max() <= 1e-12


def test_translating_the_points_translates_the_root(gpu_lib):
    """On "pt16" with every slot present (a blanked slot is put back at the truth's pose): a frame that lacks slots has a
    valley along the angles they would have held, and the end point moves along it by the rounding of the translated points -
    2e-16 x 3 m over a sigma of 5 mm, 1e-13 in a whitened residual - times cond(A_free), 1e5 there (2.7e-09 measured on the
    input as it stands); with every slot the reference itself moves by 2e-13.  Offsets without a z component: z has a bound
    (build.bounds_table), and a third of the truth states sit on it."""
    inp = ref.inputs("pt16")
    pts = np.where(np.isnan(inp["points"]), inp["truth_pos"], inp["points"])
    x0 = ref.Problem(inp["skel"], pts, inp["cov"], inp["lo"], inp["hi"], **ref.FIT).x0
    base = fit("pt16", points=pts, x0=x0)
    assert (base["status"] == 0).all()
    for d in (np.array([1.0, 0.0, 0.0]), np.array([0.0, -2.0, 0.0]), np.array([0.3, -0.5, 0.0])):
        x0d = x0.copy()
        x0d[:, :3] += d
        moved = fit("pt16", points=pts + d, x0=x0d)
        err = {"root": np.abs(moved["x"][:, :3] - d - base["x"][:, :3]).max(), "x": np.abs(moved["x"][:, 3:] - base["x"][:, 3:]).max(),
               "positions": np.abs(moved["positions"] - d - base["positions"]).max()}
        for key in ("cost", "cov_x", "cov_positions", "std_positions"):
            err[key] = np.abs(moved[key] - base[key]).max()
        print(f"d = {d}: " + ", ".join(f"{k} {v:.1e}" for k, v in err.items()))
        assert max(err.values()) <= 1e-11
        for key in ("n_markers", "status", "iters", "pinned"):
            assert np.array_equal(moved[key], base[key]), key


def test_isotropic_form_is_a_covariance_of_sigma_iso_squared(gpu_lib):
    """cov=None, sigma_iso=s against cov = s^2 I: every output within 1e-12 of its largest entry, on the frames both return."""
    pts = ref.inputs("pt16")["points"]
    s = 0.02
    iso = fit("pt16", cov=None, sigma_iso=s)
    full = fit("pt16", cov=np.broadcast_to(s * s * np.eye(3), pts.shape[:2] + (3, 3)).copy(), sigma_iso=123.0)
    assert np.array_equal(iso["n_markers"], np.isfinite(pts).all(-1).sum(1))
    back = iso["status"] < 2
    assert np.array_equal(back, full["status"] < 2) and back.sum() == 23
    for key in FLOATS:
        err = np.abs(iso[key][back] - full[key][back]).max() / np.abs(full[key][back]).max()
        print(f"{key}: {err:.2e}")
        assert err <= 1e-12, key
    for key in ("n_markers", "status", "pinned"):
        assert np.array_equal(iso[key], full[key]), key


def test_a_callers_start_equal_to_the_default_start_changes_nothing(gpu_lib):
    """The kernel's own start is what a call whose single trial is refused returns (lam0 = 1e300: a step of 1e-300 leaves F
    where it is); handed back as x0 it gives the output of the default call bit for bit.  It is the reference's default start."""
    start = fit("shipped", lam0=1e300, max_iter=1, return_cov=False)
    back = start["status"] < 2
    assert (start["status"][back] == 1).all() and (start["iters"][back] == 1).all() and back.sum() == 23
    want = ref.solved("shipped")["prob"].x0
    print(f"default start against the reference's: {np.abs(start['x'][back] - want[back]).max():.1e}")
    assert np.abs(start["x"][back] - want[back]).max() <= 1e-14 and np.array_equal(start["x"][back][:, 3:], want[back][:, 3:])
    x0 = np.where(back[:, None], start["x"], want)
    given = fit("shipped", x0=x0)
    for key in KEYS:
        assert np.array_equal(given[key], gpu("shipped")[key], equal_nan=True), key


def test_grid_stride_beyond_the_grid_cap(gpu_lib):
    """2048 + 300 frames, a tiled 64-frame block of "pt32" with a slot pattern of its own in every frame: frame i is frame
    i mod 64, bit for bit."""
    inp = ref.inputs("pt32")
    sk, P = inp["skel"], inp["lo"].shape[1]
    pts, cov = np.tile(inp["points"], (3, 1, 1))[:64].copy(), np.tile(inp["cov"], (3, 1, 1, 1))[:64].copy()
    pts[np.random.default_rng(1).random(pts.shape[:2]) < 0.25] = np.nan              # a quarter of the slots, seeded
    lo, hi = np.tile(inp["lo"][:1], (64, 1)), np.tile(inp["hi"][:1], (64, 1))        # the same box in every frame
    n = 2048 + 300
    tile = lambda a: np.tile(a, (n // 64 + 1,) + (1,) * (a.ndim - 1))[:n]
    rep = lambda a: torch.as_tensor(tile(a), device="cuda")
    out = build.pose_fit(model_of(sk, tile(lo), tile(hi)), rep(pts), rep(cov), **ref.FIT)
    first = build.pose_fit(model_of(sk, lo, hi), pts, cov, **ref.FIT)
    has = np.isfinite(pts).all(-1).any(1)
    print(f"64-frame block: status 0 on {(first['status'] == 0).sum()} of {has.sum()}, {len(set(first['iters'].tolist()))} distinct trial counts")
    assert len(set(first["iters"].tolist())) >= 4
    assert len({tuple(np.isfinite(p).all(-1)) for p in pts}) >= 32
    idx = torch.arange(n, device="cuda") % 64
    for key in KEYS:
        a = out[key]
        assert a.shape[0] == n
        same = a.view(torch.int64) == a[:64][idx].view(torch.int64) if a.dtype == torch.float64 else a == a[:64][idx]
        assert bool(same.all()), key
        w = torch.as_tensor(first[key], device="cuda")
        assert bool((a[:64].view(torch.int64) == w.view(torch.int64)).all() if a.dtype == torch.float64 else (a[:64] == w).all()), key


def test_tensors_in_tensors_out(gpu_lib, golden_dir):
    """The dict of model_triangulation in place of points and cov, on the device from the model's detections to the pose."""
    m = scases.case(golden_dir, "pt16")["model"]
    dev = torch.device("cuda", torch.cuda.current_device())
    tri = build.model_triangulation(m)
    assert isinstance(tri["points"], torch.Tensor) and tri["points"].shape == (12, 6, 3) and tri["cov"].shape == (12, 6, 3, 3)
    out = build.pose_fit(m, tri, return_cov=False)
    assert set(out) == {"x", "x_full", "positions", "cost", "n_markers", "status", "iters", "pinned"}
    for key, val in out.items():
        assert isinstance(val, torch.Tensor) and val.device == dev, key
    assert out["x"].shape == (12, 15) and out["x_full"].shape == (12, m.P) and out["positions"].shape == (12, 6, 3)
    host = build.pose_fit(m, tri["points"].cpu().numpy(), tri["cov"].cpu().numpy())
    for key, val in out.items():
        assert isinstance(host[key], np.ndarray) and np.array_equal(val.cpu().numpy(), host[key], equal_nan=True), key
    assert np.array_equal(out["n_markers"].cpu().numpy(), (tri["status"] < 2).sum(1).cpu().numpy())
    assert (out["status"].cpu().numpy() < 2).any()
    with pytest.raises(ValueError):
        build.pose_fit(m, tri, cov=tri["cov"])


def test_pose_fit_start_of_the_solve(gpu_lib, golden_dir):
    """init="pose_fit" is pose_fit_start and nothing else; the start lies in the box, 0 outside the active states."""
    m = scases.case(golden_dir, "pt16")["model"]
    act = np.asarray(m.active)
    x_fit = build.pose_fit_start(m)
    assert x_fit.shape == (12, m.P) and (np.delete(x_fit, act, axis=1) == 0).all() and np.isfinite(x_fit).all()
    assert ((x_fit >= m.lo) & (x_fit <= m.hi))[:, act].all()
    res, info = build.solve_model(m, init="pose_fit", max_iter=30)
    res_x0, info_x0 = build.solve_model(m, x0=x_fit, max_iter=30)
    print(f"12-frame pt16 model from the pose-fit start: {info['iterations']} iterations, cost {info['cost_initial']:.3f} -> "
          f"{info['cost_final']:.3f}, status {info['status_name']}")
    assert np.array_equal(res["x"], res_x0["x"]) and np.array_equal(res["positions"], res_x0["positions"])
    assert info["iterations"] == info_x0["iterations"] and info["cost_final"] == info_x0["cost_final"]
    with pytest.raises(ValueError, match="'line' or 'pose_fit'"):
        build.solve_model(m, init="bogus")
