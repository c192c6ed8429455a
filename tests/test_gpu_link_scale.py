"""Link-scale fit on the GPU (build.link_scale_system, build.fit_link_scales, k_skel_link_scale) against the numpy reference
of tests/link_scale_ref.py, on the inputs of tests/skel_pose_fit_ref.py (24 frames: one with every slot, one with slot 0 alone,
one with three slots, one with none; ~10 bound-active entries) and on their scaled-truth variant (link_scale_ref.scaled_inputs,
seed link_scale_ref.SEED; test_link_scale_host.py holds the CPU driver alone to the 4-bar condition on it).

The per-frame outputs are compared at the device's own x and pinned.  The bar comes from the reference: evaluated in fp64 and in
np.longdouble, 256 times their difference (the convention of test_gpu_fte_step_reference), floored at 256 eps times the magnitude
of the terms each entry sums - for what is linear in a residual, with |pose| + |point| in place of the residual, since the
residual of centimetres is a difference of metres."""
import functools

import numpy as np
import pytest

import link_scale_ref as lref
import skel_pose_fit_ref as pref
from acinoset_amd import build, calib

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
THETAS = {"unit": 0.0, "off": 1.0}       # the scales of "off": exp(0.1 cos(1 + 2 g)), up to 10 % from the points' skeleton


def model_of(sk, lo, hi, **more):
    prog = build.skeleton.compile_skeleton(sk)
    act = build.active_states(sk)
    n, P = len(lo), 3 + 3 * prog["n_angles"]
    lo_f, hi_f = np.full((n, P), -np.inf), np.full((n, P), np.inf)
    lo_f[:, act], hi_f[:, act] = lo, hi
    kw = dict(skel=sk, prog=prog, names=prog["names"], active=act, lo=lo_f, hi=hi_f, meas=np.zeros((n, 1, len(prog["names"]), 2)),
              weights=np.zeros((n, 1, len(prog["names"]))), h=1.0 / 120.0, model_weight=0.002, loss="l1")
    return build.SkeletonModel(**dict(kw, **more))


@functools.lru_cache(maxsize=None)
def model(name):
    inp = pref.inputs(name)
    return model_of(inp["skel"], inp["lo"], inp["hi"])


def groups(name):
    return lref.groups_of(pref.inputs(name)["skel"], lref.GROUPS[name])


@functools.lru_cache(maxsize=None)
def run(name, which):
    """The device's system at the device's own pose fit, and the reference there in both precisions."""
    grp, K = groups(name)
    scales = np.exp(0.1 * THETAS[which] * np.cos(1.0 + 2.0 * np.arange(K)))
    inp = pref.inputs(name)
    prob = lref.problem(name, scales=scales)
    mdl = build.scale_links(model(name), scales, grp)
    fit = build.pose_fit(mdl, inp["points"], inp["cov"], x0=prob.x0, return_cov=False, **pref.FIT)
    got = build.link_scale_system(mdl, inp["points"], inp["cov"], fit, grp, prior_sigma=pref.FIT["prior_sigma"], m=prob.x0)
    refs = [lref.system(prob, fit["x"], fit["pinned"], fit["status"], dt) for dt in (np.float64, np.longdouble)]
    return dict(prob=prob, fit=fit, got=got, ref64=refs[0], ref80=refs[1], K=K)


@pytest.mark.parametrize("which", tuple(THETAS))
@pytest.mark.parametrize("name", lref.NAMES)
def test_per_frame_outputs(gpu_lib, name, which):
    r = run(name, which)
    got, r64, r80, fit = r["got"], r["ref64"], r["ref80"], r["fit"]
    N, P, K = r["prob"].N, r["prob"].P, r["K"]
    assert got["S_frames"].shape == (N, K, K) and got["r_frames"].shape == (N, K) and got["sens"].shape == (N, P, K)
    assert got["cost_frames"].shape == got["used"].shape == got["status"].shape == (N,)
    assert np.array_equal(got["used"], r64["used"]) and np.array_equal(got["used"], fit["status"] < 2)
    assert np.array_equal(got["status"], fit["status"]) and got["n_used"] == 23
    used = got["used"]
    assert np.allclose(got["cost_frames"][used], fit["cost"][used], rtol=1e-12, atol=1e-12)
    worst = {}
    for key, mag in (("S_frames", "mag_S"), ("r_frames", "mag_r"), ("cost_frames", "mag_F"), ("sens", "mag_sens")):
        err = np.abs(got[key][used].astype(np.longdouble) - r80[key][used])
        bar = np.maximum(np.abs(r64[key][used].astype(np.longdouble) - r80[key][used]), EPS * r80[mag][used])
        ratio = np.where(err == 0, 0.0, err / np.where(bar > 0, bar, 1e-300)).astype(np.float64)
        worst[key] = float(ratio.max())
    rel = np.abs(r80["r_frames"][used]).max() / np.abs(r80["mag_r"][used]).max()
    print(f"{name} {which}: error / bar (allowed 256) " + ", ".join(f"{k} {v:.1f}" for k, v in worst.items()) +
          f"; |r| max {float(np.abs(got['r_frames']).max()):.2e}, |S| max {float(np.abs(got['S_frames']).max()):.2e}, r / its terms {float(rel):.1e}")
    if which == "off":
        assert np.abs(got["r_frames"]).max() > 1.0           # far from 0: the scales do not fit the points
    assert max(worst.values()) <= 256.0, worst


@pytest.mark.parametrize("name", lref.NAMES)
def test_exact_facts(gpu_lib, name):
    r = run(name, "off")
    got, prob, fit = r["got"], r["prob"], r["fit"]
    S, rr, sens = got["S_frames"], got["r_frames"], got["sens"]
    # the frame without a slot
    assert not got["used"][3] and got["status"][3] == 2 and (S[3] == 0).all() and (rr[3] == 0).all() and got["cost_frames"][3] == 0
    assert np.isnan(sens[3]).all() and np.isfinite(sens[got["used"]]).all()
    # groups no entering slot hangs on: an exact zero row and column (frame 1 has the root's slot alone: every group)
    D = lref.dpos_dtheta(prob, np.where(np.isfinite(fit["x"]), fit["x"], prob.x0))
    count = 0
    for n in np.nonzero(got["used"])[0]:
        hangs = np.abs(D[n][prob.enter[n]]).max(axis=(0, 1)) > 0
        for g in np.nonzero(~hangs)[0]:
            assert (S[n, g, :] == 0).all() and (S[n, :, g] == 0).all() and rr[n, g] == 0 and (sens[n, :, g] == 0).all()
            count += 1
    assert count >= r["K"] and (S[1] == 0).all()
    assert np.array_equal(S, S.transpose(0, 2, 1))
    pinned = 0
    for which in THETAS:                         # (at the scales 1 the fit pins what the reference pins: at least one entry)
        pin = run(name, which)["fit"]["pinned"].astype(bool)
        assert (run(name, which)["got"]["sens"][pin] == 0).all()
        pinned += int(pin.sum())
    assert pinned >= 1
    print(f"{name}: {count} (frame, group) pairs without an entering slot, {pinned} pinned entries")


@pytest.mark.parametrize("name", ("shipped", "p51"))
def test_totals_are_the_in_order_sums(gpu_lib, name):
    got = run(name, "off")["got"]
    K = run(name, "off")["K"]
    S, rr, F = np.zeros((K, K)), np.zeros(K), 0.0
    for n in range(len(got["used"])):
        S, rr, F = S + got["S_frames"][n], rr + got["r_frames"][n], F + got["cost_frames"][n]
    assert np.array_equal(got["S"], S) and np.array_equal(got["r"], rr) and got["cost"] == F and got["n_used"] == got["used"].sum()
    assert np.array_equal(got["S"], got["S"].T)


def test_sixteen_groups_on_51_states(gpu_lib):
    """p51 with the op index mod 16 as groups: K = 16, P + K = 67 > 64, so the columns 64 .. 66 of [Jw Js] - c of the groups 13,
    14 and 15 - are summed by the lanes 0 .. 2 in a second round.  A kernel that sums one column per lane leaves those three
    entries of c as the LDS held them and r_n of these groups off by the whole of c."""
    inp = pref.inputs("p51")
    grp, K = lref.groups_of(inp["skel"], np.arange(len(lref.base_offsets(inp["skel"]))) % 16)
    scales = np.exp(0.1 * np.cos(1.0 + 2.0 * np.arange(K)))
    prob = lref.ScaledProblem(inp["skel"], inp["points"], inp["cov"], inp["lo"], inp["hi"], groups=grp, scales=scales, **pref.FIT)
    assert K == 16 and prob.P + K == 67 and prob.N == 24
    mdl = build.scale_links(model("p51"), scales, grp)
    fit = build.pose_fit(mdl, inp["points"], inp["cov"], x0=prob.x0, return_cov=False, **pref.FIT)
    got = build.link_scale_system(mdl, inp["points"], inp["cov"], fit, grp, prior_sigma=pref.FIT["prior_sigma"], m=prob.x0)
    r64, r80 = [lref.system(prob, fit["x"], fit["pinned"], fit["status"], dt) for dt in (np.float64, np.longdouble)]
    used = got["used"]
    assert np.array_equal(used, r64["used"]) and used.sum() == 23
    worst = {}
    for key, mag in (("S_frames", "mag_S"), ("r_frames", "mag_r"), ("sens", "mag_sens")):
        err = np.abs(got[key][used].astype(np.longdouble) - r80[key][used])
        bar = np.maximum(np.abs(r64[key][used].astype(np.longdouble) - r80[key][used]), EPS * r80[mag][used])
        worst[key] = float(np.where(err == 0, 0.0, err / np.where(bar > 0, bar, 1e-300)).astype(np.float64).max())
    print("p51, 16 groups: error / bar (allowed 256) " + ", ".join(f"{k} {v:.1f}" for k, v in worst.items()) +
          f"; |r| of the groups 13 .. 15 max {float(np.abs(got['r_frames'][:, 13:]).max()):.2e}")
    assert np.abs(r80["r_frames"][:, 13:]).max() > 1.0          # (what the three entries carry is far from 0)
    assert max(worst.values()) <= 256.0, worst
    rr = np.zeros(K)
    for n in range(prob.N):
        rr = rr + got["r_frames"][n]
    assert np.array_equal(got["r"], rr)


def test_without_sens_and_total_the_frames_get_the_same_bits(gpu_lib):
    """acino_skel_link_scale with d_sens = NULL and d_total = NULL: S, r, F, used and frame_status as the full call writes them."""
    import ctypes as C

    import torch
    from acinoset_amd._lib import check, lib, ptr, stream_ptr
    r, inp = run("pt16", "off"), pref.inputs("pt16")
    grp, K = groups("pt16")
    mdl = build.scale_links(model("pt16"), np.exp(0.1 * np.cos(1.0 + 2.0 * np.arange(K))), grp)
    act = np.asarray(mdl.active, dtype=np.int32)
    N, dev = r["prob"].N, calib._dev()
    assert N == 24
    p = build._skel_params(mdl, len(act))
    nbytes = lib().acino_skel_link_scale_workspace_bytes(C.byref(p))
    f64 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=dev)      # noqa: E731
    u8 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.uint8), device=dev)         # noqa: E731
    ins = [f64(inp["points"]), f64(inp["cov"]), f64(r["fit"]["x"]), f64(r["prob"].x0), u8(r["fit"]["pinned"]), u8(r["fit"]["status"])]
    outs = [torch.full(shape, 7, dtype=dt, device=dev) for shape, dt in (((N, K, K), torch.float64), ((N, K), torch.float64),
                                                                         ((N,), torch.float64), ((N,), torch.uint8), ((N,), torch.uint8))]
    ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=dev)
    check(lib().acino_skel_link_scale(C.byref(p), build._ops_array(mdl.prog), (C.c_int32 * len(act))(*[int(a) for a in act]),
                                      (C.c_int32 * len(grp))(*[int(g) for g in grp]), K, pref.FIT["prior_sigma"], 0.01,
                                      *[ptr(t) for t in ins], N, *[ptr(t) for t in outs], None, None,
                                      C.c_void_p((ws.data_ptr() + 255) // 256 * 256), nbytes, stream_ptr()))
    torch.cuda.synchronize()
    for t, key in zip(outs, ("S_frames", "r_frames", "cost_frames", "used", "status")):
        assert np.array_equal(t.cpu().numpy().astype(r["got"][key].dtype), r["got"][key]), key


@functools.lru_cache(maxsize=None)
def fitted(drop_slot=None):
    sc, inp = lref.scaled_inputs("pt16"), pref.inputs("pt16")
    pts = sc["points"].copy()
    if drop_slot is not None:
        pts[:, drop_slot] = np.nan
    return build.fit_link_scales(model("pt16"), pts, inp["cov"])


def test_fit_recovers_the_scaled_truth(gpu_lib):
    """pt16, seed link_scale_ref.SEED: status ok, the cost never rises, every group within 4 bars of the truth, and scales and
    bars equal to the CPU driver's within 10 x tol."""
    sc, out, want = lref.scaled_inputs("pt16"), fitted(), lref.fitted("pt16")
    z = (out["scales"] - sc["factors"]) / out["std_scales"]
    costs = [h["cost"] for h in out["history"]]
    print(f"factors {np.round(sc['factors'], 4)}\nscales  {np.round(out['scales'], 4)} (CPU driver {np.round(want['scales'], 4)})\n"
          f"std     {np.round(out['std_scales'], 4)}; z {np.round(z, 2)}; {len(costs)} outer steps, cost {costs[0]:.3f} -> {costs[-1]:.3f}; "
          f"to the CPU driver: scales {np.abs(out['scales'] - want['scales']).max():.1e}, std {np.abs(out['std_scales'] - want['std_scales']).max():.1e}")
    assert out["status"] == "ok" and all(b <= a for a, b in zip(costs, costs[1:]))
    assert out["observed"].all() and (np.abs(z) < 4.0).all()
    assert np.abs(out["scales"] - want["scales"]).max() <= 1e-5 and np.abs(out["std_scales"] - want["std_scales"]).max() <= 1e-5
    assert np.array_equal(out["model"].link_scales, out["scales"]) and not hasattr(model("pt16"), "link_scales")
    assert np.allclose(out["cov_log_scales"], out["cov_log_scales"].T) and out["fit"]["x"].shape == (24, 15)


def test_an_unobserved_group_stays_at_one(gpu_lib):
    """Every point below one link removed in all frames: the link's group is not observed, keeps the scale 1 and has no bar;
    the others are the reference's with that group fixed."""
    prog = model("pt16").prog
    parents = {op[1] for op in prog["ops"]}
    k = max(i for i, op in enumerate(prog["ops"]) if op[0] not in parents)          # a leaf link: only its own slot hangs on it
    slot, g = prog["ops"][k][0], int(groups("pt16")[0][k])
    out, want = fitted(slot), lref.fitted("pt16", slot)
    assert not out["observed"][g] and out["scales"][g] == 1.0 and np.isinf(out["std_scales"][g]) and out["status"] == "ok"
    assert (out["cov_log_scales"][g] == 0).all() and (out["cov_log_scales"][:, g] == 0).all()
    assert (out["system"]["S"][g] == 0).all() and out["system"]["r"][g] == 0
    rest = np.arange(len(out["scales"])) != g
    assert out["observed"][rest].all() and np.array_equal(out["observed"], want["observed"])
    print(f"group {g} unobserved; the others to the reference: {np.abs(out['scales'] - want['scales']).max():.1e}")
    assert np.abs(out["scales"] - want["scales"])[rest].max() <= 1e-5 and np.abs(out["std_scales"] - want["std_scales"])[rest].max() <= 1e-5


def test_the_scaled_model_solves_to_a_lower_cost(gpu_lib):
    """solve_models on the returned model against the unscaled one, the detections being the scaled truth seen by two pinhole
    cameras 10 m from the origin.  The truth states are drawn per frame, so the smoothness weight is set to almost nothing: what
    is compared is how well either skeleton meets the pixels."""
    sc, inp = lref.scaled_inputs("pt16"), pref.inputs("pt16")
    truth = lref.problem("pt16", scales=sc["factors"]).fk(inp["truth"])
    K = np.tile(np.array([[800.0, 0.0, 640.0], [0.0, 800.0, 360.0], [0.0, 0.0, 1.0]]), (2, 1, 1))
    R = np.stack([np.eye(3), np.array([[0.0, 0.0, -1.0], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0]])])
    t, D = np.tile(np.array([[0.0], [0.0], [10.0]]), (2, 1, 1)), np.zeros((2, 5))
    N, L = truth.shape[:2]
    meas = np.stack([calib.project_points(truth.reshape(-1, 3), K[c], D[c], R[c], t[c]).reshape(N, L, 2) for c in range(2)], axis=1)
    base = model_of(inp["skel"], inp["lo"], inp["hi"], meas=meas, weights=np.full((N, 2, L), 1.0 / 3.0), K=K, D=D, R=R, t=t,
                    camera_model="pinhole", model_weight=1e-12, init_x=np.zeros((N, 3 + 3 * model("pt16").prog["n_angles"])))
    scaled = build.scale_links(base, fitted()["scales"], fitted()["groups"])
    costs = []
    for mdl in (base, scaled):
        (res, info), = build.solve_models([mdl], init="pose_fit", max_iter=100)
        assert np.isfinite(res["x"]).all() and info["status_name"] != "numeric"
        costs.append(info["cost_final"])
    print(f"solve_models cost: unscaled skeleton {costs[0]:.3f}, fitted scales {costs[1]:.3f}")
    assert costs[1] < costs[0]
