"""Link-scale fit from the detections on the GPU (build.link_scale_system_pixels, build.fit_link_scales_pixels,
k_skel_link_scale_px) against the numpy reference of tests/link_scale_px_ref.py, on inputs of tests/skel_pose_fit_px_ref.py (24
frames, 14 for p51-wide16: every PT, both camera models, 1 to 16 cameras, pushed detections, an empty frame, bound-active
states) and on the scaled-truth variant of pt16-two (link_scale_px_ref.scaled_inputs, seed link_scale_px_ref.SEED;
test_link_scale_px_host.py holds the CPU driver alone to the 4-bar condition on it).

The per-frame outputs are compared at the device's own x, pinned and status from build.pose_fit_pixels.  The bar comes from the
reference: evaluated in fp64 and in np.longdouble, 256 times their difference (the convention of test_gpu_fte_step_reference),
floored at 256 eps times the magnitude of the terms each entry sums (link_scale_px_ref: mag_*; |uv| + |det| in place of |r|)."""
import functools

import numpy as np
import pytest

import link_scale_px_ref as xref
import skel_pose_fit_px_ref as ppx
from acinoset_amd import build

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
THETAS = {"unit": 0.0, "off": 1.0}       # the scales of "off": exp(0.1 cos(1 + 2 g)), up to 10 % from the detections' skeleton
CASES = tuple((name, None) for name in xref.NAMES) + (("p51-wide16", "mod16"),)      # mod16: K = 16, P + K = 67 > 64
KEYS = (("S_frames", "S"), ("r_frames", "r"), ("cost_frames", "F"), ("sens", "sens"))


@functools.lru_cache(maxsize=None)
def run(name, which, groups=None):
    """The device's system at the device's own pixel pose fit, and the reference there in both precisions."""
    grp, K = xref.groups_for(name, groups)
    scales = np.exp(0.1 * THETAS[which] * np.cos(1.0 + 2.0 * np.arange(K)))
    prob = xref.problem(name, scales=scales, groups=groups)
    mdl = build.scale_links(ppx.model_of(name), scales, grp)
    fit = build.pose_fit_pixels(mdl, x0=prob.x0, return_cov=False, **ppx.OPTS)
    got = build.link_scale_system_pixels(mdl, fit, grp, prior_sigma=ppx.OPTS["prior_sigma"], m=prob.x0)
    refs = [xref.system(prob, fit["x"], fit["pinned"], fit["status"], dt) for dt in (np.float64, np.longdouble)]
    return dict(prob=prob, mdl=mdl, grp=grp, fit=fit, got=got, ref64=refs[0], ref80=refs[1], K=K)


def ratios(got, r64, r80, frames, exact=None):
    """Per key the worst |device - value| / max(|ref64 - ref80|, eps * magnitude) over ``frames``; value: ref80, or
    ``exact[key]`` for the keys it holds (the other keys are left out then)."""
    worst = {}
    for key, short in KEYS:
        if exact is not None and key not in exact:
            continue
        err = np.abs(got[key][frames].astype(np.longdouble) - (r80[key][frames] if exact is None else exact[key]))
        bar = np.maximum(np.abs(r64[key][frames].astype(np.longdouble) - r80[key][frames]), EPS * r80[f"mag_{short}"][frames])
        worst[key] = float(np.where(err == 0, 0.0, err / np.where(bar > 0, bar, 1e-300)).astype(np.float64).max())
    return worst


@pytest.mark.parametrize("which", tuple(THETAS))
@pytest.mark.parametrize("name,groups", CASES)
def test_per_frame_outputs(gpu_lib, name, groups, which):
    r = run(name, which, groups)
    got, r64, r80, fit = r["got"], r["ref64"], r["ref80"], r["fit"]
    N, P, K = r["prob"].N, r["prob"].P, r["K"]
    assert got["S_frames"].shape == (N, K, K) and got["r_frames"].shape == (N, K) and got["sens"].shape == (N, P, K)
    assert got["cost_frames"].shape == got["used"].shape == got["status"].shape == (N,)
    assert np.array_equal(got["used"], r64["used"]) and np.array_equal(got["used"], fit["status"] < 2)
    assert np.array_equal(got["status"], fit["status"]) and got["n_used"] == got["used"].sum() >= N - 1
    used = got["used"]
    assert np.allclose(got["cost_frames"][used], fit["cost"][used], rtol=1e-12, atol=1e-12)
    worst = ratios(got, r64, r80, used)
    print(f"{name} {groups or ''} {which} (K = {K}, P + K = {P + K}): error / bar (allowed 256) " +
          ", ".join(f"{k} {v:.1f}" for k, v in worst.items()) +
          f"; |r| max {float(np.abs(got['r_frames']).max()):.2e}, |S| max {float(np.abs(got['S_frames']).max()):.2e}")
    if which == "off":
        assert np.abs(got["r_frames"]).max() > 1.0           # far from 0: the scales do not fit the detections
    assert max(worst.values()) <= 256.0, worst


@pytest.mark.parametrize("name,groups", CASES)
def test_exact_facts(gpu_lib, name, groups):
    r = run(name, "off", groups)
    got, prob, fit = r["got"], r["prob"], r["fit"]
    S, rr, sens, used = got["S_frames"], got["r_frames"], got["sens"], got["used"]
    # a frame without a pose: zeros, used False, NaN sens
    out = np.nonzero(fit["status"] >= 2)[0]
    if ppx.inputs(name)["pushed"]:
        assert list(out) == [ppx.EMPTY_FRAME]
    for n in out:
        assert not used[n] and (S[n] == 0).all() and (rr[n] == 0).all() and got["cost_frames"][n] == 0 and np.isnan(sens[n]).all()
    assert np.isfinite(sens[used]).all() and np.isfinite(S).all() and np.isfinite(rr).all()
    # groups no valid detection hangs on: an exact zero row and column
    D = xref.dpos_dtheta(prob, np.where(np.isfinite(fit["x"]), fit["x"], prob.x0))
    count = 0
    for n in np.nonzero(used)[0]:
        seen = prob.valid[n].any(0)
        hangs = np.abs(D[n][seen]).max(axis=(0, 1)) > 0
        for g in np.nonzero(~hangs)[0]:
            assert (S[n, g, :] == 0).all() and (S[n, :, g] == 0).all() and rr[n, g] == 0 and (sens[n, :, g] == 0).all()
            count += 1
    if name == "pt16-two":
        assert count >= 1
    assert np.array_equal(S, S.transpose(0, 2, 1))
    pinned = 0
    for which in THETAS:
        pin = run(name, which, groups)["fit"]["pinned"].astype(bool)
        assert (run(name, which, groups)["got"]["sens"][pin] == 0).all()
        pinned += int(pin.sum())
    if name == "pt32-three":                     # (its box cuts the truth off in 12 frames)
        assert pinned >= 1
    print(f"{name} {groups or ''}: {count} (frame, group) pairs without a valid detection, {pinned} pinned entries, frames out {list(out)}")


@pytest.mark.parametrize("name,groups", (("shipped-pinhole-pushed", None), ("p51-wide16", "mod16")))
def test_totals_are_the_in_order_sums_and_two_calls_give_the_same_bits(gpu_lib, name, groups):
    r = run(name, "off", groups)
    got, K = r["got"], r["K"]
    S, rr, F = np.zeros((K, K)), np.zeros(K), 0.0
    for n in range(len(got["used"])):
        S, rr, F = S + got["S_frames"][n], rr + got["r_frames"][n], F + got["cost_frames"][n]
    assert np.array_equal(got["S"], S) and np.array_equal(got["r"], rr) and got["cost"] == F and got["n_used"] == got["used"].sum()
    assert np.array_equal(got["S"], got["S"].T)
    again = build.link_scale_system_pixels(r["mdl"], r["fit"], r["grp"], prior_sigma=ppx.OPTS["prior_sigma"], m=r["prob"].x0)
    for key in ("S", "r", "S_frames", "r_frames", "cost_frames", "sens", "used", "status"):
        assert np.array_equal(got[key], again[key], equal_nan=True), key
    assert got["cost"] == again["cost"]


def test_without_sens_and_total_the_frames_get_the_same_bits(gpu_lib):
    """acino_skel_link_scale_px with d_sens = NULL and d_total = NULL: S, r, F, used and frame_status as the full call writes them."""
    import ctypes as C

    import torch
    from acinoset_amd import _lib, calib
    from acinoset_amd._lib import check, lib, ptr, stream_ptr
    r = run("pt16-two", "off")
    mdl, grp, K, fit = r["mdl"], r["grp"], r["K"], r["fit"]
    act = np.asarray(mdl.active, dtype=np.int32)
    N, Cn, dev = r["prob"].N, int(np.shape(mdl.meas)[1]), calib._dev()
    assert N == 24
    p = build._skel_params(mdl, len(act))
    nbytes = lib().acino_skel_link_scale_px_workspace_bytes(C.byref(p))
    camera_model = getattr(mdl, "camera_model", "fisheye")
    prm = _lib.PoseFitPxParams(calib.CAMERAS[camera_model].code, 1, 1, 0, 1e-3, 1e-10, 1e-10, ppx.OPTS["prior_sigma"], 0.5, 5.0,
                               build._model_sigma_px(mdl))      # (the defaults of link_scale_system_pixels: what run() passed)
    f64 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=dev)      # noqa: E731
    u8 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.uint8), device=dev)         # noqa: E731
    det, cams = f64(build._model_detections(mdl)), f64(calib.camera_records(camera_model, mdl.K, mdl.D, mdl.R, mdl.t))
    ins = [f64(fit["x"]), f64(r["prob"].x0), u8(fit["pinned"]), u8(fit["status"])]
    outs = [torch.full(shape, 7, dtype=dt, device=dev) for shape, dt in (((N, K, K), torch.float64), ((N, K), torch.float64),
                                                                         ((N,), torch.float64), ((N,), torch.uint8), ((N,), torch.uint8))]
    ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=dev)
    check(lib().acino_skel_link_scale_px(C.byref(prm), C.byref(p), build._ops_array(mdl.prog), (C.c_int32 * len(act))(*[int(a) for a in act]),
                                         (C.c_int32 * len(grp))(*[int(g) for g in grp]), K, ptr(det), N, Cn, ptr(cams),
                                         *[ptr(t) for t in ins], *[ptr(t) for t in outs], None, None,
                                         C.c_void_p((ws.data_ptr() + 255) // 256 * 256), nbytes, stream_ptr()))
    torch.cuda.synchronize()
    for t, key in zip(outs, ("S_frames", "r_frames", "cost_frames", "used", "status")):
        assert np.array_equal(t.cpu().numpy().astype(r["got"][key].dtype), r["got"][key]), key


def test_mono_identity(gpu_lib):
    """One camera, one scale for every link (test_link_scale_px_host.py): S_n = 0, sens_n[:3, 0] = root - camera centre,
    sens_n[3:, 0] = 0 on the frames with a free root, within the bars of the per-frame outputs."""
    r = run("generic-mono", "unit", "global")
    got, r64, r80, prob, fit = r["got"], r["ref64"], r["ref80"], r["prob"], r["fit"]
    assert r["K"] == 1 and prob.C == 1
    frames = np.nonzero(got["used"] & ~fit["pinned"][:, :3].astype(bool).any(1))[0]
    assert len(frames) >= 12
    want = np.zeros((len(frames), prob.P, 1))
    want[:, :3, 0] = fit["x"][frames, :3] - xref.camera_centre(prob.rig)
    worst = ratios(got, r64, r80, frames, exact=dict(S_frames=np.zeros((len(frames), 1, 1)), sens=want))
    Cn = np.array([xref.frame_terms(prob, n, fit["x"])["C"][0, 0] for n in frames])
    print(f"generic-mono, global, {len(frames)} frames: |S_n| / C_n {np.abs(got['S_frames'][frames, 0, 0] / Cn).max():.2e}; to the exact "
          f"values, error / bar (allowed 256): " + ", ".join(f"{k} {v:.1f}" for k, v in worst.items()))
    assert max(worst.values()) <= 256.0, worst


@functools.lru_cache(maxsize=None)
def fitted(drop_slot=None):
    det = xref.dropped(xref.scaled_inputs("pt16-two")["det"], drop_slot)
    return build.fit_link_scales_pixels(xref.model_of("pt16-two", det), x0=ppx.inputs("pt16-two")["x0"])


def test_fit_recovers_the_scaled_truth(gpu_lib):
    """pt16-two, seed link_scale_px_ref.SEED: status ok, the cost never rises, every group within 4 bars of the truth, and scales
    and bars equal to the CPU driver's within 10 x tol."""
    sc, out, want = xref.scaled_inputs("pt16-two"), fitted(), xref.fitted("pt16-two")
    z = (out["scales"] - sc["factors"]) / out["std_scales"]
    costs = [h["cost"] for h in out["history"]]
    print(f"factors {np.round(sc['factors'], 4)}\nscales  {np.round(out['scales'], 4)} (CPU driver {np.round(want['scales'], 4)})\n"
          f"std     {np.round(out['std_scales'], 4)}; z {np.round(z, 2)}; {len(costs)} outer steps, cost {costs[0]:.3f} -> {costs[-1]:.3f}; "
          f"to the CPU driver: scales {np.abs(out['scales'] - want['scales']).max():.1e}, std {np.abs(out['std_scales'] - want['std_scales']).max():.1e}")
    assert out["status"] == "ok" and all(b <= a for a, b in zip(costs, costs[1:]))
    assert out["observed"].all() and (np.abs(z) < 4.0).all()
    assert np.abs(out["scales"] - want["scales"]).max() <= 1e-5 and np.abs(out["std_scales"] - want["std_scales"]).max() <= 1e-5
    assert np.array_equal(out["model"].link_scales, out["scales"]) and out["fit"]["x"].shape == (24, 15)
    assert np.allclose(out["cov_log_scales"], out["cov_log_scales"].T)


def test_an_unobserved_group_stays_at_one(gpu_lib):
    """A leaf slot's detections removed in every camera and frame: the link's group is not observed, keeps the scale 1 and has no
    bar; the others are the reference's with that group fixed."""
    prog = ppx.model_of("pt16-two").prog
    parents = {op[1] for op in prog["ops"]}
    k = max(i for i, op in enumerate(prog["ops"]) if op[0] not in parents)          # a leaf link: only its own slot hangs on it
    slot, g = prog["ops"][k][0], int(xref.groups_for("pt16-two")[0][k])
    out, want = fitted(slot), xref.fitted("pt16-two", slot)
    assert not out["observed"][g] and out["scales"][g] == 1.0 and np.isinf(out["std_scales"][g]) and out["status"] == "ok"
    assert (out["cov_log_scales"][g] == 0).all() and (out["cov_log_scales"][:, g] == 0).all()
    assert (out["system"]["S"][g] == 0).all() and out["system"]["r"][g] == 0
    rest = np.arange(len(out["scales"])) != g
    assert out["observed"][rest].all() and np.array_equal(out["observed"], want["observed"])
    print(f"group {g} unobserved; the others to the reference: {np.abs(out['scales'] - want['scales']).max():.1e}")
    assert np.abs(out["scales"][rest] - want["scales"][rest]).max() <= 1e-5
    assert np.abs(out["std_scales"][rest] - want["std_scales"][rest]).max() <= 1e-5
