"""GPU (-m gpu): the skeleton FTE under the redescending measurement loss (build_model(loss="redescending");
k_skel_assemble<., ., true> and its Fisher form <true, ., true, double>, k_skel_reproj<., true>) against the CPU reference tests/skel_loss_ref.py.

    1  the HIP solve walks oracle.fte.lm_solve's path on the robust problem, at the tolerances of the L1 path test
       (tests/test_skel_fte.py): from the saturated straight-line start, from the GPU's own L1 end point, on a pinhole rig
    2  a batch equals the clips one by one; an L1 model in a robust batch is refused
    3  the two-stage solve is the L1 solve followed by the robust solve, bit for bit
    4  moved detections are rejected (weight <= 0.05), every other weighted component counts (>= 0.9); weight and mahal2
       against the reference at the same x; uv / res / flags carry the L1 report's bits
    5  covariance, rates and samples against their references fed with the blocks sum w^2 h J^T J (bar(d0) of those tests),
       and the bars equal the L1 bars of the same data with the outliers unweighted, to 1 %
    6  solve_video(loss="redescending") is the stitch of the windows' two-stage solves
    7  an L1 model gives the bits of a params block whose `loss` was never written
Every test fails without the feature (build_model has no ``loss``).  pytest -s prints the observed figures."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from oracle import skel_fte as osf

import pinhole_fte_ref as pref
import skel_cov_rates_ref as rates_ref
import skel_cov_ref as cref
import skel_loss_cases as lcases
import skel_loss_ref as lref
import skel_sample_ref as sref

pytestmark = pytest.mark.gpu

ZERO_TOL = dict(ftol=0.0, xtol=0.0, gtol=0.0)


@pytest.fixture(scope="module")
def fx(golden_dir):
    g = np.load(os.path.join(golden_dir, "skel_fte_model.npz"))
    det = np.load(os.path.join(golden_dir, "human_dlc_slice.npz"))["det"].astype(np.float64)
    return g, json.loads(str(g["skeleton_json"])), det


def _tables(det, parts):
    return [(list(parts), det[:, c]) for c in range(det.shape[1])]


def _scene(g, cam="fisheye"):
    return (g["K"], np.tile(pref.D5, (len(g["K"]), 1)), g["R"], g["t"]) if cam == "pinhole" else (g["K"], g["D"], g["R"], g["t"])


def _model(fx, n, sf, pairing="name", cam="fisheye", loss="redescending", det=None):
    from acinoset_amd import build
    g, sk, slice_det = fx
    return build.build_model(sk, scene=_scene(g, cam), dlc_tables=_tables(slice_det if det is None else det, g["parts"]), n_frames=n,
                             start_frame=sf, pairing=pairing, camera_model=cam, loss=loss)[0]


# ---- 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["reference8", "name40", "pinhole8"])
def test_solve_walks_the_reference_lm_path(gpu_lib, fx, case):
    """reference8: the 8-frame fixture (the model of build.py as written) from init_x - every residual beyond c, the loss
    saturated: the reference accepts 1, 2, 5, 7 steps, so rejected steps are walked too.  name40: 40 frames by name from the GPU's
    own L1 end point.  pinhole8: the 8-frame fixture on the pinhole rig of the pinhole skeleton tests (D5), iterations 0 .. 5."""
    from acinoset_amd import build
    g, sk, _det = fx
    cam = "pinhole" if case == "pinhole8" else "fisheye"
    if case == "name40":
        model = _model(fx, 40, 60)
        x0 = build.solve_model(lcases.with_loss(model, "l1"), max_iter=200)[0]["x"]
    else:
        model = _model(fx, int(g["n_frames"]), int(g["start_frame"]), "reference", cam, det=g["det"])
        x0 = model.init_x
    prob = lref.problem(sk, model, _scene(g, cam), cam)
    act = prob.ACT
    F0 = prob.evaluate(x0[:, act], need_jac=False)[0]
    accepted = {}
    for k in (0, 1, 2, 5) + (() if case == "pinhole8" else (12,)):
        res, info = build.solve_model(model, x0=x0, max_iter=k, l1_start=False, **ZERO_TOL)
        xo, oinfo = osf.lm_solve(prob, x0[:, act], max_iter=k, **ZERO_TOL) if k else (x0[:, act], dict(cost=F0, accepted=0))
        accepted[k] = oinfo["accepted"]
        e_c, e_x = abs(info["cost_final"] - oinfo["cost"]) / abs(oinfo["cost"]), float(np.abs(res["x"][:, act] - xo).max())
        print(f"{case}, {k} iterations: accepted {info['accepted']} / {oinfo['accepted']}, cost {info['cost_final']:.6f}, "
              f"relative difference {e_c:.2e}, max |dx| {e_x:.2e}")
        assert "l1" not in info
        assert abs(info["cost_initial"] - F0) < 1e-12 * abs(F0)
        assert info["accepted"] == oinfo["accepted"], (k, info, oinfo)
        ctol, xtol_ = (1e-10, 1e-8) if k <= 5 else (1e-8, 1e-6)
        assert e_c < ctol and e_x < xtol_
        assert np.all(res["x"][:, np.setdiff1d(np.arange(model.P), act)] == 0)
        assert np.abs(res["positions"] - prob.outputs(xo)["positions"]).max() < xtol_
    if case == "reference8":
        assert accepted[12] < 12, "the saturated start was meant to walk rejected steps"


# ---- 2 ---------------------------------------------------------------------------------------------------------------
def test_batch_of_clips_equals_the_clips_one_by_one(gpu_lib, fx):
    from acinoset_amd import build
    models = [_model(fx, 40, sf) for sf in (60, 150, 300)]
    kw = dict(max_iter=100, ftol=1e-6)
    one = [build.solve_model(m, **kw) for m in models]
    many = build.solve_models(models, **kw)
    for (r1, i1), (rb, ib) in zip(one, many):
        assert i1 == ib and "l1" in ib, (i1, ib)
        assert np.array_equal(r1["x"], rb["x"]) and np.array_equal(r1["positions"], rb["positions"])
    assert len({ib["iterations"] for _r, ib in many} | {ib["l1"]["iterations"] for _r, ib in many}) > 1
    with pytest.raises(ValueError, match="share the loss"):
        build.solve_models(models[:2] + [lcases.with_loss(models[2], "l1")], **kw)


# ---- 3 ---------------------------------------------------------------------------------------------------------------
def test_two_stage_solve_is_the_l1_solve_then_the_robust_solve(gpu_lib, fx):
    from acinoset_amd import build
    model = _model(fx, 40, 60)
    twin = lcases.with_loss(model, "l1")
    kw = dict(max_iter=60, ftol=1e-7)
    res, info = build.solve_model(model, **kw)
    res1, info1 = build.solve_model(twin, **kw)
    res2, info2 = build.solve_model(model, x0=res1["x"], l1_start=False, **kw)
    assert info["l1"] == info1 and {k: v for k, v in info.items() if k != "l1"} == info2
    for k in ("x", "positions", "dx", "ddx"):
        assert np.array_equal(res[k], res2[k]), k
    assert info2["cost_initial"] < info1["cost_initial"] and info2["cost_final"] <= info2["cost_initial"]
    print(f"L1 stage {info1['cost_initial']:.1f} -> {info1['cost_final']:.1f} in {info1['iterations']} iterations; robust stage "
          f"{info2['cost_initial']:.1f} -> {info2['cost_final']:.1f} in {info2['iterations']} ({info2['accepted']} accepted)")


# ---- 4 ---------------------------------------------------------------------------------------------------------------
MOVED = ((7, 0, 13), (8, 0, 5), (11, 0, 6), (6, 1, 13), (10, 1, 7))        # (frame, camera, pose slot): weighted detections of the clip


def test_moved_detections_are_rejected_and_the_report_says_so(gpu_lib, fx):
    """12 frames by name; five weighted detections moved by (80, -60) px."""
    from acinoset_amd import build
    g, sk, _det = fx
    model = _model(fx, 12, 60)
    moved = np.zeros(model.weights.shape, dtype=bool)
    for n, c, l in MOVED:
        assert model.weights[n, c, l] > 0
        model.meas[n, c, l] += np.array([80.0, -60.0])
        moved[n, c, l] = True
    res, info = build.solve_model(model, max_iter=300)
    x = res["x"]
    got = build.model_reprojection([model], [x], cov=False)[0]
    want = lref.report(sk, x, model.meas, model.weights, _scene(g), gate_w=float(model.weights.max()))
    on = (want["flags"] & 1) != 0
    assert np.array_equal(got["flags"], want["flags"]) and moved[on].sum() == 5
    e = np.abs(want["e"])[on]
    assert (e < 1e-5).mean() <= 1e-3, "input condition: residuals at the kink of h"
    h_moved, h_rest = got["weight"][moved], got["weight"][on & ~moved]
    d = np.abs(got["weight"] - want["weight"])[on]
    print(f"robust solve: {info['status_name']} after {info['iterations']} iterations; weight of the moved detections <= {h_moved.max():.4f} "
          f"(reference {want['weight'][moved].max():.4f}), of the others >= {h_rest.min():.4f}; max |d weight| {d.max():.2e}")
    assert h_moved.max() <= 0.05 and h_rest.min() >= 0.9
    assert d[e >= 1e-5].max(initial=0.0) <= 1e-9 and d[e < 1e-5].max(initial=0.0) <= 1e-4
    assert np.all(got["weight"][~on] == 0)
    l1 = build.model_reprojection([lcases.with_loss(model, "l1")], [x], cov=False)[0]
    for k in ("uv", "res", "flags"):
        assert np.array_equal(got[k], l1[k], equal_nan=True), k
    assert np.array_equal(l1["weight"], np.where(on[..., None], 1.0, 0.0) * np.ones(2))
    ok = ~np.isnan(want["mahal2"])
    assert np.array_equal(np.isnan(got["mahal2"]), ~ok)
    e_m = float((np.abs(got["mahal2"] - want["mahal2"])[ok] / lref.mahal2_bar(want, "fisheye")[ok]).max())
    print(f"mahal2 / bar = {e_m:.2e}; twice the L1 report's: {np.nanmax(np.abs(got['mahal2'] / l1['mahal2'] - 2.0)):.1e}")
    assert e_m <= 1.0
    rep = build.detection_report(got)
    assert rep["n_rejected"].sum() == 5 and build.detection_report(l1)["n_rejected"].sum() == 0
    assert all(rep["n_rejected"][c, l] >= 1 for _n, c, l in MOVED)


# ---- 5 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pt", [16, 48])
def test_covariance_is_the_curvature_of_the_robust_objective(gpu_lib, golden_dir, pt):
    """PT 16: the 12-frame sub-tree; PT 48: the full generic skeleton on 40 frames (at 12 frames its two CPU references disagree
    by more than the bar's 1e-8 condition).  cov_x against the dense inverse and the banded probes, cov_pos and std_pos against
    the dense inverse, within skel_cov_ref.bar(d0); the bars over those of the L1 twin with the outliers unweighted in [0.99, 1.01]."""
    from acinoset_amd import build
    c = lcases.cov_case(golden_dir, pt)
    model, x, r, act = c["model"], c["x"], c["ref"], c["prob"].ACT
    assert r["d0"] <= 1e-8
    tol = cref.bar(r["d0"])
    out = build.model_covariance([model], [x])[0]
    cov = out["cov_x"][:, act[:, None], act[None, :]]
    e_a, e_b = cref.rel_err(cov, r["Sa"]), cref.rel_err(cov[r["frames"]], r["Sb"])
    e_p = cref.rel_err(out["cov_pos"].reshape(model.N, -1), r["cov_pos"].reshape(model.N, -1))
    e_s = float(np.max(np.abs(out["std_pos"] - r["std_pos"]) / r["std_pos"]))
    twin = build.model_covariance([c["twin"]], [x])[0]
    sd, sd_t = np.sqrt(np.einsum("npp->np", cov)), np.sqrt(np.einsum("npp->np", twin["cov_x"][:, act[:, None], act[None, :]]))
    ratio, ratio_p = sd / sd_t, out["std_pos"] / twin["std_pos"]
    plain = build.model_covariance([lcases.with_loss(model, "l1")], [x])[0]
    print(f"PT {pt}: d0 {r['d0']:.2e}, bar {tol:.2e}; cov_x vs dense {e_a:.2e}, vs probes {e_b:.2e}; cov_pos {e_p:.2e}; std_pos {e_s:.2e}; "
          f"{int(c['is_out'].sum())} outliers of {int(c['weighted'].sum())}; std over the L1 twin's {ratio.min():.4f} .. {ratio.max():.4f} (poses "
          f"{ratio_p.min():.4f} .. {ratio_p.max():.4f}); plain L1 bars with the outliers counted: {(plain['std_pos'] / twin['std_pos']).min():.4f} of the twin's")
    assert out["status"] == 0 and twin["status"] == 0
    assert e_a <= tol and e_b <= tol and e_p <= tol and e_s <= tol
    assert 0.99 <= ratio.min() and ratio.max() <= 1.01 and 0.99 <= ratio_p.min() and ratio_p.max() <= 1.01
    assert (plain["std_pos"] <= twin["std_pos"] * (1 + 1e-12)).all()       # L1 counts the outliers fully: its bars only shrink


def test_covariance_of_the_robust_objective_on_the_pinhole_rig(gpu_lib, golden_dir):
    """k_skel_assemble<true, true, true, double>, the Fisher assembly under the redescending loss on the pinhole camera, which
    no other test launches: the PT 16 sub-tree on 5 frames (the shortest clip with a third difference) and the fixture's 2
    cameras, judged as the test above.  With 5 frames most iterates leave the two CPU references further apart than the bar's
    1e-8 condition (d0 2e-8 .. 1e-5 for the seeds 0 .. 5 of skel_cov_cases.iterate); seed 82 is one that does not (2.6e-9, the
    12-frame case's figure) - chosen on the CPU references alone."""
    from acinoset_amd import build
    c = lcases.cov_case(golden_dir, 16, camera_model="pinhole", n_frames=5, x_seed=82)
    model, x, r, act = c["model"], c["x"], c["ref"], c["prob"].ACT
    assert model.camera_model == "pinhole" and model.loss == "redescending" and model.N == 5 and model.meas.shape[1] == 2
    assert r["d0"] <= 1e-8 and c["is_out"].sum() >= 1
    tol = cref.bar(r["d0"])
    out = build.model_covariance([model], [x])[0]
    cov = out["cov_x"][:, act[:, None], act[None, :]]
    e_a, e_b = cref.rel_err(cov, r["Sa"]), cref.rel_err(cov[r["frames"]], r["Sb"])
    e_p = cref.rel_err(out["cov_pos"].reshape(model.N, -1), r["cov_pos"].reshape(model.N, -1))
    e_s = float(np.max(np.abs(out["std_pos"] - r["std_pos"]) / r["std_pos"]))
    print(f"pinhole, 5 frames: d0 {r['d0']:.2e}, bar {tol:.2e}; cov_x vs dense {e_a:.2e}, vs probes {e_b:.2e}; cov_pos {e_p:.2e}; "
          f"std_pos {e_s:.2e}; {int(c['is_out'].sum())} outliers of {int(c['weighted'].sum())}")
    assert out["status"] == 0
    assert e_a <= tol and e_b <= tol and e_p <= tol and e_s <= tol
    # the outliers carry no information (h = 0): the matrix is not the L1 Fisher matrix of the same detections
    plain = build.model_covariance([lcases.with_loss(model, "l1")], [x])[0]
    assert (plain["std_pos"] < out["std_pos"]).any()


def test_rates_and_samples_share_the_robust_matrix(gpu_lib, golden_dir):
    from acinoset_amd import build
    c = lcases.cov_case(golden_dir, 16)
    model, x, r, act = c["model"], c["x"], c["ref"], c["prob"].ACT
    rr = rates_ref.reference(r["ab"], r["fixed"], r["G"], model.h)
    out = build.model_covariance([model], [x], rates=True)[0]
    got = dict(cov_dx=out["cov_dx"][:, act[:, None], act[None, :]], cov_ddx=out["cov_ddx"][:, act[:, None], act[None, :]],
               cov_vel=out["cov_vel"], std_vel=out["std_vel"])
    e = rates_ref.out_err(got, rr["c"])
    z = np.random.default_rng(5).standard_normal((3,) + r["fixed"].shape)
    sr = sref.reference(r["ab"], r["fixed"], z)
    draw = build.model_samples([model], [x], z=z[None])[0]
    delta = draw["x_samples"][:, :, act] - x[None, :, act]
    e_d, e_b = sref.map_err(delta, sr["dense"]), sref.map_err(delta, sr["banded"])
    print(f"rates: d0 {rr['d0']:.2e}, bar {rr['bar']:.2e}; " + ", ".join(f"{k} {v:.2e}" for k, v in e.items())
          + f"; samples: d0 {sr['d0']:.2e}, bar {sr['bar']:.2e}, against dense {e_d:.2e}, banded {e_b:.2e}")
    assert out["status"] == 0 and draw["status"] == 0
    assert max(e.values()) <= rr["bar"], e
    assert e_d <= sr["bar"] and e_b <= sr["bar"]


# ---- 6 ---------------------------------------------------------------------------------------------------------------
def test_solve_video_runs_the_robust_stage_from_the_windows_l1_results(gpu_lib, fx, monkeypatch):
    from acinoset_amd import build
    g, sk, det = fx
    kw = dict(scene=_scene(g), dlc_tables=_tables(det, g["parts"]), first_frame=60, last_frame=119, window=40, overlap=20,
              pairing="name", max_iter=60, ftol=1e-7)
    calls = []
    real = build.solve_models

    def spy(models, x0=None, **k):
        calls.append((list(models), x0, dict(k)))
        return real(models, x0, **k)
    monkeypatch.setattr(build, "solve_models", spy)
    res, infos, starts = build.solve_video(sk, loss="redescending", **kw)
    monkeypatch.undo()
    plain, infos_l1, starts_l1 = build.solve_video(sk, **kw)
    assert starts == starts_l1 == [60, 80] and res["robust_failed_windows"] == [] and "robust_failed_windows" not in plain
    assert all(build.model_loss(m) == "l1" for m in calls[0][0]) and all(build.model_loss(m) == "redescending" for m in calls[-1][0])
    assert calls[-1][2]["l1_start"] is False and len(calls[-1][0]) == 2
    # the test's own two stages on the windows of the first call, stitched by the depth rule
    first = real([lcases.with_loss(m, "l1") for m in calls[0][0]], calls[0][1], max_iter=60, ftol=1e-7)
    second = real([lcases.with_loss(m, "redescending") for m in calls[0][0]], [r["x"] for r, _i in first], l1_start=False, max_iter=60,
                  ftol=1e-7)
    assert len(calls) == 2, "no window was warm-started: the first call's results are the L1 stage's"
    total, window = 60, 40
    depth, x, pos = np.full(total, -1.0), np.zeros((total, 48)), np.zeros((total, 15, 3))
    for st, (r, _i) in zip(starts, second):
        d = np.minimum(np.arange(window), window - 1 - np.arange(window)).astype(np.float64)
        sl = slice(st - 60, st - 60 + window)
        take = d > depth[sl]
        x[sl][take], pos[sl][take] = r["x"][take], r["positions"][take]
        depth[sl] = np.maximum(depth[sl], d)
    assert np.array_equal(res["x"], x) and np.array_equal(res["positions"], pos)
    assert not np.array_equal(res["x"], plain["x"])
    for i, (i2, i1) in enumerate(zip(infos, infos_l1)):
        assert i2["mean_abs_residual_px"] == i1["mean_abs_residual_px"] == build.window_residual_px(calls[0][0][i], first[i][1])
        assert i2["l1"] == first[i][1] and i2["cost_final"] == second[i][1]["cost_final"]


# ---- 7 ---------------------------------------------------------------------------------------------------------------
def test_an_l1_model_gives_the_bits_of_a_params_block_without_the_field(gpu_lib, fx):
    """solve_model and model_covariance of an "l1" model against the same C calls with a hand-built params block whose ``loss`` is
    never written (ctypes zero-initialises it: what every caller from before the field sends)."""
    import torch
    from acinoset_amd import _lib, build
    from acinoset_amd._lib import ptr
    model = _model(fx, 40, 60, loss="l1")
    lm = dict(max_iter=25, lam0=1e-3, ftol=1e-10, xtol=1e-10, gtol=1e-8, l1_eps=1e-2, lam_max=1e16)
    res, info = build.solve_model(model, max_iter=25)

    def params(max_iter):
        p = _lib.SkelFteParams()
        p.n_frames, p.n_cams, p.n_pose, p.n_ops = model.N, int(model.meas.shape[1]), len(model.names), len(model.prog["ops"])
        p.n_angles, p.n_active, p.max_iter = model.prog["n_angles"], len(model.active), max_iter
        p.h, p.model_weight, p.l1_eps = float(model.h), float(model.model_weight), 1e-2
        p.lam0, p.ftol, p.xtol, p.gtol, p.lam_max = 1e-3, 1e-10, 1e-10, 1e-8, 1e16
        return p
    io_ = build._skel_inputs([model], [model.init_x.copy()], lambda p, B: _lib.lib().acino_skel_fte_workspace_bytes_batch(C.byref(p), B),
                             start=True, **lm)
    p = params(25)
    head = (C.byref(p),) + io_["head"][1:]
    infos = (_lib.SkelFteInfo * 1)()
    _lib.check(_lib.lib().acino_skel_fte_solve_batch(*head[:2], *head[3:], None, *io_["tail"][:2], infos, io_["tail"][2]))
    act = np.asarray(model.active)
    assert np.array_equal(io_["x"].cpu().numpy()[0], res["x"][:, act]) and infos[0].as_dict() == info
    cov = build.model_covariance([model], [res["x"]], pin_unobserved=True)[0]
    io_ = build._skel_inputs([model], [res["x"]], lambda p, B: _lib.lib().acino_skel_fte_covariance_pinned_workspace_bytes(C.byref(p), B, 1),
                             l1_eps=1e-2)
    p = params(0)
    Pa = len(act)
    cov_x = torch.empty((1, model.N, Pa, Pa), dtype=torch.float64, device=io_["dev"])
    std_pos = torch.empty((1, model.N, len(model.names)), dtype=torch.float64, device=io_["dev"])
    mask = torch.zeros((1, Pa), dtype=torch.uint8, device=io_["dev"])
    status = (C.c_int32 * 1)()
    _lib.check(_lib.lib().acino_skel_fte_covariance_pinned(C.byref(p), *io_["head"][1:], ptr(cov_x), None, ptr(std_pos), status,
                                                           *io_["tail"], 1, ptr(mask)))
    assert status[0] == 0 == cov["status"]
    assert np.array_equal(cov_x.cpu().numpy()[0], cov["cov_x"][:, act[:, None], act[None, :]])
    assert np.array_equal(std_pos.cpu().numpy()[0], cov["std_pos"], equal_nan=True)
