"""The FTE solve on the OpenCV pinhole camera (k_fte_assemble<JAC, 0, SPLIT, true>, acino_fte_create_pinhole, camera_model="pinhole")
against the test-side numpy reference tests/pinhole_fte_ref.py (oracle.fte on oracle.camera.project_points)."""
import numpy as np
import pytest

import pinhole_fte_ref as pref
from oracle import fk as ofk
from oracle import fte as ofte

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mods(gpu_lib):
    from acinoset_amd import calib, fte, synth
    return calib, fte, synth


def _prob(seq):
    det = seq["det"]
    return pref.PinholeFTEProblem(det[..., :2], det[..., 2], seq["K"], seq["D"], seq["R"], seq["t"], seq["Ts"])


def _rig(seq):
    return seq["K"], seq["D"], seq["R"], seq["t"]


@pytest.mark.parametrize("n", [60, 2400])
@pytest.mark.parametrize("split", [1, 2])
@pytest.mark.parametrize("d", [pref.D12, pref.D5], ids=["d12", "d5"])
def test_pinhole_cost_gradient_hessian(mods, monkeypatch, n, split, d):
    """Phase C on the pinhole model: cost (current iterate and ctx.cost of any x), gradient and Gauss-Newton blocks equal
    the reference's, in both launch shapes (SPLIT = 2: two lanes per (frame, marker), SPLIT = 1: the long-chain launch)."""
    calib, fte, synth = mods
    monkeypatch.setenv("ACINO_ASM_SPLIT", str(split))
    seq = pref.pinhole_sequence(n, "trot", d=d)
    prob = _prob(seq)
    rng = np.random.default_rng(2)
    xa = np.clip(seq["q_true"][:, ofk.ACTIVE] + rng.normal(0, 0.02, (n, 25)), prob.lo, prob.hi)
    Fo, go, Ho, nbo = prob.evaluate(xa)
    ctx = fte.FTEContext(seq["det"], *_rig(seq), seq["Ts"], camera_model="pinhole")
    try:
        ctx.set_x(xa)
        st = ctx.state()
        assert abs(st["cost"] - Fo) < 1e-12 * abs(Fo), (st["cost"], Fo)
        assert st["n_behind"] == nbo
        xb = np.clip(xa + rng.normal(0, 0.01, xa.shape), prob.lo, prob.hi)
        Fb = prob.evaluate(xb, need_jac=False)[0]
        assert abs(ctx.cost(xb) - Fb) < 1e-12 * abs(Fb)
        g, h = (a.cpu().numpy() for a in ctx.grad_hess())
        idx = np.arange(25)
        Ho[:, idx, idx] += 2 * prob.q_w[None, :] * prob.s_band()[0][:, None]
        assert np.abs(g - go).max() < 1e-11 * np.abs(go).max()
        assert np.abs(h - Ho).max() < 1e-11 * np.abs(Ho).max()
        with pytest.raises(ValueError, match="pinhole"):
            ctx.set_precision("bf16")
    finally:
        ctx.close()


def _behind_sequence(n):
    """The sprint seen by the pinhole ring with camera 0 moved beside the run, 3 m to its left at mid-run and turned 60
    degrees forward: the first quarter of the run lies behind it.  Six detections of markers behind camera 0 are made
    confident false positives (what a keypoint detector does report), so n_behind > 0 from the start to the end of the
    solve - the reference keeps their mirrored projections, which pay the saturated loss."""
    from acinoset_amd import fte, synth
    K, D, R, t = pref.pinhole_rig(pref.D12)
    heading = 0.35                                        # synth.trajectory's sprint
    fwd = np.array([np.cos(heading), np.sin(heading), 0.0])
    left = np.array([-np.sin(heading), np.cos(heading), 0.0])
    centre = synth.LOOK_AT + 3.0 * left
    zc = np.cos(np.pi / 3) * (-left) + np.sin(np.pi / 3) * fwd
    xc = np.cross(zc, [0.0, 0.0, 1.0])
    xc /= np.linalg.norm(xc)
    R[0] = np.stack([xc, np.cross(zc, xc), zc])
    t[0, :, 0] = -R[0] @ centre
    q = synth.trajectory(n, "sprint")
    pos = fte.cheetah_fk(q)
    det = pref.pinhole_detections(pos, K, D, R, t)
    zc0 = pos @ R[0][2] + t[0, 2, 0]
    fr, mk = np.nonzero(zc0 < -0.5)
    assert fr.size > 100                                  # (the geometry does put markers behind camera 0)
    pick = np.random.default_rng(5).choice(fr.size, 6, replace=False)
    det[fr[pick], 0, mk[pick], :] = [1300.0, 700.0, 0.95]
    return dict(K=K, D=D, R=R, t=t, q_true=q, pos_true=pos, det=det, Ts=1.0 / synth.FPS)


@pytest.mark.parametrize("n,kind,behind", [(99, "sprint", False), (99, "sprint", True), (600, "trot", False)])
def test_pinhole_lm_path_identity(mods, n, kind, behind):
    """The HIP solve walks oracle.fte.lm_solve on the pinhole problem: the same trial cost and accept / reject decision in
    every iteration, the same iteration count and stopping test, end positions within 1e-8 m, the same n_behind."""
    calib, fte, synth = mods
    seq = _behind_sequence(n) if behind else pref.pinhole_sequence(n, kind)
    prob = _prob(seq)
    x0 = fte.nose_line_init(seq["det"], *_rig(seq), 0.5, camera_model="pinhole")
    hist = []
    xo, oinfo = ofte.lm_solve(prob, x0[:, ofk.ACTIVE], max_iter=100, history=hist)
    ctx = fte.FTEContext(seq["det"], *_rig(seq), seq["Ts"], camera_model="pinhole", bcr_levels=0)
    try:
        ctx.set_x(x0[:, ofk.ACTIVE])
        st = ctx.state()
        assert st["n_behind"] == prob.evaluate(np.clip(x0[:, ofk.ACTIVE], prob.lo, prob.hi), need_jac=False)[3]
        acc = 0
        for it, hh in enumerate(hist):
            ctx.step()
            st = ctx.state()
            assert abs(st["cost_trial"] - hh["Ft"]) < 1e-9 * abs(hh["Ft"]), (it, st["cost_trial"], hh["Ft"])
            assert (st["accepted"] > acc) == (hh["Ft"] < hh["F"]), it
            acc = st["accepted"]
        if st["status"] == 0:
            ctx.step()                # (a gradient test that ends the solve takes one more iteration, without history)
            st = ctx.state()
        assert st["status_name"] == oinfo["status"] and st["iter"] == oinfo["iterations"], (st, oinfo)
        assert st["accepted"] == oinfo["accepted"] and st["n_behind"] == oinfo["n_behind"]
        if behind:
            assert oinfo["n_behind"] > 0
        assert abs(st["cost"] - oinfo["cost"]) < 1e-11 * abs(oinfo["cost"])
        pos = ctx.result()[1].cpu().numpy()
    finally:
        ctx.close()
    pos_o = ofte.fte_outputs(prob, xo, x0)["positions"]
    assert np.abs(pos - pos_o).max() < 1e-8


def test_pinhole_clips_equal_per_clip_solves(mods):
    calib, fte, synth = mods
    clip = 45
    seqs = [pref.pinhole_sequence(clip, "sprint", seed=20210313 + i) for i in range(4)]
    rig = _rig(seqs[0])
    x0s = []
    for s in seqs:
        x0 = np.zeros((clip, 45))
        x0[:, fte.ACTIVE] = s["q_true"][:, fte.ACTIVE]
        x0s.append(x0)
    fused = fte.fte_solve_clips([s["det"] for s in seqs], *rig, seqs[0]["Ts"], x0s=x0s, max_iter=120, ftol=1e-13,
                                camera_model="pinhole")
    total = 0.0
    for s, x0, (res, info) in zip(seqs, x0s, fused):
        one, info1 = fte.fte_solve(s["det"][..., :2], s["det"][..., 2], *rig, Ts=s["Ts"], x0=x0, max_iter=120, ftol=1e-13,
                                   camera_model="pinhole")
        total += info1["cost"]
        assert info["status_name"] in ("ftol", "xtol", "gtol") and info["clips"] == 4
        assert np.abs(res["positions"] - one["positions"]).max() < 1e-3
    assert abs(fused[0][1]["cost"] - total) < 1e-6 * abs(total)


def _rms(a, b):
    return float(np.sqrt(((np.asarray(a) - np.asarray(b)) ** 2).sum(-1).mean()))


@pytest.mark.parametrize("init", ["nose_line", "triangulation"])
def test_pinhole_end_to_end_recovers_markers(mods, init):
    """Initial guess and solve on the pinhole rig (calib.triangulate_pairs_dense(model="pinhole") and
    k_fte_assemble<., 0, ., true>), from detections made by calib.project_points with synth's noise and outliers: the ground
    truth is recovered as well as the fisheye solve recovers the same trajectory seen through the fisheye rig."""
    calib, fte, synth = mods
    n = 99
    fish = synth.make_sequence(n, "sprint")
    pin = pref.pinhole_sequence(n, "sprint")
    assert np.array_equal(fish["pos_true"], pin["pos_true"])
    err = {}
    for name, seq, model in (("fisheye", fish, "fisheye"), ("pinhole", pin, "pinhole")):
        res, info = fte.fte_solve(seq["det"][..., :2], seq["det"][..., 2], *_rig(seq), seq["Ts"], init=init,
                                  max_iter=200, camera_model=model)
        assert info["status_name"] in ("ftol", "xtol", "gtol"), (name, info)
        err[name] = _rms(res["positions"], seq["pos_true"])
    assert err["pinhole"] <= 1.5 * err["fisheye"] + 1e-3, err
    # the reference's injection seam selects the same path
    res2, _ = fte.fte_solve(pin["det"][..., :2], pin["det"][..., 2], *_rig(pin), pin["Ts"], init=init, max_iter=200,
                            project_func=calib.project_points)
    assert _rms(res2["positions"], pin["pos_true"]) == err["pinhole"]


def test_context_cache_keeps_the_models_apart(mods):
    """reuse_context: a fisheye sequence, then a pinhole sequence of the same shape on the same K, R, t - the pinhole
    solve must get a pinhole context (bit-identical to a fresh one), not the cached fisheye one."""
    calib, fte, synth = mods
    n = 60
    fish = synth.make_sequence(n, "sprint")
    pin = pref.pinhole_sequence(n, "sprint")
    try:
        fte.fte_solve(fish["det"][..., :2], fish["det"][..., 2], *_rig(fish), fish["Ts"], max_iter=40, reuse_context=True)
        cached, ic = fte.fte_solve(pin["det"][..., :2], pin["det"][..., 2], *_rig(pin), pin["Ts"], max_iter=40,
                                   reuse_context=True, camera_model="pinhole")
    finally:
        fte.clear_context_cache()
    fresh, i_f = fte.fte_solve(pin["det"][..., :2], pin["det"][..., 2], *_rig(pin), pin["Ts"], max_iter=40,
                               camera_model="pinhole")
    assert np.array_equal(cached["x"], fresh["x"]) and ic["iter"] == i_f["iter"]


def test_fisheye_keyword_is_the_default_path(mods):
    calib, fte, synth = mods
    seq = synth.make_sequence(600, "trot", seed=99)
    args = (seq["det"][..., :2], seq["det"][..., 2], *_rig(seq), seq["Ts"])
    a, ia = fte.fte_solve(*args, max_iter=30)
    b, ib = fte.fte_solve(*args, max_iter=30, camera_model="fisheye")
    c, ic = fte.fte_solve(*args, max_iter=30, project_func=calib.project_points_fisheye)
    assert np.array_equal(a["x"], b["x"]) and np.array_equal(a["x"], c["x"])
    assert ia["iter"] == ib["iter"] == ic["iter"]
