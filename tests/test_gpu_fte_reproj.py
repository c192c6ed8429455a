"""The FTE solve in image space on the GPU (k_fte_reproj, acino_fte_reprojection, FTEContext.reprojection,
return_reprojection) against the CPU reference tests/fte_reproj_ref.py.

Every test takes x = ctx.result()[0] and cov_pos = ctx.covariance()[1] FROM THE GPU and feeds the same arrays to the
reference, so only the new kernel is under test.  All N * C * 20 entries are compared; NaN patterns and flags exactly.  Bars
(taken from the project, not from the kernel):
    uv, res     max abs difference <= 1e-9 px (fisheye), 1e-8 px (pinhole): tests/test_gpu_parity.py's bars for the projections
    cov_uv      per entry ||S_gpu - S_ref||_F <= 1e-11 ||S_ref||_F (test_gpu_parity.py's bar for H); both off-diagonals the same
                bits; eigenvalues >= -1e-12 * largest
    weight      h = (rho'(e) - rho'(0+)) / e is a secant whose two evaluations differ by the rounding of rho' (~1e-15) over
                e: <= 1e-9 where e >= 1e-5, <= 1e-4 below; at most 1e-3 of the weighted components may lie below (a condition on
                the input, checked on the reference); exactly 0 where bit 0 is clear; all in [0, 1]
    mahal2      d^2 is quadratic in res: <= 1e-9 d + 1e-10 d^2 + 1e-18 (pinhole: ten times that), d from the reference
Observed on the MI355X (pytest -s prints them; max over the entries; also DESIGN section 8):
    fisheye 120, converged / 3 it   uv, res 1.4e-12 / 1.4e-12 px   cov_uv 2.6e-15 / 2.4e-15   weight 0 / 3.7e-14   mahal2 < 1e-3 bar
    pinhole 120, converged / 3 it   uv, res 1.7e-11 / 1.1e-11 px   cov_uv 1.4e-14 / 1.4e-14   weight 0 / 2.1e-14   mahal2 <= 1e-3 bar
    gap 120                         uv, res 1.1e-12 px             cov_uv 2.2e-15             weight 0             std_uv ratio 21.5
    loop 10 000 (64 probes)         uv, res 1.6e-12 px             cov_uv 2.6e-15             weight 5.1e-14
    cost from the report against state["cost"]: <= 6.2e-16 relative; no weighted component of these inputs has e < 1e-5
"""
import numpy as np
import pytest
import torch

import fte_reproj_ref as rref
import pinhole_fte_ref as pref
from oracle import fk as ofk
from oracle import fte as ofte

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mods(gpu_lib):
    from acinoset_amd import _lib, fte, synth
    return _lib, fte, synth


def _rig(seq):
    return seq["K"], seq["D"], seq["R"], seq["t"]


def _context(fte, seq, model="fisheye", max_iter=100, converged=True, **kw):
    ctx = fte.FTEContext(seq["det"], *_rig(seq), seq["Ts"], camera_model=model, **kw)
    x0 = fte.nose_line_init(seq["det"], *_rig(seq), 0.5, camera_model=model)
    ctx.set_x(x0[:, ofk.ACTIVE])
    info = ctx.solve(max_iter)
    assert info["status_name"] in ("ftol", "xtol", "gtol") or (not converged and info["status_name"] == "running"), info
    return ctx


def _np(rep):
    return {k: (None if v is None else v.cpu().numpy()) for k, v in rep.items()}


def _compare(name, got, ref, model, with_cov=True):
    """The bars of the module docstring on every entry; returns the observed maxima."""
    f = 1.0 if model == "fisheye" else 10.0
    assert np.array_equal(got["flags"], ref["flags"]), f"{name}: flags differ"
    keys = ("uv", "res", "mahal2") + (("cov_uv",) if with_cov else ())
    for k in keys:
        assert np.array_equal(np.isnan(got[k]), np.isnan(ref[k])), f"{name}: NaN pattern of {k}"
    assert np.isfinite(got["weight"]).all()
    on = (ref["flags"] & 1) != 0
    share, small = rref.small_component_share(ref)
    assert share <= 1e-3, f"{name}: {share:.2e} of the weighted components have e < 1e-5 (the input is unfit for the weight bar)"
    e_uv = float(np.nanmax(np.abs(got["uv"] - ref["uv"])))
    e_res = float(np.nanmax(np.abs(got["res"] - ref["res"])))
    dw = np.abs(got["weight"] - ref["weight"])
    big = on[..., None] & ~small
    e_w = float(dw[big].max())
    e_ws = float(dw[small].max()) if small.any() else 0.0
    d = np.sqrt(ref["mahal2"])
    with np.errstate(invalid="ignore"):
        m_ratio = np.abs(got["mahal2"] - ref["mahal2"]) / (f * (1e-9 * d + 1e-10 * d * d + 1e-18))
    e_m = float(np.nanmax(m_ratio))
    line = f"\n[{name}] max |d uv| = {e_uv:.2e} px   |d res| = {e_res:.2e} px   |d weight| = {e_w:.2e} (e >= 1e-5), {e_ws:.2e} " \
           f"(below: {int(small.sum())} of {int(on.sum()) * 2})   mahal2 / bar = {e_m:.3f}"
    e_c = 0.0
    if with_cov:
        ok = ~np.isnan(ref["cov_uv"][..., 0, 0])
        num = np.linalg.norm((got["cov_uv"] - ref["cov_uv"])[ok].reshape(-1, 4), axis=1)
        den = np.linalg.norm(ref["cov_uv"][ok].reshape(-1, 4), axis=1)
        e_c = float((num / den).max())
        line += f"   cov_uv rel = {e_c:.2e}"
    print(line)
    assert e_uv <= f * 1e-9 and e_res <= f * 1e-9
    assert e_w <= 1e-9 and e_ws <= 1e-4
    assert np.all(got["weight"][~on] == 0.0) and np.all((got["weight"] >= 0.0) & (got["weight"] <= 1.0))
    assert e_m <= 1.0
    if with_cov:
        assert e_c <= 1e-11
        S = got["cov_uv"][ok]
        assert np.array_equal(S[:, 0, 1], S[:, 1, 0])
        w = np.linalg.eigvalsh(S)
        assert np.all(w[:, 0] >= -1e-12 * w[:, 1])
        std = got["std_uv"][ok]
        assert np.array_equal(std, np.sqrt(S[:, 0, 0] + S[:, 1, 1]))
    return dict(uv=e_uv, res=e_res, weight=e_w, weight_small=e_ws, mahal2=e_m, cov_uv=e_c)


def _check_context(name, ctx, seq, model, frames=None):
    x = ctx.result()[0]
    cov_pos = ctx.covariance()[1]
    got = _np(ctx.reprojection(cov_pos=cov_pos))
    plain = _np(ctx.reprojection(cov=False))
    sl = slice(None) if frames is None else frames
    xs, cs, det = x.cpu().numpy()[sl], cov_pos.cpu().numpy()[sl], seq["det"][sl]
    ref = rref.reprojection(xs, cs, det, _rig(seq), model)
    ref0 = rref.reprojection(xs, None, det, _rig(seq), model)
    _compare(name, {k: (None if v is None else v[sl]) for k, v in got.items()}, ref, model)
    _compare(name + ", no cov", {k: (None if v is None else v[sl]) for k, v in plain.items()}, ref0, model, with_cov=False)
    assert plain["cov_uv"] is None and plain["std_uv"] is None
    for k in ("uv", "res", "weight", "flags"):
        assert np.array_equal(got[k], plain[k], equal_nan=True)
    return x, got


def _sequence(synth, model, n=120):
    return synth.make_sequence(n, "sprint") if model == "fisheye" else pref.pinhole_sequence(n, "sprint")


@pytest.mark.parametrize("iters", [100, 3])
@pytest.mark.parametrize("model", ["fisheye", "pinhole"])
def test_report_equals_the_reference(mods, model, iters):
    """120 frames of the sprint, solved to convergence and stopped after 3 iterations, both camera models."""
    _lib, fte, synth = mods
    seq = _sequence(synth, model)
    ctx = _context(fte, seq, model, max_iter=iters, converged=iters > 3)
    try:
        _check_context(f"{model} 120, {iters} it", ctx, seq, model)
    finally:
        ctx.close()


@pytest.mark.parametrize("iters", [100, 3])
@pytest.mark.parametrize("model", ["fisheye", "pinhole"])
def test_report_ties_to_the_solver_state(mods, model, iters):
    """sum of rho(inv_r res) over the weighted detections (+ rho(0) per dropped component: the objective counts a dropped
    detection as a residual of 0, and rho(0) is not 0) + the smoothness term = state["cost"] to 1e-11 relative
    (test_gpu_parity.py's bar for the cost); the detections above the threshold with bit 1 set are state["n_behind"]."""
    _lib, fte, synth = mods
    seq = _sequence(synth, model)
    det = seq["det"]
    ctx = _context(fte, seq, model, max_iter=iters, converged=iters > 3)
    try:
        st = ctx.state()
        x = ctx.result()[0].cpu().numpy()
        rep = _np(ctx.reprojection(cov=False))
    finally:
        ctx.close()
    prob = ofte.FTEProblem(det[..., :2], det[..., 2], seq["K"], np.zeros((det.shape[1], 4)), seq["R"], seq["t"], seq["Ts"])
    cost = rref.measurement_cost(rep) + prob.smooth_terms(x)[0]
    rel = abs(cost - st["cost"]) / abs(st["cost"])
    counted = np.isfinite(det[..., :2]).all(-1) & (det[..., 2] > 0.5) & ((rep["flags"] & 2) != 0)
    print(f"\n[{model}, {iters} it] cost {st['cost']:.12f}, from the report {cost:.12f} (rel {rel:.2e}); behind: "
          f"{int(counted.sum())} / n_behind {st['n_behind']}")
    assert rel <= 1e-11
    assert int(counted.sum()) == st["n_behind"]


def test_detection_gap_widens_the_pixel_error_bars(mods):
    """The input of test_detection_gap_shows_in_the_error_bars (no likelihood above 0 in frames 45..74): median std_uv over
    frames 50..69 >= 10 x the median over frames 0..39 and 80..119; inside the gap nothing is weighted, yet the pixels and
    the residuals are there."""
    _lib, fte, synth = mods
    seq = synth.make_sequence(120, "sprint")
    seq["det"][45:75, :, :, 2] = 0.0
    ctx = _context(fte, seq)
    try:
        _, got = _check_context("gap 120", ctx, seq, "fisheye")
    finally:
        ctx.close()
    inside, outside = got["std_uv"][50:70], np.concatenate([got["std_uv"][:40], got["std_uv"][80:]])
    ratio = float(np.median(inside) / np.median(outside))
    print(f"[gap 120] median std_uv inside {np.median(inside):.2f} px, outside {np.median(outside):.2f} px, ratio {ratio:.1f}")
    assert ratio >= 10.0
    assert np.all((got["flags"][45:75] & 1) == 0) and np.all(got["weight"][45:75] == 0.0)
    assert np.isfinite(got["uv"][45:75]).all() and np.isfinite(got["res"][45:75]).all()


def test_solve_entries(mods, monkeypatch):
    """return_reprojection alone and with return_cov give bit-identical cov_uv; every clip of fte_solve_clips equals the call
    on a context of that clip alone at the same x, bit for bit; a bf16 context reports with cov=False and raises the
    covariance's RuntimeError with cov=True."""
    _lib, fte, synth = mods
    seq = synth.make_sequence(60, "sprint")
    args = (seq["det"][..., :2], seq["det"][..., 2], *_rig(seq), seq["Ts"])
    plain, _ = fte.fte_solve(*args, max_iter=60)
    alone, _ = fte.fte_solve(*args, max_iter=60, return_reprojection=True)
    both, _ = fte.fte_solve(*args, max_iter=60, return_reprojection=True, return_cov=True)
    new = {"uv", "cov_uv", "std_uv", "residuals", "weights", "mahal2", "flags"}
    assert set(alone) - set(plain) == new and set(both) - set(alone) == {"cov_x", "cov_positions", "std_positions"}
    assert all(np.array_equal(plain[k], alone[k]) for k in plain if k != "start_frame")
    for k in new:
        assert isinstance(alone[k], np.ndarray) and np.array_equal(alone[k], both[k], equal_nan=True), k
    assert alone["cov_uv"].shape == (60, 6, 20, 2, 2) and alone["flags"].dtype == np.uint8
    rep = fte.detection_report(alone, gate=9.21)
    assert rep["n_weighted"].shape == (6, 20) and np.all(rep["n_inlier"] <= rep["n_weighted"]) and rep["n_inlier"].sum() > 0
    # clips: 4 x 250 frames (both contexts assemble with the same launch shape, so that they hold the same H)
    monkeypatch.setenv("ACINO_ASM_SPLIT", "1")
    S, B = 250, 4
    seqs = [synth.make_sequence(S, "trot", seed=20210313 + i) for i in range(B)]
    rig, Ts = _rig(seqs[0]), seqs[0]["Ts"]
    out = fte.fte_solve_clips([s["det"] for s in seqs], *rig, Ts, max_iter=100, return_reprojection=True, return_numpy=False)
    for s, (res, info) in zip(seqs, out):
        one = fte.FTEContext(s["det"], *rig, Ts)
        try:
            one.set_x(res["x"])
            rep = one.reprojection()
        finally:
            one.close()
        for k, name in fte._REPROJ_KEYS.items():
            assert tuple(res[name].shape[:3]) == (S, 6, 20)
            assert np.array_equal(res[name].cpu().numpy(), rep[k].cpu().numpy(), equal_nan=True), k
    # and the kernel alone: same x, the SAME cov_pos array, the clip's slice of one launch against the clip's own launch
    det = np.concatenate([s["det"] for s in seqs])
    ctx = fte.FTEContext(det, *rig, Ts, clip_len=S)
    try:
        ctx.set_x(torch.cat([res["x"] for res, _ in out]))
        cov_pos = ctx.covariance()[1]
        whole = ctx.reprojection(cov_pos=cov_pos)
    finally:
        ctx.close()
    for b, s in enumerate(seqs):
        one = fte.FTEContext(s["det"], *rig, Ts)
        try:
            one.set_x(out[b][0]["x"])
            rep = one.reprojection(cov_pos=cov_pos[b * S:(b + 1) * S].contiguous())
        finally:
            one.close()
        for k in fte._REPROJ_KEYS:
            assert torch.equal(torch.nan_to_num(whole[k][b * S:(b + 1) * S].double(), nan=-7.0),
                               torch.nan_to_num(rep[k].double(), nan=-7.0)), k
    # bf16
    ctx = fte.FTEContext(seq["det"], *_rig(seq), seq["Ts"], precision="bf16")
    try:
        ctx.set_x(plain["x"])
        rep = _np(ctx.reprojection(cov=False))
        ref = rref.reprojection(plain["x"], None, seq["det"], _rig(seq))
        _compare("bf16 context", rep, ref, "fisheye", with_cov=False)
        with pytest.raises(RuntimeError, match="not supported"):
            ctx.reprojection()
    finally:
        ctx.close()


def test_long_sequence(mods):
    """10 000 frames as one sequence: 64 probe frames (both ends, the frames either side of a workgroup boundary, random
    interior frames) against the reference at the bars above; everything else finite with sane flags."""
    _lib, fte, synth = mods
    n = 10000
    seq = synth.make_sequence(n, "loop")
    ctx = _context(fte, seq, max_iter=60, converged=False)
    try:
        rng = np.random.default_rng(11)
        frames = np.unique(np.concatenate([[0, 1, 7, 8, n - 9, n - 8, n - 2, n - 1], rng.integers(10, n - 10, 80)]))[:64]
        assert len(frames) == 64
        _, got = _check_context("loop 10000 (64 probes)", ctx, seq, "fisheye", frames=frames)
    finally:
        ctx.close()
    assert np.all(got["flags"] <= 7)
    ok = (got["flags"] & 4) == 0
    assert np.isfinite(got["uv"][ok]).all() and np.isfinite(got["cov_uv"][ok]).all() and np.isfinite(got["weight"]).all()
    assert np.all(np.isnan(got["uv"][~ok]))
    finite = np.isfinite(seq["det"][..., :2]).all(-1)
    assert np.array_equal(np.isfinite(got["res"]).all(-1), finite & ok)
    assert np.array_equal((got["flags"] & 1) != 0, finite & ok & (seq["det"][..., 2] > 0.5))
