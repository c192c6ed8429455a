"""Posterior covariance of the FTE trajectory on the GPU (k_fte_cov_sweep / k_fte_cov_combine, acino_fte_covariance,
FTEContext.covariance, return_cov) against the CPU reference tests/fte_cov_ref.py.

Error metric  e = max_n ||S_gpu[n] - S_ref[n]||_F / ||S_ref[n]||_F.  The bar is set by the REFERENCES, per input:
d0 = the same metric between two independent references on the very matrix under test - (a) dense LU inverse and (b)
banded Cholesky probes, or, where the dense inverse is out of reach (1 000 / 10 000 frames), (b) and (b') banded LU
probes - and  e <= max(64 d0, 1e-13)  (fte_cov_ref.bar, which also refuses an input with d0 > 1e-8).  The matrix has a
condition number of 2.5e8 (sprint, 120 frames) to 1.4e10 (the detection gap): the weights 2 q span 1e4 .. 5e8.

d0 on the oracle's converged solve of the same seeded inputs (CPU, fisheye; two-sweep: the numpy restatement of the kernels):
    sprint   7 frames  d0 = 3.5e-10   two-sweep e = 9.0e-10        sprint 120  d0 = 2.4e-10   two-sweep e = 5.0e-10
    sprint 121 frames  d0 = 2.4e-10   two-sweep e = 4.2e-10        sprint 122  d0 = 3.6e-10   two-sweep e = 5.7e-10
    gap    120 frames  d0 = 7.4e-10   two-sweep e = 1.8e-09        bound  120  d0 = 3.9e-10   two-sweep e = 3.4e-10
Every test prints its d0 and e (pytest -s) before it asserts.  Measured on the MI355X (d0 of the test's own matrix -> worst e
of cov_x / cov_pos / std_pos; also DESIGN section 6):
    fisheye   7  3.8e-10 -> 8.3e-10    120  2.6e-10 -> 4.9e-10    121  4.0e-10 -> 4.7e-10    122  2.2e-10 -> 4.3e-10
    pinhole   7  3.4e-10 -> 3.5e-10    120  2.7e-10 -> 5.5e-10    121  2.6e-10 -> 3.0e-10    122  2.1e-10 -> 4.4e-10
    bound 120  2.5e-10 -> 3.8e-10      gap 120  5.0e-10 -> 5.1e-10 (median std inside / outside the gap: 0.114 / 0.0053 m)
    loop 10 000 (12 probes)  1.6e-10 -> 8.5e-10      clips 8 x 1 000 (12 probes)  1.9e-10 -> 4.6e-10, clip alone: identical
(A first version of the sweeps, with the correction taken through the explicit inverse, gave 7.5e-6 at 7 frames, 1.5e-7 at
121 and 7.6e-8 on the clips - every input that ends in a node of one frame - and was replaced, not the bar.)

cov_pos / std_pos are referred to the oracle's ANALYTIC FK Jacobian, which tests/test_fte_cov_host.py pins to central
differences of the oracle FK: the differences themselves carry 2e-9 of rounding (1e-8 of cov_pos) and could not carry a
bar of this size.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import fte_cov_ref as ref
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


def _tables(Ts):
    """q_w, lo, hi of the problem (they do not depend on the detections or the camera model)."""
    dummy = ofte.FTEProblem(np.zeros((1, 1, 20, 2)), np.zeros((1, 1, 20)), np.eye(3)[None], np.zeros((1, 4)), np.eye(3)[None],
                            np.zeros((1, 3)), Ts)
    return dummy.q_w, dummy.lo, dummy.hi


def _reference_system(ctx, clip_len=0):
    """x, the pinned set and the banded matrix from what the context ALREADY exported before this feature: grad_hess()
    (blocks with the smoothness diagonal) and result()."""
    q_w, lo, hi = _tables(ctx.Ts)
    g, Hd = (a.cpu().numpy() for a in ctx.grad_hess())
    x = ctx.result()[0].cpu().numpy()
    band = ref.clip_band(ctx.N, clip_len)
    fixed = ref.active_set(x, g, Hd, lo, hi)
    return x, fixed, ref.banded(Hd, fixed, q_w, band)


def _solved_context(fte, seq, model="fisheye", max_iter=100, converged=True, **kw):
    ctx = fte.FTEContext(seq["det"], *_rig(seq), seq["Ts"], camera_model=model, **kw)
    x0 = fte.nose_line_init(seq["det"], *_rig(seq), 0.5, camera_model=model)
    ctx.set_x(x0[:, ofk.ACTIVE])
    info = ctx.solve(max_iter)
    assert info["status_name"] in ("ftol", "xtol", "gtol") or (not converged and info["status_name"] == "running"), info
    return ctx


def _check_blocks(name, cov_x, cov_pos, std_pos, x, fixed, ref_x, frames, tol):
    """cov_x / cov_pos / std_pos of `frames` against the reference blocks ref_x; symmetry; positive semi-definiteness."""
    J = ref.fk_jacobian_exact(x[frames])
    ref_pos, ref_std = ref.marker_cov(ref_x, J)
    n = len(frames)
    cx, cp, sp = cov_x[frames], cov_pos[frames], std_pos[frames]
    e_x = ref.rel_err(cx, ref_x)
    e_p = ref.rel_err(cp.reshape(n * 20, 9), ref_pos.reshape(n * 20, 9))
    e_s = float(np.max(np.abs(sp - ref_std) / ref_std))
    print(f"\n[{name}] bar = {tol:.2e}   e(cov_x) = {e_x:.2e}   e(cov_pos) = {e_p:.2e}   e(std_pos) = {e_s:.2e}")
    assert np.isfinite(cx).all() and np.isfinite(cp).all() and np.isfinite(sp).all()
    assert np.all(cx[fixed[frames]] == 0.0) and np.all(cx.transpose(0, 2, 1)[fixed[frames]] == 0.0)
    assert e_x <= tol and e_p <= tol and e_s <= tol, (e_x, e_p, e_s, tol)
    assert np.abs(cx - cx.transpose(0, 2, 1)).max() <= 1e-12 * np.abs(cx).max()
    assert np.abs(cp - cp.transpose(0, 1, 3, 2)).max() <= 1e-12 * np.abs(cp).max()
    for blocks in (cx, cp.reshape(n * 20, 3, 3)):
        w = np.linalg.eigvalsh(0.5 * (blocks + blocks.transpose(0, 2, 1)))
        assert np.all(w[:, 0] >= -1e-12 * w[:, -1])
    return e_x, e_p, e_s


def _check_dense(name, ctx):
    x, fixed, ab = _reference_system(ctx)
    a = ref.dense_blocks(ab, fixed)
    frames = np.arange(ctx.N)
    d0 = ref.rel_err(ref.probe_blocks(ab, fixed, frames), a)
    print(f"\n[{name}] d0 = {d0:.2e}")
    cov_x, cov_pos, std_pos = (t.cpu().numpy() for t in ctx.covariance())
    std_only = ctx.covariance(std_only=True)
    assert std_only[0] is None and std_only[1] is None and np.array_equal(std_only[2].cpu().numpy(), std_pos)
    _check_blocks(name, cov_x, cov_pos, std_pos, x, fixed, a, frames, ref.bar(d0))
    return x, fixed, std_pos


@pytest.mark.parametrize("n", [7, 120, 121, 122])
@pytest.mark.parametrize("model", ["fisheye", "pinhole"])
def test_covariance_equals_the_dense_inverse(mods, n, model):
    """Whole and ragged last nodes (7 = 2 nodes + 1 frame, 121, 122), both camera models, after a converged solve."""
    _lib, fte, synth = mods
    seq = synth.make_sequence(n, "sprint") if model == "fisheye" else pref.pinhole_sequence(n, "sprint")
    ctx = _solved_context(fte, seq, model)
    try:
        _check_dense(f"{model} {n}", ctx)
    finally:
        ctx.close()


def test_bound_active_variables_have_no_spread(mods):
    """A front knee whose true angle lies 0.3 rad beyond its box: the estimate sits on the bound in every frame, the
    variable is pinned - its rows and columns of cov_x are exactly 0, everything else equals the reference."""
    _lib, fte, synth = mods
    n = 120
    q = synth.trajectory(n, "sprint")
    q[:, ofk.ACTIVE[12]] = np.pi / 2 + 0.3
    pos = fte.cheetah_fk(q)
    K, D, R, t = synth.make_rig()
    seq = dict(K=K, D=D, R=R, t=t, det=synth.detections_from_positions(pos, K, D, R, t), Ts=1.0 / synth.FPS)
    ctx = _solved_context(fte, seq)
    try:
        x, fixed, _ = _check_dense("bound 120", ctx)
        assert fixed[:, 12].sum() >= n // 2, "the active set is (almost) empty: the test is void"
        cov_x = ctx.covariance()[0].cpu().numpy()
        assert np.all(cov_x[:, 12, :][fixed[:, 12]] == 0.0) and np.all(cov_x[:, :, 12][fixed[:, 12]] == 0.0)
    finally:
        ctx.close()


def test_detection_gap_shows_in_the_error_bars(mods):
    """No camera sees anything for 30 frames: the prior alone carries the estimate across, and the markers' error bars say
    so (the oracle's solve of this input on the CPU: median std inside / outside = 21)."""
    _lib, fte, synth = mods
    seq = synth.make_sequence(120, "sprint")
    seq["det"][45:75, :, :, 2] = 0.0
    ctx = _solved_context(fte, seq)
    try:
        x, fixed, std_pos = _check_dense("gap 120", ctx)
        inside, outside = std_pos[50:70], np.concatenate([std_pos[:40], std_pos[80:]])
        ratio = float(np.median(inside) / np.median(outside))
        print(f"[gap 120] median std inside {np.median(inside):.4f} m, outside {np.median(outside):.4f} m, ratio {ratio:.1f}")
        assert ratio >= 10.0
    finally:
        ctx.close()


def _probe_check(name, ctx, frames, clip_len=0):
    x, fixed, ab = _reference_system(ctx, clip_len)
    b = ref.probe_blocks(ab, fixed, frames)
    d0 = ref.rel_err(ref.probe_blocks(ab, fixed, frames, lu=True), b)
    print(f"\n[{name}] d0 (banded Cholesky against banded LU) = {d0:.2e}")
    cov = tuple(t.cpu().numpy() for t in ctx.covariance())
    _check_blocks(name, *cov, x, fixed, b, frames, ref.bar(d0))
    return cov, ref.bar(d0)


def test_long_sequence_probe_frames(mods):
    """10 000 frames as ONE sequence (3 334 dependent nodes per sweep): both ends, the frames either side of two node
    boundaries, random interior frames, against banded solves with their unit vectors.  (The covariance is defined at any
    iterate: 60 iterations from the nose line are taken whether or not a stopping test has fired by then.)"""
    _lib, fte, synth = mods
    n = 10000
    seq = synth.make_sequence(n, "loop")
    ctx = _solved_context(fte, seq, max_iter=60, converged=False)
    try:
        rng = np.random.default_rng(7)
        frames = np.unique(np.concatenate([[0, 1, n - 2, n - 1, 2999, 3000, 7502, 7503], rng.integers(10, n - 10, 4)]))
        assert len(frames) == 12
        _probe_check("loop 10000", ctx, frames)
    finally:
        ctx.close()


def test_clips_equal_the_clips_alone(mods, monkeypatch):
    """clip_len = 1000, 8 clips in one context: every clip's covariance equals that of a context holding the clip alone at
    the same iterate (no coupling across a seam), and probe frames at the seams equal the reference.  (Both contexts
    assemble with the same launch shape, so that they hold the same H and the comparison is about the seams.)"""
    _lib, fte, synth = mods
    monkeypatch.setenv("ACINO_ASM_SPLIT", "1")
    S, B = 1000, 8
    seqs = [synth.make_sequence(S, "trot", seed=20210313 + i) for i in range(B)]
    rig, Ts = _rig(seqs[0]), seqs[0]["Ts"]
    det = np.concatenate([s["det"] for s in seqs])
    x0 = np.concatenate([fte.nose_line_init(s["det"], *rig, 0.5) for s in seqs])[:, ofk.ACTIVE]
    ctx = fte.FTEContext(det, *rig, Ts, clip_len=S)
    try:
        ctx.set_x(x0)
        info = ctx.solve(100)
        assert info["status_name"] in ("ftol", "xtol", "gtol"), info
        frames = np.array([0, 1, 998, 999, 1000, 1001, 1002, 3500, 6999, 7000, 7998, 7999])
        (cov_x, cov_pos, std_pos), tol = _probe_check("clips 8 x 1000", ctx, frames, clip_len=S)
        x = ctx.result()[0]
    finally:
        ctx.close()
    worst = 0.0
    for b in range(B):
        one = fte.FTEContext(seqs[b]["det"], *rig, Ts)
        try:
            one.set_x(x[b * S:(b + 1) * S].contiguous())
            ox, op, os_ = (t.cpu().numpy() for t in one.covariance())
        finally:
            one.close()
        sl = slice(b * S, (b + 1) * S)
        e = max(ref.rel_err(cov_x[sl], ox), ref.rel_err(cov_pos[sl].reshape(S * 20, 9), op.reshape(S * 20, 9)),
                float(np.max(np.abs(std_pos[sl] - os_) / os_)))
        worst = max(worst, e)
    print(f"[clips 8 x 1000] clip in the batch against the clip alone: worst e = {worst:.2e} (bar {tol:.2e})")
    assert worst <= tol


def test_fte_solve_return_cov(mods):
    """return_cov adds the three arrays (numpy in, numpy out) and changes nothing else; fte_solve_clips / fte_solve_batch hand
    out per-clip arrays equal to FTEContext.covariance of the same clip.  (Two evaluations of the same x may differ in the
    last bit of H - the assembly has two launch shapes -; a relative perturbation of 2.2e-16 of a matrix of condition 2.5e8
    moves its inverse by at most 5.5e-8, a standard deviation by half of that: the bound is 1e-7.)"""
    _lib, fte, synth = mods
    seq = synth.make_sequence(60, "sprint")
    args = (seq["det"][..., :2], seq["det"][..., 2], *_rig(seq), seq["Ts"])
    plain, ip = fte.fte_solve(*args, max_iter=60)
    withc, ic = fte.fte_solve(*args, max_iter=60, return_cov=True)
    assert set(withc) - set(plain) == {"cov_x", "cov_positions", "std_positions"}
    assert all(np.array_equal(plain[k], withc[k]) for k in plain if k != "start_frame") and ip["iter"] == ic["iter"]
    assert withc["cov_x"].shape == (60, 25, 25) and withc["cov_positions"].shape == (60, 20, 3, 3)
    assert isinstance(withc["std_positions"], np.ndarray) and withc["std_positions"].shape == (60, 20)
    assert np.all(withc["std_positions"] > 0) and np.all(withc["std_positions"] < 1.0)
    ctx = fte.FTEContext(seq["det"], *_rig(seq), seq["Ts"])
    try:
        ctx.set_x(withc["x"])
        std = ctx.covariance(std_only=True)[2].cpu().numpy()
    finally:
        ctx.close()
    assert np.abs(std - withc["std_positions"]).max() <= 1e-7 * std.max()
    seqs = [synth.make_sequence(45, "sprint", seed=20210313 + i) for i in range(3)]
    for out in (fte.fte_solve_clips([s["det"] for s in seqs], *_rig(seq), seq["Ts"], max_iter=60, return_cov=True,
                                    return_numpy=False),
                fte.fte_solve_batch([s["det"] for s in seqs], *_rig(seq), seq["Ts"], max_iter=60, return_cov=True,
                                    return_numpy=False)):
        for s, (res, info) in zip(seqs, out):
            assert isinstance(res["cov_x"], torch.Tensor) and tuple(res["cov_x"].shape) == (45, 25, 25)
            one = fte.FTEContext(s["det"], *_rig(seq), seq["Ts"])
            try:
                one.set_x(res["x"])
                std = one.covariance(std_only=True)[2]
            finally:
                one.close()
            assert float((std - res["std_positions"]).abs().max()) <= 1e-7 * float(std.max())


def test_step_after_covariance_is_bit_identical(mods):
    """The call leaves solver state, buffers and the captured graph alone: two contexts walk the same steps, one of them
    computes covariances in between, on a side stream with graphs enabled."""
    _lib, fte, synth = mods
    seq = synth.make_sequence(600, "trot")
    x0 = fte.nose_line_init(seq["det"], *_rig(seq), 0.5)[:, ofk.ACTIVE]
    outs = []
    stream = torch.cuda.Stream()
    for with_cov in (False, True):
        with torch.cuda.stream(stream):
            ctx = fte.FTEContext(seq["det"], *_rig(seq), seq["Ts"])
            try:
                ctx.enable_graph(True)
                ctx.set_x(x0)
                trace = []
                for it in range(6):
                    ctx.step()
                    if with_cov and it in (1, 3, 4):
                        ctx.covariance()
                    st = ctx.state()
                    trace.append((st["cost"], st["cost_trial"], st["lam"], st["iter"], st["accepted"]))
                assert ctx.graphs_active() & 16
                outs.append((ctx.result()[0].clone(), trace))
            finally:
                ctx.close()
        stream.synchronize()
    assert torch.equal(outs[0][0], outs[1][0])
    assert outs[0][1] == outs[1][1]


def test_unsupported_contexts_are_refused_without_a_launch(mods):
    """Sharded (pinned separator), windowed (own range) and bf16 contexts: ACINO_ERR_UNSUPPORTED (-5), a message that says
    why, outputs untouched."""
    _lib, fte, synth = mods
    seq = synth.make_sequence(60, "sprint")
    lib = _lib.lib()
    for kw, why in ((dict(pin_right=True, n_global=120), "sharded"), (dict(own_first=3, own_count=30), "windowed"),
                    (dict(precision="bf16"), "bf16")):
        ctx = fte.FTEContext(seq["det"], *_rig(seq), seq["Ts"], **kw)
        try:
            nbytes = lib.acino_fte_covariance_workspace_bytes(C.byref(ctx.params))
            ws = torch.zeros(nbytes + 256, dtype=torch.uint8, device=ctx.device)
            std = torch.full((60, 20), -1.0, dtype=torch.float64, device=ctx.device)
            base = (ws.data_ptr() + 255) // 256 * 256
            rc = lib.acino_fte_covariance(ctx._h, C.c_void_p(base), nbytes, None, None, _lib.ptr(std), _lib.stream_ptr())
            assert rc == -5
            assert why in lib.acino_last_error_string().decode()
            torch.cuda.synchronize()
            assert bool((std == -1.0).all()) and not bool(ws.any())
            with pytest.raises(RuntimeError, match="not supported"):
                ctx.covariance()
        finally:
            ctx.close()
    # a workspace that is too small is refused too
    ctx = fte.FTEContext(seq["det"], *_rig(seq), seq["Ts"])
    try:
        ctx.set_x(np.zeros((60, 25)))
        ws = torch.zeros(1024, dtype=torch.uint8, device=ctx.device)
        std = torch.empty((60, 20), dtype=torch.float64, device=ctx.device)
        base = (ws.data_ptr() + 255) // 256 * 256
        assert lib.acino_fte_covariance(ctx._h, C.c_void_p(base), 512, None, None, _lib.ptr(std), _lib.stream_ptr()) == -3
    finally:
        ctx.close()
