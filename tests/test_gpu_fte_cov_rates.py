"""Covariance of dx, ddx and of the marker velocities on the GPU (k_fte_cov_rates, acino_fte_covariance_rates,
FTEContext.covariance_rates, return_rate_cov) against the CPU reference tests/fte_cov_rates_ref.py.

Metric and bar are those of tests/test_gpu_fte_cov.py, per OUTPUT: e = fte_cov_ref.rel_err, d0 = the same metric between
two independent CPU references on the very matrix and the very output under test - dense LU inverse against banded
Cholesky probes of the 75 unit vectors of every window, or banded Cholesky against banded LU probes where the dense
inverse is out of reach - and e <= fte_cov_ref.bar(d0) = max(64 d0, 1e-13), which refuses d0 > 1e-8.  Every test prints
its d0 and e (pytest -s) before it asserts.  On the CPU (oracle H at the true trajectory, sprint 7 / 121 / 122) d0 of
cov_dx / cov_ddx is 0.7e-10 .. 2.8e-10 and the numpy restatement of the kernel's factor form is at 0.7e-10 .. 4.2e-10.
The measured figures of the MI355X are in DESIGN section 6.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import fte_cov_ref as ref
import fte_cov_rates_ref as rref
import pinhole_fte_ref as pref
from oracle import fk as ofk
from oracle import fte as ofte

pytestmark = pytest.mark.gpu
NAMES = ("cov_dx", "cov_ddx", "cov_vel", "std_vel")


@pytest.fixture(scope="module")
def mods(gpu_lib):
    from acinoset_amd import _lib, fte, synth
    return _lib, fte, synth


def _rig(seq):
    return seq["K"], seq["D"], seq["R"], seq["t"]


def _tables(Ts):
    dummy = ofte.FTEProblem(np.zeros((1, 1, 20, 2)), np.zeros((1, 1, 20)), np.eye(3)[None], np.zeros((1, 4)), np.eye(3)[None],
                            np.zeros((1, 3)), Ts)
    return dummy.q_w, dummy.lo, dummy.hi


def _reference_system(ctx, clip_len=0):
    """x, the pinned set and the banded matrix from grad_hess() and result(): nothing of the code under test."""
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


def _check(name, got, want, other, frames=None):
    """got (GPU, all frames) at `frames` against `want`; d0 per output from `other` against `want`."""
    got = tuple(g if frames is None else g[frames] for g in got)
    d0 = rref.errs(other, want)
    e = rref.errs(got, want)
    print(f"\n[{name}] " + "   ".join(f"{k}: d0 = {d:.2e} e = {v:.2e}" for k, d, v in zip(NAMES, d0, e)))
    assert all(np.isfinite(g).all() for g in got)
    for k, d, v in zip(NAMES, d0, e):
        assert v <= ref.bar(d), (name, k, d, v)
    for blocks in got[:3]:
        b = blocks.reshape(-1, blocks.shape[-2], blocks.shape[-1])
        assert np.abs(b - b.transpose(0, 2, 1)).max() <= 1e-12 * np.abs(b).max()
        w = np.linalg.eigvalsh(0.5 * (b + b.transpose(0, 2, 1)))
        assert np.all(w[:, 0] >= -1e-12 * np.maximum(w[:, -1], 1e-300))
    return d0, e


def _check_dense(name, ctx):
    x, fixed, ab = _reference_system(ctx)
    a = rref.reference(ab, fixed, x, ctx.Ts, how="dense")
    b = rref.reference(ab, fixed, x, ctx.Ts, how="chol")
    got = tuple(t.cpu().numpy() for t in ctx.covariance_rates())
    std_only = ctx.covariance_rates(std_only=True)
    assert all(o is None for o in std_only[:3]) and np.array_equal(std_only[3].cpu().numpy(), got[3])
    _check(name, got, a, b)
    return x, fixed, ab, got


@pytest.mark.parametrize("n,model", [(7, "fisheye"), (120, "fisheye"), (121, "fisheye"), (122, "fisheye"), (120, "pinhole")])
def test_rate_covariances_equal_the_dense_inverse(mods, n, model):
    """Whole and ragged last nodes, windows inside a node and across two, the start-up frames; and the sanity check that
    needs no tolerance table: for n >= 2 and free variables sqrt(diag cov_dx) is smaller than sqrt(2 diag cov_x) / Ts, what
    independent frames would give."""
    _lib, fte, synth = mods
    seq = synth.make_sequence(n, "sprint") if model == "fisheye" else pref.pinhole_sequence(n, "sprint")
    ctx = _solved_context(fte, seq, model)
    try:
        x, fixed, ab, got = _check_dense(f"{model} {n}", ctx)
        cov_x = ctx.covariance()[0].cpu().numpy()
        dx, ddx = (t.cpu().numpy() for t in ctx.result()[2:])
        rdx, rddx = rref.derivatives_from_rows(x, ctx.Ts)                # the rows are the rows of what result() returns
        assert np.abs(dx - rdx).max() <= 1e-9 * np.abs(dx).max() and np.abs(ddx - rddx).max() <= 1e-9 * np.abs(ddx).max()
        sd = np.sqrt(np.einsum("npp->np", got[0]))[2:]
        ind = np.sqrt(2 * np.einsum("npp->np", cov_x))[2:] / ctx.Ts
        free = ~(fixed[2:] | fixed[1:-1])
        factor = ind[free] / sd[free]
        print(f"[{model} {n}] independent frames overstate std(dx) by a factor {factor.min():.1f} .. {factor.max():.1f}"
              f" (median {np.median(factor):.1f})")
        assert np.all(sd[free] < ind[free])
    finally:
        ctx.close()


def test_bound_active_variables_have_no_spread(mods):
    """The front knee on its bound in (almost) every frame: where it is pinned in all frames of a window its rows and
    columns of cov_dx / cov_ddx are exactly 0; everything else equals the reference."""
    _lib, fte, synth = mods
    n = 120
    q = synth.trajectory(n, "sprint")
    q[:, ofk.ACTIVE[12]] = np.pi / 2 + 0.3
    pos = fte.cheetah_fk(q)
    K, D, R, t = synth.make_rig()
    seq = dict(K=K, D=D, R=R, t=t, det=synth.detections_from_positions(pos, K, D, R, t), Ts=1.0 / synth.FPS)
    ctx = _solved_context(fte, seq)
    try:
        x, fixed, ab, got = _check_dense("bound 120", ctx)
        full = fixed[2:, 12] & fixed[1:-1, 12] & fixed[:-2, 12]
        assert full.sum() >= n // 2, "the active set is (almost) empty: the test is void"
        for blocks in (got[0][2:], got[1][2:]):
            assert np.all(blocks[:, 12, :][full] == 0.0) and np.all(blocks[:, :, 12][full] == 0.0)
    finally:
        ctx.close()


def test_detection_gap_shows_in_the_velocity_error_bars(mods):
    """No camera sees anything for 30 frames: std_vel inside the gap exceeds the median outside."""
    _lib, fte, synth = mods
    seq = synth.make_sequence(120, "sprint")
    seq["det"][45:75, :, :, 2] = 0.0
    ctx = _solved_context(fte, seq)
    try:
        x, fixed, ab, got = _check_dense("gap 120", ctx)
        std_vel = got[3]
        inside, outside = std_vel[50:70], np.concatenate([std_vel[:40], std_vel[80:]])
        ratio = float(np.median(inside) / np.median(outside))
        print(f"[gap 120] median std_vel inside {np.median(inside):.4f} m/s, outside {np.median(outside):.4f} m/s, "
              f"ratio {ratio:.2f}")
        assert np.median(inside) > np.median(outside)
    finally:
        ctx.close()


def _probe_check(name, ctx, frames, clip_len=0):
    x, fixed, ab = _reference_system(ctx, clip_len)
    b = rref.reference(ab, fixed, x, ctx.Ts, frames, clip_len, how="chol")
    lu = rref.reference(ab, fixed, x, ctx.Ts, frames, clip_len, how="lu")
    got = tuple(t.cpu().numpy() for t in ctx.covariance_rates())
    _check(name, got, b, lu, frames)
    return got


def test_long_sequence_probe_frames(mods):
    """10 000 frames as ONE sequence: both ends (the start-up frames), frames either side of node boundaries, random
    interior frames; banded Cholesky against banded LU probes."""
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
    """8 clips of 1 000 frames in one context: probe frames at the seams equal the reference, and a clip inside the batch is
    bit-identical to a context that holds the clip alone at the same iterate (same H: same launch shape of the assembly)."""
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
        got = _probe_check("clips 8 x 1000", ctx, frames, clip_len=S)
        x = ctx.result()[0]
        g_all, H_all = ctx.grad_hess()
    finally:
        ctx.close()
    same = 0
    for b in (0, 3, 7):
        sl = slice(b * S, (b + 1) * S)
        one = fte.FTEContext(seqs[b]["det"], *rig, Ts)
        try:
            one.set_x(x[sl].contiguous())
            g1, H1 = one.grad_hess()
            alone = tuple(t.cpu().numpy() for t in one.covariance_rates())
        finally:
            one.close()
        if torch.equal(H1, H_all[sl]) and torch.equal(g1, g_all[sl]):
            same += 1
            for k, a, o in zip(NAMES, got, alone):
                assert np.array_equal(a[sl], o), f"clip {b}: {k} differs from the clip alone"
    print(f"[clips 8 x 1000] {same} of 3 clips compared bit for bit (identical inputs)")
    assert same >= 1, "no clip had bit-identical H / g in both contexts: the comparison is void"


def test_superset_is_bit_identical_to_covariance(mods):
    """cov_x, cov_pos, std_pos out of the new entry are those of acino_fte_covariance on the same context, bit for bit, and
    the rates do not depend on whether they were asked for."""
    _lib, fte, synth = mods
    seq = synth.make_sequence(121, "sprint")
    ctx = _solved_context(fte, seq)
    try:
        old = ctx.covariance()
        rates, new = ctx.covariance_rates(with_cov=True)
        only = ctx.covariance_rates()
        assert all(torch.equal(a, b) for a, b in zip(old, new))
        assert all(torch.equal(a, b) for a, b in zip(rates, only))
    finally:
        ctx.close()


def test_step_after_rate_covariance_is_bit_identical(mods):
    """The call leaves solver state, buffers and the captured graph alone (side stream, graph replay on)."""
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
                        ctx.covariance_rates(with_cov=(it == 3))
                    st = ctx.state()
                    trace.append((st["cost"], st["cost_trial"], st["lam"], st["iter"], st["accepted"]))
                assert ctx.graphs_active() & 16
                outs.append((ctx.result()[0].clone(), trace))
            finally:
                ctx.close()
        stream.synchronize()
    assert torch.equal(outs[0][0], outs[1][0])
    assert outs[0][1] == outs[1][1]


def test_fte_solve_return_rate_cov(mods):
    """return_rate_cov adds the four arrays with their shapes and changes nothing else; with return_cov both sets come."""
    _lib, fte, synth = mods
    seq = synth.make_sequence(60, "sprint")
    args = (seq["det"][..., :2], seq["det"][..., 2], *_rig(seq), seq["Ts"])
    plain, ip = fte.fte_solve(*args, max_iter=60)
    withr, ir = fte.fte_solve(*args, max_iter=60, return_rate_cov=True)
    new = {"cov_dx", "cov_ddx", "cov_velocities", "std_velocities"}
    assert set(withr) - set(plain) == new
    assert all(np.array_equal(plain[k], withr[k]) for k in plain if k != "start_frame") and ip["iter"] == ir["iter"]
    assert withr["cov_dx"].shape == (60, 25, 25) and withr["cov_ddx"].shape == (60, 25, 25)
    assert withr["cov_velocities"].shape == (60, 20, 3, 3) and withr["std_velocities"].shape == (60, 20)
    assert isinstance(withr["std_velocities"], np.ndarray) and np.all(withr["std_velocities"] > 0)
    both, _ = fte.fte_solve(*args, max_iter=60, return_cov=True, return_rate_cov=True)
    assert set(both) - set(plain) == new | {"cov_x", "cov_positions", "std_positions"}
    assert all(np.array_equal(both[k], withr[k]) for k in new)
    seqs = [synth.make_sequence(45, "sprint", seed=20210313 + i) for i in range(3)]
    for out in (fte.fte_solve_clips([s["det"] for s in seqs], *_rig(seq), seq["Ts"], max_iter=60, return_rate_cov=True,
                                    return_numpy=False),
                fte.fte_solve_batch([s["det"] for s in seqs], *_rig(seq), seq["Ts"], max_iter=60, return_rate_cov=True,
                                    return_numpy=False)):
        for s, (res, info) in zip(seqs, out):
            assert "cov_x" not in res
            assert isinstance(res["cov_dx"], torch.Tensor) and tuple(res["cov_dx"].shape) == (45, 25, 25)
            assert tuple(res["cov_velocities"].shape) == (45, 20, 3, 3) and tuple(res["std_velocities"].shape) == (45, 20)
            assert torch.equal(res["std_velocities"][0], res["std_velocities"][1])      # frame 0 of a clip repeats frame 1


def test_unsupported_contexts_are_refused_without_a_launch(mods):
    """Sharded, windowed and bf16 contexts: ACINO_ERR_UNSUPPORTED (-5), outputs and workspace untouched; a workspace that
    is too small: ACINO_ERR_WORKSPACE (-3)."""
    _lib, fte, synth = mods
    seq = synth.make_sequence(60, "sprint")
    lib = _lib.lib()

    def call(ctx, base, nbytes, std):
        return lib.acino_fte_covariance_rates(ctx._h, ctx.Ts, C.c_void_p(base), nbytes, None, None, None, None, None, None,
                                              _lib.ptr(std), _lib.stream_ptr())

    for kw, why in ((dict(pin_right=True, n_global=120), "sharded"), (dict(own_first=3, own_count=30), "windowed"),
                    (dict(precision="bf16"), "bf16")):
        ctx = fte.FTEContext(seq["det"], *_rig(seq), seq["Ts"], **kw)
        try:
            nbytes = lib.acino_fte_covariance_rates_workspace_bytes(C.byref(ctx.params))
            ws = torch.zeros(nbytes + 256, dtype=torch.uint8, device=ctx.device)
            std = torch.full((60, 20), -1.0, dtype=torch.float64, device=ctx.device)
            base = (ws.data_ptr() + 255) // 256 * 256
            assert call(ctx, base, nbytes, std) == -5
            msg = lib.acino_last_error_string().decode()
            assert why in msg
            if why == "bf16":
                assert "acino_fte_covariance_rates" in msg          # (the entry that was called, not acino_fte_covariance)
            torch.cuda.synchronize()
            assert bool((std == -1.0).all()) and not bool(ws.any())
            with pytest.raises(RuntimeError, match="not supported"):
                ctx.covariance_rates()
        finally:
            ctx.close()
    ctx = fte.FTEContext(seq["det"], *_rig(seq), seq["Ts"])
    try:
        ctx.set_x(np.zeros((60, 25)))
        ws = torch.zeros(1024, dtype=torch.uint8, device=ctx.device)
        std = torch.empty((60, 20), dtype=torch.float64, device=ctx.device)
        base = (ws.data_ptr() + 255) // 256 * 256
        assert call(ctx, base, 512, std) == -3
    finally:
        ctx.close()
