"""Posterior samples of the FTE trajectory on the GPU (k_fte_cov_sweep<true> / k_fte_sample_factors / k_fte_sample_backsub,
acino_fte_sample, FTEContext.sample, n_samples) against the CPU reference tests/fte_sample_ref.py.

The map z -> delta = L^-T z is deterministic, so it is checked to the digits, not statistically:
    e = max_s max_n ||delta_gpu[s, n] - delta_ref[s, n]||_2 / max_n ||delta_ref[s, n]||_2     (fte_sample_ref.map_err)
against reference 1 (banded Cholesky + banded triangular solve), with the bar set by the REFERENCES on the very matrix and z
under test: d0 = the same metric between reference 1 and reference 2 (dense Cholesky up to 160 frames, the node-block
recursion in numpy beyond), e <= max(64 d0, 1e-13) (fte_cov_ref.bar).  Every test prints d0 and e (pytest -s) before it
asserts; the figures measured on the MI355X are in DESIGN section 6 and profiles/fte_cov/pytest_gpu_fte_sample.txt.
Inputs and context set-up: those of tests/test_gpu_fte_cov.py (its helpers are module-private and restated here).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import fte_cov_rates_ref as rref
import fte_cov_ref as ref
import fte_sample_ref as sref
import pinhole_fte_ref as pref
from oracle import fk as ofk
from oracle import fte as ofte

pytestmark = pytest.mark.gpu
P = 25


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
    """x, the pinned set and the banded matrix from grad_hess() and result(): nothing of the feature under test."""
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


def _knee_sequence(fte, synth, n=120):
    q = synth.trajectory(n, "sprint")
    q[:, ofk.ACTIVE[12]] = np.pi / 2 + 0.3
    pos = fte.cheetah_fk(q)
    K, D, R, t = synth.make_rig()
    return dict(K=K, D=D, R=R, t=t, det=synth.detections_from_positions(pos, K, D, R, t), Ts=1.0 / synth.FPS)


def _input(fte, synth, name):
    kind, n = name.split()
    n = int(n)
    if kind == "pinhole":
        return pref.pinhole_sequence(n, "sprint"), "pinhole"
    if kind == "bound":
        return _knee_sequence(fte, synth, n), "fisheye"
    seq = synth.make_sequence(n, "sprint")
    if kind == "gap":
        seq["det"][45:75, :, :, 2] = 0.0
    return seq, "fisheye"


def _gpu_delta(ctx, z, x_hat):
    out = ctx.sample(z.shape[0], z=torch.as_tensor(z, device=ctx.device), positions=False)
    assert set(out) == {"x"}
    return out["x"].cpu().numpy() - x_hat[None]


def _check_map(name, ctx, clip_len=0, sizes=(48, 1)):
    """Test 1 on one context: fixed z from the CPU, S = 48 (not a multiple of the panel) and S = 1, ALL frames."""
    x, fixed, ab = _reference_system(ctx, clip_len)
    N = ctx.N
    worst = []
    for S in sizes:
        z = np.random.default_rng(1000 + S).normal(size=(S, N, P))
        r1 = sref.banded_map(ab, fixed, z)
        r2 = sref.dense_map(ab, fixed, z) if N <= 160 else sref.block_map(ab, fixed, z, clip_len)
        d0 = sref.map_err(r2, r1)
        d = _gpu_delta(ctx, z, x)
        e = sref.map_err(d, r1)
        print(f"\n[{name}] S = {S}: d0 = {d0:.2e}   bar = {ref.bar(d0):.2e}   e = {e:.2e}")
        assert np.isfinite(d).all()
        assert np.all(d[:, fixed] == 0.0), "delta of a pinned variable must be exactly 0"
        worst.append((e, ref.bar(d0)))
    for e, tol in worst:
        assert e <= tol, (name, e, tol)
    return x, fixed, ab


@pytest.mark.parametrize("name", ["fisheye 7", "fisheye 120", "fisheye 121", "fisheye 122", "pinhole 120", "bound 120",
                                  "gap 120"])
def test_exact_map_short_inputs(mods, name):
    """delta = L^-T z to the references' own spread: whole and ragged last nodes, both camera models, the bound-active knee,
    the detection gap."""
    _lib, fte, synth = mods
    seq, model = _input(fte, synth, name)
    ctx = _solved_context(fte, seq, model)
    try:
        x, fixed, ab = _check_map(name, ctx)
        if name.startswith("bound"):
            assert fixed[:, 12].sum() >= ctx.N // 2, "the active set is (almost) empty: the test is void"
    finally:
        ctx.close()


def test_exact_map_long_sequence(mods):
    """10 000 frames as ONE sequence (3 334 dependent nodes), compared on ALL frames; 60 iterations from the nose line, as
    the covariance test of the same input."""
    _lib, fte, synth = mods
    seq = synth.make_sequence(10000, "loop")
    ctx = _solved_context(fte, seq, max_iter=60, converged=False)
    try:
        _check_map("loop 10000", ctx)
    finally:
        ctx.close()


def test_exact_map_clips_and_clips_alone(mods, monkeypatch):
    """clip_len = 1000, 8 clips in one context: the map on all frames (every clip on its own band), and clips 0, 3 and 7
    against a context holding the clip alone at the same iterate with the same slice of z: bit-identical.  (Both contexts
    assemble with the same launch shape, so that they hold the same H.)"""
    _lib, fte, synth = mods
    monkeypatch.setenv("ACINO_ASM_SPLIT", "1")
    S, B = 1000, 8
    seqs = [synth.make_sequence(S, "trot", seed=20210313 + i) for i in range(B)]
    rig, Ts = _rig(seqs[0]), seqs[0]["Ts"]
    det = np.concatenate([s["det"] for s in seqs])
    x0 = np.concatenate([fte.nose_line_init(s["det"], *rig, 0.5) for s in seqs])[:, ofk.ACTIVE]
    z = torch.as_tensor(np.random.default_rng(77).normal(size=(20, B * S, P)), device="cuda")
    ctx = fte.FTEContext(det, *rig, Ts, clip_len=S)
    try:
        ctx.set_x(x0)
        info = ctx.solve(100)
        assert info["status_name"] in ("ftol", "xtol", "gtol"), info
        _check_map("clips 8 x 1000", ctx, clip_len=S)
        x = ctx.result()[0]
        both = ctx.sample(20, z=z, positions=False)["x"]
    finally:
        ctx.close()
    for b in (0, 3, 7):
        sl = slice(b * S, (b + 1) * S)
        one = fte.FTEContext(seqs[b]["det"], *rig, Ts)
        try:
            one.set_x(x[sl].contiguous())
            alone = one.sample(20, z=z[:, sl].contiguous(), positions=False)["x"]
        finally:
            one.close()
        same = torch.equal(alone, both[:, sl])
        print(f"[clips 8 x 1000] clip {b} in the batch against the clip alone: bit-identical = {same}, "
              f"max |diff| = {float((alone - both[:, sl]).abs().max()):.2e}")
        assert same


@pytest.mark.parametrize("name", ["fisheye 7", "fisheye 120", "bound 120"])
def test_identity_z_gives_all_of_the_inverse(mods, name):
    """z = the S = 25 N unit vectors: sum_s delta[s, n] delta[s, m]^T is block (n, m) of A^-1 - cov_x[n] of
    FTEContext.covariance() for m = n, the dense inverse for m != n (all pairs at 7 frames; lags 1, 3, 10, 60 at 120) - with
    the covariance tests' metric and bar.  Rows and columns of pinned variables: exactly 0."""
    _lib, fte, synth = mods
    seq, model = _input(fte, synth, name)
    ctx = _solved_context(fte, seq, model)
    try:
        x, fixed, ab = _reference_system(ctx)
        N = ctx.N
        a = ref.dense_blocks(ab, fixed)
        d0 = ref.rel_err(ref.probe_blocks(ab, fixed, np.arange(N)), a)
        tol = ref.bar(d0)
        z = torch.eye(N * P, dtype=torch.float64, device=ctx.device).view(N * P, N, P)
        delta = ctx.sample(N * P, z=z, positions=False)["x"].cpu().numpy() - x[None]
        cov_x = ctx.covariance()[0].cpu().numpy()
        e0 = ref.rel_err(sref.cross_blocks(delta, 0), cov_x)
        print(f"\n[{name}] covariance d0 = {d0:.2e}   bar = {tol:.2e}   lag 0 against cov_x: e = {e0:.2e}")
        Ai = np.linalg.inv(ref.dense(ab))
        errs = [e0]
        for lag in (range(1, N) if N == 7 else (1, 3, 10, 60)):
            e = ref.rel_err(sref.cross_blocks(delta, lag), sref.inverse_blocks(Ai, fixed, lag))
            print(f"[{name}] lag {lag} against the dense inverse: e = {e:.2e}")
            errs.append(e)
        flat = delta.reshape(N * P, N * P)
        pinned = fixed.reshape(-1)
        if name.startswith("bound"):
            assert pinned.sum() >= N // 2, "no pinned variable: the test is void"
        assert np.all(flat[:, pinned] == 0.0) and np.all(flat[pinned, :] == 0.0)
        assert max(errs) <= tol, (errs, tol)
    finally:
        ctx.close()


def test_monte_carlo_sanity_and_seeds(mods):
    """S = 4096 draws of 120 frames: per free variable the sample variance over diag cov_x lies in 1 +- 6 sqrt(2 / (S - 1))
    and |mean| <= 6 sqrt(cov / S) - the estimators' standard errors, six of them for ~3 000 simultaneous comparisons.  The
    same band is applied FIRST to the CPU reference's delta from the same z, so that a failure of the band is told apart from
    a failure of the kernel.  Same seed: bit-identical; another seed: different."""
    _lib, fte, synth = mods
    seq, model = _input(fte, synth, "fisheye 120")
    ctx = _solved_context(fte, seq, model)
    try:
        S = 4096
        x, fixed, ab = _reference_system(ctx)
        gen = torch.Generator(device=ctx.device)
        gen.manual_seed(11)
        z = torch.randn((S, ctx.N, P), dtype=torch.float64, device=ctx.device, generator=gen)
        out = ctx.sample(S, seed=11, positions=False)
        again = ctx.sample(S, seed=11, positions=False)
        other = ctx.sample(S, seed=12, positions=False)
        assert torch.equal(out["x"], again["x"]) and not torch.equal(out["x"], other["x"])
        assert torch.equal(out["x"], ctx.sample(S, z=z, positions=False)["x"]), "seed = the documented generator"
        var_ref = np.einsum("npp->np", ref.dense_blocks(ab, fixed))
        free = ~fixed
        lo, hi = 1 - 6 * np.sqrt(2 / (S - 1)), 1 + 6 * np.sqrt(2 / (S - 1))
        for who, d in (("reference", sref.banded_map(ab, fixed, z.cpu().numpy())), ("gpu", out["x"].cpu().numpy() - x[None])):
            ratio = d.var(axis=0, ddof=1)[free] / var_ref[free]
            mean = np.abs(d.mean(axis=0))[free] / np.sqrt(var_ref[free] / S)
            print(f"\n[monte carlo, {who}] variance ratio in [{ratio.min():.4f}, {ratio.max():.4f}] (band [{lo:.4f}, {hi:.4f}]), "
                  f"max |mean| = {mean.max():.2f} standard errors (band 6)")
            assert ratio.min() >= lo and ratio.max() <= hi, who
            assert mean.max() <= 6.0, who
    finally:
        ctx.close()


def test_positions_rates_and_clip(mods):
    """positions = the oracle FK of the returned x (the tolerance of test_gpu_parity's acino_fk_active check), dx / ddx = the
    numpy restatement of k_derivatives on every sample and clip (same operations: 1e-12 of the largest entry), clip=True
    stays inside the box."""
    _lib, fte, synth = mods
    seq, model = _input(fte, synth, "bound 120")
    ctx = _solved_context(fte, seq, model)
    try:
        out = ctx.sample(5, seed=3, rates=True)
        assert set(out) == {"x", "positions", "dx", "ddx"}
        xs = out["x"].cpu().numpy()
        assert xs.shape == (5, 120, 25) and tuple(out["positions"].shape) == (5, 120, 20, 3)
        q = np.zeros((5 * 120, 45))
        q[:, ofk.ACTIVE] = xs.reshape(-1, 25)
        assert np.abs(out["positions"].cpu().numpy().reshape(-1, 20, 3) - ofk.cheetah_fk(q)).max() < 1e-13
        for s in range(5):
            dx, ddx = rref.derivatives(xs[s], ctx.Ts)
            assert np.abs(out["dx"][s].cpu().numpy() - dx).max() <= 1e-12 * np.abs(dx).max()
            assert np.abs(out["ddx"][s].cpu().numpy() - ddx).max() <= 1e-12 * np.abs(ddx).max()
        lo, hi = fte.bounds45()
        lo, hi = lo[fte.ACTIVE], hi[fte.ACTIVE]
        z = 40.0 * torch.randn((64, 120, 25), dtype=torch.float64, device=ctx.device)      # 40 sigma: far outside the box
        big = ctx.sample(64, z=z)["x"].cpu().numpy()
        assert (big < lo).any() and (big > hi).any(), "no sample leaves the box: clip=True would be untested"
        cl = ctx.sample(64, z=z, clip=True)
        xc = cl["x"].cpu().numpy()
        assert np.all(xc >= lo) and np.all(xc <= hi) and np.array_equal(xc, np.clip(big, lo, hi))
        q = np.zeros((64 * 120, 45))
        q[:, ofk.ACTIVE] = xc.reshape(-1, 25)
        assert np.abs(cl["positions"].cpu().numpy().reshape(-1, 20, 3) - ofk.cheetah_fk(q)).max() < 1e-13
    finally:
        ctx.close()
    # per clip: no difference across a seam
    seqs = [synth.make_sequence(30, "sprint", seed=20210313 + i) for i in range(2)]
    ctx = fte.FTEContext(np.concatenate([s["det"] for s in seqs]), *_rig(seqs[0]), seqs[0]["Ts"], clip_len=30)
    try:
        ctx.set_x(np.concatenate([fte.nose_line_init(s["det"], *_rig(s), 0.5) for s in seqs])[:, ofk.ACTIVE])
        ctx.solve(60)
        out = ctx.sample(2, seed=1, rates=True)
        xs = out["x"].cpu().numpy()
        for s in range(2):
            for b in range(2):
                dx, ddx = rref.derivatives(xs[s, b * 30:(b + 1) * 30], ctx.Ts)
                assert np.abs(out["dx"][s, b * 30:(b + 1) * 30].cpu().numpy() - dx).max() <= 1e-12 * np.abs(dx).max()
                assert np.abs(out["ddx"][s, b * 30:(b + 1) * 30].cpu().numpy() - ddx).max() <= 1e-12 * np.abs(ddx).max()
    finally:
        ctx.close()


def test_step_and_covariance_after_sample_are_bit_identical(mods):
    """The call leaves solver state, buffers and the captured graph alone: two contexts walk the same steps on a side stream
    with graphs enabled, one of them samples in between; its covariance before and after a sample is the same bits."""
    _lib, fte, synth = mods
    seq = synth.make_sequence(600, "trot")
    x0 = fte.nose_line_init(seq["det"], *_rig(seq), 0.5)[:, ofk.ACTIVE]
    outs = []
    stream = torch.cuda.Stream()
    for with_samples in (False, True):
        with torch.cuda.stream(stream):
            ctx = fte.FTEContext(seq["det"], *_rig(seq), seq["Ts"])
            try:
                ctx.enable_graph(True)
                ctx.set_x(x0)
                trace = []
                for it in range(6):
                    ctx.step()
                    if with_samples and it in (1, 3, 4):
                        before = ctx.covariance()
                        ctx.sample(70, seed=it)
                        after = ctx.covariance()
                        assert all(torch.equal(a, b) for a, b in zip(before, after))
                    st = ctx.state()
                    trace.append((st["cost"], st["cost_trial"], st["lam"], st["iter"], st["accepted"]))
                assert ctx.graphs_active() & 16
                outs.append((ctx.result()[0].clone(), trace))
            finally:
                ctx.close()
        stream.synchronize()
    assert torch.equal(outs[0][0], outs[1][0])
    assert outs[0][1] == outs[1][1]


def test_unsupported_contexts_and_bad_workspaces_are_refused(mods):
    """Sharded (pinned separator), windowed (own range) and bf16 contexts: ACINO_ERR_UNSUPPORTED (-5) before any launch, a
    message that says why, outputs and workspace untouched; a short or misaligned workspace: ACINO_ERR_WORKSPACE (-3)."""
    _lib, fte, synth = mods
    seq = synth.make_sequence(60, "sprint")
    lib = _lib.lib()
    z = torch.zeros((2, 60, 25), dtype=torch.float64, device="cuda")
    for kw, why in ((dict(pin_right=True, n_global=120), "sharded"), (dict(own_first=3, own_count=30), "windowed"),
                    (dict(precision="bf16"), "bf16")):
        ctx = fte.FTEContext(seq["det"], *_rig(seq), seq["Ts"], **kw)
        try:
            nbytes = lib.acino_fte_sample_workspace_bytes(C.byref(ctx.params))
            ws = torch.zeros(nbytes + 256, dtype=torch.uint8, device=ctx.device)
            xs = torch.full((2, 60, 25), -1.0, dtype=torch.float64, device=ctx.device)
            base = (ws.data_ptr() + 255) // 256 * 256
            rc = lib.acino_fte_sample(ctx._h, 2, _lib.ptr(z), C.c_void_p(base), nbytes, _lib.ptr(xs), None, _lib.stream_ptr())
            assert rc == -5
            assert why in lib.acino_last_error_string().decode()
            torch.cuda.synchronize()
            assert bool((xs == -1.0).all()) and not bool(ws.any())
            with pytest.raises(RuntimeError, match="not supported"):
                ctx.sample(2)
        finally:
            ctx.close()
    ctx = fte.FTEContext(seq["det"], *_rig(seq), seq["Ts"])
    try:
        ctx.set_x(np.zeros((60, 25)))
        nbytes = lib.acino_fte_sample_workspace_bytes(C.byref(ctx.params))
        ws = torch.zeros(nbytes + 512, dtype=torch.uint8, device=ctx.device)
        xs = torch.empty((2, 60, 25), dtype=torch.float64, device=ctx.device)
        base = (ws.data_ptr() + 255) // 256 * 256
        args = (_lib.ptr(xs), None, _lib.stream_ptr())
        assert lib.acino_fte_sample(ctx._h, 2, _lib.ptr(z), C.c_void_p(base), nbytes - 8, *args) == -3
        assert lib.acino_fte_sample(ctx._h, 2, _lib.ptr(z), C.c_void_p(base + 8), nbytes, *args) == -3
        with pytest.raises(ValueError):
            ctx.sample(0)
        with pytest.raises(ValueError):
            ctx.sample(2, z=torch.zeros((3, 60, 25), dtype=torch.float64, device="cuda"))
    finally:
        ctx.close()


def test_solve_entries_return_samples(mods):
    """n_samples=8 on fte_solve / fte_solve_clips: keys, shapes, numpy in -> numpy out, and the point-estimate entries
    bit-identical to the same call with n_samples=0; fte_solve_batch with tensors out."""
    _lib, fte, synth = mods
    seq = synth.make_sequence(60, "sprint")
    args = (seq["det"][..., :2], seq["det"][..., 2], *_rig(seq), seq["Ts"])
    plain, ip = fte.fte_solve(*args, max_iter=60)
    withs, iw = fte.fte_solve(*args, max_iter=60, n_samples=8, sample_seed=5)
    assert set(withs) - set(plain) == {"x_samples", "positions_samples"}
    assert all(np.array_equal(plain[k], withs[k]) for k in plain if k != "start_frame") and ip["iter"] == iw["iter"]
    assert isinstance(withs["x_samples"], np.ndarray) and withs["x_samples"].shape == (8, 60, 25)
    assert isinstance(withs["positions_samples"], np.ndarray) and withs["positions_samples"].shape == (8, 60, 20, 3)
    assert np.isfinite(withs["x_samples"]).all() and np.abs(withs["x_samples"] - withs["x"][None]).max() > 0.0
    seqs = [synth.make_sequence(45, "sprint", seed=20210313 + i) for i in range(3)]
    dets = [s["det"] for s in seqs]
    plain_c = fte.fte_solve_clips(dets, *_rig(seq), seq["Ts"], max_iter=60)
    with_c = fte.fte_solve_clips(dets, *_rig(seq), seq["Ts"], max_iter=60, n_samples=8)
    for (rp, _ip), (rw, _iw) in zip(plain_c, with_c):
        assert set(rw) - set(rp) == {"x_samples", "positions_samples"}
        assert all(np.array_equal(rp[k], rw[k]) for k in rp if k != "start_frame")
        assert isinstance(rw["x_samples"], np.ndarray) and rw["x_samples"].shape == (8, 45, 25)
        assert rw["positions_samples"].shape == (8, 45, 20, 3)
        assert np.isfinite(rw["x_samples"]).all() and np.abs(rw["x_samples"] - rw["x"][None]).max() > 0.0
    for res, _info in fte.fte_solve_batch(dets, *_rig(seq), seq["Ts"], max_iter=60, n_samples=8, return_numpy=False):
        assert isinstance(res["x_samples"], torch.Tensor) and tuple(res["x_samples"].shape) == (8, 45, 25)
        assert tuple(res["positions_samples"].shape) == (8, 45, 20, 3)
