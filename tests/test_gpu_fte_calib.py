"""FTE error bars that include the calibration, on the GPU (k_fte_calib_rhs / k_fte_sample_fwdsub / k_fte_sample_backsub<true> /
k_fte_calib_combine, acino_fte_calibration_sensitivity, FTEContext.calibration_sensitivity, cov_cams=) against the CPU reference
tests/fte_calib_ref.py.

The sensitivity S = -A^-1 G is checked per column, with the metric of fte_sample_ref.map_err (fte_calib_ref.col_err):
    e = max_col ( max_n ||S_gpu[n, :, col] - S_ref[n, :, col]||_2 / max_n ||S_ref[n, :, col]||_2 )
against reference 1 (banded Cholesky solve), with the bar set by the REFERENCES on the very matrix under test: d0 = the same
metric between reference 1 and reference 2 (dense LU solve), e <= max(64 d0, 1e-13) (fte_cov_ref.bar).  Every test prints d0
and e (pytest -s) before it asserts; the figures measured on the MI355X are in DESIGN section 6.
Inputs and context set-up: those of tests/test_gpu_fte_sample.py (its helpers are module-private and restated here).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import fte_calib_ref as kref
import fte_cov_ref as ref
import pinhole_fte_ref as pref
from oracle import fk as ofk
from oracle import fte as ofte

pytestmark = pytest.mark.gpu
P = 25
EPS = np.finfo(float).eps


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


def _solved_context(fte, seq, model="fisheye", max_iter=100, init_cams=None, **kw):
    """init_cams: the cameras the nose-line initial guess triangulates from (its pair mask holds at most 8)."""
    ctx = fte.FTEContext(seq["det"], *_rig(seq), seq["Ts"], camera_model=model, **kw)
    ic = slice(None) if init_cams is None else slice(0, init_cams)
    x0 = fte.nose_line_init(seq["det"][:, ic], *(a[ic] for a in _rig(seq)), 0.5, camera_model=model)
    ctx.set_x(x0[:, ofk.ACTIVE])
    info = ctx.solve(max_iter)
    assert info["status_name"] in ("ftol", "xtol", "gtol"), info
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
    if kind == "rig12":
        return synth.make_sequence(n, "sprint", rig=synth.make_rig(12)), "fisheye"
    seq = synth.make_sequence(n, "sprint")
    if kind == "gap":
        seq["det"][45:75, :, :, 2] = 0.0
    return seq, "fisheye"


def _references(ctx, seq, model, clip_len=0):
    """(x, fixed, S1, S2, d0): the two CPU solves of the context's own matrix with the oracle's cross term at its iterate."""
    x, fixed, ab = _reference_system(ctx, clip_len)
    G = kref.cross_term(x, np.asarray(seq["det"]), _rig(seq), seq["Ts"], model)
    S1, S2 = kref.sens_banded(ab, fixed, G), kref.sens_dense(ab, fixed, G)
    return x, fixed, S1, S2, kref.col_err(S2, S1)


def _check_sens(name, ctx, seq, model):
    x, fixed, S1, S2, d0 = _references(ctx, seq, model)
    out = ctx.calibration_sensitivity()
    assert set(out) == {"sens", "cov_x_cal", "cov_pos_cal", "std_pos_cal"}
    assert out["cov_x_cal"] is None and out["cov_pos_cal"] is None and out["std_pos_cal"] is None
    S = out["sens"].cpu().numpy()
    assert S.shape == (ctx.N, P, 6 * ctx.C)
    e = kref.col_err(S, S1)
    print(f"\n[{name}] d0 = {d0:.2e}   bar = {ref.bar(d0):.2e}   e = {e:.2e}   max |S| = {np.abs(S1).max():.2f}")
    assert np.isfinite(S).all()
    assert np.all(S[fixed] == 0.0), "rows of a pinned variable must be exactly 0"
    assert e <= ref.bar(d0), (name, e, ref.bar(d0))
    return fixed


@pytest.mark.parametrize("name", ["fisheye 7", "fisheye 121", "fisheye 122", "pinhole 30", "gap 120", "bound 120"])
def test_sensitivity_against_the_banded_solve(mods, name):
    """Test 1: S on all frames and all 36 columns - whole and ragged last nodes (7 = 3 + 3 + 1), both camera models, the
    detection gap, the bound-active knee (rows of pinned variables exactly 0)."""
    _lib, fte, synth = mods
    seq, model = _input(fte, synth, name)
    ctx = _solved_context(fte, seq, model)
    try:
        fixed = _check_sens(name, ctx, seq, model)
        if name.startswith("bound"):
            assert fixed[:, 12].sum() >= ctx.N // 2, "the active set is (almost) empty: the test is void"
    finally:
        ctx.close()


def test_more_than_one_panel_of_columns(mods):
    """Test 2: 12 cameras = 72 columns, two panels of 64 with a ragged second one (30 frames).  synth.make_rig(12) walks the
    ring of six centres twice; every marker must be seen by >= 2 cameras in the reference or the rig is not usable."""
    _lib, fte, synth = mods
    seq, model = _input(fte, synth, "rig12 30")
    w = kref.problem(seq["det"], _rig(seq), seq["Ts"]).w
    assert seq["det"].shape[1] == 12 and int((w > 0).sum(axis=1).min()) >= 2, "a marker is seen by fewer than 2 cameras"
    ctx = _solved_context(fte, seq, model, init_cams=6)
    try:
        _check_sens("rig12 30", ctx, seq, model)
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def sprint(mods):
    """One solved 120-frame sprint context with its references, shared by the tests below (none of them changes it)."""
    _lib, fte, synth = mods
    seq, model = _input(fte, synth, "fisheye 120")
    ctx = _solved_context(fte, seq, model)
    x, fixed, S1, S2, d0 = _references(ctx, seq, model)
    yield dict(ctx=ctx, seq=seq, x=x, fixed=fixed, S1=S1, S2=S2, d0=d0)
    ctx.close()


def test_translating_the_rig_moves_the_trajectory(sprint):
    """Test 3: for gen = [0, -R_0 a, 0, -R_1 a, ...] S_n gen = (a, 0, ..., 0) on every frame whose head position is free - no
    reference needed.  Held to bar(d_id), d_id the reference's own error in the identity."""
    S = sprint["ctx"].calibration_sensitivity()["sens"].cpu().numpy()
    R = sprint["seq"]["R"]
    for a in (np.array([1.0, 0.0, 0.0]), np.array([0.0, 0.0, 1.0]), np.array([0.3, -0.5, 0.2])):
        d_id = kref.identity_error(sprint["S1"], sprint["fixed"], R, a)
        e = kref.identity_error(S, sprint["fixed"], R, a)
        print(f"\n[identity] a = {a}: d_id = {d_id:.2e}   bar = {ref.bar(d_id):.2e}   e = {e:.2e}")
        assert e <= ref.bar(d_id)


def _glob_err(A, A_ref):
    """max_n ||A[n] - A_ref[n]|| / max_n ||A_ref[n]|| (Frobenius per frame): the per-column metric's shape for per-frame blocks."""
    A, R = np.asarray(A).reshape(A.shape[0], -1), np.asarray(A_ref).reshape(A_ref.shape[0], -1)
    return float(np.linalg.norm(A - R, axis=1).max() / np.linalg.norm(R, axis=1).max())


def test_calibration_covariances(sprint):
    """Test 4: cov_x_cal, cov_pos_cal, std_pos_cal against S1 Sigma S1^T through the oracle's FK Jacobian, Sigma a fixed-seed PSD
    matrix with camera 0 held (zero rows: it must never be factored).  Bar per output: 64 times what the two references
    make of the same output (fte_cov_ref.bar).  cov_x_cal and cov_pos_cal equal their transposes bit for bit; std^2 = trace
    to the rounding of one square root and one square (4 eps)."""
    ctx = sprint["ctx"]
    sigma = kref.random_psd(6)
    out = ctx.calibration_sensitivity(sigma)
    want1 = kref.calib_cov(sprint["S1"], sigma, sprint["x"])
    want2 = kref.calib_cov(sprint["S2"], sigma, sprint["x"])
    got = [out[k].cpu().numpy() for k in ("cov_x_cal", "cov_pos_cal", "std_pos_cal")]
    assert got[0].shape == (120, 25, 25) and got[1].shape == (120, 20, 3, 3) and got[2].shape == (120, 20)
    worst = []
    for name, g, w1, w2 in zip(("cov_x_cal", "cov_pos_cal", "std_pos_cal"), got, want1, want2):
        d0, e = _glob_err(w2, w1), _glob_err(g, w1)
        print(f"\n[{name}] d0 = {d0:.2e}   bar = {ref.bar(d0):.2e}   e = {e:.2e}")
        assert np.isfinite(g).all()
        worst.append((name, e, ref.bar(d0)))
    print(f"[std_pos_cal] median {np.median(got[2]) * 1e3:.3f} mm")
    assert np.array_equal(got[0], got[0].transpose(0, 2, 1)) and np.array_equal(got[1], got[1].transpose(0, 1, 3, 2))
    assert np.all(got[0][sprint["fixed"]] == 0.0)
    tr = np.einsum("nlii->nl", got[1])
    assert np.all(np.abs(got[2] ** 2 - tr) <= 4 * EPS * tr)
    assert torch.equal(out["sens"], ctx.calibration_sensitivity()["sens"]), "sens does not depend on cov_cams"
    for name, e, tol in worst:
        assert e <= tol, (name, e, tol)


def test_clips_equal_the_clips_alone(mods, monkeypatch):
    """Test 5: 3 clips of 8 frames in one context against each clip alone at the same iterate: bit-identical (both contexts
    assemble with the same launch shape, so that they hold the same H)."""
    _lib, fte, synth = mods
    monkeypatch.setenv("ACINO_ASM_SPLIT", "1")
    S, B = 8, 3
    seqs = [synth.make_sequence(S, "sprint", seed=20210313 + i) for i in range(B)]
    rig, Ts = _rig(seqs[0]), seqs[0]["Ts"]
    det = np.concatenate([s["det"] for s in seqs])
    x0 = np.concatenate([fte.nose_line_init(s["det"], *rig, 0.5) for s in seqs])[:, ofk.ACTIVE]
    sigma = kref.random_psd(6)
    ctx = fte.FTEContext(det, *rig, Ts, clip_len=S)
    try:
        ctx.set_x(x0)
        ctx.solve(60)
        x = ctx.result()[0]
        both = ctx.calibration_sensitivity(sigma)
    finally:
        ctx.close()
    assert bool(torch.isfinite(both["sens"]).all()) and float(both["sens"].abs().max()) > 0.0
    for b in range(B):
        sl = slice(b * S, (b + 1) * S)
        one = fte.FTEContext(seqs[b]["det"], *rig, Ts)
        try:
            one.set_x(x[sl].contiguous())
            alone = one.calibration_sensitivity(sigma)
        finally:
            one.close()
        for k in ("sens", "cov_x_cal", "cov_pos_cal", "std_pos_cal"):
            same = torch.equal(alone[k], both[k][sl])
            print(f"[clips 3 x 8] clip {b} {k}: bit-identical = {same}")
            assert same, (b, k)


def test_nothing_else_moved_and_a_repeat_is_bit_identical(sprint):
    """Test 6: result(), covariance() and sample(4, z=...) give the same bits before and after a call; a second call gives the
    bits of the first."""
    ctx = sprint["ctx"]
    sigma = kref.random_psd(6)
    z = torch.as_tensor(np.random.default_rng(5).normal(size=(4, ctx.N, P)), device=ctx.device)

    def snapshot():
        return list(ctx.result()) + list(ctx.covariance()) + [ctx.sample(4, z=z, positions=False)["x"]]

    before = snapshot()
    first = ctx.calibration_sensitivity(sigma)
    after = snapshot()
    second = ctx.calibration_sensitivity(sigma)
    assert all(torch.equal(a, b) for a, b in zip(before, after))
    assert all(torch.equal(first[k], second[k]) for k in first)


def test_statuses(mods):
    """Test 7: all outputs NULL and d_cov_x_cal without d_cov_cams: ACINO_ERR_INVALID_ARG (-1); a misaligned or short workspace:
    ACINO_ERR_WORKSPACE (-3); a bf16 or a windowed context: ACINO_ERR_UNSUPPORTED (-5).  None of them launches anything:
    outputs and workspace keep their fill."""
    _lib, fte, synth = mods
    seq = synth.make_sequence(60, "sprint")
    lib = _lib.lib()
    call = lib.acino_fte_calibration_sensitivity
    sigma = torch.as_tensor(kref.random_psd(6), device="cuda")

    def buffers(ctx):
        nbytes = lib.acino_fte_calibration_workspace_bytes(C.byref(ctx.params))
        ws = torch.zeros(nbytes + 512, dtype=torch.uint8, device=ctx.device)
        sens = torch.full((60, 25, 36), -1.0, dtype=torch.float64, device=ctx.device)
        cov = torch.full((60, 25, 25), -1.0, dtype=torch.float64, device=ctx.device)
        return nbytes, ws, (ws.data_ptr() + 255) // 256 * 256, sens, cov

    def untouched(ws, sens, cov):
        torch.cuda.synchronize()
        return bool((sens == -1.0).all()) and bool((cov == -1.0).all()) and not bool(ws.any())

    for kw, why in ((dict(own_first=3, own_count=30), "windowed"), (dict(precision="bf16"), "bf16")):
        ctx = fte.FTEContext(seq["det"], *_rig(seq), seq["Ts"], **kw)
        try:
            nbytes, ws, base, sens, cov = buffers(ctx)
            rc = call(ctx._h, _lib.ptr(sigma), C.c_void_p(base), nbytes, _lib.ptr(sens), _lib.ptr(cov), None, None,
                      _lib.stream_ptr())
            assert rc == -5 and why in lib.acino_last_error_string().decode()
            assert untouched(ws, sens, cov)
            with pytest.raises(RuntimeError, match="not supported"):
                ctx.calibration_sensitivity()
        finally:
            ctx.close()
    ctx = fte.FTEContext(seq["det"], *_rig(seq), seq["Ts"])
    try:
        ctx.set_x(np.zeros((60, 25)))
        nbytes, ws, base, sens, cov = buffers(ctx)
        tail = (None, None, _lib.stream_ptr())
        assert call(ctx._h, _lib.ptr(sigma), C.c_void_p(base), nbytes, None, None, *tail) == -1
        assert call(ctx._h, None, C.c_void_p(base), nbytes, _lib.ptr(sens), _lib.ptr(cov), *tail) == -1
        assert "d_cov_cams" in lib.acino_last_error_string().decode()
        assert call(ctx._h, _lib.ptr(sigma), C.c_void_p(base + 8), nbytes, _lib.ptr(sens), _lib.ptr(cov), *tail) == -3
        assert call(ctx._h, _lib.ptr(sigma), C.c_void_p(base), nbytes - 8, _lib.ptr(sens), _lib.ptr(cov), *tail) == -3
        assert untouched(ws, sens, cov)
        for bad in (np.zeros((30, 30)), np.full((36, 36), np.nan), np.triu(np.ones((36, 36)))):
            with pytest.raises(ValueError):
                ctx.calibration_sensitivity(bad)
    finally:
        ctx.close()


def test_solve_entries_return_the_calibration_term(mods):
    """Test 8: fte_solve(..., cov_cams=Sigma, return_cov=True): the new keys and shapes, std_positions_total = the formula; the
    same call without cov_cams has exactly today's key set; cov_cams alone adds no total; the dict of sba.covariance is taken
    by its "cov_cams"; fte_solve_clips slices per clip."""
    _lib, fte, synth = mods
    from acinoset_amd import calib
    seq = synth.make_sequence(60, "sprint")
    args = (seq["det"][..., :2], seq["det"][..., 2], *_rig(seq), seq["Ts"])
    sigma = calib.extrinsic_cov(6, 0.05, 2e-3, fixed=(0,))
    plain, _ = fte.fte_solve(*args, max_iter=60, return_cov=True)
    assert set(plain) == {"positions", "x", "dx", "ddx", "start_frame", "cov_x", "cov_positions", "std_positions"}
    full, _ = fte.fte_solve(*args, max_iter=60, return_cov=True, cov_cams=sigma)
    new = {"sens_cams", "cov_x_calib", "cov_positions_calib", "std_positions_calib", "std_positions_total"}
    assert set(full) - set(plain) == new
    assert all(np.array_equal(plain[k], full[k]) for k in plain if k != "start_frame")
    assert full["sens_cams"].shape == (60, 25, 36) and full["cov_x_calib"].shape == (60, 25, 25)
    assert full["cov_positions_calib"].shape == (60, 20, 3, 3) and full["std_positions_calib"].shape == (60, 20)
    assert all(isinstance(full[k], np.ndarray) and np.isfinite(full[k]).all() for k in new)
    want = np.sqrt(full["std_positions"] ** 2 + full["std_positions_calib"] ** 2)
    assert np.all(np.abs(full["std_positions_total"] - want) <= 4 * EPS * want)
    assert float(full["std_positions_calib"].min()) > 0.0
    only, _ = fte.fte_solve(*args, max_iter=60, cov_cams=dict(cov_cams=sigma, cov_points=None))
    assert set(only) - {"positions", "x", "dx", "ddx", "start_frame"} == new - {"std_positions_total"}
    assert np.array_equal(only["sens_cams"], full["sens_cams"])
    seqs = [synth.make_sequence(45, "sprint", seed=20210313 + i) for i in range(2)]
    for res, _info in fte.fte_solve_clips([s["det"] for s in seqs], *_rig(seq), seq["Ts"], max_iter=60, return_cov=True,
                                          cov_cams=sigma, return_numpy=False):
        assert isinstance(res["sens_cams"], torch.Tensor) and tuple(res["sens_cams"].shape) == (45, 25, 36)
        assert tuple(res["std_positions_total"].shape) == (45, 20)
    for res, _info in fte.fte_solve_batch([s["det"] for s in seqs], *_rig(seq), seq["Ts"], max_iter=60, cov_cams=sigma):
        assert res["sens_cams"].shape == (45, 25, 36) and "std_positions_total" not in res
