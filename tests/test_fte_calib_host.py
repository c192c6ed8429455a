"""FTE error bars that include the calibration, the part that needs no GPU: the C ABI of acino_fte_calibration_sensitivity
(header, export, signature, argument validation before any device call), the Python interface (FTEContext.
calibration_sensitivity, cov_cams= on the solve entries, calib.extrinsic_cov) and the CPU reference tests/fte_calib_ref.py
pinned to itself: J_c against central differences of the oracle projection, the banded against the dense solve, and the
exact identity "translate the rig, the trajectory follows"."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import fte_calib_ref as kref
import fte_cov_ref as cref
import fte_reproj_ref as rref
import pinhole_fte_ref as pref
from oracle import fk as ofk
from oracle import synth as osynth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "acino_fte_calibration_sensitivity"
EPS = np.finfo(float).eps


def test_header_export_signature_and_argument_checks():
    """Fails without the feature: both functions are declared, exported and bound; the ABI version stays 3; a null context,
    all-null outputs and a cov / std output without d_cov_cams are ACINO_ERR_INVALID_ARG (-1) before anything touches a
    device; the workspace is the covariance workspace + 2 * 6C * N * 25 doubles."""
    from acinoset_amd import _lib
    with open(os.path.join(ROOT, "include", "acinoset_hip.h")) as f:
        header = f.read()
    for name in (NAME, "acino_fte_calibration_workspace_bytes"):
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name} not declared in acinoset_hip.h"
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES[NAME][1]) == 9
    assert "NOT a derivative" in header and "fte_calib.hip" in _lib.SOURCES
    import __graft_entry__ as entry
    entry.build()
    h = _lib.lib()
    assert hasattr(h, NAME)
    assert h.acino_abi_version() == 3
    fake = C.c_void_p(256)                                   # never dereferenced: the argument checks come first
    assert h.acino_fte_calibration_sensitivity(None, None, fake, 0, fake, None, None, None, None) == -1
    assert "invalid argument" in h.acino_last_error_string().decode()
    assert h.acino_fte_calibration_sensitivity(fake, fake, fake, 0, None, None, None, None, None) == -1
    assert "no output" in h.acino_last_error_string().decode()
    for outs in ((fake, None, None), (None, fake, None), (None, None, fake)):
        assert h.acino_fte_calibration_sensitivity(fake, None, fake, 0, fake, *outs, None) == -1
        assert "d_cov_cams" in h.acino_last_error_string().decode()
    p = _lib.FteParams()
    p.n_frames, p.n_cams, p.clip_len = 121, 6, 0
    cov = h.acino_fte_covariance_workspace_bytes(C.byref(p))
    assert h.acino_fte_calibration_workspace_bytes(C.byref(p)) == cov + 2 * 36 * 121 * 25 * 8
    p.n_cams = 0
    assert h.acino_fte_calibration_workspace_bytes(C.byref(p)) == 0


def test_python_interface_defaults_off_and_value_errors():
    from acinoset_amd import calib, fte
    sig = inspect.signature(fte.FTEContext.calibration_sensitivity).parameters
    assert list(sig) == ["self", "cov_cams"] and sig["cov_cams"].default is None
    for fn in (fte.fte_solve, fte.fte_solve_clips, fte.fte_solve_batch):
        assert inspect.signature(fn).parameters["cov_cams"].default is None
    res = {}
    fte._attach_posterior(res, None, lambda a: a)
    assert res == {}
    good = calib.extrinsic_cov(6, 0.05, 2e-3, fixed=(0,))
    assert fte._cov_cams_matrix(None, 6) is None
    assert np.array_equal(fte._cov_cams_matrix(good, 6), good)
    assert np.array_equal(fte._cov_cams_matrix(dict(cov_cams=good, cov_points=None), 6), good)
    bad_nan = good.copy()
    bad_nan[7, 7] = np.nan
    bad_asym = good.copy()
    bad_asym[7, 8] = 1e-6
    for bad in (good[:30, :30], good[:, :30], bad_nan, bad_asym, dict(cov_points=good)):
        with pytest.raises(ValueError):
            fte._cov_cams_matrix(bad, 6)
    # the solve entries refuse a malformed matrix before they need a device
    z = np.zeros((4, 6, 20, 3))
    rig = osynth.make_rig()
    with pytest.raises(ValueError, match="cov_cams"):
        fte.fte_solve(z[..., :2], z[..., 2], *rig, 1 / 90, cov_cams=good[:30, :30])
    with pytest.raises(ValueError, match="cov_cams"):
        fte.fte_solve_clips([z, z], *rig, 1 / 90, cov_cams=bad_asym)
    with pytest.raises(ValueError, match="cov_cams"):
        fte.fte_solve_batch([z, z], *rig, 1 / 90, cov_cams=bad_nan)


class _FakeContext:
    """The five public calls FTEContext._posterior composes, on the CPU: constants of the documented shapes, every call logged."""

    def __init__(self, n=10, c=6):
        import torch
        self.calls = []
        self._new = lambda *shape: torch.ones((n,) + shape, dtype=torch.float64)
        self.n, self.c = n, c

    def _cov(self):
        return self._new(25, 25), self._new(20, 3, 3), 3.0 * self._new(20)

    def _rates(self):
        return self._new(25, 25), self._new(25, 25), self._new(20, 3, 3), self._new(20)

    def covariance(self):
        self.calls.append("covariance")
        self.cov = self._cov()
        return self.cov

    def covariance_rates(self, with_cov=False):
        self.calls.append(("covariance_rates", with_cov))
        self.cov = self._cov() if with_cov else None
        return (self._rates(), self.cov) if with_cov else self._rates()

    def reprojection(self, cov_pos=None):
        self.calls.append("reprojection")
        self.cov_pos_given = cov_pos
        s = (self.c, 20)
        return dict(uv=self._new(*s, 2), cov_uv=self._new(*s, 2, 2), std_uv=self._new(*s), res=self._new(*s, 2),
                    weight=self._new(*s, 2), mahal2=self._new(*s), flags=self._new(*s))

    def calibration_sensitivity(self, cov_cams=None):
        self.calls.append("calibration_sensitivity")
        return dict(sens=self._new(25, 6 * self.c), cov_x_cal=self._new(25, 25), cov_pos_cal=self._new(20, 3, 3),
                    std_pos_cal=4.0 * self._new(20))


COV_KEYS = {"cov_x", "cov_positions", "std_positions"}
RATE_KEYS = {"cov_dx", "cov_ddx", "cov_velocities", "std_velocities"}
REPROJ_KEYS = {"uv", "cov_uv", "std_uv", "residuals", "weights", "mahal2", "flags"}
CALIB_KEYS = {"sens_cams", "cov_x_calib", "cov_positions_calib", "std_positions_calib"}


def test_posterior_composition_rules():
    """FTEContext._posterior on a context of CPU stand-ins: covariance and rates come from ONE covariance_rates(with_cov=True)
    (the three and the four keys), the reprojection is handed that call's cov_positions, std_positions_total exists only when both the covariance
    and the calibration term do and is sqrt(3^2 + 4^2) = 5 here; _attach_posterior slices every key on the frame axis."""
    from acinoset_amd import fte
    post_of = fte.FTEContext._posterior
    sigma = np.eye(36)
    ctx = _FakeContext()
    assert post_of(ctx) == {} and ctx.calls == []
    post = post_of(ctx, return_cov=True, return_rate_cov=True)
    assert ctx.calls == [("covariance_rates", True)] and set(post) == COV_KEYS | RATE_KEYS and len(post) == 7
    assert post["cov_positions"] is ctx.cov[1]
    ctx = _FakeContext()
    assert set(post_of(ctx, return_cov=True)) == COV_KEYS and ctx.calls == ["covariance"]
    ctx = _FakeContext()
    assert set(post_of(ctx, return_rate_cov=True)) == RATE_KEYS and ctx.calls == [("covariance_rates", False)]
    ctx = _FakeContext()
    post = post_of(ctx, return_cov=True, return_reprojection=True)
    assert ctx.calls == ["covariance", "reprojection"] and ctx.cov_pos_given is ctx.cov[1]
    assert set(post) == COV_KEYS | REPROJ_KEYS
    ctx = _FakeContext()
    assert set(post_of(ctx, return_reprojection=True)) == REPROJ_KEYS and ctx.cov_pos_given is None
    ctx = _FakeContext()
    assert set(post_of(ctx, cov_cams=sigma)) == CALIB_KEYS and ctx.calls == ["calibration_sensitivity"]
    ctx = _FakeContext()
    assert set(post_of(ctx, return_rate_cov=True, cov_cams=sigma)) == RATE_KEYS | CALIB_KEYS
    ctx = _FakeContext()
    post = post_of(ctx, return_cov=True, return_rate_cov=True, return_reprojection=True, cov_cams=sigma)
    assert ctx.calls == [("covariance_rates", True), "reprojection", "calibration_sensitivity"]
    assert ctx.cov_pos_given is ctx.cov[1]
    assert set(post) == COV_KEYS | RATE_KEYS | REPROJ_KEYS | CALIB_KEYS | {"std_positions_total"}
    res = {}
    fte._attach_posterior(res, post, lambda a: a.numpy(), slice(5, 10))
    assert set(res) == set(post) and all(v.shape[0] == 5 for v in res.values())
    assert res["sens_cams"].shape == (5, 25, 36) and res["cov_uv"].shape == (5, 6, 20, 2, 2)
    assert res["std_positions_total"].shape == (5, 20) and np.all(res["std_positions_total"] == 5.0)


def test_extrinsic_cov():
    from acinoset_amd import calib
    S = calib.extrinsic_cov(3, 0.05, 2e-3, fixed=(1,))
    assert S.shape == (18, 18) and S.dtype == np.float64 and np.array_equal(S, np.diag(np.diag(S)))
    d = np.diag(S)
    assert np.allclose(d[:3], np.deg2rad(0.05) ** 2, rtol=1e-15) and np.allclose(d[3:6], 4e-6, rtol=1e-15)
    assert np.all(d[6:12] == 0.0) and np.array_equal(d[12:], d[:6])
    for args in ((0, 0.05, 2e-3), (3, -1.0, 2e-3), (3, 0.05, np.nan), (3, 0.05, 2e-3, (3,))):
        with pytest.raises(ValueError):
            calib.extrinsic_cov(*args)


# ---- the reference pinned to itself ---------------------------------------------------------------------------------
def _rig(seq):
    return seq["K"], seq["D"], seq["R"], seq["t"]


def _pinhole_sequence(n):
    """tests/pinhole_fte_ref.pinhole_sequence without the GPU: oracle FK and oracle.camera.project_points."""
    K, _, R, t = osynth.make_rig()
    D = np.tile(pref.D12, (K.shape[0], 1))
    q = osynth.trajectory(n, "sprint")
    pos = ofk.cheetah_fk(q)
    rng = np.random.default_rng(20210313)
    det = np.zeros((n, K.shape[0], 20, 3))
    for c in range(K.shape[0]):
        uv = pref.oracle_project(pos.reshape(-1, 3), K[c], D[c], R[c], t[c]).reshape(n, 20, 2)
        det[:, c, :, :2] = uv + rng.normal(0.0, 2.0, uv.shape)
        det[:, c, :, 2] = np.where(rng.uniform(size=(n, 20)) < 0.15, 0.2, 0.9)
    return dict(K=K, D=D, R=R, t=t, q_true=q, det=det, Ts=1.0 / osynth.FPS)


@pytest.mark.parametrize("model", ["fisheye", "pinhole"])
def test_camera_jacobian_against_central_differences(model):
    """J_c against central differences (step h = 1e-6) of the oracle projection under R <- exp([dw]x) R, t <- t + dt.  The bar
    is the rounding of the difference quotient: each of the two projections carries a few eps of its pixel value (taken
    as 4 eps max|uv|), so the quotient carries 4 eps max|uv| / h - about 1e-6 px per rad or m on entries up to 1e3; the
    truncation h^2 / 6 times a third derivative is orders below."""
    seq = osynth.make_sequence(9, "sprint") if model == "fisheye" else _pinhole_sequence(9)
    K, D, R, t = _rig(seq)
    pos = rref.positions(seq["q_true"][:, ofk.ACTIVE])
    h = 1e-6
    worst, biggest, uvmax = 0.0, 0.0, 0.0
    for c in range(K.shape[0]):
        uv, _, Jc, _ = kref.camera_jacobian(pos, _rig(seq), c, model)
        uvmax = max(uvmax, float(np.abs(uv).max()))
        biggest = max(biggest, float(np.abs(Jc).max()))
        for j in range(6):
            def f(s):
                Rn, tn = np.array(R, dtype=np.float64), np.array(t, dtype=np.float64).reshape(-1, 3)
                d = np.zeros(3)
                d[j % 3] = s * h
                if j < 3:
                    Rn[c] = kref.rot_exp(d) @ Rn[c]
                else:
                    tn[c] = tn[c] + d
                return rref.project(pos, (K, D, Rn, tn), c, model)[0]
            fd = (f(1) - f(-1)) / (2 * h)
            worst = max(worst, float(np.abs(fd - Jc[..., j]).max()))
    bar = 4 * EPS * uvmax / h
    print(f"\n[{model}] max |J_c - central differences| = {worst:.2e} (bar {bar:.2e}) on entries up to {biggest:.2e}")
    assert worst <= bar


def _problem(n, model="fisheye"):
    seq = osynth.make_sequence(n, "sprint") if model == "fisheye" else _pinhole_sequence(n)
    prob = kref.problem(seq["det"], _rig(seq), seq["Ts"], model)
    x = np.clip(seq["q_true"][:, ofk.ACTIVE], prob.lo, prob.hi)
    _, g, H, _ = prob.evaluate(x)
    Hd = cref.with_smooth_diag(H, prob.q_w, prob.s_band())
    fixed = cref.active_set(x, g, Hd, prob.lo, prob.hi)
    ab = cref.banded(Hd, fixed, prob.q_w, prob.s_band())
    return seq, x, fixed, ab, kref.cross_term(x, seq["det"], _rig(seq), seq["Ts"], model)


def _identity_scale(S, gen):
    """sum over the columns of |gen_col| times the column's largest frame norm: what a relative error of 1 in every column of
    S (the metric of col_err) can move S_n gen by."""
    return float((np.abs(gen) * np.linalg.norm(S, axis=1).max(axis=0)).sum())


@pytest.mark.parametrize("model,n", [("fisheye", 7), ("fisheye", 24), ("pinhole", 24)])
def test_references_agree_and_the_rig_translation_identity_holds(model, n):
    """Reference 1 (banded Cholesky) against reference 2 (dense LU) in the per-column metric: d0 <= 1e-8, the precondition of
    fte_cov_ref.bar.  Then the identity: for gen = [0, -R_0 a, 0, -R_1 a, ...] J_c gen = -J_pi a = -J_x e_a and the
    third-difference prior annihilates constants, so A (a, 0, ..., 0)_n = -G gen and S_n gen = (a, 0, ..., 0) for every frame
    whose head position is free.  It needs no reference; what the solves leave of it is bounded by their own relative
    error per column, bar(d0), times the identity's scale (_identity_scale)."""
    seq, x, fixed, ab, G = _problem(n, model)
    assert not fixed[:, :3].any(), "the head position is never at a bound here"
    S1, S2 = kref.sens_banded(ab, fixed, G), kref.sens_dense(ab, fixed, G)
    d0 = kref.col_err(S2, S1)
    print(f"\n[{model} {n}] references: d0 = {d0:.2e}   max |S| = {np.abs(S1).max():.2f}")
    tol = cref.bar(d0)
    assert np.all(S1[fixed] == 0.0) and np.all(S2[fixed] == 0.0)
    for a in (np.array([1.0, 0.0, 0.0]), np.array([0.0, 0.0, 1.0]), np.array([0.3, -0.5, 0.2])):
        gen = kref.translation_gen(seq["R"], a)
        for S in (S1, S2):
            e = kref.identity_error(S, fixed, seq["R"], a)
            print(f"[{model} {n}] a = {a}: |S gen - (a, 0)| = {e:.2e}   bar = {tol * _identity_scale(S, gen):.2e}")
            assert e <= tol * _identity_scale(S, gen)


def test_calibration_covariance_of_the_reference():
    """cov_x_cal = S Sigma S^T for a PSD Sigma with camera 0 held: symmetric, PSD, std^2 = trace, zero rows where S has them;
    a pure rig translation Sigma = gen gen^T sigma^2 moves every marker by sigma |a|: std_pos_cal = sigma |a| (the identity
    in covariance form)."""
    seq, x, fixed, ab, G = _problem(24)
    S = kref.sens_banded(ab, fixed, G)
    sigma = kref.random_psd(6)
    assert np.all(sigma[:6] == 0.0) and np.all(sigma[:, :6] == 0.0) and np.linalg.eigvalsh(sigma).min() >= -1e-20
    cov_x, cov_pos, std_pos = kref.calib_cov(S, sigma, x)
    assert np.abs(cov_x - cov_x.transpose(0, 2, 1)).max() <= 1e-14 * np.abs(cov_x).max()
    assert np.all(cov_x[fixed] == 0.0)
    assert np.allclose(std_pos ** 2, np.einsum("nlii->nl", cov_pos), rtol=1e-12, atol=0)
    a = np.array([0.3, -0.5, 0.2])
    gen = kref.translation_gen(seq["R"], a)
    _, _, std_t = kref.calib_cov(S, 1e-6 * np.outer(gen, gen), x)
    # (what the solve leaves of the identity: its relative error per column, bar(d0), times the identity's scale)
    tol = cref.bar(kref.col_err(kref.sens_dense(ab, fixed, G), S)) * _identity_scale(S, gen)
    assert np.abs(std_t - 1e-3 * np.linalg.norm(a)).max() <= 1e-3 * tol
