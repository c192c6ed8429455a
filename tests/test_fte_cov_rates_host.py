"""Covariance of dx, ddx and of the marker velocities, the part that needs no GPU: the C ABI (header, exports,
signatures), the Python interface, and the CPU reference of tests/fte_cov_rates_ref.py checked against itself - dense
inverse, banded probes and the numpy restatement of the factor form the kernel uses."""
import inspect
import os
import re

import numpy as np
import pytest

import fte_cov_ref as ref
import fte_cov_rates_ref as rref
from oracle import fk as ofk
from oracle import fte as ofte
from oracle import synth as osynth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("acino_fte_covariance_rates_workspace_bytes", "acino_fte_covariance_rates")


def test_header_exports_signatures_and_python_defaults():
    """Fails without the feature: the two functions are declared, exported and bound; the ABI version stays 3 (functions
    were only added); the new Python arguments exist and default off."""
    import ctypes as C
    from acinoset_amd import _lib, fte
    with open(os.path.join(ROOT, "include", "acinoset_hip.h")) as f:
        header = f.read()
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name} not declared in acinoset_hip.h"
        assert name in _lib.SIGNATURES
    import __graft_entry__ as entry
    entry.build()
    h = _lib.lib()
    for name in NAMES + ("acino_fte_covariance", "acino_fte_covariance_workspace_bytes"):
        assert hasattr(h, name)
    assert h.acino_abi_version() == 3
    for n, clip in ((7, 0), (121, 0), (8000, 1000)):
        p = fte.make_params(n, 6, 1.0 / 120, clip_len=clip)
        assert (h.acino_fte_covariance_rates_workspace_bytes(C.byref(p))
                == h.acino_fte_covariance_workspace_bytes(C.byref(p)) > 0)
    assert inspect.signature(fte.FTEContext.covariance_rates).parameters["std_only"].default is False
    for fn in (fte.fte_solve, fte.fte_solve_clips, fte.fte_solve_batch):
        assert inspect.signature(fn).parameters["return_rate_cov"].default is False
        assert inspect.signature(fn).parameters["return_cov"].default is False


@pytest.mark.parametrize("L", [1, 2, 3, 4, 9])
def test_coefficient_rows_reproduce_k_derivatives(L):
    """The rows the covariances are taken with give the dx / ddx of k_derivatives (restated in numpy) on a random
    trajectory, start-up frames and short clips included: products of the same numbers in another order, 1e-12 relative."""
    rng = np.random.default_rng(L)
    x = rng.normal(size=(L, 25))
    Ts = 1.0 / 120
    dx, ddx = rref.derivatives(x, Ts)
    dx2, ddx2 = rref.derivatives_from_rows(x, Ts)
    assert np.abs(dx - dx2).max() <= 1e-12 * max(np.abs(dx).max(), 1.0)
    assert np.abs(ddx - ddx2).max() <= 1e-12 * max(np.abs(ddx).max(), 1.0)
    if L >= 3:
        assert np.array_equal(ddx[0], ddx[2]) and np.array_equal(ddx[1], ddx[2])
        assert np.allclose(dx[0], dx[1] - Ts * ddx[2], rtol=0, atol=1e-9)


def _problem(n, seed=20210313, pin_knee=False):
    if pin_knee:
        q = osynth.trajectory(n, "sprint")
        q[:, ofk.ACTIVE[12]] = np.pi / 2 + 0.3               # a front knee held beyond its box: the estimate sits on the bound
        pos = ofk.cheetah_fk(q)
        K, D, R, t = osynth.make_rig()
        det = osynth.detections_from_positions(pos, K, D, R, t, seed=seed)
        seq = dict(K=K, D=D, R=R, t=t, q_true=q, det=det, Ts=1.0 / osynth.FPS)
    else:
        seq = osynth.make_sequence(n, "sprint", seed=seed)
    det = seq["det"]
    prob = ofte.FTEProblem(det[..., :2], det[..., 2], seq["K"], seq["D"], seq["R"], seq["t"], seq["Ts"])
    x = np.clip(seq["q_true"][:, ofk.ACTIVE], prob.lo, prob.hi)
    _, g, H, _ = prob.evaluate(x)
    band = prob.s_band()
    Hd = ref.with_smooth_diag(H, prob.q_w, band)
    fixed = ref.active_set(x, g, Hd, prob.lo, prob.hi)
    return prob, x, g, H, Hd, fixed, band, seq["Ts"]


def _symmetric_psd(blocks):
    blocks = blocks.reshape(-1, blocks.shape[-2], blocks.shape[-1])
    assert np.abs(blocks - blocks.transpose(0, 2, 1)).max() <= 1e-9 * np.abs(blocks).max()
    w = np.linalg.eigvalsh(0.5 * (blocks + blocks.transpose(0, 2, 1)))
    assert np.all(w[:, 0] >= -1e-9 * np.maximum(w[:, -1], 1e-300))


@pytest.mark.parametrize("n,pin", [(7, False), (121, False), (122, False), (122, True)])
def test_reference_ways_agree_and_the_factor_form_reproduces_them(n, pin):
    """(a) dense inverse, (b) banded Cholesky probes, (b') banded LU probes and the factor form of the kernel give the same
    cov_dx / cov_ddx / cov_vel / std_vel, every output on its own d0 (fte_cov_ref.bar)."""
    prob, x, g, H, Hd, fixed, band, Ts = _problem(n, pin_knee=pin)
    assert fixed.any() == pin
    ab = ref.banded(Hd, fixed, prob.q_w, band)
    a = rref.reference(ab, fixed, x, Ts, how="dense")
    b = rref.reference(ab, fixed, x, Ts, how="chol")
    lu = rref.reference(ab, fixed, x, Ts, how="lu")
    ff = rref.factor_form(ab, fixed, x, Ts)
    d0 = rref.errs(b, a)
    e_lu, e_ff = rref.errs(lu, a), rref.errs(ff, a)
    print(f"\n[{n} pin={pin}] d0 = {d0}\n   lu = {e_lu}\n   factor form = {e_ff}")
    for d, e1, e2 in zip(d0, e_lu, e_ff):
        assert e1 <= ref.bar(d) and e2 <= ref.bar(d), (d, e1, e2)
    for blocks in a[:3]:
        _symmetric_psd(blocks)
    if pin:
        full = fixed[2:] & fixed[1:-1] & fixed[:-2]                    # pinned in every frame of the window of frame n >= 2
        assert full.any()
        for blocks in (a[0][2:], a[1][2:], ff[0][2:], ff[1][2:]):
            assert np.all(blocks[full] == 0.0) and np.all(blocks.transpose(0, 2, 1)[full] == 0.0)
    # neighbouring frames are correlated: independent frames would give sqrt(2 diag cov_x) / Ts
    cov_x = ref.dense_blocks(ab, fixed)
    sd = np.sqrt(np.einsum("npp->np", a[0]))[2:]
    ind = np.sqrt(2 * np.einsum("npp->np", cov_x))[2:] / Ts
    free = ~(fixed[2:] | fixed[1:-1])
    assert np.all(sd[free] < ind[free])


def test_two_clips_equal_each_clip_alone():
    """Two clips laid end to end: the windows stop at the seam - start-up frames of the second clip included - and every
    output equals the clip alone."""
    n = 16
    pa = _problem(n, seed=1)
    pb = _problem(n, seed=2)
    prob, Ts = pa[0], pa[7]
    x = np.concatenate([pa[1], pb[1]])
    Hd = np.concatenate([pa[4], pb[4]])
    fixed = np.concatenate([pa[5], pb[5]])
    ab = ref.banded(Hd, fixed, prob.q_w, ref.clip_band(2 * n, n))
    a = rref.reference(ab, fixed, x, Ts, clip_len=n, how="dense")
    b = rref.reference(ab, fixed, x, Ts, clip_len=n, how="chol")
    ff = rref.factor_form(ab, fixed, x, Ts, clip_len=n)
    tol = [ref.bar(d) for d in rref.errs(b, a)]
    assert all(e <= t for e, t in zip(rref.errs(ff, a), tol))
    for i, p in enumerate((pa, pb)):
        ab1 = ref.banded(p[4], p[5], prob.q_w, prob.s_band())
        alone = rref.reference(ab1, p[5], p[1], Ts, how="dense")
        part = tuple(o[i * n:(i + 1) * n] for o in a)
        assert all(e <= t for e, t in zip(rref.errs(part, alone), tol))
        assert np.array_equal(part[2][0], part[2][1]) and np.array_equal(part[3][0], part[3][1])   # frame 0 repeats frame 1
