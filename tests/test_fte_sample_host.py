"""Posterior samples of the FTE trajectory, the part that needs no GPU: the C ABI (header, exports, signatures, argument
validation before any device call), the Python interface, and the CPU reference of tests/fte_sample_ref.py checked against
itself and against the dense inverse of tests/fte_cov_ref.py."""
import ctypes as C
import inspect
import os
import re
import types

import numpy as np
import pytest

import fte_cov_ref as ref
import fte_sample_ref as sref
from oracle import fk as ofk
from oracle import fte as ofte
from oracle import synth as osynth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("acino_fte_sample_workspace_bytes", "acino_fte_sample")
P = 25


def test_header_exports_signatures_and_argument_checks():
    """Fails without the feature: both functions are declared, exported and bound; the ABI version stays 3; the workspace
    is the covariance's; a null context, n_samples < 1 and null buffers are refused with ACINO_ERR_INVALID_ARG (-1) before
    anything touches a device."""
    from acinoset_amd import _lib, fte
    with open(os.path.join(ROOT, "include", "acinoset_hip.h")) as f:
        header = f.read()
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name} not declared in acinoset_hip.h"
        assert name in _lib.SIGNATURES
    import __graft_entry__ as entry
    entry.build()
    h = _lib.lib()
    for name in NAMES:
        assert hasattr(h, name)
    assert h.acino_abi_version() == 3
    for n, clip in ((7, 0), (121, 0), (8000, 1000)):
        p = fte.make_params(n, 6, 1.0 / 120, clip_len=clip)
        assert h.acino_fte_sample_workspace_bytes(C.byref(p)) == h.acino_fte_covariance_workspace_bytes(C.byref(p)) > 0
    assert h.acino_fte_sample_workspace_bytes(None) == 0
    assert h.acino_fte_sample(None, 4, None, None, 0, None, None, None) == -1
    assert "invalid argument" in h.acino_last_error_string().decode()
    fake = C.c_void_p(256)                                   # never dereferenced: the argument checks come first
    assert h.acino_fte_sample(fake, 0, fake, fake, 1 << 20, fake, None, None) == -1
    assert "n_samples" in h.acino_last_error_string().decode()
    assert h.acino_fte_sample(fake, -3, fake, fake, 1 << 20, fake, None, None) == -1
    assert h.acino_fte_sample(fake, 4, None, fake, 1 << 20, fake, None, None) == -1
    assert h.acino_fte_sample(fake, 4, fake, fake, 1 << 20, None, None, None) == -1
    assert h.acino_fte_sample(fake, 4, fake, None, 1 << 20, fake, None, None) == -1


def test_python_interface_defaults_off():
    from acinoset_amd import fte
    sig = inspect.signature(fte.FTEContext.sample).parameters
    assert [k for k in sig][:2] == ["self", "n_samples"]
    assert sig["seed"].default == 0 and sig["z"].default is None and sig["positions"].default is True
    assert sig["rates"].default is False and sig["clip"].default is False
    for fn in (fte.fte_solve, fte.fte_solve_clips, fte.fte_solve_batch):
        assert inspect.signature(fn).parameters["n_samples"].default == 0
        assert inspect.signature(fn).parameters["sample_seed"].default == 0
    res = {}
    fte._attach_posterior(res, None, lambda a: a)
    assert res == {}
    xs, ps = np.zeros((3, 10, 25)), np.zeros((3, 10, 20, 3))
    asked = []
    ctx = types.SimpleNamespace(sample=lambda n, seed=0: asked.append((n, seed)) or dict(x=xs, positions=ps))
    assert fte.FTEContext._posterior(ctx, n_samples=0, sample_seed=7) == {} and asked == []
    post = fte.FTEContext._posterior(ctx, n_samples=3, sample_seed=7)
    assert asked == [(3, 7)]
    fte._attach_posterior(res, post, lambda a: a, slice(5, 10))
    assert set(res) == {"x_samples", "positions_samples"}
    assert res["x_samples"].shape == (3, 5, 25) and res["positions_samples"].shape == (3, 5, 20, 3)


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
    return prob, Hd, fixed, band


@pytest.mark.parametrize("n,pin", [(7, False), (31, False), (32, True)])
def test_sample_map_squares_to_the_inverse(n, pin):
    """M = L^-T (z = the unit vectors): M M^T equals inv(A) - every block, between frames as well - with rows and columns
    of pinned variables exactly 0, and the three ways of the reference agree on M itself.  Bars: the covariance rule on the
    references' own spread."""
    prob, Hd, fixed, band = _problem(n, pin_knee=pin)
    assert fixed.any() == pin
    ab = ref.banded(Hd, fixed, prob.q_w, band)
    m1 = sref.sample_matrix(ab, fixed, "banded")
    m2 = sref.sample_matrix(ab, fixed, "dense")
    m3 = sref.sample_matrix(ab, fixed, "block")
    d0 = sref.map_err(m1, m2)
    e3 = sref.map_err(m3, m2)
    print(f"\n[{n} pin={pin}] map: d0 (banded vs dense) = {d0:.2e}   block recursion = {e3:.2e}")
    assert e3 <= ref.bar(d0)
    Ai = np.linalg.inv(ref.dense(ab))
    d0c = ref.rel_err(ref.probe_blocks(ab, fixed, np.arange(n)), ref.dense_blocks(ab, fixed))
    for lag in (0, 1, 3, n - 1):
        want = sref.inverse_blocks(Ai, fixed, lag)
        for m in (m1, m3):
            e = ref.rel_err(sref.cross_blocks(m, lag), want)
            print(f"   lag {lag}: e = {e:.2e} (bar {ref.bar(d0c):.2e})")
            assert e <= ref.bar(d0c)
    flat = m1.reshape(n * P, n * P)                                   # [sample = column of M, variable = row of M]
    pinned = fixed.reshape(-1)
    assert np.all(flat[:, pinned] == 0.0) and np.all(flat[pinned, :] == 0.0)
    if pin:
        assert pinned.sum() >= n // 2


def test_block_recursion_equals_banded_on_a_long_input_with_clips():
    """Two clips of 50 frames (17 nodes each, the last of 2 frames) laid end to end, random z: the node recursion equals the
    banded factorisation, and each clip equals the clip alone."""
    n = 50
    pa, pb = _problem(n, seed=1), _problem(n, seed=2)
    prob = pa[0]
    Hd, fixed = np.concatenate([pa[1], pb[1]]), np.concatenate([pa[2], pb[2]])
    ab = ref.banded(Hd, fixed, prob.q_w, ref.clip_band(2 * n, n))
    z = np.random.default_rng(5).normal(size=(6, 2 * n, P))
    a = sref.banded_map(ab, fixed, z)
    b = sref.block_map(ab, fixed, z, clip_len=n)
    d0 = sref.map_err(a, sref.dense_map(ab, fixed, z))
    e = sref.map_err(b, a)
    print(f"\n[2 x {n}] d0 = {d0:.2e}   block vs banded = {e:.2e}")
    assert e <= ref.bar(d0)
    for i, p in enumerate((pa, pb)):
        alone = sref.banded_map(ref.banded(p[1], p[2], prob.q_w, prob.s_band()), p[2], z[:, i * n:(i + 1) * n])
        assert sref.map_err(a[:, i * n:(i + 1) * n], alone) <= ref.bar(d0)
