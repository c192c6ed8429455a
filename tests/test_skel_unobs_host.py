"""Host side of the observability rule of the skeleton-FTE posterior (no GPU): the ABI entries, the argument checks that come
before any device call, and the numpy reference of tests/skel_unobs_ref.py against itself and against the figures the feature
was specified with (inputs: tests/skel_unobs_cases.py)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import skel_cov_ref as cref
import skel_unobs_cases as ucases
import skel_unobs_ref as uref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("acino_skel_fte_observability", "acino_skel_fte_covariance_pinned", "acino_skel_fte_sample_pinned")
SYMBOLS = ENTRIES + tuple(e + "_workspace_bytes" for e in ENTRIES)


def _c_arity(header, name):
    """Number of parameters of ``name``'s declaration in the header (comments stripped)."""
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, name
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_header_library_and_binding_carry_the_new_entries():
    from acinoset_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "acinoset_hip.h")).read()
    handle = C.CDLL(_lib.SO_PATH)
    for name in SYMBOLS:
        assert hasattr(handle, name) and name in _lib.SIGNATURES, name
        assert _c_arity(header, name) == len(_lib.SIGNATURES[name][1]), name
    # the _pinned entries are the existing signatures plus (int pin_unobserved, uint8_t* d_unobserved)
    for base in ("acino_skel_fte_covariance", "acino_skel_fte_sample"):
        old, new = _lib.SIGNATURES[base][1], _lib.SIGNATURES[base + "_pinned"][1]
        assert new[:len(old)] == old and new[len(old):] == [C.c_int, C.c_void_p]
        old, new = _lib.SIGNATURES[base + "_workspace_bytes"][1], _lib.SIGNATURES[base + "_pinned_workspace_bytes"][1]
        assert new[:len(old)] == old and new[len(old):] == [C.c_int]
    # observability: the covariance's leading arguments p .. d_x, three outputs, then d_ws, ws_bytes, stream
    cov, obs = _lib.SIGNATURES["acino_skel_fte_covariance"][1], _lib.SIGNATURES["acino_skel_fte_observability"][1]
    assert obs[:11] == cov[:11] and obs[11:] == [C.c_void_p] * 3 + cov[-3:]
    assert re.search(r"#define ACINO_ABI_VERSION 3\b", header) and _lib.ABI_VERSION == 3 and _lib.lib().acino_abi_version() == 3
    assert re.search(r"#define ACINO_SKEL_UNOBS_REL 1e-24\b", header) and uref.SK_UNOBS_REL == 1e-24
    assert callable(build.model_observability)
    for fn in ("model_covariance", "model_samples", "model_reprojection", "solve_model", "solve_models", "solve_video"):
        par = inspect.signature(getattr(build, fn)).parameters
        assert "pin_unobserved" in par and par["pin_unobserved"].default is False, fn


def _params(n_active=36):
    from acinoset_amd import _lib
    p = _lib.SkelFteParams()
    p.n_frames, p.n_cams, p.n_pose, p.n_ops, p.n_angles, p.n_active = 100, 2, 15, 14, 15, n_active
    p.h, p.model_weight, p.l1_eps, p.lam0 = 1.0 / 120.0, 0.002, 1e-2, 1e-3
    return p


def test_workspace_queries():
    from acinoset_amd import _lib
    L = _lib.lib()
    p = _params()
    obs, cov, covp = (L.acino_skel_fte_observability_workspace_bytes, L.acino_skel_fte_covariance_workspace_bytes,
                      L.acino_skel_fte_covariance_pinned_workspace_bytes)
    smp, smpp = L.acino_skel_fte_sample_workspace_bytes, L.acino_skel_fte_sample_pinned_workspace_bytes
    for b in (1, 8):
        assert 0 < obs(C.byref(p), b) < cov(C.byref(p), b) <= covp(C.byref(p), b, 0) == covp(C.byref(p), b, 1)
        assert obs(C.byref(p), b) % 256 == 0 and covp(C.byref(p), b, 1) % 256 == 0
        assert covp(C.byref(p), b, 1) - cov(C.byref(p), b) < 1 << 16          # one problem description and the mask
        assert smpp(C.byref(p), b, 4, 1) == covp(C.byref(p), b, 1) and smp(C.byref(p), b, 4) == cov(C.byref(p), b)
    assert covp(C.byref(p), 1, 2) == 0 and covp(C.byref(p), 1, -1) == 0 and smpp(C.byref(p), 1, 4, 2) == 0
    assert smpp(C.byref(p), 1, 0, 1) == 0 and obs(C.byref(p), 0) == 0 and obs(None, 1) == 0 and covp(None, 1, 1) == 0
    for bad in (65, 2):
        assert obs(C.byref(_params(bad)), 1) == 0 and covp(C.byref(_params(bad)), 1, 1) == 0


def test_invalid_arguments_are_refused_without_a_device():
    from acinoset_amd import _lib
    L = _lib.lib()
    p = _params()
    ops, act = (_lib.SkelOp * 14)(), (C.c_int32 * 36)()
    status = (C.c_int32 * 2)()
    fake = C.c_void_p(1 << 20)
    err = lambda: L.acino_last_error_string()   # noqa: E731

    def obs(prm=p, n_clips=2, cam=0, outs=(fake, fake, fake), x=fake, ws=fake):
        return L.acino_skel_fte_observability(C.byref(prm), n_clips, cam, ops, act, fake, fake, fake, fake, fake, x, *outs, ws, 0, None)

    def cov(prm=p, n_clips=2, cam=0, pin=1, mask=fake, outs=(fake, fake, fake)):
        return L.acino_skel_fte_covariance_pinned(C.byref(prm), n_clips, cam, ops, act, fake, fake, fake, fake, fake, fake, *outs,
                                                  status, fake, 0, None, pin, mask)

    rows = 2 * 4 * 100
    z, xs, pos = 1 << 30, (1 << 30) + 8 * rows * 36, (1 << 30) + 16 * rows * 36

    def smp(prm=p, n_clips=2, pin=1, mask=fake, n_samples=4, d_z=z):
        return L.acino_skel_fte_sample_pinned(C.byref(prm), n_clips, 0, ops, act, fake, fake, fake, fake, fake, fake, n_samples,
                                              C.c_void_p(d_z), C.c_void_p(xs), C.c_void_p(pos), status, fake, 0, None, pin, mask)

    # valid up to the workspace of 0 bytes: ACINO_ERR_WORKSPACE, still no device call
    assert obs() == -3 and cov() == -3 and smp() == -3 and cov(pin=0, mask=None) == -3 and smp(pin=0, mask=None) == -3
    assert obs(outs=(None, None, fake)) == -3 and cov(mask=None) == -3
    for call, kw, what in ((obs, dict(outs=(None, None, None)), b"d_info"), (obs, dict(n_clips=0), b"n_clips"),
                           (obs, dict(cam=2), b"camera_model"), (obs, dict(prm=_params(65)), b"n_active"),
                           (obs, dict(x=None), b"null buffer"), (obs, dict(ws=None), b"null buffer"),
                           (cov, dict(pin=2), b"pin_unobserved"), (cov, dict(pin=-1), b"pin_unobserved"),
                           (cov, dict(outs=(None, None, None)), b"d_cov_x"), (cov, dict(n_clips=0), b"n_clips"),
                           (cov, dict(cam=3), b"camera_model"), (cov, dict(prm=_params(2)), b"n_active"),
                           (smp, dict(pin=2), b"pin_unobserved"), (smp, dict(pin=-7), b"pin_unobserved"),
                           (smp, dict(n_samples=0), b"n_samples"), (smp, dict(d_z=xs), b"overlaps d_x_samples"),
                           (smp, dict(n_clips=0), b"n_clips")):
        assert call(**kw) == -1, (call.__name__, kw)
        assert what in err(), (call.__name__, kw, err())
    # an unaligned workspace is refused as such by all three
    odd = C.c_void_p((1 << 20) + 8)
    assert obs(ws=odd) == -3 and b"aligned" in err()


def test_python_argument_checks_come_before_the_gpu(golden_dir):
    import torch
    from acinoset_amd import build
    c = ucases.case(golden_dir, "shipped12")
    model, x = c["model"], c["x"]
    with pytest.raises(ValueError, match="iterates"):
        build.model_observability([model], [x, x])
    with pytest.raises(ValueError, match="must be"):
        build.model_observability([model], [x[:, :-1]])
    with pytest.raises(ValueError, match="no models"):
        build.model_observability([], [])
    if not torch.cuda.is_available():
        for call in (lambda: build.model_observability([model], [x]),
                     lambda: build.model_covariance([model], [x], pin_unobserved=True),
                     lambda: build.model_samples([model], [x], n_samples=2, pin_unobserved=True)):
            with pytest.raises(RuntimeError, match="GPU"):
                call()


def test_the_reference_reproduces_the_specified_figures(golden_dir):
    """Shipped skeleton: active positions 25 and 33 (full-state 33 and 43), Fisher and G columns EXACTLY 0 in every frame, d0
    3.2e-10 / 6.5e-10 at 40 / 12 frames.  Lost limb: active positions 6, 9, 17, 20, 28, 31, d0 1.6e-9 / 8.2e-10 at 12 / 40
    frames, the dependent poses exactly elbow1 and wrist1 in every frame, weakest observed state 5e-5 of the strongest.  The limb
    seen in frames 0 and 1 only: nothing unobserved, the matrix singular all the same, n_seen says which states."""
    for name, d0_max in (("shipped40", 3.3e-10), ("shipped12", 6.6e-10)):
        c = ucases.solved(golden_dir, name)
        r = c["ref"]
        assert np.nonzero(r["unobserved"])[0].tolist() == [25, 33] and ucases.full_index(c, [25, 33]) == [33, 43]
        assert np.all(r["HF"][:, [25, 33], :] == 0) and np.all(r["G"][..., [25, 33]] == 0)
        assert not r["dependent"].any() and np.isfinite(r["std_pos"]).all()
        assert r["d0"] <= d0_max
        print(f"{name}: d0 {r['d0']:.2e}, condition {np.linalg.cond(cref.dense(r['ab'])):.1e}")
    six = [6, 9, 17, 20, 28, 31]
    for name, d0_max in (("lost12", 1.6e-9), ("lost40", 8.3e-10), ("lost12pin", 1e-8), ("lost12p51", 1e-8)):
        c = ucases.solved(golden_dir, name)
        r = c["ref"]
        names = list(c["model"].names)
        limb = sorted(names.index(k) for k in ucases.LIMB)
        assert int(r["unobserved"].sum()) == 6
        if r["info"].size == 36:
            assert np.nonzero(r["unobserved"])[0].tolist() == six
        assert all(np.nonzero(row)[0].tolist() == limb for row in r["dependent"])
        assert np.isinf(r["std_pos"][:, limb]).all() and np.isnan(r["cov_pos"][:, limb]).all()
        assert np.isfinite(np.delete(r["std_pos"], limb, axis=1)).all()
        seen = r["info"][~r["unobserved"]]
        assert 3e-5 < seen.min() / seen.max() < 6e-5
        assert r["d0"] <= d0_max
        print(f"{name}: d0 {r['d0']:.2e}, weakest observed state {seen.min() / seen.max():.1e} of the strongest")
    r = ucases.case(golden_dir, "two12")["ref"]
    assert not r["unobserved"].any()
    assert np.nonzero(r["n_seen"] < 3)[0].tolist() == six and (r["n_seen"][six] == 2).all()
    assert (np.delete(r["n_seen"], six) == 12).all()
    ev = np.linalg.eigvalsh(cref.dense(r["ab"]))
    print(f"two12: eigenvalues {ev[0]:.1e} .. {ev[-1]:.1e}")
    assert ev[0] < 1e-12 * ev[-1]                              # singular: the factorisation must say 5
    r = ucases.case(golden_dir, "slice40")["ref"]
    assert not r["unobserved"].any() and (r["n_seen"] == 40).all()


def test_a_clip_without_detections_has_every_state_unobserved():
    info, n_seen, un = uref.observability(np.zeros((5, 7, 7)))
    assert un.all() and (n_seen == 0).all() and (info == 0).all()


def test_pinning_equals_deleting_the_rows_and_columns(golden_dir):
    """The reference against itself on the lost-limb 12-frame input: the per-frame blocks with the six states pinned equal the
    blocks of the inverse of the matrix with those six rows and columns deleted in every frame, within bar(d0)."""
    c = ucases.solved(golden_dir, "lost12")
    r = c["ref"]
    xa = c["x"][:, c["prob"].ACT]
    want = uref.deleted_inverse_blocks(c["prob"], r["HF"], cref.pin_set(c["prob"], xa), r["unobserved"])
    e_a, e_b = cref.rel_err(r["Sa"], want), cref.rel_err(r["Sb"], want[r["frames"]])
    print(f"lost12: d0 {r['d0']:.2e}, bar {uref.bar(r['d0']):.2e}; pinned dense inverse vs deleted {e_a:.2e}, probes vs deleted {e_b:.2e}")
    assert e_a <= uref.bar(r["d0"]) and e_b <= uref.bar(r["d0"])
    un = r["unobserved"]
    assert np.all(r["Sa"][:, un, :] == 0) and np.all(r["Sa"][:, :, un] == 0)
