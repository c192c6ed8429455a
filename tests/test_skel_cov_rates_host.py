"""Host side of the skeleton-FTE rate covariances (no GPU): the coefficient rows against build._finite_diff_states, the CPU
references of tests/skel_cov_rates_ref.py against each other on the inputs of tests/skel_cov_rates_cases.py - (c), the
cancellation-free form the GPU is held to, against (c') from the reversed factorisation, (a) the dense inverse, (b) banded probes
and (s) the streaming form the kernel uses - and the argument checks of the ABI entry."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import skel_cov_rates_cases as rcases
import skel_cov_rates_ref as rref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("acino_skel_fte_covariance_rates_workspace_bytes", "acino_skel_fte_covariance_rates")


@pytest.mark.parametrize("N", [1, 2, 3, 4, 5, 6])
def test_coefficient_rows_reproduce_the_finite_differences_of_the_solve(N):
    from acinoset_amd import build
    rng = np.random.default_rng(N)
    x, h = rng.standard_normal((N, 7)), 1.0 / 120.0
    dx, ddx = build._finite_diff_states(x, h)
    rdx, rddx = rref.finite_diff(x, h)
    scale = max(np.abs(dx).max(), np.abs(ddx).max(), 1.0)
    assert np.abs(rdx - dx).max() <= 1e-12 * scale and np.abs(rddx - ddx).max() <= 1e-12 * scale
    if N == 2:
        assert np.all(dx[0] == 0) and np.all(ddx == 0) and np.all(rdx[0] == 0) and np.all(rddx == 0)
    for n in range(N):
        frames = rref.coef_rows(N, n, h)[0]
        assert len(frames) == min(N, 3) and frames == tuple(range(frames[0], frames[0] + len(frames))) and frames[-1] < N


@pytest.mark.parametrize("name", rcases.PARITY)
def test_the_references_agree_and_the_streaming_form_is_within_the_bar(golden_dir, name):
    """d0 <= 1e-8 on every parity input (``bar`` asserts it); (a), (b) and the streaming form (s) within bar(d0) of (c).  The
    printed distances of (s) are the route decision: it differences nearly equal blocks, and stays orders below d0."""
    c = rcases.case(golden_dir, name)
    r = c["ref"]
    args = (r["ab"], r["fixed"], r["G"], r["h"])
    tol = rref.bar(r["d0"])
    print(f"{name}: N {c['model'].N}, P {r['fixed'].shape[1]}, d0 {r['d0']:.2e} "
          f"({', '.join(f'{k} {v:.1e}' for k, v in r['d0_by_key'].items())}), bar {tol:.2e}")
    for tag, fn in (("a", rref.by_dense_inverse), ("b", rref.by_banded_probes), ("s", rref.by_recursion)):
        e = rref.out_err(fn(*args), r["c"])
        print(f"   ({tag}) vs (c): " + ", ".join(f"{k} {v:.2e}" for k, v in e.items()))
        assert max(e.values()) <= tol, (tag, e)
    cv = r["c"]
    assert np.all(cv["std_vel"] > 0) and np.array_equal(cv["std_vel"][0], cv["std_vel"][1])
    assert np.array_equal(cv["cov_ddx"][0], cv["cov_ddx"][2]) and np.array_equal(cv["cov_ddx"][1], cv["cov_ddx"][2])


@pytest.mark.parametrize("N", rcases.SHORT)
def test_the_reference_accepts_every_short_clip(golden_dir, N):
    """N = 1 .. 5 on the PT 16 sub-tree with synthetic detections and the free twists switched off: both factorisations exist
    and agree to 1e-8 (``bar`` asserts it); (a), (b) and the streaming form within bar(d0) of (c); the rules of the short clips
    hold in (c) itself."""
    c = rcases.case(golden_dir, f"short{N}")
    r = c["ref"]
    assert c["model"].N == N and r["fixed"].shape == (N, 12) and not r["fixed"].any()
    args = (r["ab"], r["fixed"], r["G"], r["h"])
    tol = rref.bar(r["d0"])
    print(f"short{N}: d0 {r['d0']:.2e}, bar {tol:.2e}")
    for tag, fn in (("a", rref.by_dense_inverse), ("b", rref.by_banded_probes), ("s", rref.by_recursion)):
        e = rref.out_err(fn(*args), r["c"])
        print(f"   ({tag}) vs (c): " + ", ".join(f"{k} {v:.2e}" for k, v in e.items()))
        assert max(e.values()) <= tol, (tag, e)
    cv = r["c"]
    if N == 1:
        assert all(np.all(cv[k] == 0) for k in rref.KEYS)
    else:
        assert np.all(cv["std_vel"] > 0) and np.array_equal(cv["cov_vel"][0], cv["cov_vel"][1])
        assert np.all(cv["cov_dx"][0] == 0) == (N == 2) and np.all(np.diagonal(cv["cov_dx"][1]) > 0)
        assert np.all(cv["cov_ddx"] == 0) == (N == 2)


def test_short_clip_fisher_blocks_leave_the_twist_of_one_child_joints_free(golden_dir):
    """Why the short clips switch three angles off: on the whole PT 16 sub-tree a frame's Fisher block has three zero
    eigenvalues, with every slot seen by every camera; without the angles of ``SHORT_OFF`` it has none."""
    import skel_cov_cases as cases
    import skel_cov_ref as cref
    import skel_sample_cases as scases
    g, sk0, _det = scases.fixture(golden_dir)
    for regular, n_zero in ((False, 3), (True, 0)):
        sk = rcases.short_skeleton(sk0, regular=regular)
        model, x = rcases.synthetic(g, sk, 3)
        prob = cases.problem(sk, model, scases.scene(g), "fisheye")
        assert list(prob.ACT) == list(model.active) and len(model.active) == 15 - 3 * regular
        ev = np.linalg.eigvalsh(cref.fisher_blocks(prob, x[:, prob.ACT]))
        assert np.all(np.abs(ev[:, :n_zero]) <= 1e-12 * ev[:, -1:]) and np.all(ev[:, n_zero] > 1e-6 * ev[:, -1])


def test_pinned_variables_contribute_nothing(golden_dir):
    """A state pinned in every frame has rows and columns exactly 0; a variable pinned in frame 5 only still carries frame 4's
    share in dx_5; (c) agrees with the dense inverse with the rows and columns of S_ab dropped."""
    c = rcases.case(golden_dir, "pt16n8")
    r = c["ref"]
    fixed = r["fixed"].copy()
    fixed[:, 4] = True                                         # a state pinned in every frame: exactly 0 everywhere
    fixed[5, 7] = True                                         # pinned in frame 5 only
    import skel_cov_ref as cref
    ab = cref.banded(c["prob"], cref.fisher_blocks(c["prob"], c["x"][:, c["prob"].ACT]), fixed)
    got = rref.by_factor(ab, fixed, r["G"], r["h"])
    for k in ("cov_dx", "cov_ddx"):
        assert np.all(got[k][:, 4, :] == 0) and np.all(got[k][:, :, 4] == 0)
    assert np.all(np.delete(got["cov_dx"][5, 7, :], 4) != 0)   # dx_5 still holds x_4's share of the variable
    want = rref.by_dense_inverse(ab, fixed, r["G"], r["h"])
    assert max(rref.out_err(want, got).values()) <= rref.bar(r["d0"])


def test_header_library_and_binding_carry_the_two_entries():
    from acinoset_amd import _lib
    header = open(os.path.join(ROOT, "include", "acinoset_hip.h")).read()
    handle = C.CDLL(_lib.SO_PATH)
    for name in SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert hasattr(handle, name) and name in _lib.SIGNATURES
    assert _lib.ABI_VERSION == 3 and _lib.lib().acino_abi_version() == 3
    p = _lib.SkelFteParams()
    p.n_frames, p.n_cams, p.n_pose, p.n_ops, p.n_angles, p.n_active = 100, 2, 15, 14, 15, 36
    lib = _lib.lib()
    for pin in (0, 1):
        got = lib.acino_skel_fte_covariance_rates_workspace_bytes(C.byref(p), 3, pin)
        assert got > 0 and got % 256 == 0 and got == lib.acino_skel_fte_covariance_pinned_workspace_bytes(C.byref(p), 3, pin)
    assert lib.acino_skel_fte_covariance_rates_workspace_bytes(C.byref(p), 3, 2) == 0
    assert lib.acino_skel_fte_covariance_rates_workspace_bytes(C.byref(p), 0, 0) == 0
    p.n_active = 65
    assert lib.acino_skel_fte_covariance_rates_workspace_bytes(C.byref(p), 1, 0) == 0


def test_the_entry_rejects_bad_arguments_before_any_device_call():
    """No GPU here: every call below must return from the argument checks (a device call would fail with another code)."""
    from acinoset_amd import _lib
    lib = _lib.lib()
    p = _lib.SkelFteParams()
    p.n_frames, p.n_cams, p.n_pose, p.n_ops, p.n_angles, p.n_active = 8, 2, 2, 1, 1, 6
    p.h, p.model_weight, p.l1_eps, p.lam0, p.lam_max = 1.0 / 120.0, 2e-3, 1e-2, 1e-3, 1e16
    ops = (_lib.SkelOp * 1)()
    ops[0].child, ops[0].parent, ops[0].angle, ops[0].flags = 1, 0, 0, 7
    act = (C.c_int32 * 6)(0, 1, 2, 3, 4, 5)
    status = (C.c_int32 * 1)()
    buf, null = C.c_void_p(4096), C.c_void_p(0)
    nbytes = lib.acino_skel_fte_covariance_rates_workspace_bytes(C.byref(p), 1, 1)
    assert nbytes > 0

    def call(n_clips=1, cam=0, x=buf, outs=(buf,) * 7, ws=buf, ws_bytes=nbytes, pin=0, params=p):
        return lib.acino_skel_fte_covariance_rates(C.byref(params), n_clips, cam, ops, act, buf, buf, buf, buf, buf, x, *outs, status,
                                                   ws, ws_bytes, null, pin, null)

    err = lambda: lib.acino_last_error_string().decode()      # noqa: E731
    assert call(outs=(null,) * 7) == -1 and "d_std_vel" in err()
    assert call(pin=2) == -1 and "pin_unobserved" in err()
    assert call(cam=2) == -1 and "camera_model" in err()
    assert call(n_clips=0) == -1
    assert call(x=null) == -1 and "null buffer" in err()
    assert call(ws=C.c_void_p(4096 + 8)) == -3 and "aligned" in err()
    assert call(ws_bytes=256) == -3 and "acino_skel_fte_covariance_rates_workspace_bytes" in err()
    bad = _lib.SkelFteParams.from_buffer_copy(p)
    bad.n_active = 65
    assert call(params=bad) == -1


def test_python_keyword_checks_come_before_the_gpu(golden_dir):
    import torch
    from acinoset_amd import build
    c = rcases.case(golden_dir, "pt16n8")
    with pytest.raises(ValueError, match="iterates"):
        build.model_covariance([c["model"]], [c["x"], c["x"]], rates=True)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="GPU"):
            build.model_covariance([c["model"]], [c["x"]], rates=True)
