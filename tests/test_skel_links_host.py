"""Host side of the skeleton-FTE link sensitivity (no GPU): the cross term G of tests/skel_links_ref.py against central
differences of the oracle projections through the oracle FK at scaled offsets, the two CPU references against each other on
the inputs the GPU tests use, build.link_cov_matrix, the ABI entries and the argument checks that come before any device call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import skel_links_ref as lkref
import skel_sample_cases as scases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("acino_skel_fte_link_workspace_bytes", "acino_skel_fte_link_sensitivity")
P51_GROUPS = np.arange(20) % 16
# the GPU tests' inputs: name -> groups
CASES = {"pt16": "links", "pt32": "links", "slice12": "links", "slice40": "global", "p51": P51_GROUPS, "slice40pin": "links",
         "pt16pin": "links"}
_REF = {}


def ref(golden_dir, name):
    if name not in _REF:
        c = scases.case(golden_dir, name)
        _REF[name] = lkref.reference(c["prob"], c["x"][:, c["prob"].ACT], c["ab"], c["fixed"], CASES[name])
    return _REF[name]


@pytest.mark.parametrize("name", ["slice12", "pt16pin", "p51"])
def test_cross_term_against_central_differences(golden_dir, name):
    """G against sum J_x^T w^2 (uv(theta + h e_g) - uv(theta - h e_g)) / 2h, h = 1e-6, relative to max |G|.  The bar is the error
    model's (skel_links_ref.cross_term_fd: 8 eps max|uv| / h of rounding and h^2 max|J_theta| of truncation per pixel component,
    carried through the weighted sum).  Observed: slice12 3.3e-10, pt16pin 3.5e-10, p51 4.3e-10 against bars of 3.2e-8, 3.7e-8 and
    3.2e-8 (the rounding term of the model is the larger one and is a worst case)."""
    c = scases.case(golden_dir, name)
    prob = c["prob"]
    xa = c["x"][:, prob.ACT]
    grp, K = lkref.groups_of(prob.skel, CASES[name])
    G = lkref.cross_term(prob, xa, grp, K)
    G_fd, err = lkref.cross_term_fd(prob, xa, grp, K, h=1e-6)
    top = np.abs(G).max()
    e, bar = np.abs(G_fd - G).max() / top, err.max() / top
    print(f"{name}: K {K}, max|G| {top:.3e}: |G_fd - G| / max|G| = {e:.2e}, the error model's bar {bar:.2e}")
    assert top > 0 and e <= bar
    assert bar <= 1e-6                                          # (the model itself stays a tight statement)


@pytest.mark.parametrize("name", list(CASES))
def test_the_two_references_agree(golden_dir, name):
    c, r = scases.case(golden_dir, name), ref(golden_dir, name)
    print(f"{name}: N {c['fixed'].shape[0]}, P {c['fixed'].shape[1]}, K {r['K']}, d0 {r['d0']:.2e}")
    assert r["d0"] <= 1e-8
    assert np.all(r["S1"][c["fixed"]] == 0) and np.all(r["S2"][c["fixed"]] == 0)


@pytest.mark.parametrize("name", ["slice12", "p51"])
def test_group_nine_hangs_no_weighted_slot(golden_dir, name):
    """The skeleton defines hip1 twice: the first definition's link (group 9) is on no weighted slot's path, its column of G is
    exactly 0 and the direct term is all the group does."""
    r = ref(golden_dir, name)
    assert np.all(r["G"][:, :, 9] == 0) and np.all(r["S1"][:, :, 9] == 0)
    assert np.array_equal(r["T1"][..., 9], r["D"][..., 9])
    assert np.abs(r["G"]).max(axis=(0, 1))[np.arange(r["K"]) != 9].min() > 0


def test_link_cov_matrix():
    from acinoset_amd import build
    import torch
    rng = np.random.default_rng(0)
    A = rng.standard_normal((5, 5))
    good = A @ A.T
    sig, unk = build.link_cov_matrix(good, 5)
    assert np.array_equal(sig, good) and sig.dtype == np.float64 and unk.dtype == bool and not unk.any()
    sig_t, _ = build.link_cov_matrix(torch.as_tensor(good), 5)
    assert np.array_equal(sig_t, good)
    assert build.link_cov_matrix(None, 5) == (None, None)
    obs = np.array([True, True, False, True, False])
    fit = dict(cov_log_scales=good.copy(), observed=obs, scales=np.ones(5))
    fit["cov_log_scales"][2, 2] = np.inf                        # (whatever an unobserved group's entries hold)
    sig_d, unk_d = build.link_cov_matrix(fit, 5)
    assert np.array_equal(unk_d, ~obs) and np.all(sig_d[~obs] == 0) and np.all(sig_d[:, ~obs] == 0)
    assert np.array_equal(sig_d[np.ix_(obs, obs)], good[np.ix_(obs, obs)])
    bad_nan, bad_asym = good.copy(), good.copy()
    bad_nan[1, 1] = np.nan
    bad_asym[0, 3] += 1e-6
    for bad in (good[:4, :4], np.zeros((5, 6)), np.zeros(5), bad_nan, bad_asym, dict(scales=np.ones(5)),
                dict(cov_log_scales=good, observed=obs[:4])):
        with pytest.raises(ValueError, match="cov_links"):
            build.link_cov_matrix(bad, 5)


def test_header_library_and_binding_carry_the_two_entries():
    from acinoset_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "acinoset_hip.h")).read()
    handle = C.CDLL(_lib.SO_PATH)
    for name in SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert hasattr(handle, name) and name in _lib.SIGNATURES
    assert "skel_links.hip" in _lib.SOURCES and callable(build.model_link_sensitivity) and callable(build.link_cov_matrix)


def _params(n_active=36, n_cams=2, loss=0):
    from acinoset_amd import _lib
    p = _lib.SkelFteParams()
    p.n_frames, p.n_cams, p.n_pose, p.n_ops, p.n_angles, p.n_active = 100, n_cams, 7, 6, 15, n_active
    p.h, p.model_weight, p.l1_eps, p.lam0 = 1.0 / 120.0, 0.002, 1e-2, 1e-3
    p.loss = loss
    return p


def test_workspace_bytes():
    from acinoset_amd import _lib
    wsb, cov = _lib.lib().acino_skel_fte_link_workspace_bytes, _lib.lib().acino_skel_fte_covariance_pinned_workspace_bytes
    p = _params()
    col = (8 * 16 * 100 * 36 + 255) // 256 * 256                # one column buffer [1][16][N][n_active]
    assert wsb(C.byref(p), 1, 0) == cov(C.byref(p), 1, 0) + 2 * col and wsb(C.byref(p), 1, 1) == cov(C.byref(p), 1, 1) + 2 * col
    assert wsb(C.byref(p), 1, 2) == 0 and wsb(C.byref(p), 0, 0) == 0 and wsb(None, 1, 0) == 0
    assert wsb(C.byref(_params(65)), 1, 0) == 0


def test_invalid_arguments_are_refused_without_a_device():
    from acinoset_amd import _lib
    fn = _lib.lib().acino_skel_fte_link_sensitivity
    p = _params()
    ops, act = (_lib.SkelOp * 6)(), (C.c_int32 * 36)()
    status = (C.c_int32 * 2)()
    fake = C.c_void_p(1 << 20)
    I6 = C.c_int32 * 6

    def call(prm=p, group=I6(0, 1, 2, -1, 0, 1), K=3, sigma=fake, unknown=None, outs=(fake, fake, fake, fake, fake), pin=0, ws=fake,
             ws_bytes=0, n_clips=2):
        return fn(C.byref(prm), n_clips, 0, ops, act, fake, fake, fake, fake, fake, fake, group, K, sigma, unknown, *outs, status, ws,
                  ws_bytes, None, pin, None)

    err = _lib.lib().acino_last_error_string
    assert call() == -3 and b"too small" in err()               # (valid up to the workspace of 0 bytes: no device call)
    assert call(ws=C.c_void_p((1 << 20) + 8), ws_bytes=1 << 40) == -3 and b"aligned" in err()
    for kw, what in ((dict(outs=(None,) * 5), b"at least one"), (dict(sigma=None), b"d_cov_links"),
                     (dict(sigma=None, outs=(None, None, None, None, fake)), b"d_cov_links"),
                     (dict(K=0), b"n_groups"), (dict(K=17), b"n_groups"), (dict(group=I6(0, 1, 3, -1, 0, 1)), b"h_group"),
                     (dict(group=I6(0, 1, -2, -1, 0, 1)), b"h_group"), (dict(group=None), b"h_group"),
                     (dict(prm=_params(loss=1)), b"L1 loss only"), (dict(pin=2), b"pin_unobserved"), (dict(n_clips=0), b"n_clips"),
                     (dict(prm=_params(65)), b"n_active")):
        assert call(**kw) == -1, kw
        assert what in err(), (kw, err())
    assert call(sigma=None, outs=(fake, fake, None, None, None)) == -3    # S and T_l alone need no covariance


def test_python_argument_checks_come_before_the_gpu(golden_dir, monkeypatch):
    """Robust loss, bad groups and a bad cov_links are ValueErrors of the host layer: the device layer is never asked."""
    from acinoset_amd import _lib, build
    c = scases.case(golden_dir, "slice12")
    model, x = c["model"], c["x"]

    def no_device(*_a, **_k):
        raise AssertionError("a device call was made")

    monkeypatch.setattr(_lib, "require_gpu", no_device)
    monkeypatch.setattr(build, "_skel_inputs", no_device)
    grp, K = build.link_groups(model.prog, "links")
    good = lkref.random_psd(K)
    bad_nan, bad_asym = good.copy(), good.copy()
    bad_nan[3, 3] = np.nan
    bad_asym[2, 5] += 1e-6
    for bad in (good[:6, :6], np.zeros((K, K + 1)), bad_nan, bad_asym, dict(cov_points=None)):
        with pytest.raises(ValueError, match="cov_links"):
            build.model_link_sensitivity([model], [x], "links", bad)
        with pytest.raises(ValueError, match="cov_links"):
            build.solve_models([model], [x], cov_links=bad)
        with pytest.raises(ValueError, match="cov_links"):
            build.solve_model(model, x0=x, cov_links=bad)
    for groups in ("limbs", np.zeros(len(grp) + 1, dtype=int), np.full(len(grp), 16), np.full(len(grp), -2), np.zeros(len(grp))):
        with pytest.raises(ValueError, match="group"):
            build.model_link_sensitivity([model], [x], groups, None)
        with pytest.raises(ValueError, match="group"):
            build.solve_models([model], [x], link_groups=groups)
    robust = build._with_loss(model, "redescending")
    with pytest.raises(ValueError, match="l1 loss only"):
        build.model_link_sensitivity([robust], [x], "links", good)
    with pytest.raises(ValueError, match="l1 loss only"):
        build.solve_models([robust], [x], cov_links=good)
    with pytest.raises(ValueError, match="l1 loss only"):
        build.solve_video(c["sk"], scene=c["scene"], dlc_tables=[], loss="redescending", cov_links=good)
    with pytest.raises(ValueError, match="no models"):
        build.model_link_sensitivity([], [], "links", good)
