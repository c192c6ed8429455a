"""Host side of the skeleton-FTE calibration sensitivity (no GPU): J_c of tests/skel_calib_ref.py against a central difference of
the oracle projection, the two CPU references against each other on the inputs the GPU tests use, the translation identity on
reference 1, the ABI entries and the argument checks that come before any device call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fte_calib_ref as fref
import skel_calib_ref as kref
import skel_sample_cases as scases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("acino_skel_fte_calibration_workspace_bytes", "acino_skel_fte_calibration_sensitivity")
CASES = ("pt16", "pt32", "slice12", "slice40", "p51", "slice40pin", "pt16pin")      # the GPU tests' inputs, by name
_REF = {}


def ref(golden_dir, name):
    if name not in _REF:
        c = scases.case(golden_dir, name)
        _REF[name] = kref.reference(c["prob"], c["x"][:, c["prob"].ACT], c["ab"], c["fixed"])
    return _REF[name]


@pytest.mark.parametrize("name", ["slice12", "pt16pin"])
def test_camera_jacobian_against_a_central_difference(golden_dir, name):
    """J_c against (uv(c + h e_k) - uv(c - h e_k)) / 2h of the oracle projection under R <- exp([dw]x) R, t <- t + dt."""
    c = scases.case(golden_dir, name)
    prob = c["prob"]
    pos = kref.osf.skeleton_fk_jac(prob.skel, prob.full_state(c["x"][:, prob.ACT]))[0]
    h = 1e-6
    R0, t0 = [np.array(r, dtype=np.float64) for r in prob.R], [np.array(t, dtype=np.float64) for t in prob.t]
    try:
        for ci in range(prob.C):
            uv, _Jpi, Jc, zc = kref.camera_jacobian(prob, pos, ci)
            assert np.all(np.abs(zc) > 1e-3)
            for k in range(6):
                side = []
                for sgn in (1.0, -1.0):
                    step = np.zeros(6)
                    step[k] = sgn * h
                    prob.R[ci] = fref.rot_exp(step[:3]) @ R0[ci]
                    prob.t[ci] = t0[ci] + step[3:].reshape(t0[ci].shape)
                    side.append(kref.project(prob, pos, ci)[0])
                    prob.R[ci], prob.t[ci] = R0[ci], t0[ci]
                fd = (side[0] - side[1]) / (2 * h)
                e = np.abs(fd - Jc[..., k]).max() / max(np.abs(Jc[..., k]).max(), 1.0)
                print(f"{name}: camera {ci}, parameter {k}: |fd - J_c| / max|J_c| = {e:.2e}")
                assert e <= 1e-6                               # (h^2 truncation and 1e-16 / h rounding, both ~1e-10 relative)
    finally:
        for ci in range(prob.C):
            prob.R[ci], prob.t[ci] = R0[ci], t0[ci]


@pytest.mark.parametrize("name", CASES)
def test_the_two_references_agree(golden_dir, name):
    c, r = scases.case(golden_dir, name), ref(golden_dir, name)
    print(f"{name}: N {c['fixed'].shape[0]}, P {c['fixed'].shape[1]}, d0 {r['d0']:.2e}")
    assert r["d0"] <= 1e-8
    assert np.all(r["S1"][c["fixed"]] == 0) and np.all(r["S2"][c["fixed"]] == 0)


@pytest.mark.parametrize("name", ["slice40", "pt16pin"])
def test_translating_the_rig_moves_the_trajectory(golden_dir, name):
    """gen = [0, -R_c a]: every pixel stays where it is when the trajectory moves by a, so S gen = (a, 0, ..., 0) in every frame
    (the prior does not see a constant shift)."""
    c, r = scases.case(golden_dir, name), ref(golden_dir, name)
    assert not c["fixed"][:, :3].any()
    for a in np.eye(3):
        e = kref.identity_error(r["S1"], c["prob"].R, 0.01 * a)
        print(f"{name}: a = {a}: |S gen - (a, 0)| = {e:.2e} of 0.01")
        assert e <= 1e-8 * 0.01


def test_header_library_and_binding_carry_the_two_entries():
    from acinoset_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "acinoset_hip.h")).read()
    handle = C.CDLL(_lib.SO_PATH)
    for name in SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert hasattr(handle, name) and name in _lib.SIGNATURES
    assert re.search(r"#define ACINO_ABI_VERSION 3\b", header) and _lib.ABI_VERSION == 3 and _lib.lib().acino_abi_version() == 3
    assert "skel_calib.hip" in _lib.SOURCES and callable(build.model_calibration_sensitivity)


def _params(n_active=36, n_cams=2):
    from acinoset_amd import _lib
    p = _lib.SkelFteParams()
    p.n_frames, p.n_cams, p.n_pose, p.n_ops, p.n_angles, p.n_active = 100, n_cams, 7, 6, 15, n_active
    p.h, p.model_weight, p.l1_eps, p.lam0 = 1.0 / 120.0, 0.002, 1e-2, 1e-3
    return p


def test_workspace_bytes():
    from acinoset_amd import _lib
    wsb, cov = _lib.lib().acino_skel_fte_calibration_workspace_bytes, _lib.lib().acino_skel_fte_covariance_pinned_workspace_bytes
    p = _params()
    col = (8 * 12 * 100 * 36 + 255) // 256 * 256                # one column buffer [1][6C][N][n_active]
    assert wsb(C.byref(p), 1, 0) == cov(C.byref(p), 1, 0) + 2 * col and wsb(C.byref(p), 1, 1) == cov(C.byref(p), 1, 1) + 2 * col
    assert wsb(C.byref(p), 1, 2) == 0 and wsb(C.byref(p), 0, 0) == 0 and wsb(None, 1, 0) == 0
    assert wsb(C.byref(_params(65)), 1, 0) == 0 and wsb(C.byref(_params(n_cams=17)), 1, 0) == 0


def test_invalid_arguments_are_refused_without_a_device():
    from acinoset_amd import _lib
    fn = _lib.lib().acino_skel_fte_calibration_sensitivity
    p = _params()
    ops, act = (_lib.SkelOp * 6)(), (C.c_int32 * 36)()
    status = (C.c_int32 * 2)()
    fake = C.c_void_p(1 << 20)

    def call(prm=p, sigma=fake, outs=(fake, fake, fake, fake), pin=0, ws=fake, ws_bytes=0, n_clips=2):
        return fn(C.byref(prm), n_clips, 0, ops, act, fake, fake, fake, fake, fake, fake, sigma, *outs, status, ws, ws_bytes, None,
                  pin, None)

    err = _lib.lib().acino_last_error_string
    assert call() == -3 and b"too small" in err()               # (valid up to the workspace of 0 bytes: no device call)
    assert call(ws=C.c_void_p((1 << 20) + 8), ws_bytes=1 << 40) == -3 and b"aligned" in err()
    for kw, what in ((dict(outs=(None, None, None, None)), b"at least one"), (dict(sigma=None), b"d_cov_cams"),
                     (dict(sigma=None, outs=(None, None, None, fake)), b"d_cov_cams"), (dict(prm=_params(n_cams=17)), b"n_cams"),
                     (dict(pin=2), b"pin_unobserved"), (dict(pin=-1), b"pin_unobserved"), (dict(n_clips=0), b"n_clips"),
                     (dict(prm=_params(65)), b"n_active")):
        assert call(**kw) == -1, kw
        assert what in err(), (kw, err())
    assert call(sigma=None, outs=(fake, None, None, None)) == -3          # S alone needs no covariance


def test_python_argument_checks_come_before_the_gpu(golden_dir):
    from acinoset_amd import build
    c = scases.case(golden_dir, "slice12")
    model, x = c["model"], c["x"]
    good = fref.random_psd(2)
    bad_nan, bad_asym = good.copy(), good.copy()
    bad_nan[7, 7] = np.nan
    bad_asym[6, 9] += 1e-6
    for bad in (good[:6, :6], np.zeros((12, 13)), bad_nan, bad_asym, dict(cov_points=None)):
        with pytest.raises(ValueError, match="cov_cams"):
            build.model_calibration_sensitivity([model], [x], bad)
        with pytest.raises(ValueError, match="cov_cams"):
            build.solve_models([model], [x], cov_cams=bad)
    with pytest.raises(ValueError, match="no models"):
        build.model_calibration_sensitivity([], [], good)
