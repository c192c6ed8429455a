"""The pinhole camera model of the EKF and the skeleton FTE, host side (no GPU needed): the three C entry points are
declared, exported and bound, their argument checks answer before any device call, the Python layer refuses what it
cannot do before any device work, build_model keeps a pinhole distortion vector whole, and the two test-side numpy
references (tests/pinhole_ekf_ref.py, tests/pinhole_skel_ref.py) are self-consistent."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import pinhole_ekf_ref as pekf
import pinhole_fte_ref as pref
import pinhole_skel_ref as pskel
from oracle import camera as ocam
from oracle import ekf as oekf
from oracle import fk as ofk
from oracle import synth as osynth

NEW = {"acino_ekf_run_pinhole": "acino_ekf_run", "acino_skel_fte_solve_pinhole": "acino_skel_fte_solve",
       "acino_skel_fte_solve_batch_pinhole": "acino_skel_fte_solve_batch"}
FAKE = C.c_void_p(0x1000)            # never dereferenced: the checks answer first


def _lib_handle():
    import __graft_entry__ as ge
    from acinoset_amd import _lib
    ge.build()
    return _lib, _lib.lib()


def _err(h):
    return h.acino_last_error_string().decode()


def test_new_entries_are_declared_exported_and_bound_like_their_fisheye_twins():
    _lib, h = _lib_handle()
    with open(os.path.join(_lib._HERE, "..", "include", "acinoset_hip.h")) as f:
        header = f.read()
    for name, twin in NEW.items():
        assert f"int {name}(" in header
        assert name in _lib.SIGNATURES
        fn, fn_twin = getattr(h, name), getattr(h, twin)
        assert fn.restype is C.c_int and fn.argtypes == fn_twin.argtypes
    assert h.acino_abi_version() == 3 and _lib.ABI_VERSION == 3
    # every file a source or header includes is part of source_hash() and the object cache key
    csrc = os.path.join(_lib._HERE, "csrc")
    listed = {os.path.basename(h) for h in _lib.HEADERS}
    assert "skel_assemble.hpp" in listed and "pinhole.hpp" in listed
    for name in _lib.SOURCES + [h for h in _lib.HEADERS if os.sep not in h]:
        with open(os.path.join(csrc, name)) as f:
            for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', f.read(), re.M):
                assert os.path.basename(inc) in listed, (name, inc)
    assert sorted(n for n in os.listdir(csrc) if n.endswith((".hpp", ".inc"))) == sorted(listed - {"acinoset_hip.h"})


def _ekf_params(n_cams=6):
    from acinoset_amd._lib import EkfParams
    return EkfParams(n_frames=10, n_seq=1, n_cams=n_cams, fps=120.0, dlc_thresh=0.5, cam_width=2704.0)


def test_ekf_run_pinhole_refuses_bad_arguments_without_a_device():
    _lib, h = _lib_handle()
    nbytes = h.acino_ekf_workspace_bytes(10, 1)
    for n_cams in (0, 7):
        p = _ekf_params(n_cams)
        rc = h.acino_ekf_run_pinhole(C.byref(p), FAKE, FAKE, FAKE, C.c_void_p(0x1000), nbytes, FAKE, FAKE, FAKE, None)
        assert rc == -1 and "n_cams" in _err(h)
    p = _ekf_params()
    for i in range(7):
        bufs = [FAKE] * 7
        bufs[i] = None
        det, cams, st0, ws, est, smo, outl = bufs
        rc = h.acino_ekf_run_pinhole(C.byref(p), det, cams, st0, ws, nbytes, est, smo, outl, None)
        assert rc == -1 and "null buffer" in _err(h)
    rc = h.acino_ekf_run_pinhole(C.byref(p), FAKE, FAKE, FAKE, C.c_void_p(0x1008), nbytes, FAKE, FAKE, FAKE, None)
    assert rc == -1 and "aligned" in _err(h)
    rc = h.acino_ekf_run_pinhole(C.byref(p), FAKE, FAKE, FAKE, C.c_void_p(0x1000), nbytes - 8, FAKE, FAKE, FAKE, None)
    assert rc == -1 and "too small" in _err(h)


def _skel_params(n_cams=4):
    from acinoset_amd._lib import SkelFteParams
    p = SkelFteParams()
    p.n_frames, p.n_cams, p.n_pose, p.n_ops, p.n_angles, p.n_active, p.max_iter = 10, n_cams, 3, 2, 3, 5, 5
    p.h, p.model_weight, p.l1_eps, p.lam0 = 1 / 120.0, 0.002, 1e-2, 1e-3
    return p


@pytest.mark.parametrize("batch", [False, True])
def test_skel_solve_pinhole_refuses_bad_arguments_without_a_device(batch):
    from acinoset_amd._lib import SkelFteInfo, SkelOp
    _lib, h = _lib_handle()
    ops = (SkelOp * 2)()
    act = (C.c_int32 * 5)(0, 1, 2, 3, 4)
    info = SkelFteInfo()

    def call(p, bufs, nbytes=1 << 20):
        meas, w, cams, lo, hi, x, ws = bufs
        if batch:
            return h.acino_skel_fte_solve_batch_pinhole(C.byref(p), 1, ops, act, meas, w, cams, lo, hi, x, None, ws, nbytes,
                                                        C.byref(info), None)
        return h.acino_skel_fte_solve_pinhole(C.byref(p), ops, act, meas, w, cams, lo, hi, x, None, ws, nbytes, C.byref(info),
                                              None)
    for n_cams in (0, 17):
        assert call(_skel_params(n_cams), [FAKE] * 7) == -1 and "n_cams" in _err(h)
    for i in range(7):
        bufs = [FAKE] * 7
        bufs[i] = None
        assert call(_skel_params(), bufs) == -1 and "null buffer" in _err(h)
    assert call(_skel_params(), [FAKE] * 6 + [C.c_void_p(0x1008)]) == -1 and "aligned" in _err(h)
    assert call(_skel_params(), [FAKE] * 7, nbytes=64) == -1 and "too small" in _err(h)


# ---- Python argument checks, before any device work -------------------------------------------------------------------
def _rig(d=pref.D12, n_cams=6):
    K, _, R, t = osynth.make_rig(n_cams)
    return K, np.tile(np.asarray(d, dtype=np.float64), (n_cams, 1)), R, t


def test_ekf_refuses_bad_camera_models_before_device_work():
    from acinoset_amd import calib, ekf
    K, D, R, t = _rig()
    det = np.zeros((5, 6, 20, 3))
    s0 = np.zeros(75)
    with pytest.raises(ValueError, match="camera_model"):
        ekf.ekf(det, K, D, R, t, 120.0, 0.5, (2704, 1520), states0=s0, camera_model="kannala")
    with pytest.raises(ValueError, match="contradicts"):
        ekf.ekf(det, K, D, R, t, 120.0, 0.5, (2704, 1520), states0=s0, camera_model="fisheye",
                project_func=calib.project_points)
    with pytest.raises(ValueError, match="contradicts"):
        ekf.ekf_batch([det], K, D, R, t, 120.0, 0.5, (2704, 1520), states0=[s0], camera_model="pinhole",
                      project_func=calib.project_points_fisheye)
    with pytest.raises(NotImplementedError):
        ekf.ekf(det, K, D, R, t, 120.0, 0.5, (2704, 1520), states0=s0, project_func=ocam.project_points)
    with pytest.raises(ValueError, match="contradicts"):
        ekf.initial_state(det, K, D, R, t, 120.0, 0.5, camera_model="fisheye", project_func=calib.project_points)


@pytest.fixture(scope="module")
def fx(golden_dir):
    g = np.load(os.path.join(golden_dir, "skel_fte_model.npz"))
    return g, json.loads(str(g["skeleton_json"]))


def _tables(det, parts):
    return [(list(parts), det[:, c]) for c in range(det.shape[1])]


def _build(fx, D, **kw):
    from acinoset_amd import build
    g, sk = fx
    return build.build_model(sk, scene=(g["K"], D, g["R"], g["t"]), dlc_tables=_tables(g["det"], g["parts"]),
                             n_frames=int(g["n_frames"]), start_frame=int(g["start_frame"]), initial_line=False, **kw)[0]


@pytest.mark.parametrize("n", [5, 8, 12])
def test_build_model_keeps_the_pinhole_distortion_vector(fx, n):
    from acinoset_amd import calib
    g, _sk = fx
    D = np.tile(pref.D12[:n], (len(g["K"]), 1))
    m = _build(fx, D, camera_model="pinhole")
    assert m.camera_model == "pinhole" and m.D.shape == (len(g["K"]), n) and np.array_equal(m.D, D)
    m2 = _build(fx, D, project_func=calib.project_points)
    assert m2.camera_model == "pinhole" and np.array_equal(m2.D, D)


def test_build_model_fisheye_default_and_refusals(fx):
    from acinoset_amd import calib
    g, _sk = fx
    m = _build(fx, g["D"])
    assert m.camera_model == "fisheye" and m.D.shape == (len(g["K"]), 4)
    assert np.array_equal(m.D, np.asarray(g["D"]).reshape(-1, 4))
    C_ = len(g["K"])
    with pytest.raises(ValueError):
        _build(fx, np.zeros((C_, 6)), camera_model="pinhole")                  # not an OpenCV length
    tilt = np.zeros((C_, 14))
    tilt[:, 12] = 0.01
    with pytest.raises(ValueError, match="tilt"):
        _build(fx, tilt, camera_model="pinhole")
    with pytest.raises(ValueError, match="camera_model"):
        _build(fx, g["D"], camera_model="kannala")
    with pytest.raises(ValueError, match="contradicts"):
        _build(fx, g["D"], camera_model="fisheye", project_func=calib.project_points)
    with pytest.raises(NotImplementedError):
        _build(fx, g["D"], project_func=ocam.project_points)


def test_solve_models_refuses_a_batch_of_mixed_cameras(fx):
    from acinoset_amd import build
    g, _sk = fx
    fish = _build(fx, g["D"])
    pin = _build(fx, np.tile(pref.D5, (len(g["K"]), 1)), camera_model="pinhole")
    with pytest.raises(ValueError, match="camera model"):
        build.solve_models([fish, pin])
    with pytest.raises(ValueError, match="camera model"):
        build.solve_models([pin, fish, pin])


def test_dense_sba_and_config5_refuse_bf16_pinhole_before_device_work():
    from acinoset_amd import sba
    K, D, R, t = _rig()
    det = np.zeros((4, 6, 20, 3))
    pts = np.zeros((4, 20, 3))
    with pytest.raises(ValueError, match="pinhole"):
        sba.bundle_adjust_dense_points_and_extrinsics(det, pts, K, D, R, t, precision="bf16", camera_model="pinhole")
    with pytest.raises(ValueError, match="camera_model"):
        sba.bundle_adjust_dense_points_and_extrinsics(det, pts, K, D, R, t, camera_model="kannala")
    with pytest.raises(ValueError, match="pinhole"):
        sba.refine_extrinsics_from_clips([det], K, D, R, t, 1 / 120.0, precision="bf16", camera_model="pinhole")
    with pytest.raises(ValueError, match="pinhole"):              # the entry's default precision is bf16
        sba.refine_extrinsics_from_clips([det], K, D, R, t, 1 / 120.0, camera_model="pinhole")


# ---- the references ---------------------------------------------------------------------------------------------------
def test_ekf_reference_measures_through_the_pinhole_projection():
    K, D, R, t = _rig(pref.D5)
    rng = np.random.default_rng(3)
    pose = rng.normal(0.0, 0.3, 25)
    pose[:3] = [2.0, 6.0, 0.5]
    saved = oekf.h_function
    with pekf._pinhole_measurement():
        for c in range(len(K)):
            want = ocam.project_points(oekf.marker_coords(pose), K[c], D[c], R[c], t[c])
            assert np.array_equal(oekf.h_function(pose, K[c], D[c], R[c], t[c]), want)
            assert np.array_equal(pekf.h_pinhole(pose, K[c], D[c], R[c], t[c]), want)
    assert oekf.h_function is saved                               # restored after the call
    # a noiseless pinhole sprint is tracked: the filter really measures with the pinhole model
    n = 16
    q = osynth.trajectory(n, "sprint")
    pos = ofk.cheetah_fk(q)
    det = np.zeros((n, len(K), 20, 3))
    for c in range(len(K)):
        det[:, c, :, :2] = ocam.project_points(pos.reshape(-1, 3), K[c], D[c], R[c], t[c]).reshape(n, 20, 2)
        det[:, c, :, 2] = 0.9
    s0 = oekf.initial_state(np.arange(float(n)), pos[:, 2], 0, 1 / 120)
    out = pekf.ekf(det, K, D, R, t, 120.0, 0.5, 2704, s0)
    assert oekf.h_function is saved
    assert np.abs(out["smoothed_x"][:, :3] - q[:, oekf.EKF_ORDER][:, :3]).max() < 0.08          # metres
    fish = oekf.ekf(det, K, np.zeros((len(K), 4)), R, t, 120.0, 0.5, 2704, s0)
    assert np.abs(fish["x"] - out["x"]).max() > 1e-3                                           # not the fisheye filter


@pytest.mark.parametrize("d", ["D5", "D12"])
def test_skel_reference_gradient_matches_central_differences(fx, d):
    g, sk = fx
    D = np.tile(getattr(pref, d), (len(g["K"]), 1))
    prob = pskel.PinholeSkelFTEProblem(sk, g["meas"], g["meas_err_weight"], g["K"], D, g["R"], g["t"], float(g["h"]))
    X = g["case_x"][int(g["grad_case"])][:, prob.ACT]
    F, grad, H, _nb = prob.evaluate(X)
    assert np.isfinite(F) and np.abs(H - np.swapaxes(H, 1, 2)).max() < 1e-9 * np.abs(H).max()
    rng = np.random.default_rng(11)
    step = 1e-6
    for _ in range(24):
        n, p = int(rng.integers(prob.N)), int(rng.integers(prob.P))
        xp, xm = X.copy(), X.copy()
        xp[n, p] += step
        xm[n, p] -= step
        fd = (prob.evaluate(xp, need_jac=False)[0] - prob.evaluate(xm, need_jac=False)[0]) / (2 * step)
        assert abs(fd - grad[n, p]) < 1e-5 * max(1.0, np.abs(grad).max()), (n, p, fd, grad[n, p])
    # and the measurement term is not the fisheye oracle's
    from oracle import skel_fte as osf
    fish = osf.SkelFTEProblem(sk, g["meas"], g["meas_err_weight"], g["K"], g["D"], g["R"], g["t"], float(g["h"]))
    assert abs(fish.evaluate(X, need_jac=False)[0] - F) > 1e-6 * abs(F)
