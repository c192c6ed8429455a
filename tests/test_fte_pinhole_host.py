"""The pinhole camera model of the FTE solve, host side (no GPU needed): the C entry point is exported and bound, its
argument checks answer before any device call, the Python layer refuses what the model does not support before any
device work, and the test-side numpy reference (tests/pinhole_fte_ref.py) agrees with oracle.camera."""
import ctypes as C

import numpy as np
import pytest

import pinhole_fte_ref as pref

RNG = np.random.default_rng(7)


def _lib_handle():
    import __graft_entry__ as ge
    from acinoset_amd import _lib
    ge.build()
    return _lib, _lib.lib()


def _params(precision="f64", n=30, cams=6):
    from acinoset_amd import fte
    return fte.make_params(n, cams, 1.0 / 120.0, precision=precision)


def test_create_pinhole_is_exported_and_bound_abi_unchanged():
    _lib, h = _lib_handle()
    assert "acino_fte_create_pinhole" in _lib.SIGNATURES
    fn = h.acino_fte_create_pinhole
    assert fn.restype is C.c_int and len(fn.argtypes) == 7
    assert h.acino_abi_version() == 3 and _lib.ABI_VERSION == 3
    with open(_lib.os.path.join(_lib._HERE, "..", "include", "acinoset_hip.h")) as f:
        assert "int acino_fte_create_pinhole(" in f.read()


def _err(h):
    return h.acino_last_error_string().decode()


def test_create_pinhole_null_buffers_refused_without_a_device():
    _lib, h = _lib_handle()
    p = _params()
    out = C.c_void_p()
    fake = C.c_void_p(0x1000)         # never dereferenced: the checks answer first
    for det, cams, ws in ((None, fake, fake), (fake, None, fake), (fake, fake, None)):
        rc = h.acino_fte_create_pinhole(C.byref(out), C.byref(p), det, cams, ws, 1 << 20, None)
        assert rc == -1 and "null buffer" in _err(h)
        assert not out.value


@pytest.mark.parametrize("precision", ["bf16", "bf16_residuals"])
def test_create_pinhole_bf16_refused_without_a_device(precision):
    _lib, h = _lib_handle()
    p = _params(precision)
    out = C.c_void_p()
    fake = C.c_void_p(0x1000)
    rc = h.acino_fte_create_pinhole(C.byref(out), C.byref(p), fake, fake, fake, 1 << 20, None)
    assert rc == -1 and "pinhole" in _err(h) and "fp64" in _err(h)
    assert not out.value


def test_set_precision_null_context_refused():
    _lib, h = _lib_handle()
    assert h.acino_fte_set_precision(None, 1) == -1


def _rig_and_det(n=12, d=pref.D12):
    from acinoset_amd import synth
    K, _, R, t = synth.make_rig()
    D = np.tile(d, (6, 1))
    det = np.zeros((n, 6, 20, 3))
    return det, K, D, R, t


def test_python_refuses_bf16_pinhole_before_device_work():
    from acinoset_amd import calib, fte
    det, K, D, R, t = _rig_and_det()
    with pytest.raises(ValueError, match="pinhole"):
        fte.FTEContext(det, K, D, R, t, 1 / 120.0, camera_model="pinhole", precision="bf16")
    with pytest.raises(ValueError, match="pinhole"):
        fte.fte_solve(det[..., :2], det[..., 2], K, D, R, t, 1 / 120.0, precision="bf16", camera_model="pinhole")
    with pytest.raises(ValueError, match="pinhole"):
        fte.fte_solve(det[..., :2], det[..., 2], K, D, R, t, 1 / 120.0, precision="bf16_residuals",
                      project_func=calib.project_points)
    with pytest.raises(ValueError, match="pinhole"):
        fte.fte_solve_clips([det, det], K, D, R, t, 1 / 120.0, precision="bf16", camera_model="pinhole")
    with pytest.raises(ValueError, match="pinhole"):
        fte.fte_solve_batch([det], K, D, R, t, 1 / 120.0, precision="bf16", camera_model="pinhole")


def test_python_camera_model_selection():
    from acinoset_amd import calib, fte
    assert fte.camera_model_of() == "fisheye"
    assert fte.camera_model_of("fisheye") == "fisheye"
    assert fte.camera_model_of("pinhole") == "pinhole"
    assert fte.camera_model_of(project_func=calib.project_points) == "pinhole"
    assert fte.camera_model_of(project_func=calib.project_points_fisheye) == "fisheye"
    assert fte.camera_model_of("pinhole", calib.project_points) == "pinhole"
    with pytest.raises(ValueError):
        fte.camera_model_of("pinhole", calib.project_points_fisheye)
    with pytest.raises(ValueError):
        fte.camera_model_of("orthographic")
    det, K, D, R, t = _rig_and_det()
    with pytest.raises(NotImplementedError):
        fte.fte_solve(det[..., :2], det[..., 2], K, D, R, t, 1 / 120.0, project_func=lambda *a: None)
    with pytest.raises(NotImplementedError):
        fte.FTEContext(det, K, D, R, t, 1 / 120.0, project_func=np.dot)
    # the records each model uploads: 24 doubles fisheye, 32 pinhole
    from acinoset_amd import synth
    Kf, Df, Rf, tf = synth.make_rig()
    assert fte.camera_records("fisheye", Kf, Df, Rf, tf).shape == (6, 24)
    rec = fte.camera_records("pinhole", K, D, R, t)
    assert rec.shape == (6, 32) and np.array_equal(rec[:, 4:16], D) and np.array_equal(rec, calib.pinhole_records(K, D, R, t))


def _points(n=400):
    # world points in front of camera 0 of the ring rig, over most of its image
    from acinoset_amd import synth
    K, _, R, t = synth.make_rig()
    dirs = np.stack([RNG.uniform(-0.9, 0.9, n), RNG.uniform(-0.55, 0.55, n), np.ones(n)], 1)
    Y = dirs * RNG.uniform(2.0, 12.0, n)[:, None]
    X = (Y - t[0].reshape(3)) @ R[0]
    return X, K[0], R[0], t[0]


@pytest.mark.parametrize("d", [pref.D12[:4], pref.D5, pref.D12[:8], pref.D12], ids=["d4", "d5", "d8", "d12"])
def test_reference_projection_equals_oracle(d):
    X, K, R, t = _points()
    uv, J, zc = pref.project_with_jac(X, K, d, R, t)
    want = pref.oracle_project(X, K, d, R, t)
    assert np.abs(uv - want).max() < 1e-12 and (zc > 0).all()        # px


@pytest.mark.parametrize("d", [pref.D5, pref.D12], ids=["d5", "d12"])
def test_reference_jacobian_equals_central_differences(d):
    X, K, R, t = _points(200)
    _, J, _ = pref.project_with_jac(X, K, d, R, t)
    h = 1e-6
    Jn = np.zeros_like(J)
    for j in range(3):
        e = np.zeros(3)
        e[j] = h
        up = pref.oracle_project(X + e, K, d, R, t)
        dn = pref.oracle_project(X - e, K, d, R, t)
        Jn[:, :, j] = (up - dn) / (2 * h)
    assert np.abs(J - Jn).max() < 1e-7 * np.abs(J).max()
