"""CPU: the host layer of the bundle adjustment - the two workspace sizes against their closed forms (the layout functions of
csrc/sba.hip and csrc/sba_cov.hip are the only list of the buffers, and must add up to what the entries always asked for), and
what the Python layer refuses before it asks for a device."""
import os

import numpy as np
import pytest

import __graft_entry__ as ge
import sba_cov_ref as ref
from acinoset_amd import _lib, sba

SCHUR_WG, COV_WG = 1024, 512                       # SBA_SCHUR_WG of sba.hip, CV_WG of sba_cov.hip
SIZES = [(1, 1), (1, 16), (37, 130), (255, 1000), (256, 256), (257, 1542), (1000, 5000), (100_001, 433_337),
         (1_280_000, 6_500_000), (1_300_003, 7_800_018)]


def _a256(v):
    return (v + 255) // 256 * 256


def _solve_bytes(C, P, fused):
    n = 6 * C
    b = 2 * _a256(P * 6 * 8) + 3 * _a256(P * 3 * 8)                              # V, Vinv | gp, dp, trial points
    b += _a256(P * C * 4) if fused else _a256(P * C * 18 * 8)                    # slot [P][C]  |  Wpc [P][C][18]
    b += _a256((SCHUR_WG + 32) * (n * n + n + 27 * C) * 8)                       # partial sums + 32 intermediate records
    b += _a256(SCHUR_WG * 4 * 8)                                                 # cost / prediction / trial-cost partials
    b += _a256(C * 21 * 8) + 3 * _a256(n * 8) + _a256(n * n * 8) + _a256(C * 12 * 8) + _a256(64)
    return b + 1024


def _cov_bytes(C):
    nn = 36 * C * C
    return _a256(COV_WG * nn * 8) + _a256(COV_WG * 4 * 8) + 4 * _a256(nn * 8) + _a256(64) + 1024


def test_workspace_sizes_are_the_closed_forms():
    """acino_sba_workspace_bytes and acino_sba_covariance_workspace_bytes for 1..16 cameras and point counts of 1, below, at and
    above one 256-point workgroup, and 1.3 M: the sums the entries have always returned.  Up to seven cameras the solve holds
    the slot table [P][C] (4 bytes a slot), from eight on (or with ACINO_SBA_UNFUSED) the coupling table Wpc [P][C][18]."""
    ge.build()
    lib = _lib.lib()
    unfused = os.environ.get("ACINO_SBA_UNFUSED") is not None
    for C in range(1, 17):
        fused = C <= 7 and not unfused
        for P, M in SIZES:
            assert lib.acino_sba_workspace_bytes(C, P, M) == _solve_bytes(C, P, fused), (C, P, M)
            assert lib.acino_sba_covariance_workspace_bytes(C, P, M) == _cov_bytes(C), (C, P, M)
    if not unfused:                                          # the slot table gives way to the Wpc table between 7 and 8 cameras
        P = 1000
        step = lib.acino_sba_workspace_bytes(8, P, 1) - lib.acino_sba_workspace_bytes(7, P, 1)
        assert step > _a256(P * 8 * 18 * 8) - _a256(P * 7 * 4)
    # the guards of the two exports: the solve's has no upper camera limit of its own (the entry refuses n_cams > 16)
    assert lib.acino_sba_workspace_bytes(0, 10, 10) == 0 and lib.acino_sba_workspace_bytes(3, -1, 10) == 0
    assert lib.acino_sba_workspace_bytes(3, 10, -1) == 0 and lib.acino_sba_workspace_bytes(3, 0, 0) == _solve_bytes(3, 0, not unfused)
    assert lib.acino_sba_workspace_bytes(17, 10, 10) == _solve_bytes(17, 10, False)
    assert lib.acino_sba_covariance_workspace_bytes(3, -1, 10) == 0 and lib.acino_sba_covariance_workspace_bytes(3, 10, -1) == 0
    assert lib.acino_sba_covariance_workspace_bytes(3, 0, 0) == _cov_bytes(3)


def test_solve_refuses_sizes_at_2_to_the_31_before_any_device_call():
    """SbaBuf holds the point and observation counts as int: the solve refuses what does not fit, as the covariance entry
    always has - with every other argument valid, so that nothing else can be the reason."""
    import ctypes as C
    ge.build()
    lib = _lib.lib()
    info, cinfo = _lib.SbaInfo(), _lib.SbaCovInfo()
    p8, null = C.c_void_p(256), C.c_void_p(0)
    for n_points, n_obs in ((1 << 31, 8), (4, 1 << 31)):
        prm = _lib.SbaParams(n_cams=3, optimize_cameras=1, n_points=n_points, n_obs=n_obs, f_scale=1.0, lam0=1e-3, camera_model=0)
        rc = lib.acino_sba_solve(C.byref(prm), p8, p8, p8, p8, p8, p8, p8, p8, 1 << 62, null, null, C.byref(info), null)
        assert rc == -1 and b"2^31" in lib.acino_last_error_string()
        rc = lib.acino_sba_covariance(C.byref(prm), p8, p8, p8, p8, p8, p8, p8, 0, 0, 1, null, 0, p8, 1 << 62, p8, null, null,
                                      C.byref(cinfo), null)
        assert rc == -1 and b"2^31" in lib.acino_last_error_string()
    # a short workspace keeps each entry's own answer: ACINO_ERR_INVALID_ARG from the solve, ACINO_ERR_WORKSPACE from the covariance
    prm = _lib.SbaParams(n_cams=3, optimize_cameras=1, n_points=4, n_obs=8, f_scale=1.0, lam0=1e-3, camera_model=0)
    assert lib.acino_sba_solve(C.byref(prm), p8, p8, p8, p8, p8, p8, p8, p8, 1024, null, null, C.byref(info), null) == -1
    assert b"workspace" in lib.acino_last_error_string()
    assert lib.acino_sba_covariance(C.byref(prm), p8, p8, p8, p8, p8, p8, p8, 0, 0, 1, null, 0, p8, 1024, p8, null, null,
                                    C.byref(cinfo), null) == -3
    assert b"workspace" in lib.acino_last_error_string()


def test_python_layer_builds_the_problem_before_any_device_work(monkeypatch):
    """One problem builder behind ``covariance``, the sparse solves and the dense entry: skewed fisheye intrinsics, a fisheye
    distortion vector that is not four entries, observation arrays of different lengths, a camera index out of range and a
    (point, camera) pair seen twice are refused on the host, and the device is never asked for (require_gpu would raise
    RuntimeError on a machine without one - and is made to, here)."""
    def no_device():
        raise RuntimeError("the device was asked for")
    monkeypatch.setattr(_lib, "require_gpu", no_device)
    prob = ref.make_problem(3, 8, 1)
    uv, X, pi, ci = prob["uv"], prob["X"], prob["pi"], prob["ci"]
    rig = (prob["K"], prob["D"], prob["R"], prob["t"])
    solve_kw = dict(optimize_cameras=True, f_scale=1.0, max_iter=2, ftol=1e-10, gtol=1e-10)
    # the dense entry: the two cases it used to let through
    det, pts = np.zeros((4, 3, 20, 3)), np.zeros((4, 20, 3))
    K_skew = np.array(prob["K"], dtype=np.float64)
    K_skew[1, 0, 1] = 1e-3 * K_skew[1, 0, 0]
    with pytest.raises(NotImplementedError, match="skewed fisheye"):
        sba.bundle_adjust_dense_points_and_extrinsics(det, pts, K_skew, *rig[1:])
    D5 = np.concatenate([np.asarray(prob["D"], dtype=np.float64).reshape(3, -1)[:, :4], np.full((3, 1), 1e-3)], axis=1)
    with pytest.raises(ValueError, match="4 distortion coefficients"):
        sba.bundle_adjust_dense_points_and_extrinsics(det, pts, prob["K"], D5, *rig[2:])
    with pytest.raises(RuntimeError, match="the device was asked for"):      # (five entries are a pinhole vector)
        sba.bundle_adjust_dense_points_and_extrinsics(det, pts, prob["K"], D5, *rig[2:], camera_model="pinhole")
    with pytest.raises(ValueError, match="4, 5, 8 or 12"):
        sba.bundle_adjust_dense_points_and_extrinsics(det, pts, prob["K"], np.zeros((3, 6)), *rig[2:], camera_model="pinhole")
    # covariance and the sparse solve: what they always raised
    for call in (lambda *a: sba.covariance(*a, *rig), lambda *a: sba._solve(*a, *rig, **solve_kw)):
        with pytest.raises(ValueError, match="one entry per observation"):
            call(uv, X, pi[:-1], ci)
        with pytest.raises(ValueError, match="one entry per observation"):
            call(uv, X, pi, ci[:-1])
        with pytest.raises(ValueError, match="camera_indices out of range"):
            call(uv, X, pi, ci + 1)
        with pytest.raises(ValueError, match="point_3d_indices out of range"):
            call(uv, X, pi + 1, ci)
    with pytest.raises(NotImplementedError, match="skewed fisheye"):
        sba.covariance(uv, X, pi, ci, K_skew, *rig[1:])
    dup = (np.vstack([uv, uv[:1]]), X, np.append(pi, pi[0]), np.append(ci, ci[0]))
    with pytest.raises(ValueError, match="observed twice"):
        sba._solve(*dup, *rig, **solve_kw)
    # (the covariance leaves duplicates to the library's check on the device, the solve does with host_checks=False)
    with pytest.raises(RuntimeError, match="the device was asked for"):
        sba.covariance(*dup, *rig)
    with pytest.raises(RuntimeError, match="the device was asked for"):
        sba._solve(*dup, *rig, host_checks=False, **solve_kw)
    with pytest.raises(RuntimeError, match="the device was asked for"):
        sba._solve(uv, X, pi, ci, *rig, **solve_kw)
