"""CPU: the formula behind csrc/ekf_cov.hip, its references, and the two entry points of the C ABI.

The smoothed covariances of tests/ekf_cov_ref.fp64_chain (numpy fp64: ``linearise`` + ``step_fp64(..., "push")``, lower
triangle mirrored as the kernels do) are compared with the marginals of the dense joint Gaussian posterior of the same
linearised model: the recursion P_s[i] = P_est[i] + A_i (P_s[i+1] - P_pred[i+1]) A_i^T is the right one for this filter,
gate included, on the frames 1 .. N-1.  Frame 0 is not smoothed by the reference (:836-839): it carries P_est[0], which is NOT
the joint marginal (it differs by 6 to 35 in the scale below) - a property of the reference's smoother, asserted here so that
nobody "fixes" it unnoticed.  Measured here (scaled by sqrt(P_ii P_jj)): chain against joint marginals 2.7e-11 and 3.8e-10 on
the two clips (9e-12 and 1.7e-10 with another BLAS); every fp64 step at 0.019 of ``smooth_cov_step``'s bound or less, the
bound itself 7e-13 to 6.4e-12; smallest eigenvalue of the scaled P_est - P_s -1.3e-13; smallest diagonal entry of P_s
1.3e-4; marker floor 9.8e-16."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ekf_cov_ref as cref
import ekf_step_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FPS = 120.0
# (N, cameras, seed offset k): the two clips of the joint-posterior comparison, then the step tests' 7x6 and 3x3
JOINT = ((4, [0, 3], 4), (5, [0, 1, 2, 4], 6))
MORE = ((7, [0, 1, 2, 3, 4, 5], 1), (3, [1, 2, 4], 3))


@pytest.fixture(scope="module")
def chains():
    """The fp64 chain of every case (shared, never modified)."""
    out = {}
    for n, cams, k in JOINT + MORE:
        det, rig, s0 = ref.fisheye_case(n, cams, k)
        out[(n, len(cams))] = cref.fp64_chain(det, rig, s0, FPS)
    return out


def test_header_binding_and_library_carry_the_two_entries():
    from acinoset_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "acinoset_hip.h")).read(), flags=re.S)
    handle = C.CDLL(_lib.SO_PATH)
    for name, arity in (("acino_ekf_smoothed_covariance", 5), ("acino_ekf_marker_covariance", 7)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m, f"{name} is not declared in acinoset_hip.h"
        assert len(m.group(1).split(",")) == arity == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(handle, name) and hasattr(_lib.lib(), name)
    assert re.search(r"#define ACINO_ABI_VERSION 3\b", header) and _lib.ABI_VERSION == 3 and _lib.lib().acino_abi_version() == 3
    assert "ekf_cov.hip" in _lib.SOURCES and "ekf_dev.hpp" in _lib.HEADERS
    for name in ("acino_ekf_run", "acino_ekf_run_pinhole"):                      # the existing calls keep their arity
        assert len(_lib.SIGNATURES[name][1]) == 10


def test_argument_checks_need_no_device():
    from acinoset_amd import _lib
    lib = _lib.lib()
    prm = _lib.EkfParams(n_frames=4, n_seq=1, n_cams=2, fps=120.0, dlc_thresh=0.5, cam_width=2704.0)
    need = lib.acino_ekf_workspace_bytes(4, 1)
    one, two = C.c_void_p(256), C.c_void_p(512)                              # never dereferenced: every call fails its checks
    assert lib.acino_ekf_smoothed_covariance(None, one, need, two, None) == -1
    assert lib.acino_ekf_smoothed_covariance(C.byref(prm), None, need, two, None) == -1
    assert lib.acino_ekf_smoothed_covariance(C.byref(prm), one, need, None, None) == -1
    assert lib.acino_ekf_smoothed_covariance(C.byref(prm), C.c_void_p(264), need, two, None) == -1       # alignment
    assert lib.acino_ekf_smoothed_covariance(C.byref(prm), one, need - 1, two, None) == -1               # size
    assert b"workspace too small" in lib.acino_last_error_string()
    assert lib.acino_ekf_marker_covariance(C.byref(prm), one, two, None, None, None, None) == -1         # no output at all
    assert b"no output" in lib.acino_last_error_string()
    assert lib.acino_ekf_marker_covariance(C.byref(prm), None, two, one, None, None, None) == -1
    assert lib.acino_ekf_marker_covariance(C.byref(prm), one, None, one, None, None, None) == -1
    prm.n_frames = 0
    assert lib.acino_ekf_smoothed_covariance(C.byref(prm), one, need, two, None) == -1
    assert lib.acino_ekf_marker_covariance(C.byref(prm), one, two, one, None, None, None) == -1


@pytest.mark.parametrize("value", ["nonsense", "Bars", 1, 0, None])
def test_return_cov_is_validated_before_any_device_work(value):
    from acinoset_amd import ekf
    for call in (lambda: ekf.ekf(None, None, None, None, None, 120.0, 0.5, (2704, 1520), return_cov=value),
                 lambda: ekf.ekf_batch([None], None, None, None, None, 120.0, 0.5, (2704, 1520), return_cov=value)):
        with pytest.raises(ValueError, match="return_cov"):
            call()


@pytest.mark.parametrize("case", JOINT)
def test_recursion_equals_the_joint_posterior_marginals(chains, case):
    n, cams, _k = case
    ch = chains[(n, len(cams))]
    joint = cref.joint_marginals(ch["H"], ch["Rd"], ch["P0"], 1 / FPS)
    err = [ref.cov_error(ch["P_s"][i], joint[i]) for i in range(n)]
    print(f"\n{n} frames, {len(cams)} cameras: scaled |P_s - joint marginal| per frame " + " ".join(f"{e:.2e}" for e in err))
    assert max(err[1:]) <= 1e-8, err
    # the last frame is the filter's own marginal; frame 0 is NOT smoothed by the reference and is far from the marginal
    assert np.array_equal(ch["P_s"][n - 1], ch["P_est"][n - 1]) and np.array_equal(ch["P_s"][0], ch["P_est"][0])
    assert err[0] > 1.0
    # the filtered covariance is no stand-in: on the smoothed frames it is far from the marginal as well
    assert min(ref.cov_error(ch["P_est"][i], joint[i]) for i in range(1, n - 1)) > 1e-2


def test_every_fp64_step_lies_within_the_rounding_bound(chains):
    worst, tight = 0.0, 0.0
    for (n, c), ch in chains.items():
        for i in range(1, n - 1):
            want, bound = cref.smooth_cov_step(ch["P_est"][i], ch["gain"][i], ch["P_s"][i + 1], 1 / FPS)
            ratio = float((np.abs(ch["P_s"][i] - want) / bound).max())
            d = np.sqrt(np.diag(ch["P_s"][i]))
            rel = float((bound / np.outer(d, d)).max())
            print(f"{n}x{c} frame {i}: |d| / bound {ratio:.2e}   bound / sqrt(P_ii P_jj) {rel:.2e}")
            worst, tight = max(worst, ratio), max(tight, rel)
    assert 0 < worst <= 1.0
    assert tight < 1e-10                      # the bound itself is tight (1e-12 to 6e-12 here)
    # and it notices one entry of one gain off by 1e-9 of its row
    ch = chains[(7, 6)]
    A = ch["gain"][3].copy()
    r, c = 30, int(np.argmax(np.abs(ch["P_s"][4] - ch["P_est"][4]).sum(0)))
    A[r, c] += 1e-9 * np.abs(A[r]).max()
    from oracle import ekf as oekf
    _, Q, F = oekf.model_matrices(1 / FPS)
    Pp = F @ ch["P_est"][3] @ F.T + Q
    bad = ch["P_est"][3] + A @ (ch["P_s"][4] - Pp) @ A.T
    want, bound = cref.smooth_cov_step(ch["P_est"][3], ch["gain"][3], ch["P_s"][4], 1 / FPS)
    assert float((np.abs(bad - want) / bound).max()) > 1.0


def test_smoothing_only_shrinks_and_keeps_a_positive_diagonal(chains):
    lam_min, diag_min = np.inf, np.inf
    for (n, c), ch in chains.items():
        for i in range(n):
            assert np.array_equal(ch["P_s"][i], ch["P_s"][i].T)
            lam_min = min(lam_min, cref.loewner_min(ch["P_est"][i], ch["P_s"][i]))
            diag_min = min(diag_min, float(np.diag(ch["P_s"][i]).min()))
    print(f"\nsmallest eigenvalue of the scaled P_est - P_s {lam_min:.2e}; smallest diagonal entry of P_s {diag_min:.2e}")
    assert lam_min >= -1e-12
    assert diag_min > 0
    # smoothing is worth something here: pose std of the smoothed frames of the 7-frame clip against the filtered one
    ch = chains[(7, 6)]
    ratio = np.sqrt(np.diagonal(ch["P_s"][1:6], axis1=1, axis2=2) / np.diagonal(ch["P_est"][1:6], axis1=1, axis2=2))[:, :25]
    print("pose std smoothed / filtered, 7x6, median per frame " + " ".join(f"{v:.2f}" for v in np.median(ratio, 1)))
    assert ratio.max() <= 1 + 1e-12 and np.median(ratio) < 0.95


def test_marker_tolerance_is_100x_the_measured_fp64_floor(chains):
    floor = 0.0
    for ch in chains.values():
        for key in ("P_est", "P_s"):
            for x, P in zip(ch["est"], ch[key]):
                want, scale = cref.marker_cov(x, P)
                got = cref.marker_cov_fp64(x, P)
                floor = max(floor, float((np.abs(got - want[None]).astype(np.float64) / scale[None]).max()))
    print(f"\nmarker floor {floor:.2e} (recorded {cref.MARKER_FLOOR:.2e}, tolerance {cref.MARKER_TOL:.2e})")
    assert 0 < floor <= cref.MARKER_FLOOR == cref.MARKER_TOL / 100
    # the measure notices a Jacobian entry off by 1e-9 of its row: head position and yaw of the nose
    ch = chains[(7, 6)]
    J = cref.marker_jacobian(ch["est"][3])
    want, scale = cref.marker_cov(ch["est"][3], ch["P_s"][3])
    Jb = J.copy()
    Jb[2, 0, 5] += 1e-9 * np.abs(J[2, 0]).max()
    bad = np.einsum("lip,pq,ljq->lij", Jb, ch["P_s"][3][:25, :25], Jb)
    assert float((np.abs(bad - want) / scale).max()) > cref.MARKER_TOL
    # the oracle's Jacobian is the derivative of the oracle's FK (central difference, 1e-6: error 1e-10 or so)
    from oracle import ekf as oekf
    x = ch["est"][3][:25]
    for q in (0, 5, 9, 24):
        e = np.zeros(25)
        e[q] = 1e-6
        num = (oekf.marker_coords(x + e) - oekf.marker_coords(x - e)) / 2e-6
        assert np.abs(num - J[:, :, q]).max() < 1e-8
