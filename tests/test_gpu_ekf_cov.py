"""GPU (-m gpu): the smoothed covariances and the marker error bars of csrc/ekf_cov.hip against exact math of their OWN inputs.

Every case is run once with ``return_internals=True, return_cov=True`` and then, for every sequence, from what the kernels
returned:

* recursion   smoothed_cov[i], i = 1 .. N-2, against P_est[i] + A_i (smoothed_cov[i+1] - P_pred[i+1]) A_i^T in extended
              precision from the GPU's own P_est[i], rts_gain[i] and smoothed_cov[i+1], entrywise within the rounding bound
              of tests/ekf_cov_ref.smooth_cov_step (|got - want| / bound <= 1);
* ends        smoothed_cov[0] == cov[0] and smoothed_cov[N-1] == cov[N-1] bit for bit (every frame when N < 3), and
              cov == P_est of the internals bit for bit;
* properties  every covariance symmetric bit for bit with a positive diagonal; P_est[i] - smoothed_cov[i] positive
              semidefinite to rounding (smallest eigenvalue of the scaled matrix >= -1e-12);
* markers     cov_positions / smoothed_cov_positions against J P[:25, :25] J^T from the oracle's product-rule Jacobian at the
              GPU's own state, in extended precision, entrywise relative to |J| |P| |J|^T within ekf_cov_ref.MARKER_TOL
              (100 x the fp64 floor measured by tests/test_ekf_cov_host.py);
* derived     std_positions == sqrt(trace cov_positions), std_x / std_dx / std_ddx == sqrt(diag) to 4 ulp, both sequences;
* flags       "bars" returns the arrays of True bit for bit without cov / smoothed_cov; without the flag the key set and
              every value are what they were.

Largest values the MI355X produced over all cases (``-s`` prints them per frame and per test), beside the CPU's (numpy fp64,
tests/test_ekf_cov_host.py) and the limit:

    quantity                                   MI355X     CPU        limit
    recursion |d| / bound                      1.4e-02    1.8e-02    1
    smallest eigenvalue, scaled P_est - P_s    -3.3e-14   -1.3e-13   -1e-12
    smallest diagonal entry of smoothed_cov    1.3e-04    1.3e-04    > 0
    marker covariance, relative                1.3e-14    9.8e-16    1.0e-13 (100 x the floor)
    derived bars                               0 ulp      -          4 ulp
    asymmetry of cov and smoothed_cov          0          0          0
    the whole file 3.1 s; the slowest test 0.3 s
"""
import numpy as np
import pytest

import ekf_cov_ref as cref
import ekf_step_ref as ref
import pinhole_fte_ref as pref
from oracle import ekf as oekf

pytestmark = pytest.mark.gpu

KEYS = ("x", "dx", "ddx")
SKEYS = ("smoothed_x", "smoothed_dx", "smoothed_ddx")
BARS = ("std_x", "std_dx", "std_ddx", "cov_positions", "std_positions")
BAR_KEYS = BARS + tuple("smoothed_" + k for k in BARS)
PLAIN_KEYS = set(KEYS + SKEYS) | {"outliers_ignored", "start_frame"}
EIG_MIN = -1e-12

# (N, cameras, seed offset k) - the clips of tests/test_gpu_ekf_steps.py
FISHEYE = {"7x6": (7, [0, 1, 2, 3, 4, 5], 1), "4x5": (4, [0, 1, 2, 3, 4], 2), "3x3": (3, [1, 2, 4], 3), "2x2": (2, [0, 3], 4),
           "1x1": (1, [2], 5)}


def _stack(r, keys):
    return np.hstack([r[k] for k in keys])


def _ulps(got, want):
    return float((np.abs(got - want) / np.spacing(np.abs(want))).max())


def _run(det, rig, s0, fps=120.0, thresh=0.5, res=(2704, 1520), **kw):
    from acinoset_amd import ekf
    kw.setdefault("return_internals", True)
    kw.setdefault("return_cov", True)
    return ekf.ekf(det, *rig, fps, thresh, res, states0=s0, with_positions=False, **kw)


def _check(tag, got, fps=120.0):
    """Every property of the covariance outputs of one sequence; returns the number of smoothed frames."""
    est, sm, Pe, A, cov, scov = _stack(got, KEYS), _stack(got, SKEYS), got["P_est"], got["rts_gain"], got["cov"], got["smoothed_cov"]
    n = est.shape[0]
    assert cov.shape == scov.shape == (n, 75, 75) and np.isfinite(scov).all()
    assert np.array_equal(cov, Pe), (tag, "cov is P_est")
    assert np.array_equal(scov[0], cov[0]) and np.array_equal(scov[n - 1], cov[n - 1]), (tag, "ends")
    if n < 3:
        assert np.array_equal(scov, cov)
    fails, worst = [], dict(rec=0.0, eig=np.inf, diag=np.inf, marker=0.0, ulp=0.0)
    for i in range(1, n - 1):
        want, bound = cref.smooth_cov_step(Pe[i], A[i], scov[i + 1], 1.0 / fps)
        ratio = float((np.abs(scov[i] - want) / bound).max())
        print(f"{tag} frame {i}: recursion |d| / bound {ratio:.2e}")
        worst["rec"] = max(worst["rec"], ratio)
        if not ratio <= 1.0:
            fails.append((tag, i, "recursion", ratio))
        assert not np.array_equal(scov[i], cov[i]), (tag, i, "not smoothed")
    for i in range(n):
        for name, P in (("cov", cov[i]), ("smoothed_cov", scov[i])):
            if not np.array_equal(P, P.T):
                fails.append((tag, i, name, "asymmetric", ref.cov_asymmetry(P)))
            if not np.all(np.diag(P) > 0):
                fails.append((tag, i, name, "diagonal"))
        lam = cref.loewner_min(cov[i], scov[i])
        worst["eig"], worst["diag"] = min(worst["eig"], lam), min(worst["diag"], float(np.diag(scov[i]).min()))
        if not lam >= EIG_MIN:
            fails.append((tag, i, "loewner", lam))
        for prefix, x, P in (("", est[i], cov[i]), ("smoothed_", sm[i], scov[i])):
            want, scale = cref.marker_cov(x, P)
            got_c = got[prefix + "cov_positions"][i]
            err = float((np.abs(got_c - want).astype(np.float64) / scale).max())
            worst["marker"] = max(worst["marker"], err)
            if not err <= cref.MARKER_TOL:
                fails.append((tag, i, prefix + "cov_positions", err))
            u = max(_ulps(got[prefix + "std_positions"][i], np.sqrt(np.trace(got_c, axis1=1, axis2=2))),
                    _ulps(np.hstack([got[prefix + k][i] for k in ("std_x", "std_dx", "std_ddx")]), np.sqrt(np.diag(P))))
            worst["ulp"] = max(worst["ulp"], u)
            if not u <= 4:
                fails.append((tag, i, prefix + "derived bars", u))
    for key in BAR_KEYS:
        assert got[key].shape[0] == n and np.isfinite(got[key]).all(), (tag, key)
    assert got["std_x"].shape == got["smoothed_std_ddx"].shape == (n, 25)
    assert got["cov_positions"].shape == (n, 20, 3, 3) and got["smoothed_std_positions"].shape == (n, 20)
    print(f"{tag} worst: recursion {worst['rec']:.2e} of its bound, eigenvalue {worst['eig']:.2e}, diagonal {worst['diag']:.2e}, "
          f"marker {worst['marker']:.2e} (tol {cref.MARKER_TOL:.1e}), derived {worst['ulp']:.1f} ulp")
    assert not fails, fails
    return max(n - 2, 0)


@pytest.mark.parametrize("name", list(FISHEYE))
def test_fisheye_covariances(gpu_lib, name):
    """7 and 4 frames; exactly one smoothed frame at N = 3; no recursion at N = 2, 1: smoothed_cov is cov bit for bit."""
    n, cams, k = FISHEYE[name]
    det, rig, s0 = ref.fisheye_case(n, cams, k)
    assert _check(name, _run(det, rig, s0)) == max(n - 2, 0)


def test_pivoting_smoother_gains(gpu_lib):
    """The 7-frame clip with the gains of the pivoting solver: the same filtered covariance, its own smoothed ones."""
    n, cams, k = FISHEYE["7x6"]
    det, rig, s0 = ref.fisheye_case(n, cams, k)
    chol, piv = _run(det, rig, s0), _run(det, rig, s0, smoother_pivoting=True)
    _check("7x6 pivoting", piv)
    assert np.array_equal(chol["cov"], piv["cov"]) and not np.array_equal(chol["smoothed_cov"][1], piv["smoothed_cov"][1])
    assert ref.cov_error(piv["smoothed_cov"][1], chol["smoothed_cov"][1]) < 1e-9


def test_batch_of_three_different_clips(gpu_lib):
    """n_seq = 3: a wrong seq * N + i stride in either kernel shows in the second or third sequence."""
    from acinoset_amd import ekf
    cases = [ref.fisheye_case(4, [0, 2, 5], k) for k in (7, 8, 9)]
    rig = cases[0][1]
    out = ekf.ekf_batch([c[0] for c in cases], *rig, 120.0, 0.5, (2704, 1520), states0=[c[2] for c in cases],
                        with_positions=False, return_internals=True, return_cov=True)
    for b, got in enumerate(out):
        _check(f"batch seq {b}", got)
    assert not np.array_equal(out[0]["smoothed_cov"], out[1]["smoothed_cov"])
    assert not np.array_equal(out[1]["smoothed_cov_positions"], out[2]["smoothed_cov_positions"])


def test_other_model_parameters(gpu_lib):
    """fps 90, width 1920, threshold 0.9: sT enters F and Q of the rebuilt P_pred."""
    fps, thresh, width = 90.0, 0.9, 1920
    det, rig, s0 = ref.fisheye_case(4, [0, 1, 3, 5], 10, fps=fps)
    _check("fps 90", _run(det, rig, s0, fps=fps, thresh=thresh, res=(width, 1080)), fps=fps)


def test_pinhole(gpu_lib):
    seq = pref.pinhole_sequence(3, "sprint", pref.D5, seed=20210313 + 12)
    cams = [0, 3]
    rig = tuple(seq[key][cams] for key in "KDRt")
    det = ref.corrupt(seq["det"][:, cams], 12)
    s0 = oekf.initial_state(np.arange(3.0), seq["pos_true"][:, 2], 0, 1 / 120)
    _check("pinhole D5", _run(det, rig, s0, camera_model="pinhole"))


@pytest.mark.parametrize("start", ["pose", "nose line"])
def test_generic_pose(gpu_lib, start):
    """Every joint angle away from 0: every rotation axis of the marker Jacobian is exercised."""
    det, rig, s0, line = ref.generic_pose_case()
    _check(f"generic from {start}", _run(det, rig, s0 if start == "pose" else line))


def test_flag_variants(gpu_lib):
    """ "bars" = True without the two 75 x 75 arrays, bit for bit; no flag = the dictionary of today, bit for bit."""
    n, cams, k = FISHEYE["4x5"]
    det, rig, s0 = ref.fisheye_case(n, cams, k)
    plain = _run(det, rig, s0, return_internals=False, return_cov=False)
    bars = _run(det, rig, s0, return_internals=False, return_cov="bars")
    full = _run(det, rig, s0, return_internals=False, return_cov=True)
    internals = _run(det, rig, s0, return_cov=False)
    assert set(plain) == PLAIN_KEYS
    assert set(bars) == PLAIN_KEYS | set(BAR_KEYS)
    assert set(full) == set(bars) | {"cov", "smoothed_cov"}
    assert set(internals) == PLAIN_KEYS | {"x_pred", "P_est", "rts_gain"}
    for key in PLAIN_KEYS:
        for other in (bars, full, internals):
            assert np.array_equal(plain[key], other[key]), key
    for key in BAR_KEYS:
        assert np.array_equal(bars[key], full[key]), key
    assert np.array_equal(full["cov"], internals["P_est"])
    from acinoset_amd import ekf
    with_pos = ekf.ekf(det, *rig, 120.0, 0.5, (2704, 1520), states0=s0, return_cov="bars")
    assert set(with_pos) == set(bars) | {"positions", "smoothed_positions"}
    assert np.array_equal(with_pos["smoothed_std_positions"], bars["smoothed_std_positions"])
