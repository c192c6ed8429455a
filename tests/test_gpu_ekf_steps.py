"""GPU (-m gpu): every filter step, smoother gain and recursion step of csrc/ekf.hip against exact math of its OWN inputs.

tests/test_ekf.py and tests/test_gpu_pinhole_ekf_skel.py compare whole clips with the oracle at 5e-6 / 5e-5 / 1e-3: the
reference rounds every predicted state to float32, so whole clips cannot be held tighter.  Here every case is run once with
``return_internals=True`` and then, for every sequence and every frame i, from what the kernels left in the workspace:

* predict    x_pred[i] == tests/ekf_step_ref.predict32(GPU est[i-1]) bit for bit (states0 at i = 0);
* update     one oracle step from the GPU's own est[i-1], P_est[i-1] (P0 at i = 0) gives est[i], P_est[i] within the
             constants of ekf_step_ref.py (100 x the fp64 floor measured by tests/test_ekf_step_host.py); P_est[i] symmetric
             and with a positive diagonal;
* gate       the one-step outlier counts add up to ``outliers_ignored``; every one-step gate margin exceeds 1e-6 (a
             condition on the case, not a measurement: a frame under it FAILS);
* gain       the backward error of rts_gain[i] as a solution of A P_pred = P_est[i] F^T, row by row, for both solvers;
* recursion  smoothed[i] against est[i] + A_i (smoothed[i+1] - x_pred[i+1]) in extended precision within the dot product's
             rounding bound; the frames 0 and N-1 (all frames when N < 3) equal the filtered state bit for bit.

Largest deviations the MI355X produced over all cases (``-s`` prints them per frame and per test), beside the largest CPU
floor and the constant (ekf_step_ref.py):

    quantity                     MI355X     CPU floor   constant
    from P0   pose               8.9e-12    6.3e-13     6.3e-11
              velocity           1.7e-12    4.8e-14     4.9e-12
              acceleration       3.4e-11    2.8e-12     2.9e-10
              scaled covariance  6.0e-07    7.7e-08     1e-06      (the cap, 13 x the floor; generic pose, 240 good rows)
    later     pose               2.9e-12    7.4e-13     7.4e-11
              velocity           7.9e-12    9.3e-13     9.4e-11
              acceleration       2.4e-11    3.3e-12     3.3e-10
              scaled covariance  9.1e-12    3.3e-11     1e-09      (the cap, 30 x the floor)
    P_est asymmetry              0          -           1e-13
    gain backward error, Cholesky 1.6e-17, pivoting 1.3e-16        numpy's 2.3e-15; tolerance 8.3e-13
    recursion                    1.2e-02 of the dot-product bound
    smallest gate margin         1.6e-03                            must exceed 1e-06
    the whole file 6 s; the slowest test 0.9 s

Before the forward kernel mirrored the lower triangle of P after its update, the same run gave an asymmetry of up to 8.5e-08,
later-frame deviations of up to 2.4e-10 / 6.1e-09 / 3.7e-09 / 8.9e-08 (the Cholesky factorisations read one triangle, the
products both, the oracle the whole matrix) and gain backward errors of up to 2.7e-12: every case but the bit-for-bit ones
failed.  Mutants of the forward kernel: one coefficient of Q scaled by 1 + 1e-7 passes tests/test_ekf.py and fails 12 of the 13
tests here (covariance 4e-09 .. 1.4e-08, gains); the last dependent (variant, marker) pair dropped fails both files.
"""
import numpy as np
import pytest

import ekf_step_ref as ref
import pinhole_fte_ref as pref
from oracle import ekf as oekf

pytestmark = pytest.mark.gpu

KEYS = ("x", "dx", "ddx")
SKEYS = ("smoothed_x", "smoothed_dx", "smoothed_ddx")


def _stack(r, keys):
    return np.hstack([r[k] for k in keys])


def _check_forward(tag, det, rig, s0, got, fps=120.0, thresh=0.5, width=2704, camera="fisheye"):
    """Predict, update and gate of every frame; returns the largest deviations."""
    n = det.shape[0]
    sT = 1.0 / fps
    P0 = oekf.model_matrices(sT)[0]
    est, xp, Pe = _stack(got, KEYS), got["x_pred"], got["P_est"]
    assert xp.shape == (n, 75) and Pe.shape == (n, 75, 75) and np.isfinite(xp).all() and np.isfinite(Pe).all()
    worst = dict(first=dict(pose=0.0, velocity=0.0, acceleration=0.0, cov=0.0), later=dict(pose=0.0, velocity=0.0, acceleration=0.0, cov=0.0),
                 asym=0.0, margin=np.inf)
    fails, outliers = [], 0
    for i in range(n):
        prev, P_prev = (np.asarray(s0, dtype=np.float64), P0) if i == 0 else (est[i - 1], Pe[i - 1])
        assert np.array_equal(xp[i], ref.predict32(prev, sT).astype(np.float64)), (tag, i, "predict")
        one = ref.step(det[i], rig, fps, thresh, width, prev, P_prev, camera)
        assert np.array_equal(one["x_pred"], xp[i])
        when = "first" if i == 0 else "later"
        e = dict(ref.state_errors(est[i], one["est"]), cov=ref.cov_error(Pe[i], one["P_est"]))
        tol = dict(ref.STEP_TOL_STATE_FIRST if i == 0 else ref.STEP_TOL_STATE_LATER,
                   cov=ref.STEP_TOL_COV_FIRST if i == 0 else ref.STEP_TOL_COV_LATER)
        asym = ref.cov_asymmetry(Pe[i])
        print(f"{tag} frame {i}: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()) +
              f" asym {asym:.2e} margin {one['gate_margin']:.2e} outliers {one['outliers']}")
        for k, v in e.items():
            worst[when][k] = max(worst[when][k], v)
            if not v <= tol[k]:
                fails.append((tag, i, k, v, tol[k]))
        worst["asym"] = max(worst["asym"], asym)
        worst["margin"] = min(worst["margin"], one["gate_margin"])
        if not asym <= ref.COV_SYMMETRY_TOL:
            fails.append((tag, i, "asymmetry", asym, ref.COV_SYMMETRY_TOL))
        if not np.all(np.diag(Pe[i]) > 0):
            fails.append((tag, i, "diagonal"))
        if not one["gate_margin"] > ref.GATE_MARGIN_MIN:
            fails.append((tag, i, "gate margin", one["gate_margin"]))
        outliers += one["outliers"]
    print(f"{tag} worst: {worst}")
    assert not fails, fails
    assert outliers == got["outliers_ignored"], (tag, outliers, got["outliers_ignored"])
    return outliers


def _check_smoother(tag, got, fps=120.0):
    """Gain and recursion of every smoothed frame, the untouched ends, the NaN fill of the gains the kernel does not write."""
    est, sm, xp, A, Pe = _stack(got, KEYS), _stack(got, SKEYS), got["x_pred"], got["rts_gain"], got["P_est"]
    n = est.shape[0]
    assert A.shape == (n, 75, 75)
    assert np.array_equal(sm[0], est[0]) and np.array_equal(sm[n - 1], est[n - 1])
    assert np.isnan(A[0]).all() and np.isnan(A[n - 1]).all()
    if n < 3:
        assert np.array_equal(sm, est) and np.isnan(A).all()
        return
    fails, eta_max, rec_max = [], 0.0, 0.0
    for i in range(1, n - 1):
        assert np.isfinite(A[i]).all(), (tag, i)
        eta = ref.gain_backward_error(A[i], Pe[i], 1.0 / fps)
        want, bound = ref.recursion_bound(est[i], xp[i + 1], A[i], sm[i + 1])
        ratio = float((np.abs(sm[i] - want) / bound).max())
        print(f"{tag} frame {i}: gain eta {eta:.2e} (tol {ref.GAIN_TOL:.2e})  recursion |d| / bound {ratio:.2e}")
        eta_max, rec_max = max(eta_max, eta), max(rec_max, ratio)
        if not eta <= ref.GAIN_TOL:
            fails.append((tag, i, "gain", eta))
        if not ratio <= 1.0:
            fails.append((tag, i, "recursion", ratio))
    print(f"{tag} worst: gain eta {eta_max:.2e} recursion {rec_max:.2e} of its bound")
    assert not fails, fails


def _run(det, rig, s0, fps=120.0, thresh=0.5, res=(2704, 1520), **kw):
    from acinoset_amd import ekf
    return ekf.ekf(det, *rig, fps, thresh, res, states0=s0, with_positions=False, return_internals=True, **kw)


# (N, cameras, seed offset k, the reference's outlier count on its own run or None)
FISHEYE = {"7x6": (7, [0, 1, 2, 3, 4, 5], 1, 36), "4x5": (4, [0, 1, 2, 3, 4], 2, 12), "5x4": (5, [0, 1, 2, 4], 6, 6),
           "3x3": (3, [1, 2, 4], 3, 3), "2x2": (2, [0, 3], 4, None), "1x1": (1, [2], 5, None)}


@pytest.mark.parametrize("name", list(FISHEYE))
def test_fisheye_steps(gpu_lib, name):
    """Row counts 40 C: a half 16-row tile at C = 1, 3, 5; one gain workgroup at N = 3; no smoother at N = 2, 1."""
    n, cams, k, count = FISHEYE[name]
    det, rig, s0 = ref.fisheye_case(n, cams, k)
    got = _run(det, rig, s0)
    outliers = _check_forward(name, det, rig, s0, got)
    if count is not None:
        assert outliers == count > 0          # the gate is exercised, and as on the reference's own run
    _check_smoother(name, got)


def test_both_smoother_solvers(gpu_lib):
    """The 7-frame, 6-camera clip through the pivoting solver: the same filter bit for bit, its own gains and recursion."""
    n, cams, k, _count = FISHEYE["7x6"]
    det, rig, s0 = ref.fisheye_case(n, cams, k)
    chol, piv = _run(det, rig, s0), _run(det, rig, s0, smoother_pivoting=True)
    for key in KEYS + ("x_pred", "P_est", "outliers_ignored"):
        assert np.array_equal(chol[key], piv[key]), key
    _check_smoother("7x6 cholesky", chol)
    _check_smoother("7x6 pivoting", piv)
    assert not np.array_equal(chol["rts_gain"][1], piv["rts_gain"][1])         # two solvers did run


@pytest.mark.parametrize("d,n,cams,k", [("D12", 4, [0, 1, 2, 3, 4, 5], 11), ("D5", 3, [0, 3], 12)])
def test_pinhole_steps(gpu_lib, d, n, cams, k):
    seq = pref.pinhole_sequence(n, "sprint", getattr(pref, d), seed=20210313 + k)
    rig = tuple(seq[key][cams] for key in "KDRt")
    det = ref.corrupt(seq["det"][:, cams], k)
    s0 = oekf.initial_state(np.arange(float(n)), seq["pos_true"][:, 2], 0, 1 / 120)
    got = _run(det, rig, s0, camera_model="pinhole")
    _check_forward(f"pinhole {d}", det, rig, s0, got, camera="pinhole")
    _check_smoother(f"pinhole {d}", got)


def test_batch_of_three_different_clips(gpu_lib):
    """n_seq = 3: a wrong seq * N + i stride in P_est, the gains or x_pred shows in the second or third sequence."""
    from acinoset_amd import ekf
    cases = [ref.fisheye_case(4, [0, 2, 5], k) for k in (7, 8, 9)]
    rig = cases[0][1]
    assert not np.array_equal(cases[0][0], cases[1][0]) and not np.array_equal(cases[1][0], cases[2][0])
    out = ekf.ekf_batch([c[0] for c in cases], *rig, 120.0, 0.5, (2704, 1520), states0=[c[2] for c in cases],
                        with_positions=False, return_internals=True)
    plain = ekf.ekf_batch([c[0] for c in cases], *rig, 120.0, 0.5, (2704, 1520), states0=[c[2] for c in cases],
                          with_positions=False)
    for b, ((det, _rig, s0), got) in enumerate(zip(cases, out)):
        assert set(got) - set(plain[b]) == {"x_pred", "P_est", "rts_gain"}
        for key in KEYS + SKEYS + ("outliers_ignored",):
            assert np.array_equal(got[key], plain[b][key])           # the internals change nothing else
        _check_forward(f"batch seq {b}", det, rig, s0, got)
        _check_smoother(f"batch seq {b}", got)


def test_other_model_parameters(gpu_lib):
    """fps, camera width and likelihood threshold: sT enters F, Q and the prediction."""
    fps, thresh, width = 90.0, 0.9, 1920
    det, rig, s0 = ref.fisheye_case(4, [0, 1, 3, 5], 10, fps=fps)
    got = _run(det, rig, s0, fps=fps, thresh=thresh, res=(width, 1080))
    _check_forward("fps 90", det, rig, s0, got, fps=fps, thresh=thresh, width=width)
    _check_smoother("fps 90", got, fps=fps)


@pytest.mark.parametrize("start", ["pose", "nose line"])
def test_generic_pose(gpu_lib, start):
    """All 22 joint angles away from 0 (the kernel probes the marker / parameter dependencies at one pose of its own), from a
    start at the pose and from the nose-line start, which has every angle at 0."""
    det, rig, s0, line = ref.generic_pose_case()
    s = s0 if start == "pose" else line
    got = _run(det, rig, s)
    _check_forward(f"generic from {start}", det, rig, s, got)
    _check_smoother(f"generic from {start}", got)
