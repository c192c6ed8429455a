"""CPU: where the tolerances of tests/test_gpu_ekf_steps.py come from, and the workspace read-back contract.

The floor of one filter step in fp64 is measured against the 40-digit step of tests/ekf_step_ref.py on eight frames of the
oracle's own runs of the step tests' cases (``FLOOR_FRAMES``: frame 0 of three cases among them), for the reference's
formula and for the 25 x 25 form the kernel evaluates; the state constants of ekf_step_ref.py are 100 x that floor and may
not exceed the caps below.  For the covariance 100 x the floor would exceed the caps (floors 7.7e-08 from P0 and 3.3e-11
afterwards, caps 1e-06 and 1e-09): those two constants are the caps themselves, 13 x and 30 x the floor.  The smoother gain's
floor is the backward error of numpy's P_est F^T inv(P_pred) on the same runs."""
import numpy as np
import pytest

import ekf_step_ref as ref
from oracle import ekf as oekf

FPS, THRESH, WIDTH = 120.0, 0.5, 2704
# (case, frames): 8 frames in all, frame 0 (the step from P0, where the huge prior collapses) of three cases
# and the one step of the cases in which the filter is far from its target (the nose-line start on the generic pose: the
# 25 x 25 form loses ten times more there than on any tracking frame)
FLOOR_FRAMES = ((("fisheye", 7, [0, 1, 2, 3, 4, 5], 1), (0, 1, 3, 6)), (("fisheye", 4, [0, 1, 2, 3, 4], 2), (0,)),
                (("fisheye", 3, [1, 2, 4], 3), (1,)), (("generic", 3, None, 5), (0,)), (("nose line", 3, None, 5), (1,)))
STATE_CAP, COV_CAP_FIRST, COV_CAP_LATER = 1e-8, 1e-6, 1e-9


def _case(kind, n, cams, k):
    if kind == "fisheye":
        return ref.fisheye_case(n, cams, k)
    det, rig, s0, line = ref.generic_pose_case(n, k)
    return det, rig, (s0 if kind == "generic" else line)


@pytest.fixture(scope="module")
def runs():
    """The oracle's own run of every floor case (shared, never modified)."""
    out = []
    for case, frames in FLOOR_FRAMES:
        det, rig, s0 = _case(*case)
        out.append((det, rig, s0, oekf.ekf(det, *rig, FPS, THRESH, WIDTH, s0, keep_cov=True), frames))
    return out


@pytest.fixture(scope="module")
def floors(runs):
    """Largest deviation of the two fp64 steps from the 40-digit step: state per block and scaled covariance, the step
    from P0 and the later steps apart."""
    P0 = oekf.model_matrices(1 / FPS)[0]
    fl = dict(first=dict(pose=0.0, velocity=0.0, acceleration=0.0, cov=0.0), later=dict(pose=0.0, velocity=0.0, acceleration=0.0, cov=0.0))
    for det, rig, s0, run, frames in runs:
        est = np.hstack([run["x"], run["dx"], run["ddx"]])
        for i in frames:
            prev, P_prev = (s0, P0) if i == 0 else (est[i - 1], run["P_est"][i - 1])
            lin = ref.linearise(det[i], rig, FPS, THRESH, WIDTH, prev, P_prev)
            xe, Pe = ref.step_exact(det[i], rig, FPS, THRESH, WIDTH, prev, P_prev, lin=lin)
            one = ref.step(det[i], rig, FPS, THRESH, WIDTH, prev, P_prev)
            xr, Pr = ref.step_fp64(lin, "reference")
            # ``linearise`` + "reference" is the oracle's step, statement for statement; and the run continues from it
            assert np.array_equal(xr, one["est"]) and np.array_equal(Pr, one["P_est"])
            assert np.array_equal(one["est"], est[i]) and np.array_equal(one["P_est"], run["P_est"][i])
            assert one["gate_margin"] == lin["gate_margin"] == run["gate_margin"][i] and one["outliers"] == lin["outliers"]
            f = fl["first" if i == 0 else "later"]
            for form in ("reference", "push"):
                x, P = ref.step_fp64(lin, form)
                e = dict(ref.state_errors(x, xe), cov=ref.cov_error(P, Pe))
                print(f"floor case N={det.shape[0]} C={det.shape[1]} frame {i} {form:9s} " +
                      " ".join(f"{k} {v:.2e}" for k, v in e.items()))
                for k, v in e.items():
                    f[k] = max(f[k], v)
    print("floors", fl)
    return fl


def test_step_tolerances_are_100x_the_measured_fp64_floor(floors):
    for when, state, cov, cap in (("first", ref.STEP_TOL_STATE_FIRST, ref.STEP_TOL_COV_FIRST, COV_CAP_FIRST),
                                  ("later", ref.STEP_TOL_STATE_LATER, ref.STEP_TOL_COV_LATER, COV_CAP_LATER)):
        for name, _b in ref.BLOCKS:
            assert 0 < floors[when][name] <= state[name] / 100, (when, name, floors[when][name])
            assert state[name] <= STATE_CAP, (when, name)
        # the covariance: 100 x the measured floor (7.7e-08 from P0, 3.3e-11 afterwards) would pass the caps, so the constants
        # ARE the caps and only a smaller factor can be asserted of them (ekf_step_ref.py, beside the constants)
        assert 0 < floors[when]["cov"] <= cov / ref.STEP_TOL_COV_OVER_FLOOR[when], (when, floors[when]["cov"])
        assert cov == cap, when
    # at least 500 x tighter than the whole-clip tolerances 5e-6 / 5e-5 / 1e-3 of tests/test_ekf.py
    for state in (ref.STEP_TOL_STATE_FIRST, ref.STEP_TOL_STATE_LATER):
        assert state["pose"] <= 5e-6 / 500 and state["velocity"] <= 5e-5 / 500 and state["acceleration"] <= 1e-3 / 500


def test_the_cases_exercise_the_gate_and_stay_clear_of_it(runs):
    """The reference gates detections on every floor case with outliers, and no residual sits near its gate."""
    want = {(7, 6): 36, (4, 5): 12, (3, 3): 3}
    for det, _rig, _s0, run, _frames in runs:
        key = det.shape[:2]
        if key in want:
            assert run["outliers_ignored"] == want[key] > 0
        assert run["gate_margin"].min() > 8e-3                 # (8.96e-3 on the 7-frame clip is the smallest)
    det, rig, s0 = ref.fisheye_case(5, [0, 1, 2, 4], 6)
    run = oekf.ekf(det, *rig, FPS, THRESH, WIDTH, s0, keep_cov=True)
    assert run["outliers_ignored"] == 6 and run["gate_margin"].min() > 8e-3


def test_gain_tolerance_is_100x_numpys_backward_error(runs):
    _, Q, F = oekf.model_matrices(1 / FPS)
    eta = 0.0
    for _det, _rig, _s0, run, _frames in runs:
        for i in range(1, len(run["P_est"]) - 1):
            A = run["P_est"][i] @ F.T @ np.linalg.inv(run["P_pred"][i + 1])
            assert np.array_equal(run["P_pred"][i + 1], F @ run["P_est"][i] @ F.T + Q)
            eta = max(eta, ref.gain_backward_error(A, run["P_est"][i], 1 / FPS))
    print(f"\neta_ref {eta:.3e} 75 * 2^-53 = {75 * 2.0 ** -53:.3e}")
    assert 0 < eta <= max(ref.GAIN_ETA_REF, 75 * 2.0 ** -53)
    assert ref.GAIN_TOL == 100 * max(ref.GAIN_ETA_REF, 75 * 2.0 ** -53)
    # the measure notices a gain that is wrong in one entry by 1e-9 of its row (in the column of P_pred's largest row:
    # >= 1e-9 / 75 whatever the scaling of P)
    A_bad = A.copy()
    A_bad[3, np.argmax(np.abs(run["P_pred"][i + 1]).sum(1))] += 1e-9 * np.abs(A[3]).max()
    assert ref.gain_backward_error(A_bad, run["P_est"][i], 1 / FPS) > 10 * ref.GAIN_TOL


def test_predict32_and_recursion_bound_on_the_oracle(runs):
    det, rig, s0, run, _frames = runs[0]
    est = np.hstack([run["x"], run["dx"], run["ddx"]])
    sm = np.hstack([run["smoothed_x"], run["smoothed_dx"], run["smoothed_ddx"]])
    _, _Q, F = oekf.model_matrices(1 / FPS)
    for i in range(len(est)):
        prev = s0 if i == 0 else est[i - 1]
        assert np.array_equal(ref.predict32(prev, 1 / FPS).astype(np.float64), run["x_pred"][i])
    for i in range(1, len(est) - 1):
        A = run["P_est"][i] @ F.T @ np.linalg.inv(run["P_pred"][i + 1])
        want, bound = ref.recursion_bound(est[i], run["x_pred"][i + 1], A, sm[i + 1])
        assert np.all(np.abs(sm[i] - want) <= bound)
        assert np.all(bound < 1e-10 * np.maximum(1.0, np.abs(est[i])))      # the bound itself is tight


def test_workspace_layout_matches_the_library():
    from acinoset_amd import _lib, ekf
    lib = _lib.lib()
    for n, b in ((1, 1), (2, 3), (3, 1), (7, 2), (100, 5)):
        lay = ekf.workspace_layout(n, b)
        assert lay["end"] + 1024 == lib.acino_ekf_workspace_bytes(n, b)
        t = n * b
        a256 = lambda v: (v + 255) // 256 * 256
        assert lay["P_est"] == (0, (b, n, 75, 75)) and lay["rts_gain_T"] == (a256(t * 75 * 75 * 8), (b, n, 75, 75))
        assert lay["x_pred"] == (2 * a256(t * 75 * 75 * 8), (b, n, 75))
        assert lay["private"] == lay["x_pred"][0] + a256(t * 75 * 8) <= lay["end"]
        for name in ("P_est", "rts_gain_T", "x_pred"):
            assert lay[name][0] % 256 == 0
    with pytest.raises(ValueError):
        ekf.workspace_layout(0, 1)
