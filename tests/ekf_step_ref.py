"""An exact one-step reference of the EKF + RTS smoother (numpy + mpmath, no GPU), for tests that hold every filter step,
smoother gain and recursion step of csrc/ekf.hip to the mathematics of its OWN inputs.

Whole clips cannot be held tighter than float32-ulp level: the reference rounds every predicted state to float32
(src/all_optimizations.py:628), a 1e-13 difference flips an ulp now and then and the filter carries the flip on.  One step
from a given previous state and covariance has no such amplification.  A run leaves what a per-step check needs in the
caller-owned workspace (include/acinoset_hip.h, EKF section; ``ekf.ekf(..., return_internals=True)``): x_pred, P_est and the
smoother gains.  This module gives, for those inputs,

* ``predict32``          the reference's prediction in its own operation order, rounded to float32 - compared bit for bit;
* ``step``               one oracle step (oracle.ekf.ekf on a one-frame clip, ``P_init`` = the previous covariance);
* ``step_fp64``          the same step from the pieces of ``linearise`` in fp64, in the reference's form (K = P H^T inv(S)) or
                         in the 25 x 25 push-through form the kernel evaluates;
* ``step_exact``         the same step with the covariance prediction and the update evaluated at 40 digits;
* ``gain_backward_error`` the row-wise backward error of a smoother gain as a solution of A P_pred = P_est F^T;
* ``recursion_bound``    one smoother step in extended precision with the dot product's rounding bound;
* ``corrupt`` / ``fisheye_case`` / ``generic_pose_case``  the detection recipes of the step tests.

The tolerances of the GPU step tests are the named constants below: 100 x the deviation of the two fp64 steps from
``step_exact``, measured on the CPU by tests/test_ekf_step_host.py (which re-measures them on every run and asserts that
they still lie under constant / 100).  The factor 100: the kernel evaluates FK, projection and the 1e-3 difference quotient
in its own fp64 operation order with MFMA accumulation - through the quotient a relative perturbation of H of about 1e-13,
the size of the algebra's own rounding.
"""
import mpmath as mp
import numpy as np

import pinhole_ekf_ref as pekf
from oracle import ekf as oekf
from oracle import synth as osynth

N_POSE, NS = 25, 75
BLOCKS = (("pose", slice(0, 25)), ("velocity", slice(25, 50)), ("acceleration", slice(50, 75)))
DPS = 40

# ---- tolerances of tests/test_gpu_ekf_steps.py = 100 x the CPU floor (tests/test_ekf_step_host.py::FLOOR_FRAMES) -----------
# The floor is the deviation of an fp64 step from the 40-digit step, the larger of the two forms, the largest over the eight
# frames.  It is rounding noise, so it depends on the order in which the BLAS behind numpy adds: measured with OpenBLAS
# 0.3.29's Prescott, Nehalem, Sandybridge, Haswell / Zen and SkylakeX kernels at 1, 4 and 16 threads (11 results, a spread
# of up to 12 x); the figure beside each constant is the largest of them, its range in brackets.  The "later" floors are
# set by ONE frame, the first step after P0 of the filter started on the nose line under detections of the generic pose
# (far from its target: the 25 x 25 form loses ten times more there than on any frame of a tracking filter, where it stays
# under 5.4e-14 / 2.3e-13 / 1.3e-13 / 1.6e-12).
# |d block|max / max(1, |block|max) of est after one step; "first" = the step from P0, "later" = every other step
STEP_TOL_STATE_FIRST = dict(pose=6.3e-11,            # floor 6.27e-13 (2.7e-13 .. 6.3e-13)
                            velocity=4.9e-12,        # floor 4.84e-14 (2.0e-14 .. 4.8e-14)
                            acceleration=2.9e-10)    # floor 2.80e-12 (1.2e-12 .. 2.8e-12)
STEP_TOL_STATE_LATER = dict(pose=7.4e-11,            # floor 7.37e-13 (5.1e-14 .. 7.4e-13)
                            velocity=9.4e-11,        # floor 9.33e-13 (1.2e-13 .. 9.3e-13)
                            acceleration=3.3e-10)    # floor 3.27e-12 (4.6e-13 .. 3.3e-12)
# max |dP_ij| / sqrt(P_ii P_jj) of P_est after one step.  Here 100 x the floor passes the largest value either figure may
# take (1e-06 from P0, 1e-09 afterwards), so both constants are held AT that value and are a smaller multiple of the floor:
# from P0:  floor 7.68e-08 (2.0e-08 .. 7.7e-08), all of it the REFERENCE's form K = P H^T inv(S), (I - K H) P, in which the
#           prior of 1e1 .. 1e2 collapses by cancellation (the 25 x 25 form: 2.1e-10 .. 1.5e-09) - 13 x the floor;
# later:    floor 3.28e-11 (2.8e-12 .. 3.3e-11), the nose-line frame in the 25 x 25 form - 30 x the floor.
STEP_TOL_COV_FIRST = 1e-6
STEP_TOL_COV_LATER = 1e-9
STEP_TOL_COV_OVER_FLOOR = dict(first=5, later=10)       # what tests/test_ekf_step_host.py can still assert of them
# symmetry of P_est, scaled as above
COV_SYMMETRY_TOL = 1e-13
# every one-step gate margin must exceed this: the gate decision then cannot depend on rounding
GATE_MARGIN_MIN = 1e-6
# backward error of a smoother gain: 100 x max(eta_ref, 75 * 2^-53), eta_ref = that of numpy's P_est F^T inv(P_pred) on the
# oracle's runs of the host test: measured 2.3e-15 (1.1e-15 .. 2.3e-15 over the same BLAS kernels) - under 75 * 2^-53 =
# 8.3e-15, which therefore sets the tolerance: 8.3e-13
GAIN_ETA_REF = 2.3e-15
GAIN_TOL = 100 * max(GAIN_ETA_REF, 75 * 2.0 ** -53)


# ---- the pieces of one step -------------------------------------------------------------------------------------------------
def predict32(prev, sT):
    """oracle/ekf.py's prediction (:622-628) in exactly its operation order, rounded to float32."""
    prev = np.asarray(prev, dtype=np.float64)
    acc = prev[2 * N_POSE:]
    vel = prev[N_POSE:2 * N_POSE] + sT * acc
    pos = prev[:N_POSE] + sT * vel + (0.5 * sT ** 2) * acc
    return np.concatenate([pos, vel, acc]).astype(np.float32)


def _oracle(camera):
    if camera == "fisheye":
        return oekf.ekf
    if camera == "pinhole":
        return pekf.ekf
    raise ValueError(camera)


def step(det_i, rig, fps, thresh, cam_width, prev, P_prev, camera="fisheye"):
    """One oracle step from the state ``prev`` and the covariance ``P_prev`` on the detections det_i[C, 20, 3]."""
    out = _oracle(camera)(np.asarray(det_i)[None], *rig, fps, thresh, cam_width, prev, keep_cov=True, P_init=P_prev)
    return dict(est=np.hstack([out["x"], out["dx"], out["ddx"]])[0], P_est=out["P_est"][0], x_pred=out["x_pred"][0],
                outliers=int(out["outliers_ignored"]), gate_margin=float(out["gate_margin"][0]))


def linearise(det_i, rig, fps, thresh, cam_width, prev, P_prev, camera="fisheye"):
    """What the update of one step starts from, in fp64 and with the oracle's own statements: x_pred, P_pred, Hq [rows, 25],
    the diagonal of R, the gated residual, and the gate's outlier count and margin."""
    det_i = np.asarray(det_i, dtype=np.float64)
    n_cams, m = det_i.shape[0], 2 * det_i.shape[1]
    sT = 1.0 / fps
    _, Q, F = oekf.model_matrices(sT)
    s32 = predict32(prev, sT)
    x = s32.astype(np.float64)
    P = F @ np.asarray(P_prev, dtype=np.float64) @ F.T + Q
    H = np.zeros((n_cams * m, NS))
    h = np.zeros(n_cams * m)
    with (pekf._pinhole_measurement() if camera == "pinhole" else _nothing()):
        for j in range(n_cams):
            cam = tuple(a[j] for a in rig)
            h[j * m:(j + 1) * m] = oekf.h_function(x[:N_POSE], *cam).flatten()
            H[j * m:(j + 1) * m, :N_POSE] = oekf.numerical_jacobian(oekf.h_function, s32[:N_POSE], *cam)
    sd = 25.0 * np.ones(n_cams * m)
    sd[np.repeat(det_i[..., 2].reshape(-1) < thresh, 2)] = cam_width
    Rd = sd ** 2
    res = det_i[..., :2].reshape(-1) - h
    S = (H @ P @ H.T) + np.diag(Rd)
    temp = 3 * np.sqrt(np.diag(S))
    margin = float(np.min(np.abs(np.abs(res) - temp) / temp))
    outliers = 0
    for j in range(0, len(res), 2):
        if np.abs(res[j]) > temp[j] or np.abs(res[j + 1]) > temp[j + 1]:
            res[j:j + 2] = 0
            outliers += 1
    return dict(x_pred=x, P_pred=P, H=H, Rd=Rd, residual=res, S=S, outliers=outliers, gate_margin=margin, F=F, Q=Q)


class _nothing:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


def step_fp64(lin, form):
    """The update in fp64 from ``linearise``: form "reference" = K = P H^T inv(S), P <- (I - K H) P (the oracle's statements);
    "push" = the 25 x 25 form of csrc/ekf.hip, x += P[:, :25] (I + M Pq)^-1 g, P -= P[:, :25] (I + M Pq)^-1 M P[:25, :]."""
    x, P, H, Rd, res = lin["x_pred"], lin["P_pred"], lin["H"], lin["Rd"], lin["residual"]
    if form == "reference":
        K = P @ H.T @ np.linalg.inv(lin["S"])
        return x + K @ res, (np.eye(NS) - K @ H) @ P
    Hq = H[:, :N_POSE]
    M = Hq.T @ (Hq / Rd[:, None])
    g = Hq.T @ (res / Rd)
    A = np.linalg.inv(np.eye(N_POSE) + M @ P[:N_POSE, :N_POSE])
    return x + P[:, :N_POSE] @ (A @ g), P - P[:, :N_POSE] @ (A @ M) @ P[:N_POSE, :]


_to_mp = np.vectorize(mp.mpf, otypes=[object])


def _to_f(a):
    return np.array([[float(v) for v in row] for row in a]) if a.ndim == 2 else np.array([float(v) for v in a])


def step_exact(det_i, rig, fps, thresh, cam_width, prev, P_prev, camera="fisheye", lin=None):
    """The step with P_pred = F P F^T + Q, M = H^T R^-1 H, g, (I + M Pq)^-1, the state update and the P update at 40 digits;
    H, h and the gated residual are the fp64 oracle's (``linearise``).  Returns est, P_est rounded to fp64."""
    lin = linearise(det_i, rig, fps, thresh, cam_width, prev, P_prev, camera) if lin is None else lin
    with mp.workdps(DPS):
        F, Q = _to_mp(lin["F"]), _to_mp(lin["Q"])
        P = F @ _to_mp(np.asarray(P_prev, dtype=np.float64)) @ F.T + Q
        Hq, Rd, res = _to_mp(lin["H"][:, :N_POSE]), _to_mp(lin["Rd"]), _to_mp(lin["residual"])
        HR = Hq / Rd[:, None]
        M = Hq.T @ HR
        g = HR.T @ res
        B = M @ P[:N_POSE, :N_POSE]
        for k in range(N_POSE):
            B[k, k] += 1
        Binv = np.array((mp.matrix(B.tolist()) ** -1).tolist(), dtype=object)
        Pl = P[:, :N_POSE]
        x = _to_mp(lin["x_pred"]) + Pl @ (Binv @ g)
        Pn = P - Pl @ ((Binv @ M) @ P[:N_POSE, :])
        return _to_f(x), _to_f(Pn)


# ---- error measures ---------------------------------------------------------------------------------------------------------
def state_errors(got, want):
    """name -> |d block|max / max(1, |block|max) for the pose, velocity and acceleration blocks."""
    return {name: float(np.abs(got[b] - want[b]).max() / max(1.0, np.abs(want[b]).max())) for name, b in BLOCKS}


def cov_error(got, want):
    """max |dP_ij| / sqrt(P_ii P_jj), the scale taken from ``want``."""
    d = np.sqrt(np.diag(want))
    return float((np.abs(got - want) / np.outer(d, d)).max())


def cov_asymmetry(P):
    d = np.sqrt(np.diag(P))
    return float((np.abs(P - P.T) / np.outer(d, d)).max())


def gain_backward_error(A, P_est_i, sT):
    """max over the rows r of  |a_r P_pred - b_r|_2 / (|a_r|_2 |P_pred|_F + |b_r|_2),  P_pred = F P_est F^T + Q and
    b = P_est F^T in extended precision: how far ``A`` is from solving A P_pred = P_est F^T, row by row (P spans 1e-4 to 1e5,
    a matrix norm would hide the pose rows)."""
    _, Q, F = oekf.model_matrices(sT)
    ld = np.longdouble
    F, Q, Pe, A = F.astype(ld), Q.astype(ld), np.asarray(P_est_i).astype(ld), np.asarray(A).astype(ld)
    b = Pe @ F.T
    Pp = F @ b + Q
    nP = np.sqrt((Pp * Pp).sum())
    r = A @ Pp - b
    eta = np.sqrt((r * r).sum(1)) / (np.sqrt((A * A).sum(1)) * nP + np.sqrt((b * b).sum(1)))
    return float(eta.max())


def recursion_bound(est_i, x_pred_next, A_i, smoothed_next):
    """One smoother step  est_i + A_i (smoothed_next - x_pred_next)  in extended precision, and per entry the bound
    4 * 76 * 2^-53 * (|est_r| + sum_c |A_rc| |v_c|) on what a 76-term fp64 sum of products may lose in any order."""
    ld = np.longdouble
    v = np.asarray(smoothed_next).astype(ld) - np.asarray(x_pred_next).astype(ld)
    A = np.asarray(A_i).astype(ld)
    want = np.asarray(est_i).astype(ld) + A @ v
    bound = 4 * 76 * 2.0 ** -53 * (np.abs(np.asarray(est_i, dtype=np.float64)) + (np.abs(A) @ np.abs(v)).astype(np.float64))
    return want, bound


# ---- cases ------------------------------------------------------------------------------------------------------------------
def corrupt(det, k):
    """The detection recipe of the step tests on det[N, C, 20, 3]: 5 % of the detections shifted by +-150 px in x at high
    likelihood (what the gate is for), 20 % of the likelihoods at 0.2, frame 2 all 0.1 (a frame nobody sees well), the last
    camera all 0.3 (a blind camera)."""
    det = np.array(det, dtype=np.float64)
    n, c = det.shape[:2]
    rng = np.random.default_rng(1000 + k)
    out = rng.uniform(size=det.shape[:3]) < 0.05
    det[..., 0] += np.where(out, 150.0, 0.0) * rng.choice([-1, 1], size=out.shape)
    det[..., 2] = np.where(rng.uniform(size=det.shape[:3]) < 0.2, 0.2, 0.9)
    if n > 2:
        det[2, ..., 2] = 0.1
    if c > 1:
        det[:, -1, :, 2] = 0.3
    return det


def fisheye_case(n, cams, k, fps=120.0):
    """(det, rig, s0): the synthetic sprint of seed 20210313 + k on the cameras ``cams`` through ``corrupt``; s0 from the
    regression of the true nose track."""
    seq = osynth.make_sequence(n, "sprint", seed=20210313 + k)
    rig = tuple(seq[key][cams] for key in "KDRt")
    s0 = oekf.initial_state(np.arange(float(n)), seq["pos_true"][:, 2], 0, 1.0 / fps)
    return corrupt(seq["det"][:, cams], k), rig, s0


def generic_pose_case(n=3, seed=5):
    """A pose with all 22 joint angles drawn from +-0.6 rad, held still, seen by 6 cameras with 1 px noise; returns det, rig,
    the start at that pose and the nose-line start (every angle 0 but the heading).  The kernel probes which marker depends
    on which parameter at ONE pose of its own; a filter started on the nose line has every angle at 0."""
    seq = osynth.make_sequence(n, "sprint", seed=20210313 + seed)
    rig = tuple(seq[key] for key in "KDRt")
    line = oekf.initial_state(np.arange(float(n)), seq["pos_true"][:, 2], 0, 1.0 / 120)
    rng = np.random.default_rng(2000 + seed)
    s0 = np.zeros(NS)
    s0[:3] = seq["q_true"][0, :3]
    s0[3:N_POSE] = rng.uniform(-0.6, 0.6, N_POSE - 3)
    det = np.zeros((n, 6, 20, 3))
    for c in range(6):
        uv = oekf.h_function(s0[:N_POSE], *(a[c] for a in rig))
        det[:, c, :, :2] = uv[None] + rng.normal(0.0, 1.0, (n,) + uv.shape)
    det[..., 2] = 0.9
    return det, rig, s0, line
