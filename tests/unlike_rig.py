"""A rig of UNLIKE cameras, and the table of comparisons made on it.

``synth.make_rig`` tiles one K and one D over all cameras, so a kernel that reads camera c's intrinsics from another
camera's row computes the same numbers.  ``unlike_rig`` keeps that rig's geometry and gives every camera its own focal
lengths, principal point, distortion and (``skew=True``) skew.  ``rolled`` is the mutant: the same rig with K and D rolled
by one camera, R and t in place - what a wrong row index would read.

``CASES`` lists every comparison of tests/test_gpu_unlike_rig.py: the inputs (made on the CPU, by the oracle alone, so that
the host file sees the very same data), the reference as a function of the rig, and the tolerance of every compared
quantity.  tests/test_unlike_rig_host.py evaluates every reference on the rig and on its mutants and asserts that they lie
at least GUARD x the tolerance apart: a kernel that computed the mutant could not pass.  A GPU comparison is added by
adding a case here, which brings its guard with it.
"""
import functools
from typing import Callable, NamedTuple

import numpy as np

import fte_calib_ref as kref
import fte_cov_ref as cref
import fte_reproj_ref as rref
import pinhole_ekf_ref as pekf
import pinhole_fte_ref as pref
import sba_cov_ref as sref
from oracle import camera as ocam
from oracle import ekf as oekf
from oracle import fk as ofk
from oracle import fte as ofte
from oracle import index_path as oidx
from oracle import sba as osba
from oracle import synth as osynth

GUARD = 1000.0

FX_MUL = np.array([0.80, 0.88, 0.95, 1.05, 1.12, 1.20])
FY_MUL = np.array([1.18, 0.83, 1.07, 0.92, 1.13, 0.86])
CX_ADD = np.array([-70.0, 45.0, -20.0, 60.0, -55.0, 30.0])
CY_ADD = np.array([40.0, -35.0, 55.0, -15.0, 25.0, -50.0])
D_MUL = np.array([0.5, 0.7, 0.9, 1.1, 1.3, 1.5])
SKEW = np.array([2e-3, -3e-3, 5e-3, -1e-3, 4e-3, -5e-3])
# the 8 coefficients of test_pair_index_path_pinhole_seam (k1 k2 p1 p2 k3 k4 k5 k6); 12: pinhole_fte_ref.D12
PINHOLE_D8 = np.array([0.11, -0.05, 1e-3, -7e-4, 0.01, 0.02, -0.01, 2e-3])
# per camera and coefficient, inside [0.8, 1.2] (the range that test draws from), no two rows equal
PINHOLE_MUL = np.array([[0.80, 1.10, 0.95, 1.20, 0.90, 1.05, 0.85, 1.15, 1.00, 0.92, 1.08, 0.88],
                        [1.20, 0.85, 1.10, 0.90, 1.15, 0.80, 1.00, 0.95, 0.87, 1.12, 0.93, 1.05],
                        [0.92, 1.18, 0.83, 1.07, 0.97, 1.13, 1.20, 0.86, 1.10, 0.80, 1.15, 0.95],
                        [1.08, 0.94, 1.20, 0.82, 1.12, 0.88, 0.93, 1.03, 0.85, 1.18, 0.98, 1.14],
                        [0.86, 1.02, 0.90, 1.14, 0.80, 1.20, 1.09, 0.97, 1.16, 0.89, 0.84, 1.11],
                        [1.15, 0.81, 1.04, 0.96, 1.07, 0.93, 0.88, 1.19, 0.91, 1.06, 1.20, 0.83]])
MODELS = ("fisheye", "pinhole", "pinhole12")


def unlike_rig(n_cams=6, model="fisheye", skew=False, source=osynth):
    """(K, D, R, t) of ``source.make_rig(n_cams)`` with the intrinsics of camera c (tables at index c mod 6) made its own.
    ``model``: "fisheye" (4 coefficients), "pinhole" (8) or "pinhole12" (12, with the thin-prism terms)."""
    if model not in MODELS:
        raise ValueError(f"model must be one of {MODELS}")
    K, D4, R, t = source.make_rig(n_cams)
    K = np.array(K, dtype=np.float64)
    base = {"fisheye": np.asarray(D4[0], dtype=np.float64), "pinhole": PINHOLE_D8, "pinhole12": pref.D12}[model]
    D = np.zeros((n_cams, base.size))
    for c in range(n_cams):
        m, lap = c % 6, 1.0 + 0.01 * (c // 6)
        K[c, 0, 0] *= FX_MUL[m] * lap
        K[c, 1, 1] *= FY_MUL[m] * lap
        K[c, 0, 2] += CX_ADD[m]
        K[c, 1, 2] += CY_ADD[m]
        if model == "fisheye":
            D[c] = base * D_MUL[m] * np.array([1.0, 1.0 + 0.1 * m, 1.0 - 0.1 * m, 1.0 + 0.05 * m])
        else:
            D[c] = base * PINHOLE_MUL[m, :base.size]
        if skew:
            K[c, 0, 1] = SKEW[m] * K[c, 0, 0]
    return K, D, np.array(R, dtype=np.float64), np.array(t, dtype=np.float64)


def rolled(rig):
    """The mutant: camera c carries the K and D of camera c - 1; R and t stay."""
    K, D, R, t = rig
    return np.roll(K, 1, axis=0), np.roll(D, 1, axis=0), R, t


def without_skew(rig):
    K, D, R, t = rig
    K = K.copy()
    K[:, 0, 1] = 0.0
    return K, D, R, t


def subset(rig, cams):
    return tuple(np.asarray(a)[cams] for a in rig)


MUTANTS = {"rolled": rolled, "no_skew": without_skew}


# ------------------------------------------------------------------------------------------------------------- measures
def error(got, want, kind):
    """The one measure of the GPU comparisons and of the guards: "abs" max |got - want| over the finite entries of want,
    "rel" the same over max |want|, "blocks" / "columns" / "scaled" the measures of the
    posterior references, "ekf" over max(1, max |want|) (test_hip_ekf_matches_oracle's measure)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    live = np.isfinite(want)
    d = float(np.abs(got[live] - want[live]).max())
    if kind == "rel":
        return d / float(np.abs(want[live]).max())
    if kind == "blocks":                                   # fte_cov_ref.rel_err: per leading index, Frobenius
        return cref.rel_err(got, want)
    if kind == "columns":                                  # fte_calib_ref.col_err
        return kref.col_err(got, want)
    if kind == "scaled":                                   # sba_cov_ref.scaled_error
        return sref.scaled_error(got, want)
    return d / max(1.0, float(np.abs(want[live]).max())) if kind == "ekf" else d


class Case(NamedTuple):
    group: str
    inputs: Callable          # () -> dict with "rig" and the data, cached: shared by the tests, never modified
    reference: Callable       # (inputs, rig) -> {key: array}
    tol: dict                 # key -> (kind, tolerance): the comparison the GPU test makes
    mutants: dict             # mutant -> the keys its guard holds on (all of tol unless the case says otherwise)


CASES = {}


def case(name, group, tol, mutants=("rolled",)):
    """Registers a case; ``mutants``: names, or (name, keys) where the guard can hold on some of the compared keys only."""
    def deco(pair):
        inputs, reference = pair()
        held = {m if isinstance(m, str) else m[0]: tuple(tol) if isinstance(m, str) else tuple(m[1]) for m in mutants}
        CASES[name] = Case(group, functools.lru_cache(maxsize=None)(inputs), reference, tol, held)
        return pair
    return deco


def inputs_of(name):
    return CASES[name].inputs()


@functools.lru_cache(maxsize=None)
def reference_of(name, mutant=None):
    """The reference of a case on its rig (or on a mutant of it): computed once, shared, never modified."""
    inp = inputs_of(name)
    rig = inp["rig"] if mutant is None else MUTANTS[mutant](inp["rig"])
    return CASES[name].reference(inp, rig)


def names(group):
    return [n for n, c in CASES.items() if c.group == group]


def compare(name, got):
    """The GPU side of a case: every key of the tolerance table within its tolerance (printed first); returns {key: error}."""
    want, errs = reference_of(name), {}
    for key, (kind, tol) in CASES[name].tol.items():
        assert np.array_equal(np.isfinite(got[key]), np.isfinite(want[key])), (name, key)
        errs[key] = error(got[key], want[key], kind)
    print(f"unlike rig [{name}]: " + "  ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for key, (kind, tol) in CASES[name].tol.items():
        assert errs[key] < tol, (name, key, errs[key], tol)
    return errs


# ------------------------------------------------------------------------------------------------------------- data
def cloud(n=500, seed=1):
    return osynth.LOOK_AT + np.random.default_rng(seed).normal(0.0, 2.0, (n, 3))


def cam_xyz(X, rig, c):
    return X @ rig[2][c].T + rig[3][c].reshape(1, 3)


def r2_of(X, rig, c):
    Y = cam_xyz(X, rig, c)
    return (Y[:, 0] / Y[:, 2]) ** 2 + (Y[:, 1] / Y[:, 2]) ** 2


def pinhole_sequence(n_frames, rig, kind="sprint", seed=20210313, noise_px=2.0, outlier_frac=0.15):
    """oracle.synth.make_sequence on a pinhole rig (oracle FK, oracle.camera.project_points, the same noise model)."""
    K, D, R, t = rig
    q = osynth.trajectory(n_frames, kind)
    pos = ofk.cheetah_fk(q)
    rng = np.random.default_rng(seed)
    N, L, _ = pos.shape
    det = np.zeros((N, len(K), L, 3))
    for c in range(len(K)):
        uv = ocam.project_points(pos.reshape(-1, 3), K[c], D[c], R[c], t[c]).reshape(N, L, 2)
        zc = pos @ R[c][2] + t[c].reshape(3)[2]
        uv = uv + rng.normal(0.0, noise_px, uv.shape)
        lik = rng.uniform(0.55, 1.0, (N, L))
        out = rng.uniform(size=(N, L)) < outlier_frac
        lik = np.where(out, rng.uniform(0.0, 0.4, (N, L)), lik)
        uv = np.where(out[..., None], uv + rng.uniform(-100, 100, uv.shape), uv)
        bad = (zc < 0.5) | (uv[..., 0] < 0) | (uv[..., 0] >= osynth.IMG_W) | (uv[..., 1] < 0) | (uv[..., 1] >= osynth.IMG_H)
        det[:, c, :, :2] = uv
        det[:, c, :, 2] = np.where(bad, 0.05, lik)
    return dict(K=K, D=D, R=R, t=t, q_true=q, pos_true=pos, det=det, Ts=1.0 / osynth.FPS)


def sequence(n_frames, rig, model="fisheye", kind="sprint", seed=20210313):
    if model == "fisheye":
        return osynth.make_sequence(n_frames, kind, seed=seed, rig=rig)
    return pinhole_sequence(n_frames, rig, kind, seed=seed)


def clean_pixels(pos, rig, model="fisheye"):
    """Noise-free pixels [C, N, L, 2] of the marker positions in every camera."""
    fun = ocam.project_points_fisheye if model == "fisheye" else ocam.project_points
    return np.stack([fun(pos.reshape(-1, 3), rig[0][c], rig[1][c], rig[2][c], rig[3][c]).reshape(pos.shape[:-1] + (2,))
                     for c in range(len(rig[0]))])


# ------------------------------------------------------------------------------------------------ (a) point-wise, fisheye
PAIRS = ((0, 1), (2, 5), (4, 3))


@case("a_project_fisheye_skew", "a", {"uv": ("abs", 1e-9)}, ("rolled", "no_skew"))
def _a_project():
    def inputs():
        return dict(rig=unlike_rig(6, "fisheye", skew=True), X=cloud())

    def reference(inp, rig):
        return dict(uv=np.stack([ocam.project_points_fisheye(inp["X"], *subset(rig, c)) for c in range(6)]))
    return inputs, reference


@case("a_undistort_fisheye_skew", "a", {"xy": ("abs", 1e-13)}, ("rolled", "no_skew"))
def _a_undistort():
    def inputs():
        rig, X, rng = unlike_rig(6, "fisheye", skew=True), cloud(), np.random.default_rng(11)
        px = np.stack([ocam.project_points_fisheye(X, *subset(rig, c)) for c in range(6)])
        return dict(rig=rig, X=X, px=px + rng.normal(0.0, 1.0, px.shape))

    def reference(inp, rig):
        return dict(xy=np.stack([ocam.undistort_points_fisheye(inp["px"][c], rig[0][c], rig[1][c]) for c in range(6)]))
    return inputs, reference


def in_front(X, rig, cams, z_min=0.5):
    """The points at least z_min in front of every camera of ``cams`` (test_pointwise_camera_kernels' ``front``)."""
    return np.all([cam_xyz(X, rig, c)[:, 2] > z_min for c in cams], axis=0)


@case("a_triangulate_fisheye_skew", "a", {f"{k}{a}{b}": ("abs", 1e-10) for k in ("noisy", "exact") for a, b in PAIRS},
      ("rolled", "no_skew"))
def _a_triangulate():
    def inputs():
        rig, cl, rng = unlike_rig(6, "fisheye", skew=True), cloud(), np.random.default_rng(12)
        X, px = {}, {}
        for a, b in PAIRS:                                  # the points in front of both cameras of the pair
            X[a, b] = cl[in_front(cl, rig, (a, b))]
            exact = [ocam.project_points_fisheye(X[a, b], *subset(rig, c)) for c in (a, b)]
            px["exact", a, b] = exact
            px["noisy", a, b] = [e + rng.normal(0.0, 1.0, e.shape) for e in exact]
        return dict(rig=rig, X=X, px=px)

    def reference(inp, rig):
        return {f"{k}{a}{b}": ocam.triangulate_points_fisheye(*inp["px"][k, a, b], *subset(rig, a), *subset(rig, b))
                for k in ("noisy", "exact") for a, b in PAIRS}
    return inputs, reference


# ------------------------------------------------------------------------------------------------ (b) point-wise, pinhole
def _b_project(model):
    def inputs():
        # per camera the points in front of it with r^2 < 2.5: the whole image and beyond it, pixels below 4e3.  A point of
        # the cloud close to a camera's plane projects to 1e5 .. 4e9 px through the rational model, where 1e-8 px is less
        # than one unit in the last place of the pixel and measures nothing.
        rig, cl = unlike_rig(6, model), cloud()
        return dict(rig=rig, X=[cl[in_front(cl, rig, (c,)) & (r2_of(cl, rig, c) < 2.5)] for c in range(6)])

    def reference(inp, rig):
        return {f"uv{c}": ocam.project_points(inp["X"][c], *subset(rig, c)) for c in range(6)}
    return inputs, reference


B_TOL = {f"uv{c}": ("abs", 1e-8) for c in range(6)}
case("b_project_pinhole8", "b", B_TOL)(lambda: _b_project("pinhole"))
case("b_project_pinhole12", "b", B_TOL)(lambda: _b_project("pinhole12"))


R2_MAX = 0.1


def narrow_cloud(rig, pair, X=None, r2_max=R2_MAX):
    """The points of the cloud in front of both cameras of the pair and with r^2 < r2_max in both: where OpenCV's five-step
    fixed-point undistortion has converged.  test_pointwise_camera_kernels keeps r^2 < 0.3 on its one distortion vector; on
    these six the round trip undistort(project(X)) is off by up to 1.5e-8 there and by 2e-11 inside r^2 < 0.1, which
    tests/test_unlike_rig_host.py holds to 1e-9."""
    X = cloud() if X is None else X
    a, b = pair
    return X[in_front(X, rig, pair) & (r2_of(X, rig, a) < r2_max) & (r2_of(X, rig, b) < r2_max)]


@case("b_triangulate_pinhole8", "b", {f"pair{a}{b}": ("abs", 1e-9) for a, b in PAIRS})
def _b_triangulate():
    def inputs():
        rig = unlike_rig(6, "pinhole")
        X = {p: narrow_cloud(rig, p) for p in PAIRS}
        px = {p: tuple(ocam.project_points(X[p], *subset(rig, c)) for c in p) for p in PAIRS}
        return dict(rig=rig, X=X, px=px)

    def reference(inp, rig):
        return {f"pair{a}{b}": ocam.triangulate_points(*inp["px"][(a, b)], *subset(rig, a), *subset(rig, b)) for a, b in PAIRS}
    return inputs, reference


# ------------------------------------------------------------------------------------------------ (c) dense pair kernels
CAM_SUBSET = [5, 2, 0]                                    # record order differs from camera order
PINHOLE_PAIR_FRAMES = 16


def edit_detections(det):
    """The frame, marker and NaN edits of test_pair_index_path_bit_exact."""
    det = det.copy()
    det[5, :, :, 2] = 0.0                      # a frame nobody sees
    det[7, 1:, 3, 2] = 0.0                     # a marker seen by one camera only
    det[9, 2, 4, :2] = np.nan                  # NaN coordinates with low likelihood stay harmless
    det[9, 2, 4, 2] = 0.1
    return det


def oracle_residuals(tri, det, thresh, rig):
    """acino_reproject_residuals in numpy: project(tri) - det.xy where the detection is valid and the point finite, else NaN."""
    N, C, L, _ = det.shape
    res = np.full((N, C, L, 2), np.nan)
    ok3 = np.isfinite(tri).all(-1)
    for c in range(C):
        ok = ok3 & (det[:, c, :, 2] > thresh)
        uv = ocam.project_points_fisheye(tri[ok], *subset(rig, c))
        res[:, c][ok] = uv - det[:, c][ok][:, :2]
    return res


@case("c_pairs_fisheye_skew", "c", {"tri": ("abs", 1e-10), "tri_sub": ("abs", 1e-10), "res": ("abs", 1e-9)},
      ("rolled", "no_skew"))
def _c_fisheye():
    def inputs():
        rig = unlike_rig(6, "fisheye", skew=True)
        det = edit_detections(osynth.make_sequence(20, "sprint", rig=rig)["det"])
        tri = oidx.pairwise_dense(det, 0.5, *rig, ocam.triangulate_points_fisheye)[0]
        return dict(rig=rig, det=det, det_sub=np.ascontiguousarray(det[:, CAM_SUBSET]), tri_in=tri)

    def reference(inp, rig):
        tri, cnt, mask = oidx.pairwise_dense(inp["det"], 0.5, *rig, ocam.triangulate_points_fisheye)
        ts, cs, ms = oidx.pairwise_dense(inp["det_sub"], 0.5, *subset(rig, CAM_SUBSET), ocam.triangulate_points_fisheye)
        # the residuals of FIXED points (the oracle's triangulation on the true rig) through the rig under test: 1e-9 px is the
        # tolerance of the projection (group a)
        return dict(tri=tri, cnt=cnt, mask=mask, tri_sub=ts, cnt_sub=cs, mask_sub=ms,
                    res=oracle_residuals(inp["tri_in"], inp["det"], 0.5, rig))
    return inputs, reference


@case("c_pairs_pinhole", "c", {"tri": ("abs", 1e-9), "tri_sub": ("abs", 1e-9)})
def _c_pinhole():
    def inputs():
        rig, rng = unlike_rig(6, "pinhole"), np.random.default_rng(5)
        # 16 frames: the round trip undistort(project(.)) of the markers stays below 1e-9 (7e-10; 1.6e-9 at 20 frames)
        pos = ofk.cheetah_fk(osynth.trajectory(PINHOLE_PAIR_FRAMES, "sprint"))
        N, L = pos.shape[:2]
        det = np.zeros((N, 6, L, 3))
        det[..., :2] = clean_pixels(pos, rig, "pinhole").transpose(1, 0, 2, 3) + rng.normal(0, 1.0, (N, 6, L, 2))
        det[..., 2] = np.where(rng.uniform(size=(N, 6, L)) < 0.35, 0.2, 0.9)      # (as test_pair_index_path_pinhole_seam)
        det = edit_detections(det)
        return dict(rig=rig, det=det, det_sub=np.ascontiguousarray(det[:, CAM_SUBSET]))

    def reference(inp, rig):
        tri, cnt, mask = oidx.pairwise_dense(inp["det"], 0.5, *rig, ocam.triangulate_points)
        ts, cs, ms = oidx.pairwise_dense(inp["det_sub"], 0.5, *subset(rig, CAM_SUBSET), ocam.triangulate_points)
        return dict(tri=tri, cnt=cnt, mask=mask, tri_sub=ts, cnt_sub=cs, mask_sub=ms)
    return inputs, reference


# ------------------------------------------------------------------------------------------------ (d) FTE assembly
FTE_TOL = {"cost": ("rel", 1e-12), "cost_b": ("rel", 1e-12), "grad": ("rel", 1e-11), "hess": ("rel", 1e-11)}


def fte_problem(seq, model, rig=None):
    rig = (seq["K"], seq["D"], seq["R"], seq["t"]) if rig is None else rig
    cls = ofte.FTEProblem if model == "fisheye" else pref.PinholeFTEProblem
    return cls(seq["det"][..., :2], seq["det"][..., 2], *rig, seq["Ts"])


def _d_assembly(model, skew=False):
    def inputs():
        rig = unlike_rig(6, model, skew=skew)
        seq = sequence(60, rig, model)
        prob, rng = fte_problem(seq, model), np.random.default_rng(2)
        xa = np.clip(seq["q_true"][:, ofk.ACTIVE] + rng.normal(0, 0.02, (60, 25)), prob.lo, prob.hi)
        xb = np.clip(xa + rng.normal(0, 0.01, xa.shape), prob.lo, prob.hi)
        return dict(rig=rig, seq=seq, xa=xa, xb=xb, model="fisheye" if model == "fisheye" else "pinhole")

    def reference(inp, rig):
        prob = fte_problem(inp["seq"], inp["model"], rig)
        F, g, H, nb = prob.evaluate(inp["xa"])
        idx = np.arange(25)
        H[:, idx, idx] += 2 * prob.q_w[None, :] * prob.s_band()[0][:, None]
        return dict(cost=F, cost_b=prob.evaluate(inp["xb"], need_jac=False)[0], grad=g, hess=H, n_behind=nb)
    return inputs, reference


case("d_fte_fisheye", "d", FTE_TOL)(lambda: _d_assembly("fisheye"))
case("d_fte_fisheye_skew", "d", FTE_TOL)(lambda: _d_assembly("fisheye", skew=True))       # (both sides ignore the skew)
case("d_fte_pinhole8", "d", FTE_TOL)(lambda: _d_assembly("pinhole"))
case("d_fte_pinhole12", "d", FTE_TOL)(lambda: _d_assembly("pinhole12"))


# ------------------------------------------------------------------------------------------------ (g) EKF
EKF_TOL = (("x", 5e-6), ("dx", 5e-5), ("ddx", 1e-3), ("smoothed_x", 5e-6), ("smoothed_dx", 5e-5), ("smoothed_ddx", 1e-3))
EKF_KEYS = tuple(k for k, _ in EKF_TOL)


def _g_ekf(model, skew):
    def inputs():
        rig = unlike_rig(6, model, skew=skew)
        seq = sequence(24, rig, model, seed=20210314)
        s0 = oekf.initial_state(np.arange(24.0), seq["pos_true"][:, 2], 0, 1.0 / 120.0)
        return dict(rig=rig, det=seq["det"], s0=s0, model=model)

    def reference(inp, rig):
        run = oekf.ekf if inp["model"] == "fisheye" else pekf.ekf
        out = run(inp["det"], *rig, 120.0, 0.5, 2704, inp["s0"])
        return {k: out[k] for k in EKF_KEYS + ("outliers_ignored",)}
    return inputs, reference


# The skew moves every pixel of a camera by a nearly constant 2 to 18 px over these 24 frames: it moves the filtered POSITION
# (1 500 x the tolerance of x) and hardly its derivatives (300 x that of dx, 20 x that of ddx), so the guard against a dropped
# skew holds on x and smoothed_x, which the GPU test asserts with the others; the rolled rig is guarded on every key.
case("g_ekf_fisheye_skew", "g", {k: ("ekf", tol) for k, tol in EKF_TOL},
     ("rolled", ("no_skew", ("x", "smoothed_x"))))(lambda: _g_ekf("fisheye", True))
case("g_ekf_pinhole8", "g", {k: ("ekf", tol) for k, tol in EKF_TOL})(lambda: _g_ekf("pinhole", False))


# ------------------------------------------------------------------------------------------------ (h) bundle adjustment
def moved(rig):
    """From the seventh camera on: the reused cameras, moved (so that no two cameras share a pose)."""
    K, D, R, t = rig
    C = len(K)
    R, t = np.array(R, dtype=np.float64), np.array(t, dtype=np.float64).reshape(C, 3, 1)
    for c in range(6, C):
        R[c] = ocam.rodrigues(np.array([0.02, -0.05, 0.03])) @ R[c]
        t[c] = t[c] + np.array([[0.3], [-0.2], [0.1]])
    return K, D, R, t


def lm_step_problem(rig, seed, model="fisheye", n_pts=37):
    """The problem of test_first_lm_step_with_ragged_visibility_for_every_camera_count on ``rig`` (C cameras, those from the
    seventh on are moved): points that some cameras do not see, 1 px noise, five 15 px outliers, an iterate off the truth."""
    rng = np.random.default_rng(seed)
    K, D, R, t = moved(rig)
    C, P = len(K), n_pts
    ofun = ocam.project_points_fisheye if model == "fisheye" else ocam.project_points
    X = np.array([2.0, 6.5, 0.7]) + rng.normal(0, 0.6, (P, 3))
    pi, ci = [], []
    for p in range(P):
        cams = np.sort(rng.choice(C, size=rng.integers(2, C + 1), replace=False))
        pi += [p] * len(cams)
        ci += list(cams)
    pi, ci = np.array(pi), np.array(ci)
    uv = np.stack([ofun(X[p:p + 1], K[c], D[c], R[c], t[c])[0] for p, c in zip(pi, ci)]) + rng.normal(0, 1.0, (len(pi), 2))
    uv[rng.choice(len(uv), 5, replace=False)] += rng.uniform(-15, 15, (5, 2))
    X0 = X + rng.normal(0, 0.03, X.shape)
    R0 = np.array([ocam.rodrigues(rng.normal(0, 0.01, 3)) @ R[c] for c in range(C)])
    t0 = t + rng.normal(0, 0.01, t.shape)
    return dict(C=C, P=P, K=K, D=D, R0=R0, t0=t0, X0=X0, pi=pi, ci=ci, uv=uv, model=model)


def lm_step_reference(prob, K=None, D=None, fs=1.0, lam=1e-3, cameras=True):
    """ONE Levenberg-Marquardt step formed densely in numpy from central differences of the oracle's residual function (Cauchy
    IRLS weights, (1 + lam) diagonal damping): the costs before and after and the updated parameters.  ``K``, ``D``: the
    intrinsics to compute with (default: the problem's own).  ``cameras=False``: the 3 x 3 point blocks alone."""
    C, P, pi, ci, uv, X0, R0, t0 = (prob[k] for k in ("C", "P", "pi", "ci", "uv", "X0", "R0", "t0"))
    K, D = prob["K"] if K is None else K, prob["D"] if D is None else D
    ofun = ocam.project_points_fisheye if prob["model"] == "fisheye" else ocam.project_points

    def resid(Xp, Rm, tv):
        return osba.residuals(Xp, Rm, tv, K, D, pi, ci, uv, project_func=ofun)

    def apply(dc, dp):
        Rn = np.array([ocam.rodrigues(dc[6 * c:6 * c + 3]) @ R0[c] for c in range(C)])
        return X0 + dp.reshape(P, 3), Rn, t0 + dc.reshape(C, 6)[:, 3:].reshape(C, 3, 1)

    def cost(r):
        return 0.5 * fs * fs * np.log1p((r / fs) ** 2).sum()

    r0 = resid(X0, R0, t0)
    n = 6 * C + 3 * P
    J, h = np.zeros((r0.size, n)), 1e-6
    for k in range(0 if cameras else 6 * C, n):
        e = np.zeros(n)
        e[k] = h
        J[:, k] = (resid(*apply(e[:6 * C], e[6 * C:])) - resid(*apply(-e[:6 * C], -e[6 * C:]))) / (2 * h)
    w = 1.0 / (1.0 + (r0 / fs) ** 2)
    if not cameras:
        J = J[:, 6 * C:]
    A = J.T @ (w[:, None] * J)
    delta = -np.linalg.solve(A + lam * np.diag(np.diag(A)), J.T @ (w * r0))
    if not cameras:
        delta = np.concatenate([np.zeros(6 * C), delta])
    Xn, Rn, tn = apply(delta[:6 * C], delta[6 * C:])
    return dict(c0=cost(r0), c1=cost(resid(Xn, Rn, tn)), X=Xn, R=Rn, t=tn)


def lm_step_check(sba, proj, prob, want):
    """One iteration of the HIP solver on ``prob`` against ``want`` (lm_step_reference): the assertions of
    test_first_lm_step_with_ragged_visibility_for_every_camera_count.  Returns the errors."""
    c0, c1 = want["c0"], want["c1"]
    pts, rm, tt, _res = sba.bundle_adjust_points_and_extrinsics(prob["uv"], prob["X0"], prob["pi"], prob["ci"], prob["K"], prob["D"],
                                                                prob["R0"], prob["t0"], proj, max_iter=1)
    info = dict(sba.last_info)
    assert info["iterations"] == 1 and info["accepted"] == (1 if c1 < c0 else 0)
    assert abs(info["cost_initial"] - c0) < 1e-9 * c0
    errs = dict(cost_initial=abs(info["cost_initial"] - c0) / c0)
    if c1 < c0:
        errs.update(cost_final=abs(info["cost_final"] - c1) / c1, X=np.abs(pts - want["X"]).max(), R=np.abs(rm - want["R"]).max(),
                    t=np.abs(tt - want["t"]).max())
        assert abs(info["cost_final"] - c1) < 1e-6 * c1, (info, c0, c1)
        assert np.abs(pts - want["X"]).max() < 1e-6 and np.abs(rm - want["R"]).max() < 1e-6 and np.abs(tt - want["t"]).max() < 1e-6
    return errs


SBA_TOL = {"c0": ("rel", 1e-9), "c1": ("rel", 1e-6), "X": ("abs", 1e-6), "R": ("abs", 1e-6), "t": ("abs", 1e-6)}
SBA_STEP = [(C, model) for model in ("fisheye", "pinhole") for C in (2, 5, 7, 8, 9)]


def _h_step(C, model, cameras=True, fs=1.0):
    def inputs():
        rig = unlike_rig(C, model)
        return dict(rig=rig, prob=lm_step_problem(rig, 100 + C, model))

    def reference(inp, rig):
        return lm_step_reference(inp["prob"], rig[0], rig[1], fs=fs, cameras=cameras)
    return inputs, reference


for _C, _model in SBA_STEP:
    case(f"h_step_{_model}_{_C}", "h_step", SBA_TOL)(functools.partial(_h_step, _C, _model))
case("h_points_only_fisheye_3", "h_points", {"c0": ("rel", 1e-9), "c1": ("rel", 1e-6), "X": ("abs", 1e-6)})(
    functools.partial(_h_step, 3, "fisheye", False, 50.0))


# ------------------------------------------------------------------------------------------------ (e) FTE solve
def nose_line(det, rig, model):
    """The reference's initial guess from the oracle's own adjacent-pair triangulation of the nose (marker 2)."""
    tfun = ocam.triangulate_points_fisheye if model == "fisheye" else ocam.triangulate_points
    nose = oidx.pairwise_dense(det[:, :, 2:3], 0.5, *rig, tfun)[0][:, 0]
    ok = np.isfinite(nose).all(-1)
    return ofte.nose_line_init(np.nonzero(ok)[0], nose[ok], det.shape[0])


def _e_solve(model, max_iter, ftol):
    def inputs():
        rig = unlike_rig(6, model)
        seq = sequence(60, rig, model)
        return dict(rig=rig, seq=seq, x0=nose_line(seq["det"], rig, model), model=model, max_iter=max_iter, ftol=ftol)

    def reference(inp, rig):
        prob, hist = fte_problem(inp["seq"], inp["model"], rig), []
        xo, info = ofte.lm_solve(prob, inp["x0"][:, ofk.ACTIVE], max_iter=max_iter, ftol=ftol, history=hist)
        return dict(positions=ofte.fte_outputs(prob, xo, inp["x0"])["positions"], cost=info["cost"], first_trial=hist[0]["Ft"],
                    info=info, history=hist)
    return inputs, reference


# (test_fte_solve_matches_oracle_trajectory: cost 1e-11, end point 1e-8 m; test_pinhole_lm_path_identity: trial costs 1e-9)
E_TOL = {"positions": ("abs", 1e-8), "cost": ("rel", 1e-11)}
case("e_solve_fisheye", "e", E_TOL)(lambda: _e_solve("fisheye", 80, 1e-13))
case("e_path_pinhole8", "e", dict(E_TOL, first_trial=("rel", 1e-9)))(lambda: _e_solve("pinhole", 100, 1e-10))


# ------------------------------------------------------------------------------------------------ (f) FTE posterior entries
BAR_MAX = 64.0 * 1e-8          # fte_cov_ref.bar(d0) = max(64 d0, 1e-13) refuses d0 > 1e-8: no bar can be larger than this


def _f_state(inp, rig):
    """The linear system of the oracle at the case's iterate on ``rig``: (fixed, banded matrix)."""
    prob = fte_problem(inp["seq"], "fisheye", rig)
    _F, g, H, _nb = prob.evaluate(inp["x"])
    band = cref.clip_band(len(inp["x"]))
    Hd = cref.with_smooth_diag(H, prob.q_w, band)
    fixed = cref.active_set(inp["x"], g, Hd, prob.lo, prob.hi)
    return fixed, cref.banded(Hd, fixed, prob.q_w, band)


def _f_inputs():
    rig = unlike_rig(6, "fisheye")
    seq = sequence(30, rig)
    prob = fte_problem(seq, "fisheye")
    x = np.clip(seq["q_true"][:, ofk.ACTIVE] + np.random.default_rng(2).normal(0, 0.02, (30, 25)), prob.lo, prob.hi)
    inp = dict(rig=rig, seq=seq, x=x)
    fixed, ab = _f_state(inp, rig)
    inp.update(fixed=fixed, ab=ab, cov_pos=cref.marker_cov(cref.dense_blocks(ab, fixed), cref.fk_jacobian_exact(x))[0])
    return inp


_f_shared = functools.lru_cache(maxsize=None)(_f_inputs)


@case("f_covariance", "f", {"cov_x": ("blocks", BAR_MAX)})
def _f_cov():
    def reference(inp, rig):
        fixed, ab = _f_state(inp, rig)
        return dict(cov_x=cref.dense_blocks(ab, fixed))
    return _f_shared, reference


@case("f_reprojection", "f", {"uv": ("abs", 1e-9), "cov_uv": ("blocks", 1e-11)})
def _f_reproj():
    def reference(inp, rig):
        out = rref.reprojection(inp["x"], inp["cov_pos"], inp["seq"]["det"], rig, "fisheye")
        return dict(uv=out["uv"], cov_uv=out["cov_uv"].reshape(-1, 4))
    return _f_shared, reference


@case("f_calibration_sensitivity", "f", {"sens": ("columns", BAR_MAX)})
def _f_calib():
    def reference(inp, rig):                               # (the matrix of the true rig, the cross term of the rig under test)
        G = kref.cross_term(inp["x"], inp["seq"]["det"], rig, inp["seq"]["Ts"], "fisheye")
        return dict(sens=kref.sens_banded(inp["ab"], inp["fixed"], G))
    return _f_shared, reference


# ------------------------------------------------------------------------------------------------ (h) covariance, dense entry
SBA_COV_TOL = 1.1e-7           # tests/test_gpu_sba_cov.py's TOL (asserted equal there)
SBA_COV = [(3, "fisheye"), (8, "fisheye"), (4, "pinhole")]


def _h_cov(C, model):
    def inputs():
        rig = unlike_rig(C, model)
        return dict(rig=rig, prob=sref.make_problem(C, 37, 200 + C, model, rig=rig))

    def reference(inp, rig):
        prob = dict(inp["prob"], K=rig[0], D=rig[1])
        out = sref.reference(prob, J=sref.jacobian(prob))
        return dict(out, sigma2=np.array(out["sigma2"]))
    return inputs, reference


for _C, _model in SBA_COV:
    case(f"h_cov_{_model}_{_C}", "h_cov", {"cov_cams": ("scaled", SBA_COV_TOL), "cov_points": ("scaled", SBA_COV_TOL),
                                           "sigma2": ("rel", SBA_COV_TOL)})(functools.partial(_h_cov, _C, _model))


def perturbed(R, t, rng, deg=0.5, cm=1.0):
    """test_gpu_sba.py's _perturb: every camera off by ``deg`` degrees and ``cm`` centimetres (rms)."""
    Rp = np.array([ocam.rodrigues(rng.normal(0, 1, 3) / np.sqrt(3) * np.radians(deg)) @ R[c] for c in range(len(R))])
    tp = np.asarray(t, dtype=np.float64).reshape(-1, 3, 1) + rng.normal(0, 1, (len(R), 3, 1)) / np.sqrt(3) * cm * 1e-2
    return Rp, tp


def dense_lists(det, thresh=0.5):
    """The observation lists the reference's loops build (points with > 1 view, calib.py:281): keep[N, L], pi, ci, p2."""
    seen = det[..., 2].transpose(0, 2, 1) > thresh
    keep = seen.sum(-1) >= 2
    pi, ci, p2 = [], [], []
    for pid, (n, l) in enumerate(zip(*np.nonzero(keep))):
        for c in np.nonzero(seen[n, l])[0]:
            pi.append(pid); ci.append(c); p2.append(det[n, c, l, :2])
    return keep, np.array(pi), np.array(ci), np.array(p2)


DENSE_FRAMES = 20


@case("h_dense_fisheye", "h_dense", {"cost_initial": ("rel", 1e-9)})
def _h_dense():
    def inputs():
        rig, rng = unlike_rig(6, "fisheye"), np.random.default_rng(3)
        seq = osynth.make_sequence(DENSE_FRAMES, "sprint", rig=rig)
        X0 = seq["pos_true"] + rng.normal(0, 0.01, seq["pos_true"].shape)
        Rp, tp = perturbed(rig[2], rig[3], rng)
        keep, pi, ci, p2 = dense_lists(seq["det"])
        return dict(rig=rig, det=seq["det"], X0=X0, Rp=Rp, tp=tp, keep=keep, pi=pi, ci=ci, p2=p2)

    def reference(inp, rig):
        r0 = osba.residuals(inp["X0"][inp["keep"]], inp["Rp"], inp["tp"], rig[0], rig[1], inp["pi"], inp["ci"], inp["p2"])
        return dict(cost_initial=np.array(osba.cauchy_cost(r0)))
    return inputs, reference


@functools.lru_cache(maxsize=None)
def dense_scipy():
    """The scipy oracle (calib.py:369-390 settings, consistent Jacobian mask, 60 evaluations) from the start of h_dense_fisheye."""
    inp = inputs_of("h_dense_fisheye")
    K, D = inp["rig"][:2]
    return osba.bundle_adjust_points_and_extrinsics(inp["p2"], inp["X0"][inp["keep"]], inp["pi"], inp["ci"], K, D, inp["Rp"],
                                                    inp["tp"], max_nfev=60, consistent_mask=True)[4]
