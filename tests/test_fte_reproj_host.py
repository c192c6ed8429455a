"""The FTE solve in image space, the part that needs no GPU: the C ABI of acino_fte_reprojection (header, export, signature,
argument validation before any device call), the Python interface (FTEContext.reprojection, return_reprojection,
fte.detection_report, io.reprojection_to_points_2d_df) and the CPU reference tests/fte_reproj_ref.py pinned to itself."""
import ctypes as C
import inspect
import os
import re
import types

import numpy as np
import pytest

import fte_cov_ref as cref
import fte_reproj_ref as rref
import pinhole_fte_ref as pref
from oracle import fk as ofk
from oracle import fte as ofte
from oracle import synth as osynth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "acino_fte_reprojection"


def test_header_export_signature_and_argument_checks():
    """Fails without the feature: the function is declared, exported and bound; the ABI version stays 3; a null context,
    all-null outputs and d_cov_uv without d_cov_pos are refused with ACINO_ERR_INVALID_ARG (-1) and a telling message
    before anything touches a device."""
    from acinoset_amd import _lib
    with open(os.path.join(ROOT, "include", "acinoset_hip.h")) as f:
        header = f.read()
    assert re.search(r"\b" + NAME + r"\s*\(", header), f"{NAME} not declared in acinoset_hip.h"
    assert NAME in _lib.SIGNATURES and len(_lib.SIGNATURES[NAME][1]) == 9
    import __graft_entry__ as entry
    entry.build()
    h = _lib.lib()
    assert hasattr(h, NAME)
    assert h.acino_abi_version() == 3
    fake = C.c_void_p(256)                                   # never dereferenced: the argument checks come first
    assert h.acino_fte_reprojection(None, None, fake, None, None, None, None, None, None) == -1
    msg = h.acino_last_error_string().decode()
    assert "invalid argument" in msg and "context" in msg
    assert h.acino_fte_reprojection(fake, fake, None, None, None, None, None, None, None) == -1
    assert "no output" in h.acino_last_error_string().decode()
    assert h.acino_fte_reprojection(fake, None, fake, fake, None, None, None, None, None) == -1
    assert "d_cov_pos" in h.acino_last_error_string().decode()


def test_python_interface_defaults_off():
    from acinoset_amd import fte, io
    sig = inspect.signature(fte.FTEContext.reprojection).parameters
    assert list(sig) == ["self", "cov", "cov_pos"] and sig["cov"].default is True and sig["cov_pos"].default is None
    for fn in (fte.fte_solve, fte.fte_solve_clips, fte.fte_solve_batch):
        assert inspect.signature(fn).parameters["return_reprojection"].default is False
    res = {}
    fte._attach_posterior(res, None, lambda a: a)
    fte._attach_posterior(res, {}, lambda a: a)
    assert res == {}
    rep = dict(uv=np.zeros((10, 6, 20, 2)), cov_uv=np.zeros((10, 6, 20, 2, 2)), std_uv=np.zeros((10, 6, 20)),
               res=np.zeros((10, 6, 20, 2)), weight=np.zeros((10, 6, 20, 2)), mahal2=np.zeros((10, 6, 20)),
               flags=np.zeros((10, 6, 20), dtype=np.uint8))
    asked = []                                               # a context that has only the report: no covariance to hand on
    ctx = types.SimpleNamespace(reprojection=lambda cov_pos=None: asked.append(cov_pos) or rep)
    post = fte.FTEContext._posterior(ctx, return_reprojection=True)
    assert asked == [None]
    fte._attach_posterior(res, post, lambda a: a, slice(5, 10))
    assert set(res) == {"uv", "cov_uv", "std_uv", "residuals", "weights", "mahal2", "flags"}
    assert res["uv"].shape == (5, 6, 20, 2) and res["cov_uv"].shape == (5, 6, 20, 2, 2) and res["flags"].shape == (5, 6, 20)
    sig = inspect.signature(io.reprojection_to_points_2d_df).parameters
    assert list(sig) == ["uv", "flags", "start_frame", "markers", "likelihood"] and sig["start_frame"].default == 0


def test_detection_report_on_a_hand_made_report():
    """2 frames, 1 camera, 20 markers; marker 0: one inlier (weights 1, 0.9) and one redescended detection (0.9, 0.2);
    marker 1: one inlier and one unweighted detection that agrees with the trajectory; marker 2: nothing finite."""
    from acinoset_amd import fte
    res = np.full((2, 1, 20, 2), np.nan)
    weight = np.zeros((2, 1, 20, 2))
    flags = np.zeros((2, 1, 20), dtype=np.uint8)
    mahal2 = np.full((2, 1, 20), np.nan)
    res[0, 0, 0], weight[0, 0, 0], flags[0, 0, 0], mahal2[0, 0, 0] = (3.0, -4.0), (1.0, 0.9), 1, 1.0
    res[1, 0, 0], weight[1, 0, 0], flags[1, 0, 0], mahal2[1, 0, 0] = (60.0, 1.0), (0.2, 0.9), 1, 144.0
    res[0, 0, 1], weight[0, 0, 1], flags[0, 0, 1], mahal2[0, 0, 1] = (1.0, 1.0), (1.0, 1.0), 3, 0.08
    res[1, 0, 1], weight[1, 0, 1], flags[1, 0, 1], mahal2[1, 0, 1] = (2.0, 0.0), (0.0, 0.0), 0, 0.16
    flags[:, 0, 2] = 4
    rep = dict(res=res, weight=weight, flags=flags, mahal2=mahal2)
    out = fte.detection_report(rep)
    assert set(out) == {"n_weighted", "n_inlier", "rms_inlier"}
    assert out["n_weighted"].shape == (1, 20)
    assert out["n_weighted"][0, :3].tolist() == [2, 1, 0] and out["n_inlier"][0, :3].tolist() == [1, 1, 0]
    assert out["rms_inlier"][0, 0] == 5.0 and abs(out["rms_inlier"][0, 1] - np.sqrt(2.0)) < 1e-15
    assert np.isnan(out["rms_inlier"][0, 2:]).all()
    out = fte.detection_report(rep, gate=9.21)
    assert out["n_weighted_inside"][0, :3].tolist() == [1, 1, 0] and out["n_weighted_outside"][0, :3].tolist() == [1, 0, 0]
    assert out["n_unweighted_inside"][0, :3].tolist() == [0, 1, 0] and out["n_unweighted_outside"][0, :3].tolist() == [0, 0, 0]
    # the names a solve's results use
    alt = dict(residuals=res, weights=weight, flags=flags, mahal2=mahal2)
    assert np.array_equal(fte.detection_report(alt)["n_inlier"], out["n_inlier"])


def test_predictions_round_trip_through_the_detection_table():
    """io.reprojection_to_points_2d_df -> io.dense_detections gives the array back: x, y, likelihood where the prediction is
    kept, zeros (likelihood 0: "no detection") where it is NaN or behind the camera."""
    pytest.importorskip("pandas")
    from acinoset_amd import fte, io
    rng = np.random.default_rng(3)
    N, Cn = 7, 3
    uv = rng.uniform(0, 1000, (N, Cn, 20, 2))
    flags = rng.integers(0, 2, (N, Cn, 20)).astype(np.uint8)
    lik = rng.uniform(0.5, 1.0, (N, Cn, 20))
    uv[2, 1, 5] = np.nan
    flags[2, 1, 5] = 4
    flags[3, 0, 7] |= 2
    flags[6, 2, 19] |= 2
    df = io.reprojection_to_points_2d_df(uv, flags, start_frame=40, likelihood=lik)
    assert list(df.columns) == ["frame", "camera", "marker", "x", "y", "likelihood"]
    assert len(df) == N * Cn * 20 - 3 and set(df["marker"]) == set(fte.MARKERS)
    det, lo = io.dense_detections(df, Cn, fte.MARKERS, start_frame=40, end_frame=40 + N)
    want = np.concatenate([uv, lik[..., None]], axis=-1)
    for idx in ((2, 1, 5), (3, 0, 7), (6, 2, 19)):
        want[idx] = 0.0
    assert lo == 40 and np.array_equal(det, want)
    det1, _ = io.dense_detections(io.reprojection_to_points_2d_df(uv, flags), Cn, fte.MARKERS, 0, N)
    assert np.array_equal(det1[..., 2], (want[..., 2] > 0).astype(np.float64))


# ---- the reference pinned to itself ---------------------------------------------------------------------------------
def _rig(seq):
    return seq["K"], seq["D"], seq["R"], seq["t"]


def _pinhole_sequence(n):
    """tests/pinhole_fte_ref.pinhole_sequence without the GPU: oracle FK and oracle.camera.project_points."""
    K, _, R, t = osynth.make_rig()
    D = np.tile(pref.D12, (K.shape[0], 1))
    q = osynth.trajectory(n, "sprint")
    pos = ofk.cheetah_fk(q)
    rng = np.random.default_rng(20210313)
    det = np.zeros((n, K.shape[0], 20, 3))
    for c in range(K.shape[0]):
        uv = pref.oracle_project(pos.reshape(-1, 3), K[c], D[c], R[c], t[c]).reshape(n, 20, 2)
        det[:, c, :, :2] = uv + rng.normal(0.0, 2.0, uv.shape)
        det[:, c, :, 2] = np.where(rng.uniform(size=(n, 20)) < 0.15, 0.2, 0.9)
    return dict(K=K, D=D, R=R, t=t, q_true=q, det=det, Ts=1.0 / osynth.FPS)


@pytest.mark.parametrize("model", ["fisheye", "pinhole"])
def test_projection_jacobian_against_central_differences(model):
    """(i) J_pi against central differences of the projection, at the bar tests/test_fte_cov_host.py holds the FK Jacobian
    to: 1e-8 absolute.  Pixels are ~1e3, so second-order differences with h = 1e-6 would carry eps * 1e3 / h = 2e-7 of
    rounding; the fourth-order central stencil with h = 1e-3 carries 1.5 eps * 1e3 / h = 3e-10 of rounding and h^4 / 30
    times a fifth derivative (~1e3 px / m^5 at these distances) = 3e-11 of truncation."""
    seq = osynth.make_sequence(9, "sprint") if model == "fisheye" else _pinhole_sequence(9)
    pos = rref.positions(seq["q_true"][:, ofk.ACTIVE])
    h = 1e-3
    worst = 0.0
    for c in range(seq["K"].shape[0]):
        _, J, _ = rref.project(pos, _rig(seq), c, model)
        for j in range(3):
            d = np.zeros(3)
            d[j] = h
            f = lambda s: rref.project(pos + s * d, _rig(seq), c, model)[0]      # noqa: E731
            fd = (-f(2) + 8 * f(1) - 8 * f(-1) + f(-2)) / (12 * h)
            worst = max(worst, float(np.abs(fd - J[..., j]).max()))
    print(f"\n[{model}] max |J_pi - central differences| = {worst:.2e} px/m")
    assert worst <= 1e-8


def _seven_frame_problem():
    seq = osynth.make_sequence(7, "sprint")
    det = seq["det"]
    prob = ofte.FTEProblem(det[..., :2], det[..., 2], *_rig(seq), seq["Ts"])
    x = np.clip(seq["q_true"][:, ofk.ACTIVE], prob.lo, prob.hi)
    return seq, prob, x


def test_pixel_covariance_is_the_state_covariance_through_both_jacobians():
    """(ii) cov_uv = (J_pi J_fk) cov_x (J_pi J_fk)^T, cov_x the dense inverse of tests/fte_cov_ref.py on 7 frames.  Both sides
    are the same product associated differently ((J_pi (J_fk cov_x J_fk^T)) J_pi^T against (J_pi J_fk) cov_x (J_pi J_fk)^T);
    each carries a few eps of |J_pi| |J_fk| |cov_x| |J_fk|^T |J_pi|^T (the product of the absolute values: cov_x spans
    rad^2 ... m^2 and both products cancel), so the bar per entry is 64 eps of that matrix's norm."""
    seq, prob, x = _seven_frame_problem()
    _, g, H, _ = prob.evaluate(x)
    Hd = cref.with_smooth_diag(H, prob.q_w, prob.s_band())
    fixed = cref.active_set(x, g, Hd, prob.lo, prob.hi)
    cov_x = cref.dense_blocks(cref.banded(Hd, fixed, prob.q_w, prob.s_band()), fixed)
    cov_x = 0.5 * (cov_x + cov_x.transpose(0, 2, 1))      # (an LU inverse is symmetric to cond * eps only; the report takes
    Jfk = cref.fk_jacobian_exact(x)                        #  the symmetric part of what it is given)
    cov_pos, _ = cref.marker_cov(cov_x, Jfk)
    ref = rref.reprojection(x, cov_pos, seq["det"], _rig(seq))
    G = np.einsum("nclij,nljp->nclip", ref["J"], Jfk)
    want = np.einsum("nclip,npq,ncljq->nclij", G, cov_x, G)
    Ga = np.einsum("nclij,nljp->nclip", np.abs(ref["J"]), np.abs(Jfk))
    scale = np.einsum("nclip,npq,ncljq->nclij", Ga, np.abs(cov_x), Ga)
    err = np.linalg.norm((ref["cov_uv"] - want).reshape(-1, 4), axis=1)
    bar = 64 * np.finfo(float).eps * np.linalg.norm(scale.reshape(-1, 4), axis=1)
    print(f"\nmax ||cov_uv - G cov_x G^T||_F / bar = {float((err / bar).max()):.3f}; std_uv median "
          f"{float(np.median(np.sqrt(ref['cov_uv'][..., 0, 0] + ref['cov_uv'][..., 1, 1]))):.2f} px")
    assert np.all(err <= bar)
    assert np.array_equal(ref["cov_uv"][..., 0, 1], ref["cov_uv"][..., 1, 0])
    w = np.linalg.eigvalsh(ref["cov_uv"].reshape(-1, 2, 2))
    assert np.all(w[:, 0] >= -1e-12 * w[:, 1])


@pytest.mark.parametrize("model", ["fisheye", "pinhole"])
def test_report_sums_to_the_objective(model):
    """(iii) sum of rho(w * res) over the flagged detections (+ rho(0) for each dropped component, as the objective counts
    them) equals FTEProblem.measurement_terms(x)[0] to 1e-12 relative; flags, NaN pattern and weights are consistent."""
    if model == "fisheye":
        seq, prob, x = _seven_frame_problem()
    else:
        seq = _pinhole_sequence(7)
        prob = pref.PinholeFTEProblem(seq["det"][..., :2], seq["det"][..., 2], *_rig(seq), seq["Ts"])
        x = np.clip(seq["q_true"][:, ofk.ACTIVE], prob.lo, prob.hi)
    det = seq["det"].copy()
    det[1, 2, 3, 0] = np.nan                                          # a non-finite detection above the threshold
    if model == "fisheye":
        prob = ofte.FTEProblem(det[..., :2], det[..., 2], *_rig(seq), seq["Ts"])
    else:
        prob = pref.PinholeFTEProblem(det[..., :2], det[..., 2], *_rig(seq), seq["Ts"])
    ref = rref.reprojection(x, None, det, _rig(seq), model)
    want = prob.measurement_terms(x, need_jac=False)[0]
    got = rref.measurement_cost(ref)
    print(f"\n[{model}] measurement cost {want:.12f}, from the report {got:.12f}")
    assert abs(got - want) <= 1e-12 * abs(want)
    on = (ref["flags"] & 1) != 0
    assert np.array_equal(on, prob.w > 0) and 0 < on.sum() < on.size
    assert not on[1, 2, 3] and np.isnan(ref["res"][1, 2, 3]).all() and np.isfinite(ref["uv"][1, 2, 3]).all()
    assert np.all(ref["weight"][~on] == 0.0) and np.all((ref["weight"] >= 0) & (ref["weight"] <= 1))
    assert np.isfinite(ref["res"][det[..., 2] <= 0.5][np.isfinite(det[..., :2][det[..., 2] <= 0.5]).all(-1)]).all()
    assert ref["cov_uv"] is None and np.array_equal(np.isnan(ref["mahal2"]), np.isnan(ref["res"]).any(-1))
    share, _ = rref.small_component_share(ref)
    assert share <= 1e-3
