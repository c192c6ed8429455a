"""GPU: the bundle-adjustment covariance (csrc/sba_cov.hip through acinoset_amd.sba.covariance and ``return_cov=``) against the
dense numpy reference of tests/sba_cov_ref.py.

The measure is max |Sigma - Sigma_ref| / (std_i std_j) (``ref.scaled_error``).  Observed on the MI355X over every case of this
file: 1.21e-9 (OBSERVED below); the reference's own floor - Richardson against plain central differences - is 1.1e-8.  The bar
is TOL = 10 x the larger of the two = 1.1e-7: ten times, because cond(N^T S N) varies by about that factor over the cases.
"""
import numpy as np
import pytest

import sba_cov_ref as ref

pytestmark = pytest.mark.gpu

OBSERVED = 1.21e-9         # seven cameras, baseline gauge held at camera 6, cov_cams; most cases 5e-11 .. 2.5e-10
TOL = 10 * max(OBSERVED, ref.FLOOR)


@pytest.fixture(scope="module")
def gsba(gpu_lib):
    from acinoset_amd import calib, sba
    return sba, calib


def _proj(calib, prob):
    return calib.project_points_fisheye if prob["model"] == "fisheye" else calib.project_points


def _args(prob):
    return (prob["uv"], prob["X"], prob["pi"], prob["ci"], prob["K"], prob["D"], prob["R"], prob["t"])


def _compare(tag, out, want, cameras=True):
    errs = {}
    if cameras:
        for key in ("cov_cams", "cov_cam", "cov_center"):
            errs[key] = ref.scaled_error(out[key], want[key])
        for key in ("std_rot_deg", "std_center"):
            live = want[key] > 1e-6 * want[key].max()
            errs[key] = float(np.abs(out[key][live] / want[key][live] - 1).max())
            assert np.abs(out[key][~live]).max(initial=0.0) <= 1e-6 * want[key].max()
    kept = ~want["excluded"]
    assert np.array_equal(np.isnan(out["std_points"]), ~kept) and np.array_equal(np.isnan(out["cov_points"]).any((1, 2)), ~kept)
    errs["cov_points"] = ref.scaled_error(out["cov_points"][kept], want["cov_points"][kept])
    errs["std_points"] = float(np.abs(out["std_points"][kept] / want["std_points"][kept] - 1).max())
    errs["sigma2"] = abs(out["sigma2"] / want["sigma2"] - 1)
    print(f"sba_cov {tag}: " + "  ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert out["dof"] == want["dof"] and out["n_points_excluded"] == want["n_points_excluded"]
    assert out["status_name"] == "ok"
    worst = max(errs.values())
    assert worst < TOL, (tag, errs)
    return worst


@pytest.mark.parametrize("n_cams", [2, 3, 6, 7, 8, 16])
def test_camera_counts_gauges_and_scales(gsba, n_cams):
    """The solver's fused range (2 .. 7 cameras), one past it, and the maximum, in the ONE code path of the covariance; 37
    points (23 for 16 cameras) with 2 .. C views each: neither the last batch of 256 / C points nor the last wave is full."""
    sba, calib = gsba
    prob, J = ref.cached(n_cams, 23 if n_cams == 16 else 37, 100 + n_cams)
    for gauge in ("baseline", "free"):
        for scale in ("residual", "unit"):
            out = sba.covariance(*_args(prob), project_func=_proj(calib, prob), gauge=gauge, scale=scale)
            want = ref.reference(prob, gauge=gauge, scale=scale, J=J)
            assert out["gauge"] == gauge and out["scale"] == scale and out["cov_cams"].shape == (6 * n_cams, 6 * n_cams)
            _compare(f"C={n_cams} {gauge} {scale}", out, want)
    # another reference pair of the baseline gauge
    out = sba.covariance(*_args(prob), gauge="baseline", ref_cam=n_cams - 1, scale_cam=0)
    _compare(f"C={n_cams} baseline ref {n_cams - 1}", out, ref.reference(prob, ref_cam=n_cams - 1, scale_cam=0, J=J))


def test_pinhole_model(gsba):
    sba, calib = gsba
    prob, J = ref.cached(3, 30, 17, "pinhole")
    out = sba.covariance(*_args(prob), project_func=calib.project_points)
    _compare("pinhole C=3", out, ref.reference(prob, J=J))


def test_points_only(gsba):
    """Cameras fixed, Cauchy scale 50 px as bundle_adjust_points_only: Sigma_p = sigma2 V_p^-1, no gauge."""
    sba, calib = gsba
    prob, J = ref.cached(6, 37, 31, "fisheye", False, None, False)
    for scale in ("residual", "unit"):
        out = sba.covariance(*_args(prob), optimize_cameras=False, f_scale=50, scale=scale)
        want = ref.reference(prob, optimize_cameras=False, f_scale=50, scale=scale, J=J)
        assert out["cov_cams"] is None and out["gauge"] is None and out["dof"] == 3 * 37
        _compare(f"points only {scale}", out, want, cameras=False)


def test_single_view_point_is_left_out(gsba):
    sba, _calib = gsba
    prob, J = ref.cached(6, 37, 41, "fisheye", True)
    out = sba.covariance(*_args(prob))
    want = ref.reference(prob, J=J)
    assert out["n_points_excluded"] == 1 and np.isnan(out["cov_points"][-1]).all() and np.isnan(out["std_points"][-1])
    _compare("single view", out, want)
    # everything else equals the problem built without that point
    keep = prob["pi"] != prob["P"] - 1
    sub = sba.covariance(prob["uv"][keep], prob["X"][:-1], prob["pi"][keep], prob["ci"][keep], *_args(prob)[4:])
    assert sub["dof"] == out["dof"] and sub["n_points_excluded"] == 0
    assert ref.scaled_error(sub["cov_cams"], out["cov_cams"]) < TOL
    assert ref.scaled_error(sub["cov_points"], out["cov_points"][:-1]) < TOL


def test_singular_problems_have_the_numeric_status(gsba):
    sba, _calib = gsba
    prob = ref.make_problem(6, 37, 51, blind_cam=4)             # a camera that no point sees
    assert 4 not in prob["ci"]
    with pytest.raises(RuntimeError, match="not positive definite"):
        sba.covariance(*_args(prob))
    out = sba.covariance(*_args(prob), raise_numeric=False)
    assert out["status_name"] == "numeric" and np.isnan(out["cov_cams"]).all() and np.isnan(out["cov_points"]).all()
    assert np.isnan(out["std_rot_deg"]).all() and np.isnan(out["std_points"]).all()
    # constraints of rank 6 on a healthy problem
    good, _J = ref.cached(6, 37, 106)
    gauge = ref.constraints(good, "baseline")
    gauge[:, 6] = gauge[:, 0]
    with pytest.raises(RuntimeError, match="rank below 7"):
        sba.covariance(*_args(good), gauge=gauge)
    out = sba.covariance(*_args(good), gauge=gauge, raise_numeric=False)
    assert out["status_name"] == "numeric" and out["gauge"] == "custom" and np.isnan(out["cov_cams"]).all()
    # constraints of full rank that do not fix the gauge (two cameras' rotations held: the translation stays free)
    loose = np.zeros((36, 7))
    loose[[0, 1, 2, 6, 7, 8, 12], np.arange(7)] = 1.0
    out = sba.covariance(*_args(good), gauge=loose, raise_numeric=False)
    assert out["status_name"] == "numeric" and np.isnan(out["cov_cams"]).all()
    # too few points: 2 M <= dof
    few = ref.make_problem(6, 3, 52)                            # (at most 18 observations: 2 M <= 36 < dof = 38)
    out = sba.covariance(*_args(few), raise_numeric=False)
    assert 2 * len(few["pi"]) <= out["dof"] and out["status_name"] == "numeric" and np.isnan(out["sigma2"])
    # the custom gauge that IS the baseline block gives the baseline result
    a = sba.covariance(*_args(good), gauge=ref.constraints(good, "baseline"))
    b = sba.covariance(*_args(good))
    assert ref.scaled_error(a["cov_cams"], b["cov_cams"]) < TOL


def test_relative_rotation_is_gauge_invariant_on_the_device(gsba):
    sba, _calib = gsba
    prob, _J = ref.cached(6, 37, 106)
    a = sba.covariance(*_args(prob), gauge="baseline")
    b = sba.covariance(*_args(prob), gauge="free")
    assert ref.scaled_error(a["cov_cams"], b["cov_cams"]) > 1e-2
    for ca, cb in ((1, 0), (4, 2), (5, 3)):
        ra = ref.relative_rotation_cov(a["cov_cams"], prob["R"], ca, cb)
        rb = ref.relative_rotation_cov(b["cov_cams"], prob["R"], ca, cb)
        err = ref.scaled_error(ra, rb)
        print(f"sba_cov relative rotation {ca}-{cb}, baseline vs free: {err:.2e}")
        assert err < TOL
    assert a["sigma2"] == b["sigma2"]


@pytest.mark.parametrize("n_cams,n_pts", [(6, 43), (4, 65)])
def test_one_point_alone_in_the_last_batch(gsba, n_cams, n_pts):
    """A batch is 256 / C points (42 for six cameras, 64 for four): one more leaves a single point in the last batch."""
    sba, _calib = gsba
    assert n_pts == 256 // n_cams + 1
    prob, J = ref.cached(n_cams, n_pts, 60 + n_cams)
    _compare(f"remainder C={n_cams} P={n_pts}", sba.covariance(*_args(prob)), ref.reference(prob, J=J))


def test_a_single_point(gsba):
    sba, _calib = gsba
    prob, J = ref.cached(6, 1, 71, "fisheye", False, None, False)
    out = sba.covariance(*_args(prob), optimize_cameras=False, f_scale=50)
    _compare("P=1 points only", out, ref.reference(prob, optimize_cameras=False, f_scale=50, J=J), cameras=False)


def test_return_cov_of_the_drop_ins(gsba):
    """return_cov=True changes nothing in what the solve returns and appends the covariance at the returned iterate."""
    sba, calib = gsba
    prob, _J = ref.cached(3, 30, 17)
    proj = calib.project_points_fisheye
    plain = sba.bundle_adjust_points_and_extrinsics(*_args(prob), proj)
    with_cov = sba.bundle_adjust_points_and_extrinsics(*_args(prob), proj, return_cov=True, gauge="free", scale="unit")
    assert len(plain) == 4 and len(with_cov) == 5
    for a, b in zip(plain[:3], with_cov[:3]):
        assert np.array_equal(a, b)
    assert np.array_equal(plain[3]["before"], with_cov[3]["before"]) and np.array_equal(plain[3]["after"], with_cov[3]["after"])
    pts, rm, tt, _res, cov = with_cov
    direct = sba.covariance(prob["uv"], pts, prob["pi"], prob["ci"], prob["K"], prob["D"], rm, tt, gauge="free", scale="unit")
    assert cov["gauge"] == "free" and cov["scale"] == "unit" and cov["sigma2"] == pytest.approx(direct["sigma2"], rel=1e-12)
    assert ref.scaled_error(cov["cov_cams"], direct["cov_cams"]) < TOL
    assert ref.scaled_error(cov["cov_points"], direct["cov_points"]) < TOL
    # points only: f_scale = 50 as that call uses it
    p0 = sba.bundle_adjust_points_only(*_args(prob), proj)
    p1 = sba.bundle_adjust_points_only(*_args(prob), proj, return_cov=True)
    assert len(p0) == 2 and len(p1) == 3 and np.array_equal(p0[0], p1[0]) and np.array_equal(p0[1]["after"], p1[1]["after"])
    direct = sba.covariance(prob["uv"], p1[0], prob["pi"], prob["ci"], prob["K"], prob["D"], prob["R"], prob["t"],
                            optimize_cameras=False, f_scale=50)
    assert p1[2]["cov_cams"] is None and np.array_equal(p1[2]["cov_points"], direct["cov_points"])


def test_dense_entry_scatters_the_point_bars(gsba):
    sba, _calib = gsba
    import torch
    from acinoset_amd import fte, synth
    from oracle import camera as ocam
    seq = synth.make_sequence(12, "trot", seed=20210313)
    K, D, R, t, det = seq["K"], seq["D"], seq["R"], seq["t"], np.array(seq["det"])
    det[2, 1:, 5, 2] = 0.0                                   # marker 5 of frame 2: one view; marker 11 of frame 7: none
    det[7, :, 11, 2] = 0.0
    rng = np.random.default_rng(3)
    pos = np.asarray(fte.cheetah_fk(seq["q_true"]))
    X0 = pos + rng.normal(0, 0.01, pos.shape)
    Rp = np.array([ocam.rodrigues(rng.normal(0, 0.005, 3)) @ R[c] for c in range(len(R))])
    tp = np.asarray(t, dtype=np.float64).reshape(-1, 3, 1) + rng.normal(0, 0.005, (len(R), 3, 1))
    plain = sba.bundle_adjust_dense_points_and_extrinsics(det, X0, K, D, Rp, tp, 0.5, max_iter=20)
    out = sba.bundle_adjust_dense_points_and_extrinsics(det, X0, K, D, Rp, tp, 0.5, max_iter=20, return_cov=True)
    assert "cov" not in plain[3] and torch.equal(plain[0], out[0]) and np.array_equal(plain[1], out[1]) and np.array_equal(plain[2], out[2])
    cov = out[3]["cov"]
    keep = sba.dense_observations(torch.as_tensor(det, device="cuda"), 0.5)[0].cpu().numpy()
    N, L = keep.shape
    assert cov["std_points"].shape == (N, L) and cov["cov_points"].shape == (N, L, 3, 3)
    assert not keep.all() and np.array_equal(np.isnan(cov["std_points"]), ~keep)
    assert np.array_equal(np.isnan(cov["cov_points"]).any((2, 3)), ~keep) and cov["n_points_excluded"] == 0
    assert cov["cov_cams"].shape == (6 * len(R), 6 * len(R)) and np.isfinite(cov["std_rot_deg"]).all()
    assert cov["std_rot_deg"][0] < 1e-6 * cov["std_rot_deg"].max() and cov["dof"] == 3 * int(keep.sum()) + 6 * len(R) - 7


def test_repeated_call_is_bit_identical(gsba):
    """5 000 points over six cameras (20 workgroup records in the sum): no floating-point atomics anywhere."""
    sba, _calib = gsba
    from acinoset_amd import synth
    from oracle import camera as ocam
    rng = np.random.default_rng(77)
    K, D, R, t = synth.make_rig()
    P = 5000
    X = np.array([2.0, 6.5, 0.7]) + rng.normal(0, 0.6, (P, 3))
    seen = rng.random((P, 6)) < 0.7
    seen[np.arange(P), rng.integers(0, 6, P)] = True
    seen[np.arange(P), (np.argmax(seen, 1) + 1 + rng.integers(0, 5, P)) % 6] = True      # at least two views
    uv_all = np.stack([ocam.project_points_fisheye(X, K[c], D[c], R[c], t[c]) for c in range(6)], 1)     # [P, 6, 2]
    pi, ci = np.nonzero(seen)
    uv = uv_all[pi, ci] + rng.normal(0, 1.0, (len(pi), 2))
    args = (uv, X + rng.normal(0, 0.02, X.shape), pi, ci, K, D, R, t.reshape(6, 3, 1))
    a, b = sba.covariance(*args), sba.covariance(*args)
    for key in ("cov_cams", "cov_points", "std_points", "cov_center"):
        assert np.isfinite(a[key]).all() and np.array_equal(a[key], b[key]), key
    assert a["sigma2"] == b["sigma2"] and a["n_points_excluded"] == 0 and a["sigma2"] > 0
