"""GPU (-m gpu): every kernel that reads per-camera intrinsics, through its public Python entry, on a rig of UNLIKE cameras
(tests/unlike_rig.py: own focal lengths, principal point and distortion per camera; own skew where the model carries one).

On synth.make_rig's identical cameras a kernel that reads camera c's intrinsics from another row computes the right numbers.
Here it cannot: tests/test_unlike_rig_host.py holds, for every case of unlike_rig.CASES, the reference on the rig and the
reference on the rig with K and D rolled by one camera (for the skew cases also: with the skew dropped) at least 1 000 x the
tolerance apart.  The tolerances are those of the neighbouring identical-rig tests, named at each group; the inputs are made
by the oracle alone (unlike_rig.inputs_of), the same arrays the guards see.  Every test prints its errors (pytest -s)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import fte_calib_ref as kref
import fte_cov_ref as cref
import fte_reproj_ref as rref
import unlike_rig as ur
from oracle import fk as ofk
from oracle import sba as osba
from unlike_rig import subset

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mods(gpu_lib):
    from acinoset_amd import calib, ekf, fte, sba
    return calib, ekf, fte, sba


# ---------------------------------------------------------------------------------------------- (a) point-wise, fisheye, skew
def _a_project(mods, inp):
    return dict(uv=np.stack([mods[0].project_points_fisheye(inp["X"], *subset(inp["rig"], c)) for c in range(6)]))


def _a_undistort(mods, inp):
    K, D = inp["rig"][:2]
    return dict(xy=np.stack([mods[0].undistort_points_fisheye(inp["px"][c], K[c], D[c]) for c in range(6)]))


def _a_triangulate(mods, inp):
    rig = inp["rig"]
    return {f"{k}{a}{b}": mods[0].triangulate_points_fisheye(*inp["px"][k, a, b], *subset(rig, a), *subset(rig, b))
            for k in ("noisy", "exact") for a, b in ur.PAIRS}


# ---------------------------------------------------------------------------------------------- (b) point-wise, pinhole
def _b_project(mods, inp):
    return {f"uv{c}": mods[0].project_points(inp["X"][c], *subset(inp["rig"], c)) for c in range(6)}


def _b_triangulate(mods, inp):
    rig = inp["rig"]
    return {f"pair{a}{b}": mods[0].triangulate_points(*inp["px"][(a, b)], *subset(rig, a), *subset(rig, b)) for a, b in ur.PAIRS}


# ---------------------------------------------------------------------------------------------- (c) dense pair kernels
def _c_pairs(mods, inp, name):
    """The index path bit-exact (counts, masks, NaN pattern), the values in the returned dict."""
    calib, want = mods[0], ur.reference_of(name)
    model = "pinhole" if "pinhole" in name else "fisheye"
    got = {}
    for tag, det, rig in (("", inp["det"], inp["rig"]), ("_sub", inp["det_sub"], subset(inp["rig"], ur.CAM_SUBSET))):
        tri, cnt, mask = calib.triangulate_pairs_dense(det, 0.5, *rig, model=model)
        assert np.array_equal(cnt, want["cnt" + tag]) and np.array_equal(mask, want["mask" + tag]), tag
        assert np.array_equal(np.isnan(tri), np.isnan(want["tri" + tag]))
        assert np.isnan(tri[5]).all() and np.isnan(tri[7, 3]).all() and cnt.max() == want["cnt" + tag].max() >= 2
        got["tri" + tag] = tri
        if model == "fisheye":                             # the fused call is the two separate calls, bit for bit
            t2, c2, m2, r2, s2 = calib.triangulate_reproject_dense(det, 0.5, *rig)
            r1, s1 = calib.reproject_residuals(tri, det, 0.5, *rig)
            assert np.array_equal(c2, cnt) and np.array_equal(m2, mask) and np.array_equal(t2, tri, equal_nan=True)
            assert np.array_equal(r2, r1, equal_nan=True) and s2[0] == s1[0] and s1[0] > 0
    if model == "fisheye":
        got["res"] = calib.reproject_residuals(inp["tri_in"], inp["det"], 0.5, *inp["rig"])[0]
    return got


# ---------------------------------------------------------------------------------------------- (d) FTE assembly
def _d_assembly(mods, inp, rig=None):
    fte, seq = mods[2], inp["seq"]
    ctx = fte.FTEContext(seq["det"], *(inp["rig"] if rig is None else rig), seq["Ts"], camera_model=inp["model"])
    try:
        ctx.set_x(inp["xa"])
        st = ctx.state()
        g, h = (a.cpu().numpy() for a in ctx.grad_hess())
        assert np.abs(h - h.transpose(0, 2, 1)).max() < 1e-12 * np.abs(h).max()
        return dict(cost=st["cost"], cost_b=ctx.cost(inp["xb"]), grad=g, hess=h, n_behind=st["n_behind"])
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------- (g) EKF
def _g_ekf(mods, inp):
    kw = {} if inp["model"] == "fisheye" else dict(camera_model="pinhole")
    return mods[1].ekf(inp["det"], *inp["rig"], 120.0, 0.5, (2704, 1520), states0=inp["s0"], **kw)


RUNNERS = {"a_project_fisheye_skew": _a_project, "a_undistort_fisheye_skew": _a_undistort,
           "a_triangulate_fisheye_skew": _a_triangulate, "b_project_pinhole8": _b_project, "b_project_pinhole12": _b_project,
           "b_triangulate_pinhole8": _b_triangulate, "d_fte_fisheye": _d_assembly, "d_fte_fisheye_skew": _d_assembly,
           "d_fte_pinhole8": _d_assembly, "d_fte_pinhole12": _d_assembly, "g_ekf_fisheye_skew": _g_ekf, "g_ekf_pinhole8": _g_ekf}
# every other case has a test of its own below; tests/test_unlike_rig_host.py checks that no case is left without one
OWN_TEST = {"c_pairs_fisheye_skew": "test_dense_pair_kernels", "c_pairs_pinhole": "test_dense_pair_kernels",
            "e_solve_fisheye": "test_fte_solve_matches_the_oracle", "e_path_pinhole8": "test_fte_pinhole_lm_path_identity",
            "f_covariance": "test_fte_posterior_entries", "f_reprojection": "test_fte_posterior_entries",
            "f_calibration_sensitivity": "test_fte_posterior_entries", "h_points_only_fisheye_3": "test_sba_points_only_step",
            "h_dense_fisheye": "test_sba_dense_extrinsic_refinement",
            **{n: "test_sba_first_lm_step" for n in ur.names("h_step")}, **{n: "test_sba_covariance" for n in ur.names("h_cov")}}


@pytest.mark.parametrize("name", list(RUNNERS))
def test_against_the_reference(mods, name):
    """(a) 1e-9 px, 1e-13, 1e-10 m as test_pointwise_camera_kernels; (b) 1e-8 px, 1e-9 m as the same test; (d) 1e-12, 1e-11,
    1e-11 relative as test_fte_cost_gradient_hessian and test_pinhole_cost_gradient_hessian; (g) the tolerances of
    test_hip_ekf_matches_oracle and test_ekf_pinhole_matches_the_reference."""
    inp = ur.inputs_of(name)
    got = RUNNERS[name](mods, inp)
    ur.compare(name, got)
    want = ur.reference_of(name)
    if name == "a_triangulate_fisheye_skew":               # exact pixels give the points back
        for pair in ur.PAIRS:
            med = float(np.median(np.abs(got["exact%d%d" % pair] - inp["X"][pair]).max(1)))
            print(f"  pair {pair}: median error against the true points {med:.2e} m")
            assert med < 1e-12
    if name.startswith("d_"):
        assert got["n_behind"] == want["n_behind"]
    if name.startswith("g_"):
        assert got["outliers_ignored"] == want["outliers_ignored"]
        assert np.abs(got["smoothed_positions"] - mods[1].get_3d_marker_coords(want["smoothed_x"])).max() < 1e-5


def test_pinhole_paths_ignore_a_skew_entry(mods):
    """The pinhole record has no skew, as its references have none: K with K[0, 1] set gives the bits of K without it."""
    calib = mods[0]
    inp = ur.inputs_of("b_triangulate_pinhole8")
    rig = inp["rig"]
    K_skew = rig[0].copy()
    K_skew[:, 0, 1] = ur.SKEW * K_skew[:, 0, 0]
    skewed = (K_skew,) + rig[1:]
    X = ur.cloud()
    for c in range(6):
        assert np.array_equal(calib.project_points(X, *subset(skewed, c)), calib.project_points(X, *subset(rig, c)))
    for a, b in ur.PAIRS:
        px = inp["px"][(a, b)]
        assert np.array_equal(calib.triangulate_points(*px, *subset(skewed, a), *subset(skewed, b)),
                              calib.triangulate_points(*px, *subset(rig, a), *subset(rig, b)))


@pytest.mark.parametrize("name", ur.names("c"))
def test_dense_pair_kernels(mods, name):
    """test_pair_index_path_bit_exact (1e-10 m) and test_pair_index_path_pinhole_seam (1e-9 m) with their frame, marker and NaN
    edits, and the camera subset [5, 2, 0]; the residuals of fixed points to the 1e-9 px of the projection."""
    ur.compare(name, _c_pairs(mods, ur.inputs_of(name), name))


def test_fte_skew_is_ignored_bit_for_bit(mods):
    """The FTE NLP projection carries no skew, as the reference's: the kernel on the skewed K gives the bits of the kernel on the
    same K with the skew zeroed (and equals the oracle on the skewed K: case d_fte_fisheye_skew)."""
    inp = ur.inputs_of("d_fte_fisheye_skew")
    assert np.abs(inp["rig"][0][:, 0, 1]).min() > 1.0
    a, b = _d_assembly(mods, inp), _d_assembly(mods, inp, ur.without_skew(inp["rig"]))
    assert a["cost"] == b["cost"] and a["cost_b"] == b["cost_b"]
    assert np.array_equal(a["grad"], b["grad"]) and np.array_equal(a["hess"], b["hess"])


# ---------------------------------------------------------------------------------------------- (e) FTE solve
def test_fte_solve_matches_the_oracle(mods):
    """test_fte_solve_matches_oracle_trajectory's assertions, n = 60: cost 1e-11, end point 1e-8 m, iterations within one."""
    fte = mods[2]
    inp, want = ur.inputs_of("e_solve_fisheye"), ur.reference_of("e_solve_fisheye")
    det = inp["seq"]["det"]
    res, info = fte.fte_solve(det[..., :2], det[..., 2], *inp["rig"], inp["seq"]["Ts"], x0=inp["x0"], max_iter=80, ftol=1e-13)
    oinfo = want["info"]
    assert info["status_name"] in ("ftol", "xtol", "gtol")
    e_c, e_p = abs(info["cost"] - oinfo["cost"]) / abs(oinfo["cost"]), np.abs(res["positions"] - want["positions"]).max()
    print(f"unlike rig [e_solve_fisheye]: cost {e_c:.2e}  positions {e_p:.2e} m  iterations {info['iter']} / {oinfo['iterations']}")
    assert e_c < 1e-11 and e_p < 1e-8
    assert abs(info["iter"] - oinfo["iterations"]) <= 1
    assert np.abs(res["positions"] - inp["seq"]["pos_true"]).max() < 0.06


def test_fte_pinhole_lm_path_identity(mods):
    """test_pinhole_lm_path_identity's assertions, n = 60: the trial cost (1e-9) and the decision of every iteration, the
    stopping test, the end point within 1e-8 m."""
    fte = mods[2]
    inp, want = ur.inputs_of("e_path_pinhole8"), ur.reference_of("e_path_pinhole8")
    seq, oinfo = inp["seq"], want["info"]
    ctx = fte.FTEContext(seq["det"], *inp["rig"], seq["Ts"], camera_model="pinhole", bcr_levels=0)
    try:
        ctx.set_x(inp["x0"][:, ofk.ACTIVE])
        acc, worst = 0, 0.0
        for it, hh in enumerate(want["history"]):
            ctx.step()
            st = ctx.state()
            worst = max(worst, abs(st["cost_trial"] - hh["Ft"]) / abs(hh["Ft"]))
            assert abs(st["cost_trial"] - hh["Ft"]) < 1e-9 * abs(hh["Ft"]), (it, st["cost_trial"], hh["Ft"])
            assert (st["accepted"] > acc) == (hh["Ft"] < hh["F"]), it
            acc = st["accepted"]
        if st["status"] == 0:
            ctx.step()                # (a gradient test that ends the solve takes one more iteration, without history)
            st = ctx.state()
        assert st["status_name"] == oinfo["status"] and st["iter"] == oinfo["iterations"], (st, oinfo)
        assert st["accepted"] == oinfo["accepted"] and st["n_behind"] == oinfo["n_behind"]
        assert abs(st["cost"] - oinfo["cost"]) < 1e-11 * abs(oinfo["cost"])
        pos = ctx.result()[1].cpu().numpy()
    finally:
        ctx.close()
    e_p = np.abs(pos - want["positions"]).max()
    print(f"unlike rig [e_path_pinhole8]: trial costs {worst:.2e}  positions {e_p:.2e} m  ({len(want['history'])} iterations)")
    assert e_p < 1e-8


# ---------------------------------------------------------------------------------------------- (f) FTE posterior entries
def test_fte_posterior_entries(mods):
    """covariance (tests/test_gpu_fte_cov.py: the dense inverse of the context's own matrix, bar(d0)), reprojection
    (tests/test_gpu_fte_reproj.py: 1e-9 px, 1e-11 relative on the 2 x 2 covariance) and calibration_sensitivity
    (tests/test_gpu_fte_calib.py: per column against the banded solve, bar(d0), and the "translate the rig" identity) of ONE
    solved 30-frame context on the unlike fisheye rig, each against its reference module with the rig handed to it."""
    from test_gpu_fte_calib import _references
    from test_gpu_fte_cov import _check_blocks, _reference_system
    from test_gpu_fte_reproj import _compare, _np
    fte = mods[2]
    inp = ur.inputs_of("f_covariance")
    seq, rig = inp["seq"], inp["rig"]
    ctx = fte.FTEContext(seq["det"], *rig, seq["Ts"])
    try:
        ctx.set_x(ur.nose_line(seq["det"], rig, "fisheye")[:, ofk.ACTIVE])
        info = ctx.solve(100)
        assert info["status_name"] in ("ftol", "xtol", "gtol"), info
        # covariance
        x, fixed, ab = _reference_system(ctx)
        dense = cref.dense_blocks(ab, fixed)
        frames = np.arange(ctx.N)
        d0 = cref.rel_err(cref.probe_blocks(ab, fixed, frames), dense)
        cov = tuple(t.cpu().numpy() for t in ctx.covariance())
        _check_blocks("unlike rig, f_covariance", *cov, x, fixed, dense, frames, cref.bar(d0))
        # reprojection
        cov_pos = ctx.covariance()[1]
        got = _np(ctx.reprojection(cov_pos=cov_pos))
        want = rref.reprojection(x, cov_pos.cpu().numpy(), seq["det"], rig, "fisheye")
        _compare("unlike rig, f_reprojection", got, want, "fisheye")
        # calibration sensitivity
        x, fixed, S1, _S2, d0 = _references(ctx, seq, "fisheye")
        S = ctx.calibration_sensitivity()["sens"].cpu().numpy()
        e = kref.col_err(S, S1)
        print(f"\n[unlike rig, f_calibration_sensitivity] d0 = {d0:.2e}   bar = {cref.bar(d0):.2e}   e = {e:.2e}")
        assert np.isfinite(S).all() and np.all(S[fixed] == 0.0) and e <= cref.bar(d0)
        for a in (np.array([1.0, 0.0, 0.0]), np.array([0.0, 0.0, 1.0]), np.array([0.3, -0.5, 0.2])):
            d_id, e_id = kref.identity_error(S1, fixed, rig[2], a), kref.identity_error(S, fixed, rig[2], a)
            print(f"[unlike rig, identity] a = {a}: d_id = {d_id:.2e}   bar = {cref.bar(d_id):.2e}   e = {e_id:.2e}")
            assert e_id <= cref.bar(d_id)
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------- (g) EKF batch
def test_ekf_batch_equals_the_clips_one_by_one(mods):
    """Three clips of 12, 9 and 2 frames on the skewed unlike rig in one launch: the bits of the clips one by one."""
    ekf = mods[1]
    inp = ur.inputs_of("g_ekf_fisheye_skew")
    clips = [inp["det"][:12], inp["det"][12:21], inp["det"][21:23]]
    s0 = [inp["s0"]] * 3
    batch = ekf.ekf_batch(clips, *inp["rig"], 120.0, 0.5, (2704, 1520), states0=s0)
    for det, r in zip(clips, batch):
        one = ekf.ekf(det, *inp["rig"], 120.0, 0.5, (2704, 1520), states0=s0[0])
        assert r["x"].shape == (len(det), 25) and r["outliers_ignored"] == one["outliers_ignored"]
        for k in ur.EKF_KEYS:
            assert np.array_equal(r[k], one[k]), k


# ---------------------------------------------------------------------------------------------- (h) bundle adjustment
def _proj(calib, model):
    return calib.project_points_fisheye if model == "fisheye" else calib.project_points


@pytest.mark.parametrize("n_cams,model", ur.SBA_STEP)
def test_sba_first_lm_step(mods, n_cams, model):
    """test_first_lm_step_with_ragged_visibility_for_every_camera_count's step and assertions on unlike cameras: the fused path
    with two tile rows (2, 5 cameras) and three (7), a short last chunk (5, 7), and the table path (8, 9)."""
    calib, _ekf, _fte, sba = mods
    name = f"h_step_{model}_{n_cams}"
    errs = ur.lm_step_check(sba, _proj(calib, model), ur.inputs_of(name)["prob"], ur.reference_of(name))
    print(f"unlike rig [{name}]: " + "  ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert "X" in errs, "the reference step does not lower the cost: the case checks nothing of the step"


def test_sba_points_only_step(mods):
    """The points-only step of test_first_lm_step_equals_a_dense_numpy_step (Cauchy scale 50 px), three unlike cameras."""
    calib, _ekf, _fte, sba = mods
    name = "h_points_only_fisheye_3"
    p, want = ur.inputs_of(name)["prob"], ur.reference_of(name)
    pts, _r = sba.bundle_adjust_points_only(p["uv"], p["X0"], p["pi"], p["ci"], p["K"], p["D"], p["R0"], p["t0"],
                                            calib.project_points_fisheye, f_scale=50, max_iter=1)
    info = dict(sba.last_info)
    c0, c1 = want["c0"], want["c1"]
    print(f"unlike rig [{name}]: c0 {abs(info['cost_initial'] - c0) / c0:.2e}  c1 {abs(info['cost_final'] - c1) / c1:.2e}  "
          f"X {np.abs(pts - want['X']).max():.2e}")
    assert info["iterations"] == 1 and info["accepted"] == 1 and c1 < c0
    assert abs(info["cost_initial"] - c0) < 1e-9 * c0 and abs(info["cost_final"] - c1) < 1e-6 * c1, (info, c0, c1)
    assert np.abs(pts - want["X"]).max() < 1e-6


@pytest.mark.parametrize("n_cams,model", ur.SBA_COV)
def test_sba_covariance(mods, n_cams, model):
    """sba.covariance against sba_cov_ref.reference with tests/test_gpu_sba_cov.py's comparison and bar."""
    from test_gpu_sba_cov import TOL, _args, _compare
    calib, _ekf, _fte, sba = mods
    assert TOL == pytest.approx(ur.SBA_COV_TOL, rel=1e-12)
    name = f"h_cov_{model}_{n_cams}"
    prob = ur.inputs_of(name)["prob"]
    _compare(f"unlike rig, {name}", sba.covariance(*_args(prob), project_func=_proj(calib, model)), ur.reference_of(name))


_UNFUSED_SCRIPT = r'''
import json, os, sys
sys.path[:0] = [sys.argv[1], os.path.join(sys.argv[1], "tests")]
import unlike_rig as ur
from acinoset_amd import calib, sba
p = ur.inputs_of("h_step_fisheye_5")["prob"]
pts, rm, tt, _res = sba.bundle_adjust_points_and_extrinsics(p["uv"], p["X0"], p["pi"], p["ci"], p["K"], p["D"], p["R0"], p["t0"],
                                                            calib.project_points_fisheye, max_iter=1)
info = sba.last_info
print("RESULT" + json.dumps(dict(cost0=info["cost_initial"], cost=info["cost_final"], it=info["iterations"], acc=info["accepted"],
                                 r=rm.tolist(), t=tt.tolist(), p=pts.tolist())))
'''


def test_sba_table_path_gives_the_fused_step(mods):
    """ACINO_SBA_UNFUSED=1 (read once per process: a child process) on the 5-camera unlike problem against the fused path in this
    process, to the fp64 tolerances of test_fused_path_equals_the_table_path: counts equal, costs 1e-12 / 1e-10, poses and
    points 1e-8."""
    calib, _ekf, _fte, sba = mods
    assert "ACINO_SBA_UNFUSED" not in os.environ
    p = ur.inputs_of("h_step_fisheye_5")["prob"]
    pts, rm, tt, _res = sba.bundle_adjust_points_and_extrinsics(p["uv"], p["X0"], p["pi"], p["ci"], p["K"], p["D"], p["R0"], p["t0"],
                                                                calib.project_points_fisheye, max_iter=1)
    a = dict(sba.last_info)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _UNFUSED_SCRIPT, root], env=dict(os.environ, ACINO_SBA_UNFUSED="1"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    b = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT")][-1][6:])
    assert a["iterations"] == b["it"] == 1 and a["accepted"] == b["acc"] == 1
    assert abs(a["cost_initial"] - b["cost0"]) <= 1e-12 * abs(b["cost0"])
    assert abs(a["cost_final"] - b["cost"]) <= 1e-10 * abs(b["cost"]), (a["cost_final"], b["cost"])
    errs = [np.abs(x - np.array(y)).max() for x, y in ((rm, b["r"]), (tt, b["t"]), (pts, b["p"]))]
    print(f"unlike rig [table path, 5 cameras]: R {errs[0]:.2e}  t {errs[1]:.2e}  X {errs[2]:.2e}")
    assert max(errs) < 1e-8


def test_sba_dense_extrinsic_refinement(mods):
    """test_dense_extrinsic_refinement_against_the_scipy_oracle's fp64 assertions on a 20-frame sprint through the unlike rig
    (tests/test_unlike_rig_host.py: the smallest tensor of the kind on which the scipy oracle still has all six cameras
    and lowers the cost): the observation lists, the cost of the start (1e-9, the guarded quantity) and of the end state
    through the oracle's cost function, an end at or below scipy's."""
    import torch
    _calib, _ekf, _fte, sba = mods
    name = "h_dense_fisheye"
    inp, want = ur.inputs_of(name), ur.reference_of(name)
    (K, D, _R, _t), det = inp["rig"], inp["det"]
    keep, uv, cam_idx, pt_start, _obs = sba.dense_observations(torch.as_tensor(det, device="cuda"), 0.5)
    assert np.array_equal(keep.cpu().numpy(), inp["keep"])
    assert np.array_equal(cam_idx.cpu().numpy(), inp["ci"]) and np.array_equal(uv.cpu().numpy(), inp["p2"])
    assert np.array_equal(np.diff(pt_start.cpu().numpy()), np.bincount(inp["pi"]))
    pts, rm, tt, info = sba.bundle_adjust_dense_points_and_extrinsics(det, inp["X0"], K, D, inp["Rp"], inp["tp"], 0.5, max_iter=100)
    ur.compare(name, dict(cost_initial=np.array(info["cost_initial"])))
    end = osba.residuals(pts.cpu().numpy()[inp["keep"]], rm, tt, K, D, inp["pi"], inp["ci"], inp["p2"])
    assert abs(osba.cauchy_cost(end) - info["cost_final"]) < 1e-9 * info["cost_final"]
    assert info["status_name"] in ("ftol", "gtol", "max_iter")
    assert info["n_points"] == int(inp["keep"].sum()) and info["n_obs"] == len(inp["pi"])
    oopt = ur.dense_scipy()
    print(f"unlike rig [{name}]: cost {info['cost_initial']:.4f} -> {info['cost_final']:.4f} ({info['iterations']} it), scipy {oopt.cost:.4f}")
    assert info["cost_final"] <= oopt.cost * (1 + 1e-6), (info["cost_final"], oopt.cost)
