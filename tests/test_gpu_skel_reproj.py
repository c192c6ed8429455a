"""GPU (-m gpu): acino_skel_fte_reprojection (csrc/skel_reproj.hip) through build.model_reprojection against the CPU reference
tests/skel_reproj_ref.py.  Inputs: tests/skel_cov_cases.py (generic_skeleton, R_MEAS_TEST, iterate).

Where a covariance enters, cov_pos comes from the CPU reference of the covariance (skel_cov_ref.reference) and the SAME array
goes to the kernel and to the reference: only the new kernel is under test.  Every entry is compared; NaN positions and flags
exactly.  Bars (the project's, or derived from them; none measured here):
    uv, res   max abs difference <= bar_uv = 1e-9 px (fisheye), 1e-8 px (pinhole): tests/test_gpu_parity.py's bars for the
              projections, as tests/test_gpu_fte_reproj.py uses them
    cov_uv    per entry ||S - S_ref||_F <= 1e-11 ||S_ref||_F (the project's bar for H); both off-diagonals the same bits;
              eigenvalues >= -1e-12 * the largest
    mahal2    with d = sqrt(reference), |delta| <= sqrt(2) wg d bar_uv + 1e-10 d^2 + 1e-18.  Derivation: m = r^T A^-1 r with
              A = cov_uv + (2 / wg^2) I, so lambda_min(A) >= 2 / wg^2 whatever cov_uv is.  A residual error dr changes m by
              2 r^T A^-1 dr + O(dr^2); by Cauchy-Schwarz in the A^-1 inner product |r^T A^-1 dr| <= d |dr| / sqrt(lambda_min)
              <= d |dr| wg / sqrt(2), and a residual whose error is bar_uv has |dr| <= bar_uv along the direction that
              matters: first term sqrt(2) wg d bar_uv.  (With both components off by the whole bar at once and aligned with
              the weakest direction of A the bound is sqrt(2) times that; the bar keeps the smaller figure.)  The 2 x 2 solve
              itself - four products, a determinant with cancellation bounded by the ratio of A's eigenvalues, and the error
              of cov_uv (1e-11 relative) entering through A - is a relative error of m: second term 1e-10 d^2; 1e-18 is the
              floor for d = 0.
    objective sum over the bit-0 entries of w (|res_u| + |res_v|) + the oracle's smoothness term = SkelFTEProblem.evaluate(xa)[0]
              to 1e-11 relative (tests/test_gpu_fte_reproj.py's bar for the same identity)
pytest -s prints the observed maxima of every case.
"""
import copy
import os

import numpy as np
import pytest

import pinhole_fte_ref as pref
import skel_cov_cases as cases
import skel_cov_ref as ref
import skel_reproj_ref as rref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx(golden_dir):
    g, sk = cases.load(golden_dir)
    det = np.load(os.path.join(golden_dir, "human_dlc_slice.npz"))["det"].astype(np.float64)
    return g, cases.generic_skeleton(sk), det, sk


def _scene(g, camera_model):
    if camera_model == "pinhole":
        return g["K"], np.tile(pref.D5, (len(g["K"]), 1)), g["R"], g["t"]
    return g["K"], g["D"], g["R"], g["t"]


_REF = {}


def _case(fx, name):
    """(skeleton, scene, camera model, model, x, problem, cov_pos of the CPU reference), computed once per input and shared."""
    if name in _REF:
        return _REF[name]
    g, sk, det, _raw = fx
    cam = "pinhole" if name.endswith("pin") else "fisheye"
    scene = _scene(g, cam)
    model = cases.make_model(g, sk, det, 40, cases.SLICE_STARTS[0], cam, scene)
    x = cases.iterate(g, model)
    prob = cases.problem(sk, model, scene, cam)
    cov_pos = ref.reference(prob, x[:, prob.ACT])["cov_pos"]
    _REF[name] = (sk, scene, cam, model, x, prob, cov_pos)
    return _REF[name]


def _gate_w(model):
    return float(np.asarray(model.weights).max())


def _compare(name, got, want, cam, with_cov=True):
    """The bars of the module docstring on every entry; returns the observed maxima."""
    bar_uv = rref.BAR_UV[cam]
    assert got["flags"].dtype == np.uint8 and np.array_equal(got["flags"], want["flags"]), f"{name}: flags differ"
    for k in ("uv", "res", "mahal2") + (("cov_uv", "std_uv") if with_cov else ()):
        assert got[k].shape == want[k].shape, (name, k)
        assert np.array_equal(np.isnan(got[k]), np.isnan(want[k])), f"{name}: NaN pattern of {k}"
    diff = lambda k: np.abs(got[k] - want[k])[~np.isnan(want[k])]      # noqa: E731
    e_uv, e_res = float(diff("uv").max(initial=0.0)), float(diff("res").max(initial=0.0))
    ok = ~np.isnan(want["mahal2"])
    e_m = float((np.abs(got["mahal2"] - want["mahal2"])[ok] / rref.mahal2_bar(want, cam)[ok]).max(initial=0.0))
    line = f"\n[{name}] max |d uv| = {e_uv:.2e} px   |d res| = {e_res:.2e} px   mahal2 / bar = {e_m:.2e}"
    e_c = 0.0
    if with_cov:
        okc = ~np.isnan(want["cov_uv"][..., 0, 0])
        num = np.linalg.norm((got["cov_uv"] - want["cov_uv"])[okc].reshape(-1, 4), axis=1)
        den = np.linalg.norm(want["cov_uv"][okc].reshape(-1, 4), axis=1)
        e_c = float((num / den).max(initial=0.0))
        line += f"   cov_uv rel = {e_c:.2e}"
    print(line)
    assert e_uv <= bar_uv and e_res <= bar_uv
    assert e_m <= 1.0
    if with_cov:
        assert e_c <= 1e-11
        S = got["cov_uv"][okc]
        assert np.array_equal(S[:, 0, 1], S[:, 1, 0])
        ev = np.linalg.eigvalsh(S)
        assert np.all(ev[:, 0] >= -1e-12 * ev[:, 1])
        assert np.array_equal(got["std_uv"][okc], np.sqrt(np.maximum(S[:, 0, 0] + S[:, 1, 1], 0.0)))
    else:
        assert got["cov_uv"] is None and got["std_uv"] is None
    return dict(uv=e_uv, res=e_res, mahal2=e_m, cov_uv=e_c)


def _check(name, sk, scene, cam, model, x, cov_pos):
    """model_reprojection with the given cov_pos and with cov=False, each against the reference."""
    from acinoset_amd import build
    gw = _gate_w(model)
    got = build.model_reprojection([model], [x], cov_pos=[cov_pos])[0]
    want = rref.reprojection(sk, x, model.meas, model.weights, scene, cam, cov_pos=cov_pos, gate_w=gw)
    _compare(name, got, want, cam)
    plain = build.model_reprojection([model], [x], cov=False)[0]
    want0 = rref.reprojection(sk, x, model.meas, model.weights, scene, cam, gate_w=gw)
    _compare(name + ", no cov", plain, want0, cam, with_cov=False)
    for k in ("uv", "res", "flags"):
        assert np.array_equal(got[k], plain[k], equal_nan=True), k
    assert "cov_status" not in got and "cov_status" not in plain
    return got, want


@pytest.mark.parametrize("name", ["slice40", "slice40pin"])
def test_report_equals_the_reference_and_sums_to_the_objective(gpu_lib, fx, name):
    sk, scene, cam, model, x, prob, cov_pos = _case(fx, name)
    got, _want = _check(name, sk, scene, cam, model, x, cov_pos)
    xa = x[:, prob.ACT]
    on = (got["flags"] & 1) != 0
    assert 0 < on.sum() < on.size
    cost = float((model.weights[on][:, None] * np.abs(got["res"][on])).sum()) + prob.smooth_terms(xa)[0]
    full = prob.evaluate(xa, need_jac=False)[0]
    rel = abs(cost - full) / abs(full)
    print(f"[{name}] objective {full:.12f}, from the report {cost:.12f} (rel {rel:.2e}); weighted {int(on.sum())} of {on.size}")
    assert rel <= 1e-11


def test_51_active_states_and_20_poses(gpu_lib, fx, golden_dir):
    """generic_skeleton(extra=5) at 24 frames: 2 x 20 entries per frame (no multiple of 64), 19 link ops, three workgroups."""
    g, _sk, det, _raw = fx
    sk = cases.generic_skeleton(cases.load(golden_dir)[1], extra=5)
    det5, parts5 = cases.with_extra_detections(det, g["parts"], 5)
    scene = _scene(g, "fisheye")
    model = cases.make_model(g, sk, det5, 24, 60, parts=parts5)
    x = cases.iterate(g, model)
    prob = cases.problem(sk, model, scene)
    assert prob.P == 51 and len(model.names) == 20 and (model.meas.shape[1] * 20) % 64 != 0
    cov_pos = ref.reference(prob, x[:, prob.ACT])["cov_pos"]
    _check("51 states, 20 poses, 24 frames", sk, scene, "fisheye", model, x, cov_pos)


def _sub(model, lo, hi):
    m = copy.copy(model)
    m.meas, m.weights, m.lo, m.hi = model.meas[lo:hi], model.weights[lo:hi], model.lo[lo:hi], model.hi[lo:hi]
    m.init_x = model.init_x[lo:hi]
    return m


def test_batch_of_three_clips_of_seven_frames_equals_the_clips_one_by_one(gpu_lib, fx):
    """21 frames in one launch: clips start at frames 7 and 14 of it, workgroups at 8 and 16."""
    from acinoset_amd import build
    _sk, _scene_, _cam, model, x, _prob, cov_pos = _case(fx, "slice40")
    cuts = [(3, 10), (10, 17), (25, 32)]
    models = [_sub(model, a, b) for a, b in cuts]
    xs, cps = [x[a:b] for a, b in cuts], [cov_pos[a:b] for a, b in cuts]
    r_gate = 1.0 / _gate_w(model)
    many = build.model_reprojection(models, xs, cov_pos=cps, r_gate=r_gate)
    for k in range(3):
        one = build.model_reprojection([models[k]], [xs[k]], cov_pos=[cps[k]], r_gate=r_gate)[0]
        for key in ("uv", "cov_uv", "std_uv", "res", "mahal2", "flags"):
            assert many[k][key].shape[0] == 7 and np.array_equal(one[key], many[k][key], equal_nan=True), (k, key)
    whole = build.model_reprojection([model], [x], cov_pos=[cov_pos], r_gate=r_gate)[0]
    for k, (a, b) in enumerate(cuts):                        # frames are independent: the same bits inside the 40-frame clip
        for key in ("uv", "cov_uv", "res", "mahal2", "flags"):
            assert np.array_equal(whole[key][a:b], many[k][key], equal_nan=True), (k, key)


def test_one_frame(gpu_lib, fx):
    sk, scene, cam, model, x, _prob, cov_pos = _case(fx, "slice40")
    _check("N = 1", sk, scene, cam, _sub(model, 11, 12), x[11:12], cov_pos[11:12])


def test_hand_placed_detections_and_poses(gpu_lib, fx):
    """A NaN detection with a weight; a detection with w = 0 and finite pixels; a pose ON a camera's singular plane; a pose
    behind a camera.  Exact NaN patterns and flags, and the whole clip against the reference as ever."""
    sk, scene, cam, model, x, _prob, cov_pos = _case(fx, "slice40")
    m = copy.copy(model)
    m.meas, m.weights = model.meas.copy(), model.weights.copy()
    x = x.copy()
    names = list(model.names)
    l = names.index("wrist1")
    base = rref.reprojection(sk, x, m.meas, m.weights, scene, cam, gate_w=1.0)
    for n in (4, 9, 20, 30):
        assert np.isfinite(model.meas[n, :, l]).all() and (model.weights[n, :, l] > 0).all(), "pick frames in which both cameras detect the slot"
    m.meas[4, 0, l, 1] = np.nan                              # frame 4, camera 0: missing detection, weight kept
    m.weights[9, 1, l] = 0.0                                 # frame 9, camera 1: finite pixels, no weight
    R, z = np.asarray(scene[2]), base["z_cam"]
    x[20, :3] -= z[20, 1, l] * R[1][2] / (R[1][2] @ R[1][2])           # frame 20: slot l onto camera 1's plane z_cam = 0
    x[30, :3] -= (z[30, 0, l] + 1.0) * R[0][2] / (R[0][2] @ R[0][2])   # frame 30: slot l one metre behind camera 0
    got, want = _check("hand-placed", sk, scene, cam, m, x, cov_pos)
    assert abs(want["z_cam"][20, 1, l]) < 1e-12 and abs(want["z_cam"][30, 0, l] + 1.0) < 1e-9
    e = got
    # the NaN detection: the pixel and its bar are there, the residual and the distance are not; not weighted
    assert np.isfinite(e["uv"][4, 0, l]).all() and np.isfinite(e["cov_uv"][4, 0, l]).all()
    assert np.isnan(e["res"][4, 0, l]).all() and np.isnan(e["mahal2"][4, 0, l]) and e["flags"][4, 0, l] == 0
    # w = 0, finite pixels: residual and distance (at the gate scale) are there; not weighted
    assert np.isfinite(e["res"][9, 1, l]).all() and np.isfinite(e["mahal2"][9, 1, l]) and e["flags"][9, 1, l] == 0
    assert e["flags"][9, 0, l] == 1
    # the singular plane: everything NaN, bits 1 and 2, not weighted although the detection has a weight
    assert np.isnan(e["uv"][20, 1, l]).all() and np.isnan(e["cov_uv"][20, 1, l]).all() and np.isnan(e["res"][20, 1, l]).all()
    assert np.isnan(e["mahal2"][20, 1, l]) and np.isnan(e["std_uv"][20, 1, l]) and e["flags"][20, 1, l] == 6
    # behind the camera: bit 1, still weighted (the assembly has no other cut), numbers finite
    assert e["flags"][30, 0, l] == 3 and np.isfinite(e["uv"][30, 0, l]).all() and np.isfinite(e["mahal2"][30, 0, l])
    assert int(((e["flags"] & 4) != 0).sum()) == 1


def test_shipped_human_skeleton_unmodified(gpu_lib, fx):
    """Its covariance is singular by definition (two active states move no pose): cov=False reports uv / res / flags against the
    reference; cov=True gives cov_status 5 and NaN cov_uv / std_uv / mahal2, and raises nothing."""
    from acinoset_amd import build
    g, _sk, det, raw = fx
    scene = _scene(g, "fisheye")
    model = cases.make_model(g, raw, det, 40, cases.SLICE_STARTS[0])
    x = cases.iterate(g, model)
    got = build.model_reprojection([model], [x], cov=False)[0]
    want = rref.reprojection(raw, x, model.meas, model.weights, scene, gate_w=_gate_w(model))
    _compare("human skeleton, no cov", got, want, "fisheye", with_cov=False)
    full = build.model_reprojection([model], [x])[0]
    assert full["cov_status"] == 5
    assert np.isnan(full["cov_uv"]).all() and np.isnan(full["std_uv"]).all() and np.isnan(full["mahal2"]).all()
    for k in ("uv", "res", "flags"):
        assert np.array_equal(full[k], got[k], equal_nan=True)


def test_a_detection_gap_widens_the_pixel_error_bars(gpu_lib, fx):
    """One pose slot loses its weights in all cameras over 10 interior frames: its std_uv there exceeds the untouched clip's."""
    from acinoset_amd import build
    _sk, _scene_, _cam, model, x, _prob, _cp = _case(fx, "slice40")
    l = list(model.names).index("wrist1")
    gap = copy.copy(model)
    gap.weights = model.weights.copy()
    gap.weights[15:25, :, l] = 0.0
    a, b = build.model_reprojection([model, gap], [x, x])
    assert a["cov_status"] == 0 and b["cov_status"] == 0
    ratio = b["std_uv"][15:25, :, l] / a["std_uv"][15:25, :, l]
    print(f"\n[gap] std_uv of slot {model.names[l]} in frames 15..24: {ratio.min():.2f} .. {ratio.max():.2f} times the untouched clip's "
          f"({a['std_uv'][15:25, :, l].mean():.2f} -> {b['std_uv'][15:25, :, l].mean():.2f} px)")
    assert np.all(b["std_uv"][15:25, :, l] > a["std_uv"][15:25, :, l])
    assert np.all((b["flags"][15:25, :, l] & 1) == 0) and np.isfinite(b["mahal2"][15:25, :, l]).all()


def test_solve_entries(gpu_lib, fx):
    """solve_model(return_reprojection=True), with and without return_cov, returns the arrays of a separate model_reprojection
    call at results["x"]; the solve itself is untouched."""
    from acinoset_amd import build
    _sk, _scene_, _cam, model, x, _prob, _cp = _case(fx, "slice40")
    r0, i0 = build.solve_model(model, x0=x, max_iter=6)
    r1, i1 = build.solve_model(model, x0=x, max_iter=6, return_reprojection=True)
    r2, i2 = build.solve_model(model, x0=x, max_iter=6, return_reprojection=True, return_cov=True)
    assert i0 == i1 == i2 and sorted(r0) == ["ddx", "dx", "positions", "x"]
    assert set(r1) - set(r0) == set(build.REPROJ_KEYS) and set(r2) - set(r1) == {"cov_x", "cov_pos", "std_pos"}
    assert all(np.array_equal(r0[k], r1[k]) and np.array_equal(r0[k], r2[k]) for k in r0)
    assert r1["cov_uv"] is None and r1["std_uv"] is None
    sep1 = build.model_reprojection([model], [r1["x"]], cov=False)[0]
    sep2 = build.model_reprojection([model], [r2["x"]])[0]
    assert sep2["cov_status"] == 0 and np.isfinite(r2["cov_uv"]).all()
    for k in ("uv", "res", "mahal2", "flags"):
        assert np.array_equal(r1[k], sep1[k], equal_nan=True), k
    for k in build.REPROJ_KEYS:
        assert np.array_equal(r2[k], sep2[k], equal_nan=True), k
    rep = build.detection_report(r2, gate=9.21)
    assert rep["n_weighted"].shape == model.weights.shape[1:] and rep["n_weighted"].sum() == int(((r2["flags"] & 1) != 0).sum()) > 0


def test_video_report_is_one_call_over_the_stitched_trajectory(gpu_lib, fx):
    """solve_video on 70 frames of the detection slice: two windows of 40 frames, overlap 10.  The arrays have `total` frames
    and equal the single-clip call on a 70-frame model at the stitched x (cov_uv: with the stitched cov_pos)."""
    from acinoset_amd import build
    g, sk, det, _raw = fx
    scene = _scene(g, "fisheye")
    kw = dict(scene=scene, dlc_tables=cases.tables(det, g["parts"]), first_frame=60, last_frame=129, window=40, overlap=10,
              pairing="name", r_meas=cases.R_MEAS_TEST, max_iter=15, warm_passes=0)
    plain, _i, starts = build.solve_video(sk, **kw)
    res, _i, _s = build.solve_video(sk, return_reprojection=True, gate=9.21, **kw)
    both, infos, _s = build.solve_video(sk, return_reprojection=True, return_cov=True, **kw)
    assert starts == [60, 90] and sorted(plain) == ["ddx", "dx", "positions", "seams", "start_frame", "x"]
    assert all(np.array_equal(plain[k], res[k]) and np.array_equal(plain[k], both[k]) for k in ("positions", "x", "dx", "ddx"))
    assert set(res) - set(plain) == set(build.REPROJ_KEYS) | {"outlier_frames"} and "outlier_frames" not in both
    whole, _ = build.build_model(sk, scene=scene, dlc_tables=kw["dlc_tables"], n_frames=70, start_frame=60, pairing="name",
                                 r_meas=cases.R_MEAS_TEST, initial_line=False)
    C, L = whole.meas.shape[1:3]
    assert res["uv"].shape == (70, C, L, 2) and res["flags"].shape == (70, C, L) and res["cov_uv"] is None
    one = build.model_reprojection([whole], [res["x"]], cov=False)[0]
    for k in ("uv", "res", "mahal2", "flags"):
        assert np.array_equal(res[k], one[k], equal_nan=True), k
    want = np.nonzero((((one["flags"] & 1) != 0) & (np.nan_to_num(one["mahal2"], nan=0.0) > 9.21)).any(axis=(1, 2)))[0]
    assert res["outlier_frames"] == want.tolist()
    print(f"\n[video] {len(want)} of 70 frames hold a weighted detection outside the gate")
    assert both["cov_uv"].shape == (70, C, L, 2, 2)
    one = build.model_reprojection([whole], [both["x"]], cov_pos=[both["cov_pos"]])[0]
    for k in build.REPROJ_KEYS:
        assert np.array_equal(both[k], one[k], equal_nan=True), k
    assert np.array_equal(both["uv"], res["uv"], equal_nan=True)
    assert np.isfinite(both["cov_uv"]).all() == all(i["cov_status"] == 0 for i in infos)
