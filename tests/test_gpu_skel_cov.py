"""GPU (-m gpu): acino_skel_fte_covariance (csrc/skel_cov.hip) through build.model_covariance against the CPU references of
tests/skel_cov_ref.py - (a) the dense inverse and (b) banded-Cholesky probes - within bar(d0) = max(64 d0, 1e-13), d0 their own
disagreement on the input; the inputs are those of tests/skel_cov_cases.py (why the skeleton's rest positions are moved: there)."""
import os

import numpy as np
import pytest

import pinhole_fte_ref as pref
import skel_cov_cases as cases
import skel_cov_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx(golden_dir):
    g, sk = cases.load(golden_dir)
    det = np.load(os.path.join(golden_dir, "human_dlc_slice.npz"))["det"].astype(np.float64)
    return g, cases.generic_skeleton(sk), det


def _scene(g, camera_model):
    if camera_model == "pinhole":
        return g["K"], np.tile(pref.D5, (len(g["K"]), 1)), g["R"], g["t"]
    return g["K"], g["D"], g["R"], g["t"]


_REF = {}


def _case(fx, name):
    """(model, x, problem, reference), computed once per input and shared."""
    if name in _REF:
        return _REF[name]
    g, sk, det = fx
    src, n, sf, cam = {"golden": (g["det"], int(g["n_frames"]), int(g["start_frame"]), "fisheye"),
                       "slice40": (det, 40, cases.SLICE_STARTS[0], "fisheye"),
                       "slice40b": (det, 40, cases.SLICE_STARTS[1], "fisheye"),
                       "slice40pin": (det, 40, cases.SLICE_STARTS[0], "pinhole"),
                       "slice100": (det, 100, 60, "fisheye")}[name]
    scene = _scene(g, cam)
    model = cases.make_model(g, sk, src, n, sf, cam, scene)
    x = cases.iterate(g, model)
    prob = cases.problem(sk, model, scene, cam)
    xa = x[:, prob.ACT]
    cases.assert_observed(prob, xa)
    frames = None if n <= 40 else np.array([0, 1, 2, 3, 17, 49, 50, 96, 97, 98, 99])
    _REF[name] = (model, x, prob, ref.reference(prob, xa, frames))
    return _REF[name]


@pytest.mark.parametrize("name", ["golden", "slice40", "slice40pin", "slice100"])
def test_parity_with_the_dense_inverse_and_the_banded_probes(gpu_lib, fx, name):
    from acinoset_amd import build
    model, x, prob, r = _case(fx, name)
    out = build.model_covariance([model], [x])[0]
    act = prob.ACT
    cov = out["cov_x"][:, act[:, None], act[None, :]]
    tol = ref.bar(r["d0"])
    e_a, e_b = ref.rel_err(cov, r["Sa"]), ref.rel_err(cov[r["frames"]], r["Sb"])
    e_p = ref.rel_err(out["cov_pos"].reshape(model.N, -1), r["cov_pos"].reshape(model.N, -1))
    e_s = float(np.max(np.abs(out["std_pos"] - r["std_pos"]) / r["std_pos"]))
    print(f"{name}: PT {(len(act) + 15) // 16 * 16}, d0 {r['d0']:.2e}, bar {tol:.2e}; cov_x vs (a) {e_a:.2e}, vs (b) {e_b:.2e}; cov_pos {e_p:.2e}; "
          f"std_pos {e_s:.2e}; pins {int(r['fixed'].sum())}; std_pos {out['std_pos'].min():.3e} .. {out['std_pos'].max():.3e} m")
    assert out["status"] == 0
    assert e_a <= tol and e_b <= tol and e_p <= tol and e_s <= tol
    inact = np.setdiff1d(np.arange(model.P), act)
    assert np.all(out["cov_x"][:, inact, :] == 0) and np.all(out["cov_x"][:, :, inact] == 0)
    assert np.array_equal(out["cov_x"], np.swapaxes(out["cov_x"], 1, 2))
    assert np.array_equal(build.model_covariance([model], [x], std_only=True)[0]["std_pos"], out["std_pos"])


def test_parity_with_more_than_48_active_states(gpu_lib, fx, golden_dir):
    """P padded to 64 (k_skel_selinv<64>: the panel alone takes 133 KB of LDS): the skeleton with a chain of five more parts
    below "ankle1" - 51 active states, 20 poses -, detections for them copied from the table's first columns."""
    from acinoset_amd import build
    g, _sk, det = fx
    sk = cases.generic_skeleton(cases.load(golden_dir)[1], extra=5)
    det5, parts5 = cases.with_extra_detections(det, g["parts"], 5)
    scene = _scene(g, "fisheye")
    model = cases.make_model(g, sk, det5, 24, 60, parts=parts5)
    x = cases.iterate(g, model)
    prob = cases.problem(sk, model, scene)
    assert 48 < prob.P <= 64 and len(model.names) == 20
    cases.assert_observed(prob, x[:, prob.ACT])
    r = ref.reference(prob, x[:, prob.ACT])
    out = build.model_covariance([model], [x])[0]
    cov = out["cov_x"][:, prob.ACT[:, None], prob.ACT[None, :]]
    tol = ref.bar(r["d0"])
    e_a, e_b = ref.rel_err(cov, r["Sa"]), ref.rel_err(cov, r["Sb"])
    e_p = ref.rel_err(out["cov_pos"].reshape(model.N, -1), r["cov_pos"].reshape(model.N, -1))
    print(f"P = {prob.P} (PT 64): d0 {r['d0']:.2e}, bar {tol:.2e}; cov_x vs (a) {e_a:.2e}, vs (b) {e_b:.2e}; cov_pos {e_p:.2e}")
    assert out["status"] == 0 and e_a <= tol and e_b <= tol and e_p <= tol
    assert float(np.max(np.abs(out["std_pos"] - r["std_pos"]) / r["std_pos"])) <= tol


def _tight(model, x, which):
    """Limits closed onto the iterate for the variables ``which`` [N, P_active] (so that they sit AT a bound)."""
    import copy
    m = copy.copy(model)
    act = np.asarray(model.active)
    lo, hi = model.lo.copy(), model.hi.copy()
    la, ha = lo[:, act], hi[:, act]
    la[which], ha[which] = x[:, act][which], x[:, act][which] + 1.0
    lo[:, act], hi[:, act] = la, ha
    m.lo, m.hi = lo, hi
    return m


def test_pinned_variables_have_zero_rows_and_columns(gpu_lib, fx):
    """Every third variable gets its lower limit ON the iterate: those whose gradient pushes outward are bound-active (the set is
    taken from the oracle and is not empty, nor is everything pinned); their rows and columns are exactly 0, the rest matches."""
    from acinoset_amd import build
    g, sk, _det = fx
    model, x, prob0, _r = _case(fx, "slice40")
    which = np.zeros((model.N, prob0.P), dtype=bool)
    which.reshape(-1)[::3] = True
    m = _tight(model, x, which)
    prob = cases.problem(sk, m, _scene(g, "fisheye"))
    r = ref.reference(prob, x[:, prob.ACT])
    fixed = r["fixed"]
    assert 0 < fixed.sum() < which.sum() and not (fixed & ~which).any()
    out = build.model_covariance([m], [x])[0]
    cov = out["cov_x"][:, prob.ACT[:, None], prob.ACT[None, :]]
    pin = fixed[:, :, None] | fixed[:, None, :]
    assert np.all(cov[pin] == 0)
    assert ref.rel_err(cov, r["Sa"]) <= ref.bar(r["d0"])
    assert ref.rel_err(out["cov_pos"].reshape(model.N, -1), r["cov_pos"].reshape(model.N, -1)) <= ref.bar(r["d0"])


def test_fisher_information_does_not_depend_on_the_residuals(gpu_lib, fx):
    """x, weights and the pin set fixed, the measurements moved by a few pixels: cov_x is bit-identical (the IRLS curvature
    would change).  The oracle confirms that the pin set did not move."""
    import copy
    from acinoset_amd import build
    g, sk, _det = fx
    model, x, prob, r = _case(fx, "slice40")
    m2 = copy.copy(model)
    m2.meas = model.meas + np.array([2.5, -3.25])
    prob2 = cases.problem(sk, m2, _scene(g, "fisheye"))
    assert np.array_equal(ref.pin_set(prob2, x[:, prob.ACT]), r["fixed"])
    a, b = build.model_covariance([model], [x])[0], build.model_covariance([m2], [x])[0]
    assert np.array_equal(a["cov_x"], b["cov_x"]) and np.array_equal(a["cov_pos"], b["cov_pos"])


def test_batch_of_eight_equals_the_clips_one_by_one_and_one_degenerate_clip_stands_alone(gpu_lib, fx):
    """Eight 40-frame windows in one call equal the windows one call each, bit for bit.  Then one clip loses every detection of
    one limb (elbow1, wrist1: the angles of shoulder1 and elbow1 that move only them are observed in no frame): status 5 and
    NaN outputs for it, the other clips unchanged, no exception; alone, the failure is the call's."""
    import copy
    from acinoset_amd import build
    g, sk, det = fx
    models = [cases.make_model(g, sk, det, 40, 60 + 45 * k) for k in range(8)]
    xs = [cases.iterate(g, m, seed=k) for k, m in enumerate(models)]
    many = build.model_covariance(models, xs)
    for k in (0, 3, 7):
        one = build.model_covariance([models[k]], [xs[k]])[0]
        assert many[k]["status"] == 0
        for key in ("cov_x", "cov_pos", "std_pos"):
            assert np.array_equal(one[key], many[k][key]), (k, key)
    bad = copy.copy(models[2])
    names = list(bad.names)
    bad.weights = models[2].weights.copy()
    bad.weights[:, :, [names.index("elbow1"), names.index("wrist1")]] = 0.0
    mixed = build.model_covariance(models[:2] + [bad] + models[3:], xs)
    assert [o["status"] for o in mixed] == [0, 0, 5, 0, 0, 0, 0, 0]
    act = np.asarray(bad.active)
    assert np.isnan(mixed[2]["cov_x"][:, act[:, None], act[None, :]]).all()          # (states outside `active`: zero rows, as ever)
    assert np.isnan(mixed[2]["cov_pos"]).all() and np.isnan(mixed[2]["std_pos"]).all()
    for k in (0, 1, 3, 7):
        for key in ("cov_x", "cov_pos", "std_pos"):
            assert np.array_equal(mixed[k][key], many[k][key]), (k, key)
    with pytest.raises(RuntimeError):
        build.model_covariance([bad], [xs[2]])


def test_return_cov_keyword_leaves_the_solve_untouched(gpu_lib, fx):
    from acinoset_amd import build
    model, x, _prob, _r = _case(fx, "slice40")
    r0, i0 = build.solve_model(model, x0=x, max_iter=6)
    r1, i1 = build.solve_model(model, x0=x, max_iter=6, return_cov=True)
    assert i0 == i1 and sorted(r0) == ["ddx", "dx", "positions", "x"]
    assert np.array_equal(r0["x"], r1["x"]) and np.array_equal(r0["positions"], r1["positions"])
    cv = build.model_covariance([model], [r1["x"]])[0]
    for key in ("cov_x", "cov_pos", "std_pos"):
        assert np.array_equal(cv[key], r1[key])


def test_a_joint_no_camera_sees_has_the_larger_error_bar(gpu_lib, fx):
    """Meaning: on the human slice, a pose slot detected by both cameras in a frame against the same slot in a frame where no
    camera detects it (held by the neighbours and the prior alone): the latter's std_pos is larger.  Frames are chosen from the
    data; both kinds must exist."""
    from acinoset_amd import build
    g, sk, det = fx
    model = cases.make_model(g, sk, det, 100, 300)
    x = cases.iterate(g, model)
    std = build.model_covariance([model], [x], std_only=True)[0]["std_pos"]
    seen = (model.weights > 0).sum(1)                      # [N, n_pose]: cameras that detect the slot
    C = model.weights.shape[1]
    pairs = 0
    for l in range(seen.shape[1]):
        full, none = np.nonzero(seen[:, l] == C)[0], np.nonzero(seen[:, l] == 0)[0]
        if l == list(model.names).index("neck") or full.size == 0 or none.size == 0:
            continue
        pairs += 1
        print(f"slot {model.names[l]}: std seen by {C} cameras {np.median(std[full, l]):.4f} m (median), by none {np.median(std[none, l]):.4f} m")
        assert std[none, l].min() > np.median(std[full, l])
    assert pairs > 0, "no slot with both fully detected and undetected frames in this window"


def test_video_stitches_the_bars_from_the_window_that_supplied_the_frame(gpu_lib, fx, golden_dir):
    """solve_video(return_cov=True) on 300 frames of the shipped video: four windows, ONE batched covariance call; every
    frame's std_pos / cov_pos are those of the window that supplied its positions, finite wherever that window's covariance is
    not singular, NaN where it is; without the keyword the result is what it was."""
    from acinoset_amd import build
    g, sk, _det = fx
    full = np.load(os.path.join(golden_dir, "human_dlc_full.npz"))
    tabs = [(list(full["parts"]), full[f"det{c}"].astype(np.float64)) for c in range(2)]
    kw = dict(scene=_scene(g, "fisheye"), dlc_tables=tabs, first_frame=0, last_frame=299, window=100, overlap=20, pairing="name",
              max_iter=40, warm_passes=0)
    res, infos, starts = build.solve_video(sk, return_cov=True, **kw)
    plain, _i, _s = build.solve_video(sk, **kw)
    assert sorted(plain) == ["ddx", "dx", "positions", "seams", "start_frame", "x"]
    assert all(np.array_equal(plain[k], res[k]) for k in ("positions", "x", "dx", "ddx"))
    assert res["std_pos"].shape == (300, 15) and res["cov_pos"].shape == (300, 15, 3, 3) and len(starts) == 4
    status = np.array([i["cov_status"] for i in infos])
    assert set(status) <= {0, 5} and res["cov_singular_windows"] == [int(k) for k in np.nonzero(status == 5)[0]]
    owner = res["owner"]
    print("covariance status per window:", status.tolist(), "median std_pos (m):", float(np.nanmedian(res["std_pos"])))
    for f in range(300):
        w_i = owner[f]
        own = res["window_std_pos"][w_i][f - starts[w_i]]
        assert np.array_equal(res["std_pos"][f], own, equal_nan=True)
        assert np.isfinite(res["std_pos"][f]).all() == (status[w_i] != 5)
    assert (status == 0).any()
