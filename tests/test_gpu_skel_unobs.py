"""GPU (-m gpu): the observability rule of the skeleton-FTE posterior - acino_skel_fte_observability (k_skel_observability) and
the pin_unobserved argument of acino_skel_fte_covariance_pinned / acino_skel_fte_sample_pinned - through build.model_observability
and the ``pin_unobserved`` keyword, against the numpy references of tests/skel_unobs_ref.py (the rule), tests/skel_cov_ref.py (the
dense inverse and the banded probes of the pinned matrix) and tests/skel_sample_ref.py (the two maps z -> delta).

    bar(d0) = max(64 d0, 1e-13),   d0 the disagreement of the two CPU references on the very input;   d0 > 1e-8 is refused

Inputs: tests/skel_unobs_cases.py (36 active states, PT = 48, fisheye, r_meas = 0.3 unless the name says otherwise)."""
import copy
import os

import numpy as np
import pytest

import skel_cov_cases as cases
import skel_cov_ref as cref
import skel_sample_ref as sref
import skel_unobs_cases as ucases
import skel_unobs_ref as uref

from oracle import skeleton_fk as osk

pytestmark = pytest.mark.gpu


def _unobserved(c):
    return ucases.full_index(c, np.nonzero(c["ref"]["unobserved"])[0])


def _compare(out, c, label):
    """One clip's pinned covariance against the reference of the pinned matrix: the mask, status 0, cov_x against (a) and (b),
    +inf / NaN exactly at the dependent slots, every other slot within the bar, exact zeros at the unobserved states."""
    r, act = c["ref"], c["prob"].ACT
    N = c["model"].N
    assert r["d0"] <= 1e-8
    tol = uref.bar(r["d0"])
    dep = r["dependent"]
    assert (dep == dep[0]).all()
    ok = ~dep[0]
    cov = out["cov_x"][:, act[:, None], act[None, :]]
    e_a, e_b = cref.rel_err(cov, r["Sa"]), cref.rel_err(cov[r["frames"]], r["Sb"])
    e_p = cref.rel_err(out["cov_pos"][:, ok].reshape(N, -1), r["cov_pos"][:, ok].reshape(N, -1))
    e_s = float(np.max(np.abs(out["std_pos"][:, ok] - r["std_pos"][:, ok]) / r["std_pos"][:, ok]))
    print(f"{label}: PT {(len(act) + 15) // 16 * 16}, N {N}, unobserved {out['unobserved']}, d0 {r['d0']:.2e}, bar {tol:.2e}; cov_x vs (a) "
          f"{e_a:.2e}, vs (b) {e_b:.2e}; cov_pos {e_p:.2e}; std_pos {e_s:.2e}; dependent slots {int(dep[0].sum())}")
    assert out["unobserved"] == _unobserved(c)
    assert out["status"] == 0
    assert e_a <= tol and e_b <= tol and e_p <= tol and e_s <= tol
    assert np.array_equal(np.isposinf(out["std_pos"]), dep) and np.isfinite(out["std_pos"][:, ok]).all()
    nan9 = np.isnan(out["cov_pos"]).reshape(N, -1, 9)
    assert np.array_equal(nan9.all(-1), dep) and np.array_equal(nan9.any(-1), dep)
    un = np.asarray(out["unobserved"], dtype=np.int64)
    assert np.all(out["cov_x"][:, un, :] == 0) and np.all(out["cov_x"][:, :, un] == 0)
    assert np.array_equal(out["cov_x"], np.swapaxes(out["cov_x"], 1, 2))


@pytest.mark.parametrize("name", ["shipped40", "shipped12"])
def test_the_shipped_skeleton_gets_its_error_bars(gpu_lib, golden_dir, name):
    """Case 1: the reference's human skeleton, unmodified.  Full-state 33 and 43 are pinned, every bar is finite; without the
    keyword the clip is singular as before."""
    from acinoset_amd import build
    c = ucases.solved(golden_dir, name)
    model, x = c["model"], c["x"]
    out = build.model_covariance([model], [x], pin_unobserved=True)[0]
    _compare(out, c, name)
    assert out["unobserved"] == [33, 43]
    assert np.isfinite(out["std_pos"]).all() and np.isfinite(out["cov_pos"]).all()
    off = build.model_covariance([model, model], [x, x])
    assert [o["status"] for o in off] == [5, 5] and all("unobserved" not in o for o in off)
    assert np.isnan(off[0]["std_pos"]).all()
    with pytest.raises(RuntimeError):
        build.model_covariance([model], [x], pin_unobserved=False)


def _windows(golden_dir, c, starts):
    g, _sk0, det = ucases.scases.fixture(golden_dir)
    models = [cases.make_model(g, c["sk"], det, c["model"].N, sf, c["cam"], c["scene"]) for sf in starts]
    return models, [cases.iterate(g, m, seed=k + 1) for k, m in enumerate(models)]


def test_a_lost_limb_in_a_batch_of_four(gpu_lib, golden_dir):
    """Case 2: clip 2 of four has no detection of elbow1 / wrist1.  Its six states are pinned, exactly those two poses are
    undetermined, the rest is within the bar; the other clips carry the bits of the call without the keyword."""
    from acinoset_amd import build
    c = ucases.solved(golden_dir, "lost12")
    others, xo = _windows(golden_dir, c, (105, 150, 195))
    models, xs = others[:2] + [c["model"]] + others[2:], xo[:2] + [c["x"]] + xo[2:]
    on, off = build.model_covariance(models, xs, pin_unobserved=True), build.model_covariance(models, xs)
    _compare(on[2], c, "lost12 as clip 2 of 4")
    names = list(c["model"].names)
    limb = [names.index(k) for k in ucases.LIMB]
    assert np.isposinf(on[2]["std_pos"][:, limb]).all() and np.isnan(on[2]["cov_pos"][:, limb]).all()
    assert [o["status"] for o in off] == [0, 0, 5, 0] and [o["status"] for o in on] == [0, 0, 0, 0]
    for k in (0, 1, 3):
        assert on[k]["unobserved"] == []
        for key in ("cov_x", "cov_pos", "std_pos"):
            assert np.array_equal(on[k][key], off[k][key]), (k, key)


def test_a_limb_seen_in_two_frames_stays_singular_and_n_seen_says_why(gpu_lib, golden_dir):
    """Case 3: nothing is unobserved by the rule, the prior's quadratic drift is free all the same: status 5 with the keyword on."""
    from acinoset_amd import build
    c = ucases.case(golden_dir, "two12")
    r = c["ref"]
    good, xg = _windows(golden_dir, c, (105,))
    on = build.model_covariance([good[0], c["model"]], [xg[0], c["x"]], pin_unobserved=True)
    assert [o["status"] for o in on] == [0, 5] and on[1]["unobserved"] == [] and np.isnan(on[1]["std_pos"]).all()
    with pytest.raises(RuntimeError):
        build.model_covariance([c["model"]], [c["x"]], pin_unobserved=True)
    ob = build.model_observability([c["model"]], [c["x"]])[0]
    act = c["prob"].ACT
    six = np.nonzero(r["n_seen"] < 3)[0]
    assert six.tolist() == [6, 9, 17, 20, 28, 31]
    assert ob["unobserved"] == [] and np.array_equal(ob["n_seen"][act], r["n_seen"])
    assert (ob["n_seen"][act][six] <= 2).all() and (np.delete(ob["n_seen"][act], six) >= 3).all()


def test_a_fully_observed_clip_is_untouched_by_the_keyword(gpu_lib, golden_dir):
    """Case 4."""
    from acinoset_amd import build
    c = ucases.case(golden_dir, "slice40")
    on = build.model_covariance([c["model"]], [c["x"]], pin_unobserved=True)[0]
    off = build.model_covariance([c["model"]], [c["x"]])[0]
    assert on["status"] == 0 and off["status"] == 0 and on["unobserved"] == []
    for key in ("cov_x", "cov_pos", "std_pos"):
        assert np.array_equal(on[key], off[key]), key


@pytest.mark.parametrize("name", ["lost12p51", "lost12pin"])
def test_the_lost_limb_with_51_states_and_on_the_pinhole_camera(gpu_lib, golden_dir, name):
    """Cases 5 (PT = 64: the covariance tests' skeleton with five more parts) and 6 (pinhole)."""
    from acinoset_amd import build
    c = ucases.solved(golden_dir, name)
    if name == "lost12p51":
        assert 48 < c["prob"].P <= 64
    out = build.model_covariance([c["model"]], [c["x"]], pin_unobserved=True)[0]
    _compare(out, c, name)
    assert len(out["unobserved"]) == 6


@pytest.mark.parametrize("name", ["shipped12", "lost12"])
def test_samples_hold_the_unobserved_states(gpu_lib, golden_dir, name):
    """Case 7: S = 8 with the caller's z.  x_samples = x + L^-T z of the pinned matrix within the sample bar, delta exactly 0 at
    the unobserved states (z is not), pos_samples the forward kinematics of every sample, and the same bits alone or as one
    clip of four."""
    from acinoset_amd import build
    c = ucases.solved(golden_dir, name)
    r, act, model, x = c["ref"], c["prob"].ACT, c["model"], c["x"]
    z = np.random.default_rng(5).standard_normal((8,) + r["fixed"].shape)
    ref = sref.reference(r["ab"], r["fixed"], z)               # (d0 <= 1e-8 asserted there)
    one = build.model_samples([model], [x], z=z[None], pin_unobserved=True)[0]
    delta = one["x_samples"][:, :, act] - x[None, :, act]
    e_d, e_b = sref.map_err(delta, ref["dense"]), sref.map_err(delta, ref["banded"])
    print(f"{name}: S 8, d0 {ref['d0']:.2e}, bar {ref['bar']:.2e}; vs dense {e_d:.2e}, vs banded {e_b:.2e}")
    assert one["status"] == 0 and one["unobserved"] == _unobserved(c)
    assert e_d <= ref["bar"] and e_b <= ref["bar"]
    un = r["unobserved"]
    assert np.all(z[:, :, un] != 0) and np.all(delta[:, :, un] == 0)
    xs = one["x_samples"]
    want = osk.skeleton_fk(c["sk"], xs.reshape(-1, xs.shape[-1]))[0].reshape(one["pos_samples"].shape)
    e_fk, tol_fk = np.abs(one["pos_samples"] - want).max(), 1e-13 * max(1.0, np.abs(want).max())
    print(f"  pos_samples against the oracle's FK of x_samples {e_fk:.2e} (tolerance {tol_fk:.2e})")
    assert e_fk <= tol_fk
    if name == "lost12":
        others, xo = _windows(golden_dir, c, (105, 150, 195))
    else:
        others, xo = [copy.copy(model) for _ in range(3)], [cases.iterate(ucases.scases.fixture(golden_dir)[0], model, seed=k + 1)
                                                            for k in range(3)]
    z4 = np.random.default_rng(6).standard_normal((4,) + z.shape)
    z4[2] = z
    four = build.model_samples(others[:2] + [model] + others[2:], xo[:2] + [x] + xo[2:], z=z4, pin_unobserved=True)
    assert four[2]["status"] == 0 and four[2]["unobserved"] == one["unobserved"]
    for key in ("x_samples", "pos_samples"):
        assert np.array_equal(four[2][key], one[key]), key
    with pytest.raises(RuntimeError):
        build.model_samples([model], [x], z=z[None])           # without the keyword: singular, as ever


def test_model_observability_alone(gpu_lib, golden_dir):
    """Case 8: info within 1e-12 relative of the reference's sums (an entry the reference has at exactly 0 must be 0), n_seen
    and the mask exact, the same bits in a batch and alone; both camera models; the shipped skeleton."""
    from acinoset_amd import build
    lost, two = ucases.case(golden_dir, "lost12"), ucases.case(golden_dir, "two12")
    others, xo = _windows(golden_dir, lost, (105, 195))
    refs = [uref.reference(cases.problem(lost["sk"], m, lost["scene"]), xf[:, lost["prob"].ACT]) for m, xf in zip(others, xo)]
    models, xs = [others[0], lost["model"], two["model"], others[1]], [xo[0], lost["x"], two["x"], xo[1]]
    refs = [refs[0], lost["ref"], two["ref"], refs[1]]
    batch = build.model_observability(models, xs)
    act = lost["prob"].ACT
    inact = np.setdiff1d(np.arange(lost["model"].P), act)
    for k, (ob, r) in enumerate(zip(batch, refs)):
        info = ob["info"][act]
        pos = r["info"] > 0
        e = float(np.max(np.abs(info[pos] - r["info"][pos]) / r["info"][pos]))
        print(f"clip {k}: info vs the reference {e:.2e} relative; largest info where the reference has 0: {np.abs(info[~pos]).max(initial=0.0):.2e}; "
              f"unobserved {ob['unobserved']}; n_seen {ob['n_seen'][act].min()} .. {ob['n_seen'][act].max()}")
        assert e <= 1e-12 and np.all(info[~pos] == 0)
        assert np.array_equal(ob["n_seen"][act], r["n_seen"]) and ob["n_seen"].dtype == np.int32
        assert ob["unobserved"] == [int(a) for a in act[r["unobserved"]]]
        assert np.all(ob["info"][inact] == 0) and np.all(ob["n_seen"][inact] == 0)
        alone = build.model_observability([models[k]], [xs[k]])[0]
        assert np.array_equal(alone["info"], ob["info"]) and np.array_equal(alone["n_seen"], ob["n_seen"])
        assert alone["unobserved"] == ob["unobserved"]
    for name in ("shipped12", "lost12pin"):
        c = ucases.case(golden_dir, name)
        ob = build.model_observability([c["model"]], [c["x"]])[0]
        a, r = c["prob"].ACT, c["ref"]
        pos = r["info"] > 0
        e = float(np.max(np.abs(ob["info"][a][pos] - r["info"][pos]) / r["info"][pos]))
        print(f"{name}: info vs the reference {e:.2e} relative; at the reference's zeros {np.abs(ob['info'][a][~pos]).max(initial=0.0):.2e}")
        assert e <= 1e-12 and np.all(ob["info"][a][~pos] == 0)
        assert np.array_equal(ob["n_seen"][a], r["n_seen"]) and ob["unobserved"] == _unobserved(c)


def test_reprojection_with_the_keyword(gpu_lib, golden_dir):
    """Case 9: on the lost limb cov_uv and mahal2 are NaN exactly at the two dependent slots and finite elsewhere where the
    detection is finite; the shipped skeleton gets cov_status 0 and a finite mahal2 wherever res is finite."""
    from acinoset_amd import build
    c = ucases.case(golden_dir, "lost12")
    rep = build.model_reprojection([c["model"]], [c["x"]], cov=True, pin_unobserved=True)[0]
    dep = c["ref"]["dependent"][0]
    assert rep["cov_status"] == 0 and rep["unobserved"] == _unobserved(c)
    res_ok, uv_ok = np.isfinite(rep["res"]).all(-1), np.isfinite(rep["uv"]).all(-1)
    assert res_ok[:, :, dep].any() and res_ok[:, :, ~dep].any()
    assert np.isnan(rep["mahal2"][:, :, dep]).all() and np.isnan(rep["cov_uv"][:, :, dep]).all()
    assert np.array_equal(np.isfinite(rep["mahal2"][:, :, ~dep]), res_ok[:, :, ~dep])
    assert np.array_equal(np.isfinite(rep["cov_uv"][:, :, ~dep]).all((-1, -2)), uv_ok[:, :, ~dep])
    s = ucases.case(golden_dir, "shipped12")
    rep = build.model_reprojection([s["model"]], [s["x"]], cov=True, pin_unobserved=True)[0]
    assert rep["cov_status"] == 0 and rep["unobserved"] == [33, 43]
    assert np.isfinite(rep["res"]).all(-1).any()
    assert np.array_equal(np.isfinite(rep["mahal2"]), np.isfinite(rep["res"]).all(-1))
    assert build.model_reprojection([s["model"], s["model"]], [s["x"], s["x"]], cov=True)[0]["cov_status"] == 5


def test_video_of_the_shipped_skeleton(gpu_lib, golden_dir):
    """Case 10: solve_video(return_cov=True, pin_unobserved=True) on the 300 shipped frames of the covariance tests, the shipped
    skeleton itself: every window whose unobserved states are [33, 43] and whose status is 0 has finite bars.  How many windows
    stay singular is printed, not asserted."""
    from acinoset_amd import build
    g, sk = cases.load(golden_dir)
    full = np.load(os.path.join(golden_dir, "human_dlc_full.npz"))
    tabs = [(list(full["parts"]), full[f"det{c}"].astype(np.float64)) for c in range(2)]
    res, infos, starts = build.solve_video(sk, scene=(g["K"], g["D"], g["R"], g["t"]), dlc_tables=tabs, first_frame=0, last_frame=299,
                                           window=100, overlap=20, pairing="name", max_iter=40, warm_passes=0, return_cov=True,
                                           pin_unobserved=True)
    status = [i["cov_status"] for i in infos]
    print(f"windows {len(starts)}: cov_status {status}, cov_unobserved {res['cov_unobserved']}, still singular "
          f"{len(res['cov_singular_windows'])} of {len(starts)}")
    assert len(res["cov_unobserved"]) == len(starts) == 4
    assert res["cov_singular_windows"] == [k for k, s in enumerate(status) if s == 5]
    assert all(set([33, 43]) <= set(u) for u in res["cov_unobserved"])
    for k, (u, s) in enumerate(zip(res["cov_unobserved"], status)):
        if u == [33, 43] and s == 0:
            assert np.isfinite(res["window_std_pos"][k]).all(), k
            mine = res["owner"] == k
            assert np.isfinite(res["std_pos"][mine]).all() and np.isfinite(res["cov_pos"][mine]).all()
