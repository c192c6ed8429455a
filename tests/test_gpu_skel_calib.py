"""GPU (-m gpu): acino_skel_fte_calibration_sensitivity (csrc/skel_calib.hip: k_skel_calib_rhs, k_skel_fwdsub, k_skel_calib_combine;
k_skel_factor and k_skel_sample_back of csrc/skel_sample.hip) through build.model_calibration_sensitivity and the ``cov_cams``
keyword of the solve entries, against the CPU references of tests/skel_calib_ref.py.

    e = fte_calib_ref.col_err(S_gpu, S_ref1)  <=  bar(d0) = max(64 d0, 1e-13),   d0 = col_err(S_ref2, S_ref1) on the very input
    (reference 1: banded Cholesky, reference 2: dense LU);   d0 > 1e-8 is refused

Measured on the MI355X (d0 -> e against reference 1): pt16 2.9e-9 -> 1.1e-9, pt32 3.6e-9 -> 3.9e-9, slice12 1.9e-9 -> 1.1e-9,
slice40 8.3e-10 -> 1.3e-9, p51 1.9e-9 -> 2.0e-9, slice40pin 4.3e-10 -> 4.8e-10, pt16pin 1.9e-9 -> 1.1e-9; 12 cameras 1.1e-9 ->
1.1e-9; 210 pins 5.6e-11 -> 5.2e-11.
The inputs are those of tests/skel_sample_cases.py and tests/skel_unobs_cases.py."""
import copy

import numpy as np
import pytest

import fte_calib_ref as fref
import skel_calib_ref as kref
import skel_cov_cases as cases
import skel_cov_ref as cref
import skel_sample_cases as scases
import skel_sample_ref as sref
import skel_unobs_cases as ucases

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
_REF = {}


def _ref(golden_dir, name):
    """The two reference solves of an input of skel_sample_cases, once per process."""
    if name not in _REF:
        c = scases.case(golden_dir, name)
        _REF[name] = kref.reference(c["prob"], c["x"][:, c["prob"].ACT], c["ab"], c["fixed"])
    return _REF[name]


def _sens(out, act):
    return out["sens_cams"][:, act]


def _check_sens(label, S, r):
    e1, e2 = kref.col_err(S, r["S1"]), kref.col_err(S, r["S2"])
    print(f"{label}: d0 {r['d0']:.2e}, bar {r['bar']:.2e}; e vs banded {e1:.2e}, vs dense {e2:.2e}")
    assert r["d0"] <= kref.D0_REFUSED
    assert e1 <= r["bar"] and e2 <= r["bar"]


@pytest.mark.parametrize("name", ["pt16", "pt32", "slice12", "slice40", "p51", "slice40pin", "pt16pin"])
def test_sensitivity_against_both_references(gpu_lib, golden_dir, name):
    from acinoset_amd import build
    c, r = scases.case(golden_dir, name), _ref(golden_dir, name)
    act = c["prob"].ACT
    out = build.model_calibration_sensitivity([c["model"]], [c["x"]])[0]
    N, P = c["x"].shape
    assert out["status"] == 0 and out["sens_cams"].shape == (N, P, 6 * c["prob"].C)
    assert out["cov_x_calib"] is None and out["cov_pos_calib"] is None and out["std_pos_calib"] is None
    assert np.all(out["sens_cams"][:, np.setdiff1d(np.arange(P), act)] == 0)
    _check_sens(f"{name}: PT {(len(act) + 15) // 16 * 16}, N {N}", _sens(out, act), r)
    assert np.all(_sens(out, act)[c["fixed"]] == 0)


T_OFFSETS = np.array([[0, 0, 0], [0.03, 0, 0], [0, 0.03, 0], [0, 0, 0.03], [-0.02, 0.02, 0], [0.02, 0, -0.02]], dtype=np.float64)


def test_two_column_panels_on_a_rig_of_twelve_cameras(gpu_lib, golden_dir):
    """The pt16 sub-tree (6 pose slots) seen by the fixture's two cameras six times each, the copies' t moved by T_OFFSETS, the
    detections repeated: 72 columns = one full panel of 64 and a ragged one of 8."""
    from acinoset_amd import build
    g, sk0, det = scases.fixture(golden_dir)
    sk = cases.sub_skeleton(cases.generic_skeleton(sk0), cases.SUB_TREES[16])
    K, D, R, t = scases.scene(g)
    rep = np.repeat(np.arange(len(K)), len(T_OFFSETS))
    t12 = np.asarray(t, dtype=np.float64)[rep] + np.tile(T_OFFSETS, (len(K), 1)).reshape((len(rep),) + np.asarray(t).shape[1:])
    scene = (np.asarray(K)[rep], np.asarray(D)[rep], np.asarray(R)[rep], t12)
    model = cases.make_model(g, sk, det[:, rep], 12, cases.SLICE_STARTS[0], "fisheye", scene)
    x = cases.iterate(g, model)
    prob = cases.problem(sk, model, scene)
    xa = x[:, prob.ACT]
    ab, fixed = sref.system(prob, xa)
    r = kref.reference(prob, xa, ab, fixed)
    assert r["d0"] <= 1e-8 and prob.C == 12
    out = build.model_calibration_sensitivity([model], [x])[0]
    assert out["status"] == 0 and out["sens_cams"].shape[2] == 72
    _check_sens("pt16 on 12 cameras (72 columns)", _sens(out, prob.ACT), r)


def _tight(model, x, which):
    """Limits closed onto the iterate for the variables ``which`` [N, P_active] (so that they sit AT a bound)."""
    m = copy.copy(model)
    act = np.asarray(model.active)
    lo, hi = model.lo.copy(), model.hi.copy()
    la, ha = lo[:, act], hi[:, act]
    la[which], ha[which] = x[:, act][which], x[:, act][which] + 1.0
    lo[:, act], hi[:, act] = la, ha
    m.lo, m.hi = lo, hi
    return m


def test_pinned_rows_are_exactly_zero(gpu_lib, golden_dir):
    """Every third variable of slice40 gets its lower limit ON the iterate; those the oracle finds bound-active (not none, not
    all) have S == 0 exactly, the rest matches the references of the pinned matrix."""
    from acinoset_amd import build
    c = scases.case(golden_dir, "slice40")
    model, x, prob0 = c["model"], c["x"], c["prob"]
    which = np.zeros((model.N, prob0.P), dtype=bool)
    which.reshape(-1)[::3] = True
    m = _tight(model, x, which)
    prob = cases.problem(c["sk"], m, c["scene"])
    xa = x[:, prob.ACT]
    ab, fixed = sref.system(prob, xa)
    assert 0 < fixed.sum() < which.sum() and not (fixed & ~which).any()
    r = kref.reference(prob, xa, ab, fixed)
    assert np.abs(r["G"][fixed]).max() > 0                    # (the cross term itself is not zero there: the pin makes the row zero)
    out = build.model_calibration_sensitivity([m], [x], fref.random_psd(2))[0]
    S = _sens(out, prob.ACT)
    _check_sens(f"slice40, {int(fixed.sum())} pins", S, r)
    assert np.all(S[fixed] == 0)
    cx = out["cov_x_calib"][:, prob.ACT[:, None], prob.ACT[None, :]]
    assert np.all(cx[fixed] == 0) and np.all(np.swapaxes(cx, 1, 2)[fixed] == 0)


@pytest.mark.parametrize("name", ["slice40", "pt16pin"])
def test_translating_the_rig_moves_the_trajectory(gpu_lib, golden_dir, name):
    """gen = [0, -R_c a]_c leaves every pixel where it is when the whole trajectory moves by a: S_n gen = (a, 0, ..., 0)."""
    from acinoset_amd import build
    c, r = scases.case(golden_dir, name), _ref(golden_dir, name)
    assert not c["fixed"][:, :3].any()                        # no root state of the case is pinned
    S = _sens(build.model_calibration_sensitivity([c["model"]], [c["x"]])[0], c["prob"].ACT)
    for a in 0.01 * np.eye(3):
        d_id = kref.identity_error(r["S1"], c["prob"].R, a) / 0.01
        e = kref.identity_error(S, c["prob"].R, a) / 0.01
        print(f"{name}: a = {a}: the reference's own error in the identity d_id {d_id:.2e}, bar {kref.bar(d_id):.2e}; GPU {e:.2e}")
        assert e <= kref.bar(d_id)


def _rel(a, b):
    return float(np.abs(np.asarray(a) - b).max() / np.abs(b).max())


@pytest.mark.parametrize("name", ["slice40", "p51", "pt16pin"])
def test_covariances(gpu_lib, golden_dir, name):
    """cov_x_calib, cov_pos_calib, std_pos_calib against S1 Sigma S1^T through the oracle pose Jacobian; Sigma is only PSD (camera
    0 held: zero rows).  Per output the bar is 64 x what the two references make of it (floor 1e-13)."""
    from acinoset_amd import build
    c, r = scases.case(golden_dir, name), _ref(golden_dir, name)
    prob, act = c["prob"], c["prob"].ACT
    xa = c["x"][:, act]
    sigma = fref.random_psd(2)
    assert np.all(sigma[:6] == 0) and np.all(sigma[:, :6] == 0)
    want, other = kref.calib_cov(r["S1"], sigma, prob, xa), kref.calib_cov(r["S2"], sigma, prob, xa)
    out = build.model_calibration_sensitivity([c["model"]], [c["x"]], sigma)[0]
    got = (out["cov_x_calib"][:, act[:, None], act[None, :]], out["cov_pos_calib"], out["std_pos_calib"])
    assert out["status"] == 0
    for key, g_, w_, o_ in zip(("cov_x_calib", "cov_pos_calib", "std_pos_calib"), got, want, other):
        d0, e = _rel(o_, w_), _rel(g_, w_)
        print(f"{name}: {key}: d0 {d0:.2e}, bar {kref.bar(d0):.2e}; e {e:.2e}")
        assert e <= kref.bar(d0)
    assert np.array_equal(out["cov_x_calib"], np.swapaxes(out["cov_x_calib"], 1, 2))
    assert np.array_equal(out["cov_pos_calib"], np.swapaxes(out["cov_pos_calib"], 2, 3))
    tr = np.einsum("nlii->nl", out["cov_pos_calib"])
    assert np.all(np.abs(out["std_pos_calib"] ** 2 - tr) <= 4 * EPS * np.abs(tr))
    alone = build.model_calibration_sensitivity([c["model"]], [c["x"]])[0]
    assert np.array_equal(alone["sens_cams"], out["sens_cams"])
    assert np.all(out["sens_cams"][:, np.setdiff1d(np.arange(c["model"].P), act)] == 0)


def _unobs_reference(c):
    r = c["ref"]
    xa = c["x"][:, c["prob"].ACT]
    return kref.reference(c["prob"], xa, r["ab"], r["fixed"])


@pytest.mark.parametrize("name", ["shipped12", "lost12"])
def test_pin_unobserved(gpu_lib, golden_dir, name):
    """The shipped human skeleton (two psi states no pixel sees: every bar finite) and the lost limb (six states; the two poses
    that depend on them +inf / NaN): status 0, ``unobserved`` listed, S and cov_x_calib exactly 0 in those rows; without the flag
    status 5 and NaN everywhere."""
    from acinoset_amd import build
    c = ucases.case(golden_dir, name)
    model, x, act, ur = c["model"], c["x"], c["prob"].ACT, c["ref"]
    r = _unobs_reference(c)
    sigma = fref.random_psd(2)
    out = build.model_calibration_sensitivity([model], [x], sigma, pin_unobserved=True)[0]
    un = ucases.full_index(c, np.nonzero(ur["unobserved"])[0])
    assert out["status"] == 0 and out["unobserved"] == un and len(un) == (2 if name == "shipped12" else 6)
    _check_sens(f"{name}, unobserved {un}", _sens(out, act), r)
    assert np.all(out["sens_cams"][:, un] == 0)
    assert np.all(out["cov_x_calib"][:, un, :] == 0) and np.all(out["cov_x_calib"][:, :, un] == 0)
    dep = ur["dependent"]
    want = kref.calib_cov(r["S1"], sigma, c["prob"], x[:, act])
    other = kref.calib_cov(r["S2"], sigma, c["prob"], x[:, act])
    d0, e = _rel(other[2][~dep], want[2][~dep]), _rel(out["std_pos_calib"][~dep], want[2][~dep])
    print(f"{name}: std_pos_calib on the {int((~dep[0]).sum())} determined slots: d0 {d0:.2e}, bar {kref.bar(d0):.2e}; e {e:.2e}")
    assert e <= kref.bar(d0)
    assert np.array_equal(np.isposinf(out["std_pos_calib"]), dep) and np.isfinite(out["std_pos_calib"][~dep]).all()
    nan9 = np.isnan(out["cov_pos_calib"]).reshape(dep.shape + (9,))
    assert np.array_equal(nan9.all(-1), dep) and np.array_equal(nan9.any(-1), dep)
    assert dep.any() == (name == "lost12")
    off = build.model_calibration_sensitivity([model, model], [x, x], sigma)
    assert [o["status"] for o in off] == [5, 5] and all("unobserved" not in o for o in off)
    for key in ("cov_pos_calib", "std_pos_calib"):
        assert np.isnan(off[0][key]).all(), key
    assert np.isnan(off[0]["sens_cams"][:, act]).all() and np.isnan(off[0]["cov_x_calib"][:, act[:, None], act[None, :]]).all()
    with pytest.raises(RuntimeError):
        build.model_calibration_sensitivity([model], [x], sigma)


KEYS = ("sens_cams", "cov_x_calib", "cov_pos_calib", "std_pos_calib")


def test_batch_and_repeatability(gpu_lib, golden_dir):
    """Eight clips in one call equal the clips one by one, bit for bit; a singular clip in a batch leaves the others standing; a
    second call repeats the first; model_covariance and model_samples (fixed z) return the same bits before and after."""
    from acinoset_amd import build
    c = scases.case(golden_dir, "slice40")
    g, _sk0, det = scases.fixture(golden_dir)
    models = [cases.make_model(g, c["sk"], det, 40, 60 + 45 * k) for k in range(8)]
    xs = [cases.iterate(g, m, seed=k) for k, m in enumerate(models)]
    sigma = fref.random_psd(2)
    z = np.random.default_rng(3).standard_normal((1, 3, 40, len(c["prob"].ACT)))
    cov0 = build.model_covariance([models[0]], [xs[0]])[0]
    smp0 = build.model_samples([models[0]], [xs[0]], z=z)[0]
    batch = build.model_calibration_sensitivity(models, xs, sigma)
    again = build.model_calibration_sensitivity(models, xs, sigma)
    for k in range(8):
        one = build.model_calibration_sensitivity([models[k]], [xs[k]], sigma)[0]
        assert batch[k]["status"] == 0
        for key in KEYS:
            assert np.array_equal(one[key], batch[k][key]), (k, key)
            assert np.array_equal(again[k][key], batch[k][key]), (k, key)
    bad = copy.copy(models[2])
    names = list(bad.names)
    bad.weights = models[2].weights.copy()
    bad.weights[:, :, [names.index("elbow1"), names.index("wrist1")]] = 0.0
    mixed = build.model_calibration_sensitivity(models[:2] + [bad] + models[3:4], xs[:4], sigma)
    assert [o["status"] for o in mixed] == [0, 0, 5, 0]
    act = c["prob"].ACT
    assert np.isnan(mixed[2]["sens_cams"][:, act]).all() and np.isnan(mixed[2]["std_pos_calib"]).all()
    for k in (0, 1, 3):
        for key in KEYS:
            assert np.array_equal(mixed[k][key], batch[k][key]), (k, key)
    cov1 = build.model_covariance([models[0]], [xs[0]])[0]
    smp1 = build.model_samples([models[0]], [xs[0]], z=z)[0]
    for key in ("cov_x", "cov_pos", "std_pos"):
        assert np.array_equal(cov0[key], cov1[key]), key
    for key in ("x_samples", "pos_samples"):
        assert np.array_equal(smp0[key], smp1[key]), key


def test_solve_entries(gpu_lib, golden_dir):
    """``cov_cams`` on solve_models / solve_model / solve_video: exactly the four keys (plus std_pos_total with return_cov), equal
    to model_calibration_sensitivity at the returned x; without it the key sets are what they were; the dict of sba.covariance
    is accepted by its "cov_cams"; solve_video gives every frame the arrays of the window that supplied it."""
    from acinoset_amd import build
    c = scases.case(golden_dir, "slice40")
    model, x = c["model"], c["x"]
    sigma = fref.random_psd(2)
    (r0, i0), = build.solve_models([model], [x], max_iter=4, return_cov=True)
    (r1, i1), = build.solve_models([model], [x], max_iter=4, return_cov=True, cov_cams=sigma)
    (r2, _i2), = build.solve_models([model], [x], max_iter=4, cov_cams=dict(cov_cams=sigma, cov_points=None))
    (r3, _i3), = build.solve_models([model], [x], max_iter=4)
    assert i0 == i1 and sorted(r3) == ["ddx", "dx", "positions", "x"]
    assert sorted(r0) == ["cov_pos", "cov_x", "ddx", "dx", "positions", "std_pos", "x"]
    assert set(r1) - set(r0) == set(KEYS) | {"std_pos_total"} and set(r2) - set(r3) == set(KEYS)
    assert all(np.array_equal(r0[k], r1[k]) for k in r0)
    direct = build.model_calibration_sensitivity([model], [r1["x"]], sigma)[0]
    for key in KEYS:
        assert np.array_equal(r1[key], direct[key]) and np.array_equal(r2[key], direct[key]), key
    want = np.sqrt(r1["std_pos"] ** 2 + r1["std_pos_calib"] ** 2)
    assert np.all(np.abs(r1["std_pos_total"] - want) <= 4 * EPS * want)
    r4, _i4 = build.solve_model(model, x0=x, max_iter=4, cov_cams=sigma)
    assert all(np.array_equal(r4[key], r2[key]) for key in KEYS)
    # ---- the video: two windows of 40 over 70 frames
    g, sk0, det = scases.fixture(golden_dir)
    sk = cases.generic_skeleton(sk0)
    kw = dict(scene=scases.scene(g), dlc_tables=cases.tables(det, g["parts"]), first_frame=60, last_frame=129, window=40, overlap=10,
              pairing="name", r_meas=cases.R_MEAS_TEST, max_iter=15, warm_passes=0)
    plain, _i, starts = build.solve_video(sk, return_cov=True, **kw)
    res, infos, _s = build.solve_video(sk, return_cov=True, cov_cams=sigma, **kw)
    assert starts == [60, 90] and set(res) - set(plain) == set(KEYS) | {"std_pos_total"}
    assert all(np.array_equal(plain[k], res[k], equal_nan=True) for k in ("positions", "x", "std_pos", "cov_pos"))
    P, L = res["x"].shape[1], res["positions"].shape[1]
    assert res["sens_cams"].shape == (70, P, 12) and res["cov_x_calib"].shape == (70, P, P)
    assert res["cov_pos_calib"].shape == (70, L, 3, 3) and res["std_pos_calib"].shape == (70, L)
    assert [i["cov_status"] for i in infos] == [0, 0] and np.isfinite(res["std_pos_total"]).all()
    want = np.sqrt(res["std_pos"] ** 2 + res["std_pos_calib"] ** 2)
    assert np.all(np.abs(res["std_pos_total"] - want) <= 4 * EPS * want)
    # every frame's rows are those of the window that owns it: the windows' own calls at the windows' own iterates
    models = [cases.make_model(g, sk, det, 40, st) for st in starts]
    for w_i, st in enumerate(starts):
        mine = np.nonzero(res["owner"] == w_i)[0]
        assert mine.size > 0
        # cov_pos_calib of a frame is G_l(x_f) cov_x_calib[f] G_l(x_f)^T with the frame's own x: rows of one and the same window
        prob = cases.problem(sk, models[w_i], kw["scene"])
        G = cref.pose_jacobian(prob, res["x"][st - 60:st - 60 + 40][:, prob.ACT])[mine - (st - 60)]
        cx = res["cov_x_calib"][mine][:, prob.ACT[:, None], prob.ACT[None, :]]
        cp = np.einsum("nlip,npq,nljq->nlij", G, cx, G)
        e = _rel(res["cov_pos_calib"][mine], cp)
        print(f"video window {w_i}: {mine.size} frames, cov_pos_calib against G cov_x_calib G^T at the stitched x {e:.2e}")
        assert e <= 1e-10
        for a in 0.01 * np.eye(3):      # and every frame's S is a row of a valid sensitivity (the bar of the worst accepted input)
            assert kref.identity_error(res["sens_cams"][mine][:, prob.ACT], prob.R, a) <= kref.bar(kref.D0_REFUSED) * 0.01


def test_null_output_subsets(gpu_lib, golden_dir):
    """The C entry with outputs left NULL, which the Python layer never does (pt16: 12 frames, PT 16): ``d_sens`` alone without a
    Sigma - the combine returns after S_n - and ``d_std_pos_cal`` alone with one.  What comes back is the full call's, bit for bit."""
    import ctypes as C

    import torch
    from acinoset_amd import build
    from acinoset_amd._lib import check, lib, ptr
    c = scases.case(golden_dir, "pt16")
    model, x, act = c["model"], c["x"], c["prob"].ACT
    sigma = fref.random_psd(2)
    full = build.model_calibration_sensitivity([model], [x], sigma)[0]
    io_ = build._skel_inputs([model], [x], lambda p, B: lib().acino_skel_fte_calibration_workspace_bytes(C.byref(p), B, 0), l1_eps=1e-2)
    N, L, W = model.N, len(model.names), 6 * c["prob"].C
    empty = lambda *shape: torch.empty((1, N) + shape, dtype=torch.float64, device=io_["dev"])   # noqa: E731
    sig_d = torch.as_tensor(sigma, dtype=torch.float64, device=io_["dev"]).contiguous()
    status, null = (C.c_int32 * 1)(), ptr(None)
    sens = empty(len(act), W)
    check(lib().acino_skel_fte_calibration_sensitivity(*io_["head"], null, ptr(sens), null, null, null, status, *io_["tail"], 0, null))
    assert status[0] == 0 and np.array_equal(sens[0].cpu().numpy(), full["sens_cams"][:, act])
    std = empty(L)
    check(lib().acino_skel_fte_calibration_sensitivity(*io_["head"], ptr(sig_d), null, null, null, ptr(std), status, *io_["tail"], 0, null))
    assert status[0] == 0 and np.array_equal(std[0].cpu().numpy(), full["std_pos_calib"])
