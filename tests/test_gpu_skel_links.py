"""GPU (-m gpu): acino_skel_fte_link_sensitivity (csrc/skel_links.hip: k_skel_links_rhs, k_skel_links_combine; k_skel_factor and
k_skel_sample_back of csrc/skel_sample.hip, k_skel_fwdsub of csrc/skel_calib.hip) through build.model_link_sensitivity and the
``cov_links`` / ``link_groups`` keywords of the solve entries, against the CPU references of tests/skel_links_ref.py.

    e = col_err(S_gpu, S_ref1)  <=  bar(d0) = max(64 d0, 1e-13),   d0 = col_err(S_ref2, S_ref1) on the very input
    (reference 1: banded Cholesky, reference 2: dense LU);   d0 > 1e-8 is refused

Measured on the MI355X (d0 -> e against reference 1): pt16 3.4e-9 -> 2.0e-9, pt32 3.8e-9 -> 4.1e-9, slice12 1.5e-9 -> 3.1e-9,
slice40 "global" 3.4e-10 -> 1.3e-9, p51 1.9e-9 -> 1.8e-9, slice40pin 9.6e-10 -> 1.1e-9, pt16pin 4.3e-9 -> 1.5e-9; 210 pins
4.2e-11 -> 7.6e-11; dpos_links 2.8e-11 .. 1.5e-10 against bars of 1.4e-9 .. 8.1e-9; cov_pos_links without the direct term is off by
10 to 37 %.
The inputs are those of tests/skel_sample_cases.py and tests/skel_unobs_cases.py."""
import copy

import numpy as np
import pytest

import skel_cov_cases as cases
import skel_cov_ref as cref
import skel_links_ref as lkref
import skel_sample_cases as scases
import skel_sample_ref as sref
import skel_unobs_cases as ucases

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
P51_GROUPS = np.arange(20) % 16
GROUPS = {"pt16": "links", "pt32": "links", "slice12": "links", "slice40": "global", "p51": P51_GROUPS, "slice40pin": "links",
          "pt16pin": "links"}
N_GROUPS = {"pt16": 5, "pt32": 8, "slice12": 15, "slice40": 1, "p51": 16, "slice40pin": 15, "pt16pin": 5}
KEYS = ("sens_links", "dpos_links", "cov_x_links", "cov_pos_links", "std_pos_links")
_REF = {}


def _ref(golden_dir, name, groups=None):
    """The two reference solves of an input of skel_sample_cases, once per process."""
    groups = GROUPS[name] if groups is None else groups
    key = (name, groups if isinstance(groups, str) else "array")
    if key not in _REF:
        c = scases.case(golden_dir, name)
        _REF[key] = lkref.reference(c["prob"], c["x"][:, c["prob"].ACT], c["ab"], c["fixed"], groups)
    return _REF[key]


def _rel(a, b):
    return float(np.abs(np.asarray(a) - b).max() / np.abs(b).max())


def _check_sens(label, out, act, r):
    S = out["sens_links"][:, act]
    e1, e2 = lkref.col_err(S, r["S1"]), lkref.col_err(S, r["S2"])
    print(f"{label}: d0 {r['d0']:.2e}, bar {r['bar']:.2e}; e vs banded {e1:.2e}, vs dense {e2:.2e}")
    assert r["d0"] <= lkref.D0_REFUSED
    assert e1 <= r["bar"] and e2 <= r["bar"]
    dT, eT = _rel(r["T2"], r["T1"]), _rel(out["dpos_links"], r["T1"])
    print(f"{label}: dpos_links: d0 {dT:.2e}, bar {lkref.bar(dT):.2e}; e {eT:.2e}")
    assert eT <= lkref.bar(dT)


@pytest.mark.parametrize("name", list(GROUPS))
def test_sensitivity_against_both_references(gpu_lib, golden_dir, name):
    from acinoset_amd import build
    c, r = scases.case(golden_dir, name), _ref(golden_dir, name)
    act, K = c["prob"].ACT, N_GROUPS[name]
    assert r["K"] == K
    if name == "p51":
        with pytest.raises(ValueError, match="explicit groups"):          # 20 links with an offset
            build.model_link_sensitivity([c["model"]], [c["x"]], "links")
    out = build.model_link_sensitivity([c["model"]], [c["x"]], GROUPS[name])[0]
    N, P = c["x"].shape
    L = len(c["model"].names)
    assert out["status"] == 0 and out["sens_links"].shape == (N, P, K) and out["dpos_links"].shape == (N, L, 3, K)
    assert out["cov_x_links"] is None and out["cov_pos_links"] is None and out["std_pos_links"] is None
    assert np.array_equal(out["groups"], r["grp"])
    assert np.all(out["sens_links"][:, np.setdiff1d(np.arange(P), act)] == 0)
    _check_sens(f"{name}: PT {(len(act) + 15) // 16 * 16}, N {N}, K {K}", out, act, r)
    assert np.all(out["sens_links"][:, act][c["fixed"]] == 0)


@pytest.mark.parametrize("name", ["slice12", "p51"])
def test_a_group_that_hangs_no_weighted_slot(gpu_lib, golden_dir, name):
    """Group 9 (the first definition of hip1, replaced by the second before any slot is hung below it): its column of G is
    exactly 0 in the reference, so S is exactly 0 there and T_l is the reference's direct term - on no slot's path, 0 as well."""
    from acinoset_amd import build
    c, r = scases.case(golden_dir, name), _ref(golden_dir, name)
    assert np.all(r["G"][:, :, 9] == 0) and np.abs(r["G"]).max(axis=(0, 1))[np.arange(r["K"]) != 9].min() > 0
    out = build.model_link_sensitivity([c["model"]], [c["x"]], GROUPS[name])[0]
    assert np.all(out["sens_links"][..., 9] == 0)
    assert np.array_equal(out["dpos_links"][..., 9], r["D"][..., 9])


def test_the_global_column_is_the_sum_of_the_links(gpu_lib, golden_dir):
    """Linearity on slice40: the "global" column equals the sum of the 15 per-link columns; the bar is that of the references' own
    sum, bar(d_sum) - A^-1 is applied linearly, so the summed columns and the global one share the error of the solve and its d0
    has no place here.  Measured: references 2.8e-12, GPU 2.0e-12 against 1.8e-10; dpos_links 3.8e-13, GPU 4.6e-13 against 2.5e-11."""
    from acinoset_amd import build
    c = scases.case(golden_dir, "slice40")
    act = c["prob"].ACT
    rg, rl = _ref(golden_dir, "slice40", "global"), _ref(golden_dir, "slice40", "links")
    d_sum = lkref.col_err(rl["S1"].sum(-1, keepdims=True), rg["S1"])
    glob = build.model_link_sensitivity([c["model"]], [c["x"]], "global")[0]
    link = build.model_link_sensitivity([c["model"]], [c["x"]], "links")[0]
    e = lkref.col_err(link["sens_links"][:, act].sum(-1, keepdims=True), glob["sens_links"][:, act])
    eT = _rel(link["dpos_links"].sum(-1, keepdims=True), glob["dpos_links"])
    dT = _rel(rl["T1"].sum(-1, keepdims=True), rg["T1"])
    print(f"slice40: sum of 15 columns against the global one: references {d_sum:.2e}, bar {lkref.bar(d_sum):.2e}; GPU {e:.2e}; "
          f"dpos: references {dT:.2e}, bar {lkref.bar(dT):.2e}; GPU {eT:.2e}")
    assert e <= lkref.bar(d_sum)
    assert eT <= lkref.bar(dT)


@pytest.mark.parametrize("name", ["slice40pin", "p51", "pt16pin"])
def test_covariances(gpu_lib, golden_dir, name):
    """cov_x_links, cov_pos_links, std_pos_links against S1 Sigma S1^T and T1 Sigma T1^T; Sigma is only PSD (group 0 held: zero
    row and column).  Per output the bar is 64 x what the two references make of it (floor 1e-13).  The reference WITHOUT the
    direct term D_l is further off than that: the test sees the term."""
    from acinoset_amd import build
    c, r = scases.case(golden_dir, name), _ref(golden_dir, name)
    act, K = c["prob"].ACT, r["K"]
    sigma = lkref.random_psd(K)
    assert np.all(sigma[0] == 0) and np.all(sigma[:, 0] == 0) and np.linalg.eigvalsh(sigma).min() > -1e-18
    want, other = lkref.link_cov(r["S1"], r["T1"], sigma), lkref.link_cov(r["S2"], r["T2"], sigma)
    out = build.model_link_sensitivity([c["model"]], [c["x"]], GROUPS[name], sigma)[0]
    got = (out["cov_x_links"][:, act[:, None], act[None, :]], out["cov_pos_links"], out["std_pos_links"])
    assert out["status"] == 0
    bars = {}
    for key, g_, w_, o_ in zip(("cov_x_links", "cov_pos_links", "std_pos_links"), got, want, other):
        d0, e = _rel(o_, w_), _rel(g_, w_)
        bars[key] = lkref.bar(d0)
        print(f"{name}: {key}: d0 {d0:.2e}, bar {bars[key]:.2e}; e {e:.2e}")
        assert e <= bars[key]
    no_direct = lkref.link_cov(r["S1"], r["T1"] - r["D"], sigma)
    for key, w_, m_ in (("cov_pos_links", want[1], no_direct[1]), ("std_pos_links", want[2], no_direct[2])):
        miss = _rel(m_, w_)
        print(f"{name}: {key} without D_l is off by {miss:.2e}")
        assert miss > bars[key]
    assert np.array_equal(out["cov_x_links"], np.swapaxes(out["cov_x_links"], 1, 2))
    assert np.array_equal(out["cov_pos_links"], np.swapaxes(out["cov_pos_links"], 2, 3))
    tr = np.einsum("nlii->nl", out["cov_pos_links"])
    assert np.all(np.abs(out["std_pos_links"] ** 2 - tr) <= 4 * EPS * np.abs(tr))
    alone = build.model_link_sensitivity([c["model"]], [c["x"]], GROUPS[name])[0]
    assert np.array_equal(alone["sens_links"], out["sens_links"]) and np.array_equal(alone["dpos_links"], out["dpos_links"])
    assert np.all(out["sens_links"][:, np.setdiff1d(np.arange(c["model"].P), act)] == 0)


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
    r = lkref.reference(prob, xa, ab, fixed, "links")
    assert np.abs(r["G"][fixed]).max() > 0                    # (the cross term itself is not zero there: the pin makes the row zero)
    out = build.model_link_sensitivity([m], [x], "links", lkref.random_psd(r["K"]))[0]
    _check_sens(f"slice40, {int(fixed.sum())} pins", out, prob.ACT, r)
    assert np.all(out["sens_links"][:, prob.ACT][fixed] == 0)
    cx = out["cov_x_links"][:, prob.ACT[:, None], prob.ACT[None, :]]
    assert np.all(cx[fixed] == 0) and np.all(np.swapaxes(cx, 1, 2)[fixed] == 0)


@pytest.mark.parametrize("name", ["shipped12", "lost12"])
def test_pin_unobserved(gpu_lib, golden_dir, name):
    """The shipped human skeleton (two psi states no pixel sees: every bar finite) and the lost limb (six states; the two poses
    that depend on them +inf / NaN): status 0, ``unobserved`` listed, S and cov_x_links exactly 0 in those rows; without the flag
    status 5 and NaN everywhere."""
    from acinoset_amd import build
    c = ucases.case(golden_dir, name)
    model, x, act, ur = c["model"], c["x"], c["prob"].ACT, c["ref"]
    r = lkref.reference(c["prob"], x[:, act], ur["ab"], ur["fixed"], "links")
    sigma = lkref.random_psd(r["K"])
    out = build.model_link_sensitivity([model], [x], "links", sigma, pin_unobserved=True)[0]
    un = ucases.full_index(c, np.nonzero(ur["unobserved"])[0])
    assert out["status"] == 0 and out["unobserved"] == un and len(un) == (2 if name == "shipped12" else 6)
    _check_sens(f"{name}, unobserved {un}", out, act, r)
    assert np.all(out["sens_links"][:, un] == 0)
    assert np.all(out["cov_x_links"][:, un, :] == 0) and np.all(out["cov_x_links"][:, :, un] == 0)
    dep = ur["dependent"]
    want, other = lkref.link_cov(r["S1"], r["T1"], sigma), lkref.link_cov(r["S2"], r["T2"], sigma)
    d0, e = _rel(other[2][~dep], want[2][~dep]), _rel(out["std_pos_links"][~dep], want[2][~dep])
    print(f"{name}: std_pos_links on the {int((~dep[0]).sum())} determined slots: d0 {d0:.2e}, bar {lkref.bar(d0):.2e}; e {e:.2e}")
    assert e <= lkref.bar(d0)
    assert np.array_equal(np.isposinf(out["std_pos_links"]), dep) and np.isfinite(out["std_pos_links"][~dep]).all()
    nan9 = np.isnan(out["cov_pos_links"]).reshape(dep.shape + (9,))
    assert np.array_equal(nan9.all(-1), dep) and np.array_equal(nan9.any(-1), dep)
    assert dep.any() == (name == "lost12")
    off = build.model_link_sensitivity([model, model], [x, x], "links", sigma)
    assert [o["status"] for o in off] == [5, 5] and all("unobserved" not in o for o in off)
    for key in ("dpos_links", "cov_pos_links", "std_pos_links"):
        assert np.isnan(off[0][key]).all(), key
    assert np.isnan(off[0]["sens_links"][:, act]).all() and np.isnan(off[0]["cov_x_links"][:, act[:, None], act[None, :]]).all()
    with pytest.raises(RuntimeError):
        build.model_link_sensitivity([model], [x], "links", sigma)


def test_unknown_groups(gpu_lib, golden_dir):
    """The dict of a length fit with two groups unobserved: +inf / NaN exactly on the slots below them (the slots whose direct
    term has a nonzero column there), S and T_l as without the mask, the other slots' bars those of the zeroed Sigma."""
    from acinoset_amd import build
    c, r = scases.case(golden_dir, "slice12"), _ref(golden_dir, "slice12")
    K = r["K"]
    full = lkref.random_psd(K, hold=1, seed=4)
    obs = np.ones(K, dtype=bool)
    obs[[5, 9]] = False                                       # (elbow1's link: elbow1 and wrist1 below it; group 9: no slot)
    fit = dict(cov_log_scales=full, observed=obs, groups=r["grp"])
    sigma = full.copy()
    sigma[~obs, :], sigma[:, ~obs] = 0.0, 0.0
    below = (np.abs(r["D"][0][..., ~obs]).max(axis=(1, 2)) > 0)                 # [L]: a slot of frame 0 below a flagged group
    assert below.sum() == 2
    masked = build.model_link_sensitivity([c["model"]], [c["x"]], None, fit)[0]
    plain = build.model_link_sensitivity([c["model"]], [c["x"]], "links", sigma)[0]
    assert np.array_equal(masked["groups"], r["grp"])
    for key in ("sens_links", "dpos_links", "cov_x_links"):
        assert np.array_equal(masked[key], plain[key]), key
    assert np.all(np.isposinf(masked["std_pos_links"][:, below])) and np.isnan(masked["cov_pos_links"][:, below]).all()
    assert np.array_equal(masked["std_pos_links"][:, ~below], plain["std_pos_links"][:, ~below])
    assert np.array_equal(masked["cov_pos_links"][:, ~below], plain["cov_pos_links"][:, ~below])
    assert np.isfinite(plain["std_pos_links"]).all()


def test_batch_and_repeatability(gpu_lib, golden_dir):
    """Eight clips in one call equal the clips one by one, bit for bit; a singular clip in a batch leaves the others standing; a
    second call repeats the first; model_covariance, model_samples (fixed z) and model_calibration_sensitivity return the same
    bits before and after."""
    import fte_calib_ref as fref
    from acinoset_amd import build
    c = scases.case(golden_dir, "slice40")
    g, _sk0, det = scases.fixture(golden_dir)
    models = [cases.make_model(g, c["sk"], det, 40, 60 + 45 * k) for k in range(8)]
    xs = [cases.iterate(g, m, seed=k) for k, m in enumerate(models)]
    sigma, sig_c = lkref.random_psd(15), fref.random_psd(2)
    z = np.random.default_rng(3).standard_normal((1, 3, 40, len(c["prob"].ACT)))
    cov0 = build.model_covariance([models[0]], [xs[0]])[0]
    smp0 = build.model_samples([models[0]], [xs[0]], z=z)[0]
    cal0 = build.model_calibration_sensitivity([models[0]], [xs[0]], sig_c)[0]
    batch = build.model_link_sensitivity(models, xs, "links", sigma)
    again = build.model_link_sensitivity(models, xs, "links", sigma)
    for k in range(8):
        one = build.model_link_sensitivity([models[k]], [xs[k]], "links", sigma)[0]
        assert batch[k]["status"] == 0
        for key in KEYS:
            assert np.array_equal(one[key], batch[k][key]), (k, key)
            assert np.array_equal(again[k][key], batch[k][key]), (k, key)
    bad = copy.copy(models[2])
    names = list(bad.names)
    bad.weights = models[2].weights.copy()
    bad.weights[:, :, [names.index("elbow1"), names.index("wrist1")]] = 0.0
    mixed = build.model_link_sensitivity(models[:2] + [bad] + models[3:4], xs[:4], "links", sigma)
    assert [o["status"] for o in mixed] == [0, 0, 5, 0]
    act = c["prob"].ACT
    assert np.isnan(mixed[2]["sens_links"][:, act]).all() and np.isnan(mixed[2]["std_pos_links"]).all()
    assert np.isnan(mixed[2]["dpos_links"]).all()
    for k in (0, 1, 3):
        for key in KEYS:
            assert np.array_equal(mixed[k][key], batch[k][key]), (k, key)
    cov1 = build.model_covariance([models[0]], [xs[0]])[0]
    smp1 = build.model_samples([models[0]], [xs[0]], z=z)[0]
    cal1 = build.model_calibration_sensitivity([models[0]], [xs[0]], sig_c)[0]
    for key in ("cov_x", "cov_pos", "std_pos"):
        assert np.array_equal(cov0[key], cov1[key]), key
    for key in ("x_samples", "pos_samples"):
        assert np.array_equal(smp0[key], smp1[key]), key
    for key in ("sens_cams", "cov_x_calib", "cov_pos_calib", "std_pos_calib"):
        assert np.array_equal(cal0[key], cal1[key]), key


def test_solve_entries(gpu_lib, golden_dir, monkeypatch):
    """``cov_links`` / ``link_groups`` on solve_models / solve_model / solve_video: exactly the five keys (plus std_pos_total with
    return_cov), equal to model_link_sensitivity at the returned x; without them the key sets and bits are what they were;
    std_pos_total with two and with three terms; solve_video gives every frame, bit for bit, the rows of a direct call on the
    window that owns it at that window's own iterate."""
    import fte_calib_ref as fref
    from acinoset_amd import build
    c = scases.case(golden_dir, "slice40")
    model, x = c["model"], c["x"]
    sigma, sig_c = lkref.random_psd(15), fref.random_psd(2)
    (r0, i0), = build.solve_models([model], [x], max_iter=4, return_cov=True)
    (r1, i1), = build.solve_models([model], [x], max_iter=4, return_cov=True, cov_links=sigma)
    (r2, _i2), = build.solve_models([model], [x], max_iter=4, cov_links=sigma, link_groups="links")
    (r3, _i3), = build.solve_models([model], [x], max_iter=4)
    (r5, _i5), = build.solve_models([model], [x], max_iter=4, return_cov=True, cov_links=sigma, cov_cams=sig_c)
    (r6, _i6), = build.solve_models([model], [x], max_iter=4, return_cov=True, cov_cams=sig_c)
    assert i0 == i1 and sorted(r3) == ["ddx", "dx", "positions", "x"]
    assert sorted(r0) == ["cov_pos", "cov_x", "ddx", "dx", "positions", "std_pos", "x"]
    assert set(r1) - set(r0) == set(KEYS) | {"std_pos_total"} and set(r2) - set(r3) == set(KEYS)
    assert set(r5) - set(r6) == set(KEYS) and "std_pos_total" in r6
    assert all(np.array_equal(r0[k], r1[k]) for k in r0)
    assert all(np.array_equal(r6[k], r5[k]) for k in r6 if k != "std_pos_total")
    direct = build.model_link_sensitivity([model], [r1["x"]], "links", sigma)[0]
    for key in KEYS:
        assert np.array_equal(r1[key], direct[key]) and np.array_equal(r2[key], direct[key]) and np.array_equal(r5[key], direct[key]), key
    want = np.sqrt(r1["std_pos"] ** 2 + r1["std_pos_links"] ** 2)
    assert np.all(np.abs(r1["std_pos_total"] - want) <= 4 * EPS * want)
    want3 = np.sqrt(r5["std_pos"] ** 2 + r5["std_pos_links"] ** 2 + r5["std_pos_calib"] ** 2)
    assert np.all(np.abs(r5["std_pos_total"] - want3) <= 4 * EPS * want3) and np.all(r5["std_pos_total"] >= r6["std_pos_total"])
    (rg, _ig), = build.solve_models([model], [x], max_iter=4, link_groups="global")
    assert rg["sens_links"].shape[2] == 1 and rg["cov_x_links"] is None and rg["std_pos_links"] is None
    r4, _i4 = build.solve_model(model, x0=x, max_iter=4, cov_links=sigma)
    assert all(np.array_equal(r4[key], r2[key]) for key in KEYS)
    # ---- the video: two windows of 40 over 70 frames
    g, sk0, det = scases.fixture(golden_dir)
    sk = cases.generic_skeleton(sk0)
    kw = dict(scene=scases.scene(g), dlc_tables=cases.tables(det, g["parts"]), first_frame=60, last_frame=129, window=40, overlap=10,
              pairing="name", r_meas=cases.R_MEAS_TEST, max_iter=15, warm_passes=0)
    plain, _i, starts = build.solve_video(sk, return_cov=True, **kw)
    handed = []                                                # the windows' models and iterates solve_video hands to its one call
    real_links = build._links

    def spy(models_, xs_, *a, **k):
        handed.append(([m for m in models_], [np.array(x_, copy=True) for x_ in xs_]))
        return real_links(models_, xs_, *a, **k)

    monkeypatch.setattr(build, "_links", spy)
    res, infos, _s = build.solve_video(sk, return_cov=True, cov_links=sigma, **kw)
    monkeypatch.setattr(build, "_links", real_links)
    assert len(handed) == 1 and len(handed[0][0]) == 2        # ONE batched call over both windows
    assert starts == [60, 90] and set(res) - set(plain) == set(KEYS) | {"std_pos_total"}
    assert all(np.array_equal(plain[k], res[k], equal_nan=True) for k in ("positions", "x", "std_pos", "cov_pos"))
    P, L = res["x"].shape[1], res["positions"].shape[1]
    assert res["sens_links"].shape == (70, P, 15) and res["cov_x_links"].shape == (70, P, P) and res["dpos_links"].shape == (70, L, 3, 15)
    assert res["cov_pos_links"].shape == (70, L, 3, 3) and res["std_pos_links"].shape == (70, L)
    assert [i["cov_status"] for i in infos] == [0, 0] and np.isfinite(res["std_pos_total"]).all()
    want = np.sqrt(res["std_pos"] ** 2 + res["std_pos_links"] ** 2)
    assert np.all(np.abs(res["std_pos_total"] - want) <= 4 * EPS * want)
    # every frame's rows are those of the window that owns it: a direct call on that window alone at its own iterate, bit for bit
    models = [cases.make_model(g, sk, det, 40, st) for st in starts]
    seen = 0
    for w_i, st in enumerate(starts):
        mine = np.nonzero(res["owner"] == w_i)[0]
        assert mine.size > 0
        seen += mine.size
        w_model, w_x = handed[0][0][w_i], handed[0][1][w_i]
        assert w_model.start_frame == st and np.array_equal(w_x[mine - (st - 60)], res["x"][mine])
        direct_w = build.model_link_sensitivity([w_model], [w_x], "links", sigma)[0]
        assert direct_w["status"] == 0
        for key in KEYS:
            assert np.array_equal(res[key][mine], direct_w[key][mine - (st - 60)]), (w_i, key)
        # T_l of a frame is G_l(x_f) S_f + D_l(x_f) with the frame's own x and S: rows of one and the same window
        prob = cases.problem(sk, models[w_i], kw["scene"])
        xa = res["x"][st - 60:st - 60 + 40][:, prob.ACT]
        grp, K = lkref.groups_of(prob.skel, "links")
        D = lkref.direct_term(prob, xa, grp, K)[mine - (st - 60)]
        Gl = cref.pose_jacobian(prob, xa)[mine - (st - 60)]
        T = np.einsum("nlip,npg->nlig", Gl, res["sens_links"][mine][:, prob.ACT]) + D
        e = _rel(res["dpos_links"][mine], T)
        cp = np.einsum("nlai,ij,nlbj->nlab", res["dpos_links"][mine], sigma, res["dpos_links"][mine])
        e2 = _rel(res["cov_pos_links"][mine], cp)
        e3 = _rel(res["cov_x_links"][mine], np.einsum("npi,ij,nqj->npq", res["sens_links"][mine], sigma, res["sens_links"][mine]))
        print(f"video window {w_i}: {mine.size} frames, dpos_links against G S + D at the stitched x {e:.2e}, cov_pos_links against "
              f"T Sigma T^T {e2:.2e}, cov_x_links against S Sigma S^T {e3:.2e}")
        assert e <= 1e-10 and e2 <= 1e-10 and e3 <= 1e-10
    assert seen == 70


def test_null_output_subsets(gpu_lib, golden_dir):
    """The C entry with outputs left NULL, which the Python layer never does (pt16: 12 frames, PT 16): ``d_dpos`` alone without a
    Sigma - the combine goes past S_n and cov_x to T_l - and ``d_sens`` with ``d_std_pos`` with one (no cov_x: T and T S_n^T are
    skipped).  What comes back is the full call's, bit for bit."""
    import ctypes as C

    import torch
    from acinoset_amd import build
    from acinoset_amd._lib import check, lib, ptr
    c = scases.case(golden_dir, "pt16")
    model, x, act = c["model"], c["x"], c["prob"].ACT
    grp, K = build.link_groups(model.prog, "links")
    sigma = lkref.random_psd(K)
    full = build.model_link_sensitivity([model], [x], "links", sigma)[0]
    io_ = build._skel_inputs([model], [x], lambda p, B: lib().acino_skel_fte_link_workspace_bytes(C.byref(p), B, 0), l1_eps=1e-2)
    N, L = model.N, len(model.names)
    empty = lambda *shape: torch.empty((1, N) + shape, dtype=torch.float64, device=io_["dev"])   # noqa: E731
    sig_d = torch.as_tensor(sigma, dtype=torch.float64, device=io_["dev"]).contiguous()
    grp_c = (C.c_int32 * len(grp))(*[int(g) for g in grp])
    status, null = (C.c_int32 * 1)(), ptr(None)
    dpos = empty(L, 3, K)
    check(lib().acino_skel_fte_link_sensitivity(*io_["head"], grp_c, K, null, null, null, ptr(dpos), null, null, null, status,
                                                *io_["tail"], 0, null))
    assert status[0] == 0 and np.array_equal(dpos[0].cpu().numpy(), full["dpos_links"])
    sens, std = empty(len(act), K), empty(L)
    check(lib().acino_skel_fte_link_sensitivity(*io_["head"], grp_c, K, ptr(sig_d), null, ptr(sens), null, null, null, ptr(std), status,
                                                *io_["tail"], 0, null))
    assert status[0] == 0 and np.array_equal(sens[0].cpu().numpy(), full["sens_links"][:, act])
    assert np.array_equal(std[0].cpu().numpy(), full["std_pos_links"])
