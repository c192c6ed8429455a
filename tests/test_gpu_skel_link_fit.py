"""GPU (-m gpu): acino_skel_fte_link_fit_system (csrc/skel_link_fit.hip: k_skel_link_fit_rhs, k_skel_link_fit_reduce; the factor
and the substitutions of the sensitivities) through build.link_fit_system, and build.fit_link_scales_fte, against the CPU
references of tests/skel_link_fit_ref.py.

    C, c, cost   entry by entry:  |gpu - ref| <= 256 eps x (the sum of the absolute values of the entry's elementary products)
    S, r, newton e = max |gpu - ref| / max |ref|  <=  bar(d0) = max(64 d0, 1e-13) against BOTH reductions,
                 d0 = the two reductions' own disagreement on the very input (banded Cholesky, dense LU);  d0 > 1e-8 is refused
    sens_links   the bits of build.model_link_sensitivity

Condition on the inputs: every kept |e| is above 1e-6 (the reference asserts it; tests/test_skel_link_fit_host.py checks it
on the CPU) - a residual's sign that differs between the device and numpy is not rounding.  No case needed a perturbed iterate.
The inputs are those of tests/skel_sample_cases.py and tests/skel_unobs_cases.py.

Measured on the MI355X (the table per case is in NOTES_perf.md, "Joint link-length fit"): C, c, cost at most 4.9, 3.4 and 1.7 of
eps x their terms (allowed 256); S d0 8.8e-13 .. 3.0e-11 -> e 1.5e-12 .. 4.2e-11, r 2.6e-11 .. 7.2e-10 -> 1.0e-11 .. 1.5e-9, newton
6.2e-11 .. 5.3e-9 -> 3.1e-11 .. 4.1e-9, the worst e / bar 0.11; "global" against the sum of the links 2.9e-15 (S), 1.8e-13 (r);
the identity on pt16 6.5e-10 (cov_x, bar 6.1e-8) and 2.4e-11 (cov_pos, bar 2.5e-9), with Sigma = C^-1 3.8e-2 and 3.4e-1; the driver
z = 0.71, 0.55, -0.97, 0.62, -1.08 on one clip after 17 outer steps (cost 677.69 -> 442.97)."""
import copy

import numpy as np
import pytest

import skel_cov_cases as cases
import skel_link_fit_ref as fref
import skel_links_ref as lkref
import skel_sample_cases as scases

pytestmark = pytest.mark.gpu

EPS = fref.EPS
REF_CASES = ["pt16", "pt32", "slice12", "slice40global", "p51", "pt16pin", "slice40pins", "shipped12"]


def _system(build, c, **kw):
    return build.link_fit_system([c["model"]], [c["x"]], c["groups"], pin_unobserved=c["pin_unobserved"], **kw)[0]


@pytest.mark.parametrize("name", REF_CASES)
def test_system_against_both_references(gpu_lib, golden_dir, name):
    from acinoset_amd import build
    c = fref.gpu_case(golden_dir, name)
    r, act = c["ref"], c["prob"].ACT
    K = r["K"]
    out = _system(build, c, return_sens=True)
    assert out["status"] == 0 and out["S"].shape == (K, K) and out["r"].shape == (K,) and np.array_equal(out["groups"], r["grp"])
    # ---- C, c and the cost: rounding alone
    qC = np.abs(out["C"] - r["C"]) / np.where(r["C_mag"] > 0, EPS * r["C_mag"], 1.0)
    qc = np.abs(out["c"] - r["c"]) / np.where(r["c_mag"] > 0, EPS * r["c_mag"], 1.0)
    qF = abs(out["cost"] - r["cost"]) / (EPS * r["cost"])
    print(f"{name}: K {K}: error / (eps x its terms) (allowed 256): C {qC.max():.1f}, c {qc.max():.1f}, cost {qF:.1f}")
    assert qC.max() <= 256 and qc.max() <= 256 and qF <= 256
    assert np.all(out["C"][r["C_mag"] == 0] == 0) and np.all(out["c"][r["c_mag"] == 0] == 0)
    # ---- S, r and the Newton step: both reductions
    for key, got in (("S", out["S"]), ("r", out["r"]), ("newton", out["newton"][:, act])):
        e1, e2 = fref.rel(got, r[key + "1"]), fref.rel(got, r[key + "2"])
        print(f"{name}: {key}: d0 {r['d0'][key]:.2e}, bar {r['bar'][key]:.2e}; e vs banded {e1:.2e}, vs dense {e2:.2e}")
        assert e1 <= r["bar"][key] and e2 <= r["bar"][key]
    # ---- exact facts
    assert np.array_equal(out["S"], out["S"].T) and np.array_equal(out["C"], out["C"].T)
    assert np.all(out["newton"][:, act][c["fixed"]] == 0) and np.all(out["newton"][:, np.setdiff1d(np.arange(c["model"].P), act)] == 0)
    links = build.model_link_sensitivity([c["model"]], [c["x"]], c["groups"], pin_unobserved=c["pin_unobserved"])[0]
    assert np.array_equal(out["sens_links"], links["sens_links"])
    assert np.all(out["sens_links"][:, act][c["fixed"]] == 0)
    if c["pin_unobserved"]:
        assert out["unobserved"] == links["unobserved"] and len(out["unobserved"]) == 2
    plain = _system(build, c)
    assert sorted(set(out) - set(plain)) == ["newton", "sens_links"]
    assert all(np.array_equal(plain[k], out[k]) for k in ("S", "r", "C", "c", "cost"))


def test_a_group_that_hangs_no_weighted_slot(gpu_lib, golden_dir):
    """Group 9 of slice12 (the first definition of hip1) is on no weighted slot's path: exact zeros in its row, column and entries."""
    from acinoset_amd import build
    c = fref.gpu_case(golden_dir, "slice12")
    out = _system(build, c)
    for key in ("S", "C"):
        assert np.all(out[key][9] == 0) and np.all(out[key][:, 9] == 0), key
    assert out["c"][9] == 0 and out["r"][9] == 0
    rest = np.arange(15) != 9
    assert np.all(np.diag(out["S"])[rest] > 0) and np.all(np.diag(out["C"])[rest] > 0)


def test_the_global_system_is_the_sum_of_the_links(gpu_lib, golden_dir):
    """Linearity on slice40: theta_global moves every link, so S_global = 1^T S_links 1 and r_global = 1^T r_links; the bar is that
    of the references' own sums."""
    from acinoset_amd import build
    cg, cl = fref.gpu_case(golden_dir, "slice40global"), fref.gpu_case(golden_dir, "slice40")
    glob, link = _system(build, cg), _system(build, cl)
    for key, tot in (("S", lambda a: a.sum()), ("r", lambda a: a.sum()), ("C", lambda a: a.sum()), ("c", lambda a: a.sum())):
        one = cl["ref"][key + "1"] if key in ("S", "r") else cl["ref"][key]
        ref_g = cg["ref"][key + "1"] if key in ("S", "r") else cg["ref"][key]
        d_sum = abs(tot(one) - ref_g.reshape(-1)[0]) / abs(ref_g.reshape(-1)[0])
        e = abs(tot(link[key]) - glob[key].reshape(-1)[0]) / abs(glob[key].reshape(-1)[0])
        print(f"slice40: {key}: sum of the links against the global one: references {d_sum:.2e}, bar {fref.bar(d_sum):.2e}; GPU {e:.2e}")
        assert e <= fref.bar(d_sum)


def test_batch_and_repeatability(gpu_lib, golden_dir):
    """Eight clips in one call equal the clips one by one, bit for bit; a second call repeats the first; a singular clip gives
    status 5 and NaN and leaves the others' bits standing; model_covariance, model_link_sensitivity and
    model_calibration_sensitivity return the same bits before and after."""
    import fte_calib_ref as cal
    from acinoset_amd import build
    c = scases.case(golden_dir, "slice40")
    g, _sk0, det = scases.fixture(golden_dir)
    models = [cases.make_model(g, c["sk"], det, 40, 60 + 45 * k) for k in range(8)]
    xs = [cases.iterate(g, m, seed=k) for k, m in enumerate(models)]
    sigma, sig_c = lkref.random_psd(15), cal.random_psd(2)
    keys = ("S", "r", "C", "c", "cost", "sens_links", "newton")
    cov0 = build.model_covariance([models[0]], [xs[0]])[0]
    lnk0 = build.model_link_sensitivity([models[0]], [xs[0]], "links", sigma)[0]
    cal0 = build.model_calibration_sensitivity([models[0]], [xs[0]], sig_c)[0]
    batch = build.link_fit_system(models, xs, "links", return_sens=True)
    again = build.link_fit_system(models, xs, "links", return_sens=True)
    for k in range(8):
        one = build.link_fit_system([models[k]], [xs[k]], "links", return_sens=True)[0]
        assert batch[k]["status"] == 0
        for key in keys:
            assert np.array_equal(one[key], batch[k][key]), (k, key)
            assert np.array_equal(again[k][key], batch[k][key]), (k, key)
    bad = copy.copy(models[2])
    names = list(bad.names)
    bad.weights = models[2].weights.copy()
    bad.weights[:, :, [names.index("elbow1"), names.index("wrist1")]] = 0.0
    mixed = build.link_fit_system(models[:2] + [bad] + models[3:4], xs[:4], "links", return_sens=True)
    assert [o["status"] for o in mixed] == [0, 0, 5, 0]
    act = c["prob"].ACT
    for key in ("S", "r", "C", "c"):
        assert np.isnan(mixed[2][key]).all(), key
    assert np.isnan(mixed[2]["cost"]) and np.isnan(mixed[2]["sens_links"][:, act]).all() and np.isnan(mixed[2]["newton"][:, act]).all()
    for k in (0, 1, 3):
        for key in keys:
            assert np.array_equal(mixed[k][key], batch[k][key]), (k, key)
    with pytest.raises(RuntimeError):
        build.link_fit_system([bad], [xs[2]], "links")
    cov1 = build.model_covariance([models[0]], [xs[0]])[0]
    lnk1 = build.model_link_sensitivity([models[0]], [xs[0]], "links", sigma)[0]
    cal1 = build.model_calibration_sensitivity([models[0]], [xs[0]], sig_c)[0]
    for key in ("cov_x", "cov_pos", "std_pos"):
        assert np.array_equal(cov0[key], cov1[key]), key
    for key in ("sens_links", "dpos_links", "cov_x_links", "cov_pos_links", "std_pos_links"):
        assert np.array_equal(lnk0[key], lnk1[key]), key
    for key in ("sens_cams", "cov_x_calib", "cov_pos_calib", "std_pos_calib"):
        assert np.array_equal(cal0[key], cal1[key]), key


def test_the_sums_are_the_marginals_of_the_joint_posterior(gpu_lib, golden_dir):
    """What the feature is for, on pt16: with Sigma = S^-1 from the device's S, cov_x + cov_x_links and cov_pos + cov_pos_links of
    the existing entries equal the x-blocks and the pose marginals of the dense inverse of [[A, G], [G^T, C]] within bar(d0), d0 the
    disagreement of the identity evaluated from the banded and from the dense pieces of the reference.  With the Sigma that ignores
    the coupling, C^-1, the sums are further off than that bar: the test sees the Schur term."""
    from acinoset_amd import build
    c = fref.gpu_case(golden_dir, "pt16")
    r, prob, act = c["ref"], c["prob"], c["prob"].ACT
    xa = c["x"][:, act]
    out = _system(build, c)
    dense, Sigma_dense = fref.joint_inverse([dict(ab=c["ab"], fixed=c["fixed"], G=r["G"], C=r["C"])])
    want = (dense[0]["cov_x"], fref.pose_marginals(prob, xa, r["D"], dense[0]["cov_x"], dense[0]["cross"], Sigma_dense))
    v1 = fref.block_inverse(prob, xa, r, c["ab"], c["fixed"], np.linalg.inv(r["S1"]), "1")
    v2 = fref.block_inverse(prob, xa, r, c["ab"], c["fixed"], np.linalg.inv(r["S2"]), "2")
    cov = build.model_covariance([c["model"]], [c["x"]])[0]

    def sums(Sigma):
        lk = build.model_link_sensitivity([c["model"]], [c["x"]], "links", 0.5 * (Sigma + Sigma.T))[0]
        return (cov["cov_x"] + lk["cov_x_links"])[:, act[:, None], act[None, :]], cov["cov_pos"] + lk["cov_pos_links"]

    joint, uncoupled = sums(np.linalg.inv(out["S"])), sums(np.linalg.inv(out["C"]))
    for key, got, miss, w_, a1, a2 in zip(("cov_x", "cov_pos"), joint, uncoupled, want, (v1[0], v1[2]), (v2[0], v2[2])):
        d0, e, m = fref.rel(a2, a1), fref.rel(got, w_), fref.rel(miss, w_)
        print(f"pt16: {key} + {key}_links: d0 {d0:.2e}, bar {fref.bar(d0):.2e}; e {e:.2e}; with Sigma = C^-1 off by {m:.2e}")
        assert d0 <= fref.D0_REFUSED and e <= fref.bar(d0)
        assert m > fref.bar(d0)


def test_the_driver_recovers_the_truth(gpu_lib, golden_dir):
    """build.fit_link_scales_fte on the synthetic clip of skel_link_fit_ref.synthetic_clip (seed 0, the first tried: the numpy
    driver of tests/test_skel_link_fit_host.py meets the 4-bar condition on it by itself): status ok, the cost never rises over
    accepted steps, every observed group within 4 of its own bars of the truth - compared with the truth, not with the CPU
    driver's bits: at a solve's end point the residual signs are not reproducible across implementations.  The clip cut into two
    windows that share theta: S is the sum of the windows' S, bit for bit, and the result serves ``cov_links`` as it is."""
    from acinoset_amd import build
    clip = fref.synthetic_clip(golden_dir)
    model = fref.clip_model(clip)
    act = np.asarray(model.active)
    x0 = np.zeros((model.N, model.P))
    x0[:, act] = clip["x_true"][:, act]
    out = build.fit_link_scales_fte(model, x0=x0, max_iter=60)
    z = (out["scales"] - clip["truth"]) / out["std_scales"]
    costs = [h["cost"] for h in out["history"] if h["accepted"]]
    print(f"one clip: status {out['status']}, {len(out['history'])} outer steps, cost {costs[0]:.4f} -> {out['history'][-1]['cost']:.4f}; "
          f"truth {np.round(clip['truth'], 4)}, scales {np.round(out['scales'], 4)}, std {np.round(out['std_scales'], 4)}, z {np.round(z, 2)}")
    assert out["status"] == "ok" and out["joint"] is True and out["observed"].all()
    assert all(b <= a for a, b in zip(costs, costs[1:]))
    assert (np.abs(z[out["observed"]]) < 4.0).all()
    assert len(out["models"]) == 1 and len(out["results"]) == 1 and np.array_equal(out["models"][0].link_scales, out["scales"])
    # ---- two windows that share theta
    halves = [fref.clip_model(clip, 0, 12), fref.clip_model(clip, 12, 12)]
    # (tol: with the default 1e-6 the loop goes on accepting steps that lower the cost in its sixth digit, the level at which two
    #  solves of one problem differ, and runs into max_outer with the same scales; 1e-4 is 0.01 % of a length, its bars are 0.5 % up)
    two = build.fit_link_scales_fte(halves, x0=[x0[:12], x0[12:]], max_iter=60, tol=1e-4)
    sys_ = two["system"]
    z2 = (two["scales"] - clip["truth"]) / two["std_scales"]
    print(f"two windows: status {two['status']}, {len(two['history'])} outer steps, scales {np.round(two['scales'], 4)}, z {np.round(z2, 2)}")
    assert two["status"] == "ok" and sys_["n_used"] == 2 and sys_["used"].all()
    assert np.array_equal(sys_["S"], sys_["clips"][0]["S"] + sys_["clips"][1]["S"])
    assert np.array_equal(sys_["r"], sys_["clips"][0]["r"] + sys_["clips"][1]["r"])
    direct = build.link_fit_system(two["models"], [r["x"] for r, _i in two["results"]], two["groups"])
    assert all(np.array_equal(d["S"], s["S"]) for d, s in zip(direct, sys_["clips"]))
    assert (np.abs(z2[two["observed"]]) < 4.0).all()
    # ---- the dict is a cov_links as it is: the joint posterior's total
    res = build.solve_models(two["models"], [r["x"] for r, _i in two["results"]], max_iter=60, return_cov=True, cov_links=two)
    for r_, _i in res:
        assert np.isfinite(r_["std_pos_total"]).all() and np.all(r_["std_pos_total"] >= r_["std_pos"])
