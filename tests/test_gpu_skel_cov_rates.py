"""GPU (-m gpu): acino_skel_fte_covariance_rates (csrc/skel_cov_rates.hip) through build.model_covariance(rates=True) against
the cancellation-free reference (c) of tests/skel_cov_rates_ref.py within bar(d0) = max(64 d0, 1e-13), d0 the disagreement of
(c) with the same form from the reversed factorisation on the very input; inputs: tests/skel_cov_rates_cases.py."""
import copy

import numpy as np
import pytest

import skel_cov_cases as cases
import skel_cov_rates_cases as rcases
import skel_cov_rates_ref as rref
import skel_sample_cases as scases
import skel_sample_ref as sref
import skel_unobs_cases as ucases

pytestmark = pytest.mark.gpu

RATE_KEYS = ("cov_dx", "cov_ddx", "std_dx", "std_ddx", "cov_vel", "std_vel")


def _active(out, act):
    """The four arrays of the reference's layout from a dict of model_covariance(rates=True)."""
    act = np.asarray(act)
    return dict(cov_dx=out["cov_dx"][:, act[:, None], act[None, :]], cov_ddx=out["cov_ddx"][:, act[:, None], act[None, :]],
                cov_vel=out["cov_vel"], std_vel=out["std_vel"])


def _check_layout(out, model):
    """Zero outside model.active, std_dx / std_ddx the square roots of the diagonals, shapes."""
    N, P, L = model.N, model.P, len(model.names)
    inact = np.setdiff1d(np.arange(P), np.asarray(model.active))
    for k, sk in (("cov_dx", "std_dx"), ("cov_ddx", "std_ddx")):
        assert out[k].shape == (N, P, P) and out[sk].shape == (N, P)
        assert np.all(out[k][:, inact, :] == 0) and np.all(out[k][:, :, inact] == 0)
        assert np.array_equal(out[sk], np.sqrt(np.maximum(np.einsum("npp->np", out[k]), 0.0)), equal_nan=True)
        assert np.array_equal(out[k], np.swapaxes(out[k], 1, 2), equal_nan=True)
    assert out["cov_vel"].shape == (N, L, 3, 3) and out["std_vel"].shape == (N, L)


def _parity(name, out, c):
    r = c["ref"]
    e = rref.out_err(_active(out, c["prob"].ACT), r["c"])
    print(f"{name}: N {c['model'].N}, P {r['fixed'].shape[1]}, d0 {r['d0']:.2e}, bar {r['bar']:.2e}; "
          + ", ".join(f"{k} {v:.2e}" for k, v in e.items()) + f"; pins {int(r['fixed'].sum())}; "
          f"std_vel {np.nanmin(out['std_vel']):.3e} .. {np.nanmax(out['std_vel'][np.isfinite(out['std_vel'])]):.3e} m/s")
    assert max(e.values()) <= r["bar"], e
    return e


@pytest.mark.parametrize("name", rcases.PARITY)
def test_parity_with_the_cancellation_free_reference(gpu_lib, golden_dir, name):
    from acinoset_amd import build
    c = rcases.case(golden_dir, name)
    out = build.model_covariance([c["model"]], [c["x"]], rates=True)[0]
    assert out["status"] == 0
    _check_layout(out, c["model"])
    _parity(name, out, c)
    assert np.array_equal(out["cov_vel"][0], out["cov_vel"][1]) and np.array_equal(out["std_vel"][0], out["std_vel"][1])
    assert np.array_equal(out["cov_ddx"][0], out["cov_ddx"][2]) and np.array_equal(out["cov_ddx"][1], out["cov_ddx"][2])


@pytest.mark.parametrize("N", rcases.SHORT)
def test_short_clips_against_the_reference_and_the_start_up_rules(gpu_lib, golden_dir, N):
    """N = 1 .. 5 on the PT 16 sub-tree, the iterate's own poses as detections, the three free twists switched off
    (tests/skel_cov_rates_cases.py SHORT_OFF): a clip shorter than the prior's stencil is regular, status 0, and all four arrays
    are within bar(d0) of (c) - 1e-13 for N <= 3, where the reference's two factorisations agree to 4e-16.  Beside the
    reference, what the definition fixes exactly: N = 1 all zero; N = 2 ddx = 0 and dx_0 = 0; frame 0's velocity that of frame 1;
    ddx equal over frames 0 .. 2."""
    from acinoset_amd import build
    c = rcases.case(golden_dir, f"short{N}")
    model = c["model"]
    out = build.model_covariance([model], [c["x"]], rates=True)[0]
    assert out["status"] == 0
    _check_layout(out, model)
    got = _active(out, model.active)
    assert all(np.isfinite(v).all() for v in got.values())
    if N == 1:
        assert all(np.all(v == 0) for v in got.values())
    else:
        assert np.array_equal(got["cov_vel"][0], got["cov_vel"][1]) and np.all(got["std_vel"] > 0)
        assert np.all(np.diagonal(got["cov_dx"][1]) > 0)
    if N == 2:
        assert np.all(got["cov_ddx"] == 0) and np.all(got["cov_dx"][0] == 0)
    if N >= 3:
        assert np.array_equal(got["cov_ddx"][0], got["cov_ddx"][2]) and np.array_equal(got["cov_ddx"][1], got["cov_ddx"][2])
        assert np.all(np.diagonal(got["cov_dx"][0]) > 0) and np.all(np.diagonal(got["cov_ddx"][0]) > 0)
    if N == 1:
        print(f"short1: d0 {c['ref']['d0']:.2e}, bar {c['ref']['bar']:.2e}; every output exactly 0")
        assert all(np.array_equal(got[k], c["ref"]["c"][k]) for k in rref.KEYS)
    else:
        _parity(f"short{N}", out, c)


def batch_clips(golden_dir):
    """Three different 5-frame clips of the PT 16 sub-tree on the slice's detections (frames 60, 300 and 100)."""
    g, sk0, det = scases.fixture(golden_dir)
    sk = cases.sub_skeleton(cases.generic_skeleton(sk0), cases.SUB_TREES[16])
    models = [cases.make_model(g, sk, det, 5, st, "fisheye", scases.scene(g)) for st in (60, 300, 100)]
    return sk, models, [cases.iterate(g, m, seed=k) for k, m in enumerate(models)]


def test_batch_of_three_short_clips_equals_the_clips_one_by_one(gpu_lib, golden_dir):
    """Three clips of N = 5 in one call: every frame's window lies in its own clip, so each clip equals its single-clip call bit
    for bit (frames 0 and 1 of clips 1 and 2 would read the previous clip's last frames otherwise)."""
    from acinoset_amd import build
    _sk, models, xs = batch_clips(golden_dir)
    many = build.model_covariance(models, xs, rates=True)
    assert [o["status"] for o in many] == [0, 0, 0]
    for k in range(3):
        one = build.model_covariance([models[k]], [xs[k]], rates=True)[0]
        for key in ("cov_x", "cov_pos", "std_pos") + RATE_KEYS:
            assert np.isfinite(one[key]).all() and np.array_equal(one[key], many[k][key]), (k, key)
    assert not np.array_equal(many[0]["cov_dx"], many[1]["cov_dx"])


def test_existing_outputs_keep_their_bits_and_std_vel_alone_equals_the_full_call(gpu_lib, golden_dir):
    from acinoset_amd import build
    c = rcases.case(golden_dir, "slice40")
    plain = build.model_covariance([c["model"]], [c["x"]])[0]
    full = build.model_covariance([c["model"]], [c["x"]], rates=True)[0]
    assert sorted(plain) == ["cov_pos", "cov_x", "status", "std_pos"]
    assert sorted(full) == sorted(("cov_pos", "cov_x", "status", "std_pos") + RATE_KEYS)
    for key in ("cov_x", "cov_pos", "std_pos"):
        assert np.array_equal(plain[key], full[key]), key
    alone = build._covariance([c["model"]], [c["x"]], 1e-2, ("std_vel",))[0]
    assert sorted(alone) == ["status", "std_vel"] and np.array_equal(alone["std_vel"], full["std_vel"])
    stds = build.model_covariance([c["model"]], [c["x"]], std_only=True, rates=True)[0]
    assert sorted(stds) == ["status", "std_ddx", "std_dx", "std_pos", "std_vel"]
    for key in ("std_pos", "std_dx", "std_ddx", "std_vel"):
        assert np.array_equal(stds[key], full[key]), key


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


def pinned_case(golden_dir):
    """slice40 with every third variable's lower limit ON the iterate: those whose gradient pushes outward are bound-active."""
    c0 = rcases.case(golden_dir, "slice40")
    which = np.zeros((c0["model"].N, c0["prob"].P), dtype=bool)
    which.reshape(-1)[::3] = True
    m = _tight(c0["model"], c0["x"], which)
    c = rcases.finish(c0["sk"], m, c0["scene"], c0["cam"], x=c0["x"])
    fixed = c["ref"]["fixed"]
    assert 0 < fixed.sum() < which.sum() and not (fixed & ~which).any()
    return c


def test_bound_pins_give_exact_zeros_where_the_definition_says_so(gpu_lib, golden_dir):
    """A variable pinned in frame a contributes nothing from frame a: an entry of cov_dx / cov_ddx is exactly 0 where every
    frame of the window that carries a coefficient has the row's or the column's variable pinned - the reference (c) has its
    exact zeros there and nowhere else -, and the rest matches (c)."""
    from acinoset_amd import build
    c = pinned_case(golden_dir)
    out = build.model_covariance([c["model"]], [c["x"]], rates=True)[0]
    assert out["status"] == 0
    got, want = _active(out, c["prob"].ACT), c["ref"]["c"]
    for k in ("cov_dx", "cov_ddx"):
        assert (want[k] == 0).any() and not (want[k] == 0).all()
        assert np.array_equal(got[k] == 0, want[k] == 0), k
    fixed = c["ref"]["fixed"]
    both = fixed[1:] & fixed[:-1]                              # pinned in frames n and n - 1: row and column of cov_dx[n] are 0
    assert both.any()
    for n in range(2, fixed.shape[0]):
        assert np.all(got["cov_dx"][n][both[n - 1], :] == 0) and np.all(got["cov_dx"][n][:, both[n - 1]] == 0)
    _parity("slice40 with bound pins", out, c)


def unobserved_case(golden_dir):
    """lost12 of tests/skel_unobs_cases.py (a limb no camera detects: six states unobserved) with the rates' reference."""
    u = ucases.case(golden_dir, "lost12")
    r = u["ref"]
    assert r["unobserved"].sum() == 6 and r["dependent"].any() and not r["dependent"].all()
    return dict(u, ref=rref.reference(r["ab"], r["fixed"], r["G"], u["model"].h, r["dependent"]), unobserved=r["unobserved"],
                dependent=r["dependent"])


def test_pin_unobserved_gives_zero_rows_and_infinite_bars_for_dependent_slots(gpu_lib, golden_dir):
    """The lost-limb clip is the SECOND of a batch of two (the first: the same clip with every limb detected, nothing
    unobserved), so that the kernel reads the second clip's mask, not the first's."""
    from acinoset_amd import build
    c = unobserved_case(golden_dir)
    model, act = c["model"], c["prob"].ACT
    g, _sk0, det = scases.fixture(golden_dir)
    whole = cases.make_model(g, c["sk"], det, model.N, cases.SLICE_STARTS[0], c["cam"], c["scene"])
    assert np.array_equal(ucases.lose_limb(whole).weights, model.weights) and not np.array_equal(whole.weights, model.weights)
    first, out = build.model_covariance([whole, model], [c["x"], c["x"]], pin_unobserved=True, rates=True)
    first_alone = build.model_covariance([whole], [c["x"]], pin_unobserved=True, rates=True)[0]
    assert first["status"] == 0 and first["unobserved"] == []
    for key in RATE_KEYS:
        assert np.isfinite(first[key]).all() and np.array_equal(first[key], first_alone[key]), key
    assert out["status"] == 0 and out["unobserved"] == [int(act[p]) for p in np.nonzero(c["unobserved"])[0]]
    got = _active(out, act)
    un = c["unobserved"]
    for k in ("cov_dx", "cov_ddx"):
        assert np.all(got[k][:, un, :] == 0) and np.all(got[k][:, :, un] == 0)
    dep = c["dependent"]
    dep_v = np.concatenate([dep[1:2] | dep[0:1], dep[1:] | dep[:-1]])     # either frame; frame 0 repeats frame 1
    assert np.array_equal(np.isposinf(got["std_vel"]), dep_v) and np.array_equal(np.isnan(got["cov_vel"]).all(axis=(2, 3)), dep_v)
    assert np.isfinite(got["std_vel"][~dep_v]).all() and np.isfinite(got["cov_vel"][~dep_v]).all()
    assert np.isfinite(got["cov_dx"]).all() and np.isfinite(got["cov_ddx"]).all()
    _parity("lost12, unobserved states pinned", out, c)
    alone = build.model_covariance([model], [c["x"]], pin_unobserved=True, rates=True)[0]
    for key in RATE_KEYS:
        assert np.array_equal(alone[key], out[key], equal_nan=True), key


def test_one_singular_clip_in_a_batch_of_two(gpu_lib, golden_dir):
    from acinoset_amd import build
    c = rcases.case(golden_dir, "slice40")
    bad = ucases.lose_limb(c["model"])
    good_alone = build.model_covariance([c["model"]], [c["x"]], rates=True)[0]
    good, lost = build.model_covariance([c["model"], bad], [c["x"], c["x"]], rates=True)
    assert (good["status"], lost["status"]) == (0, 5)
    act = np.asarray(bad.active)
    assert all(np.isnan(v).all() for v in _active(lost, act).values())
    assert np.isnan(lost["std_dx"][:, act]).all() and np.isnan(lost["std_ddx"][:, act]).all()
    for key in ("cov_x", "cov_pos", "std_pos") + RATE_KEYS:
        assert np.array_equal(good[key], good_alone[key]), key
    with pytest.raises(RuntimeError):
        build.model_covariance([bad], [c["x"]], rates=True)


def test_cross_check_with_the_sampler(gpu_lib, golden_dir):
    """PT 16, N = 8: model_samples with z = the identity (S = N n_active unit vectors) returns delta = the rows of L^-T, so that
    sum_s dx(delta_s) dx(delta_s)^T = C A^-1 C^T = cov_dx, likewise cov_ddx - the sampler's back-substitution instead of the
    selected inverse, and _finite_diff_states itself instead of the coefficient rows."""
    from acinoset_amd import build
    c = rcases.case(golden_dir, "pt16n8")
    model, act = c["model"], c["prob"].ACT
    N, Pa = model.N, len(act)
    out = build.model_covariance([model], [c["x"]], rates=True)[0]
    smp = build.model_samples([model], [c["x"]], z=sref.identity_z(N, Pa)[None], positions=False)[0]
    assert out["status"] == 0 and smp["status"] == 0
    delta = smp["x_samples"][:, :, act] - c["x"][None, :, act]
    d1, d2 = zip(*(build._finite_diff_states(d, float(model.h)) for d in delta))
    got = _active(out, act)
    for key, d in (("cov_dx", np.stack(d1)), ("cov_ddx", np.stack(d2))):
        e = rref.rel_err(got[key], np.einsum("snp,snq->npq", d, d))
        print(f"{key} against the sampler: {e:.2e} (bar {c['ref']['bar']:.2e})")
        assert e <= c["ref"]["bar"]


def test_the_naive_bar_is_far_too_wide(gpu_lib, golden_dir):
    """std_dx < sqrt(2 diag cov_x) / h on slice40: the prior correlates neighbouring frames, and the cross-frame blocks cancel most
    of what independent frames would give."""
    from acinoset_amd import build
    c = rcases.case(golden_dir, "slice40")
    model, act = c["model"], np.asarray(c["prob"].ACT)
    out = build.model_covariance([model], [c["x"]], rates=True)[0]
    naive = np.sqrt(2.0 * np.einsum("npp->np", out["cov_x"])[:, act]) / model.h
    ratio = out["std_dx"][:, act] / naive
    print(f"std_dx / (sqrt(2 diag cov_x) / h) on slice40: min {ratio.min():.3e}, median {np.median(ratio):.3e}, max {ratio.max():.3e}")
    assert np.all(out["std_dx"][:, act] > 0) and np.all(ratio < 1.0)


def test_return_rate_cov_joins_the_results_and_leaves_the_solve_untouched(gpu_lib, golden_dir):
    from acinoset_amd import build
    c = rcases.case(golden_dir, "pt16n8")
    model, x = c["model"], c["x"]
    r0, i0 = build.solve_model(model, x0=x, max_iter=4)
    r1, i1 = build.solve_model(model, x0=x, max_iter=4, return_rate_cov=True)
    r2, _i2 = build.solve_model(model, x0=x, max_iter=4, return_cov=True, return_rate_cov=True)
    assert i0 == i1 and sorted(r0) == ["ddx", "dx", "positions", "x"] and sorted(r1) == sorted(("ddx", "dx", "positions", "x") + RATE_KEYS)
    assert all(np.array_equal(r0[k], r1[k]) for k in r0)
    cv = build.model_covariance([model], [r1["x"]], rates=True)[0]
    for key in RATE_KEYS:
        assert np.array_equal(cv[key], r1[key]) and np.array_equal(cv[key], r2[key]), key
    for key in ("cov_x", "cov_pos", "std_pos"):
        assert np.array_equal(cv[key], r2[key]), key
    many = build.solve_models([model, model], [x, x], max_iter=4, return_rate_cov=True)
    assert all(np.array_equal(many[k][0][key], r1[key]) for k in range(2) for key in RATE_KEYS)


def test_video_stitches_the_rate_bars_by_the_depth_rule(gpu_lib, golden_dir):
    """solve_video(return_rate_cov=True) on 100 frames of the shipped video in windows of 40 (the shipped skeleton: its two
    unobserved states pinned): the stitched arrays have the video's length, every frame of a window whose covariance stands is
    finite, std_dx is the root of cov_dx's diagonal, and without the keyword the result is what it was."""
    import os
    from acinoset_amd import build
    g, sk = cases.load(golden_dir)
    full = np.load(os.path.join(golden_dir, "human_dlc_full.npz"))
    tabs = [(list(full["parts"]), full[f"det{c}"].astype(np.float64)) for c in range(2)]
    kw = dict(scene=scases.scene(g), dlc_tables=tabs, first_frame=0, last_frame=99, window=40, overlap=10, pairing="name",
              max_iter=10, warm_passes=0)
    res, infos, starts = build.solve_video(sk, return_rate_cov=True, pin_unobserved=True, **kw)
    plain, _i, _s = build.solve_video(sk, **kw)
    assert sorted(plain) == ["ddx", "dx", "positions", "seams", "start_frame", "x"]
    assert all(np.array_equal(plain[k], res[k]) for k in ("positions", "x", "dx", "ddx"))
    P, L = res["x"].shape[1], res["positions"].shape[1]
    assert res["std_dx"].shape == (100, P) and res["cov_ddx"].shape == (100, P, P) and res["cov_vel"].shape == (100, L, 3, 3)
    assert res["std_vel"].shape == (100, L) and "std_pos" not in res and len(infos) == len(starts)
    status = np.array([i["cov_status"] for i in infos])
    print("covariance status per window:", status.tolist(), "median std_vel (m/s):", float(np.nanmedian(res["std_vel"])))
    assert set(status) <= {0, 5} and (status == 0).any()
    ok = status[res["owner"]] == 0
    assert np.isfinite(res["std_dx"][ok]).all() and not np.isnan(res["std_vel"][ok]).any() and np.isnan(res["std_vel"][~ok]).all()
    assert np.array_equal(res["std_dx"], np.sqrt(np.maximum(np.einsum("npp->np", res["cov_dx"]), 0.0)), equal_nan=True)
