"""GPU (-m gpu): acino_skel_fte_sample (csrc/skel_sample.hip: k_skel_factor, k_skel_sample_back, k_skel_sample_fk) through
build.model_samples against the CPU references of tests/skel_sample_ref.py.

    e = max_s max_n ||delta_gpu[s, n] - delta_ref[s, n]||_2 / max_n ||delta_ref[s, n]||_2       (skel_sample_ref.map_err)
    e <= bar(d0) = max(64 d0, 1e-13),   d0 = map_err(banded_map, dense_map) on the very input and z;   d0 > 1e-8 is refused

The map z -> delta is deterministic, so it is held to the references sample by sample; statistics come last and only as a
sanity check.  The inputs are those of tests/skel_cov_cases.py (tests/skel_sample_cases.py builds them once per process)."""
import copy

import numpy as np
import pytest

import skel_cov_cases as cases
import skel_cov_ref as cref
import skel_sample_cases as scases
import skel_sample_ref as sref

from oracle import skeleton_fk as osk

pytestmark = pytest.mark.gpu

PANEL = 64                                                  # SKS_PANEL of csrc/skel_sample.hip: samples per workgroup
S_VALUES = (1, PANEL - 1, PANEL, PANEL + 1, 2 * PANEL + 3)


def _delta(out, c):
    """[S, N, n_active]: the samples minus the iterate, on the active states."""
    act = c["prob"].ACT
    return out["x_samples"][:, :, act] - c["x"][None, :, act]


_WIDE = {}


def _wide(golden_dir, name):
    """z of the widest S and both reference maps of it, once per input: sample s of a reference depends on z[s] alone, so the
    narrower S values use its leading samples."""
    if name not in _WIDE:
        c = scases.case(golden_dir, name)
        z = scases.normal_z(c, S_VALUES[-1])
        _WIDE[name] = (z, sref.banded_map(c["ab"], c["fixed"], z), sref.dense_map(c["ab"], c["fixed"], z))
    return _WIDE[name]


@pytest.mark.parametrize("name", ["golden", "slice40", "slice40pin", "slice100", "p51"])
def test_exact_map(gpu_lib, golden_dir, name):
    from acinoset_amd import build
    c = scases.case(golden_dir, name)
    z, db, dd = _wide(golden_dir, name)
    inact = np.setdiff1d(np.arange(c["model"].P), c["prob"].ACT)
    for S in S_VALUES:
        d0 = sref.map_err(db[:S], dd[:S])
        assert d0 <= sref.D0_REFUSED
        tol = sref.bar(d0)
        out = build.model_samples([c["model"]], [c["x"]], z=z[None, :S])[0]
        delta = _delta(out, c)
        e_d, e_b = sref.map_err(delta, dd[:S]), sref.map_err(delta, db[:S])
        print(f"{name}: PT {(c['fixed'].shape[1] + 15) // 16 * 16}, N {c['fixed'].shape[0]}, S {S}: d0 {d0:.2e}, bar {tol:.2e}; "
              f"vs dense {e_d:.2e}, vs banded {e_b:.2e}")
        assert out["status"] == 0 and out["x_samples"].shape == (S,) + c["x"].shape
        assert e_d <= tol and e_b <= tol
        assert np.array_equal(out["x_samples"][:, :, inact], np.broadcast_to(c["x"][:, inact], (S,) + c["x"][:, inact].shape))


def test_the_whole_inverse(gpu_lib, golden_dir):
    """Identity z on the 12-frame slice (S = 432): sum_s delta_n delta_n+lag^T is the block (n, n + lag) of inv(A) - lag 0 also
    against cov_x of the GPU's own covariance entry; lag 5 lies outside the factor's band."""
    from acinoset_amd import build
    c = scases.case(golden_dir, "slice12")
    N, P = c["fixed"].shape
    z = sref.identity_z(N, P)
    r = sref.reference(c["ab"], c["fixed"], z)
    out = build.model_samples([c["model"]], [c["x"]], z=z[None], positions=False)[0]
    delta = _delta(out, c)
    e_m = sref.map_err(delta, r["dense"])
    Ai = np.linalg.inv(cref.dense(c["ab"]))
    act = c["prob"].ACT
    cov = build.model_covariance([c["model"]], [c["x"]])[0]["cov_x"][:, act[:, None], act[None, :]]
    e_c = sref.block_err(sref.cross_blocks(delta, 0), cov)
    print(f"slice12 identity z (S = {N * P}): d0 {r['d0']:.2e}, bar {r['bar']:.2e}; map {e_m:.2e}; lag 0 vs cov_x (GPU) {e_c:.2e}")
    assert e_m <= r["bar"] and e_c <= r["bar"]
    for lag in (0, 1, 2, 3, 5):
        e = sref.block_err(sref.cross_blocks(delta, lag), sref.inverse_blocks(Ai, c["fixed"], lag))
        print(f"  lag {lag}: vs the dense inverse {e:.2e}")
        assert e <= r["bar"]


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


def test_pinned_variables_do_not_move(gpu_lib, golden_dir):
    """Every third variable gets its lower limit ON the iterate; those the oracle finds bound-active (not none, not all) have
    delta == 0 exactly although z is nonzero there, the rest matches the references of the pinned matrix."""
    from acinoset_amd import build
    c = scases.case(golden_dir, "slice40")
    model, x, prob0 = c["model"], c["x"], c["prob"]
    which = np.zeros((model.N, prob0.P), dtype=bool)
    which.reshape(-1)[::3] = True
    m = _tight(model, x, which)
    prob = cases.problem(c["sk"], m, c["scene"])
    ab, fixed = sref.system(prob, x[:, prob.ACT])
    assert 0 < fixed.sum() < which.sum() and not (fixed & ~which).any()
    z = np.random.default_rng(7).standard_normal((PANEL + 1,) + fixed.shape)
    assert np.all(z[:, fixed] != 0)
    r = sref.reference(ab, fixed, z)
    out = build.model_samples([m], [x], z=z[None])[0]
    delta = _delta(out, c)
    e = sref.map_err(delta, r["dense"])
    print(f"slice40, {int(fixed.sum())} pins: d0 {r['d0']:.2e}, bar {r['bar']:.2e}; vs dense {e:.2e}")
    assert np.all(delta[:, fixed] == 0)
    assert np.array_equal(out["x_samples"][:, :, prob.ACT][:, fixed], np.broadcast_to(x[:, prob.ACT][fixed], (z.shape[0], int(fixed.sum()))))
    assert e <= r["bar"] and sref.map_err(delta, r["banded"]) <= r["bar"]


def test_a_sample_depends_on_its_own_z_alone(gpu_lib, golden_dir):
    """Sample s of an S = (two panels + 3) call equals an S = 1 call with z(s), bit for bit; eight clips in one call equal the
    clips one by one."""
    from acinoset_amd import build
    c = scases.case(golden_dir, "slice40")
    z = _wide(golden_dir, "slice40")[0]
    many = build.model_samples([c["model"]], [c["x"]], z=z[None])[0]
    for s in (0, PANEL - 1, PANEL, 2 * PANEL + 2):
        one = build.model_samples([c["model"]], [c["x"]], z=z[None, s:s + 1])[0]
        for key in ("x_samples", "pos_samples"):
            assert np.array_equal(one[key][0], many[key][s]), (s, key)
    g, _sk0, det = scases.fixture(golden_dir)
    models = [cases.make_model(g, c["sk"], det, 40, 60 + 45 * k) for k in range(8)]
    xs = [cases.iterate(g, m, seed=k) for k, m in enumerate(models)]
    z8 = np.random.default_rng(3).standard_normal((8, 3, 40, len(c["prob"].ACT)))
    batch = build.model_samples(models, xs, z=z8)
    for k in (0, 3, 7):
        one = build.model_samples([models[k]], [xs[k]], z=z8[k:k + 1])[0]
        assert batch[k]["status"] == 0
        for key in ("x_samples", "pos_samples"):
            assert np.array_equal(one[key], batch[k][key]), (k, key)


def test_one_degenerate_clip_in_a_batch_stands_alone(gpu_lib, golden_dir):
    """One clip loses every detection of one limb (elbow1, wrist1), as in the covariance test: status 5 and NaN samples for it,
    the other clips unchanged, no exception; alone, the failure is the call's."""
    from acinoset_amd import build
    c = scases.case(golden_dir, "slice40")
    g, _sk0, det = scases.fixture(golden_dir)
    models = [cases.make_model(g, c["sk"], det, 40, 60 + 45 * k) for k in range(4)]
    xs = [cases.iterate(g, m, seed=k) for k, m in enumerate(models)]
    act = np.asarray(models[0].active)
    z = np.random.default_rng(4).standard_normal((4, 5, 40, len(act)))
    good = build.model_samples(models, xs, z=z)
    bad = copy.copy(models[2])
    names = list(bad.names)
    bad.weights = models[2].weights.copy()
    bad.weights[:, :, [names.index("elbow1"), names.index("wrist1")]] = 0.0
    mixed = build.model_samples(models[:2] + [bad] + models[3:], xs, z=z)
    assert [o["status"] for o in mixed] == [0, 0, 5, 0]
    assert np.isnan(mixed[2]["x_samples"][:, :, act]).all() and np.isnan(mixed[2]["pos_samples"]).all()
    for k in (0, 1, 3):
        for key in ("x_samples", "pos_samples"):
            assert np.array_equal(mixed[k][key], good[k][key]), (k, key)
    with pytest.raises(RuntimeError):
        build.model_samples([bad], [xs[2]], z=z[2:3])


@pytest.mark.parametrize("name", ["slice40", "p51"])
def test_positions_are_the_forward_kinematics_of_the_samples(gpu_lib, golden_dir, name):
    from acinoset_amd import build
    c = scases.case(golden_dir, name)
    out = build.model_samples([c["model"]], [c["x"]], n_samples=PANEL + 1, seed=2)[0]
    xs = out["x_samples"]
    want = osk.skeleton_fk(c["sk"], xs.reshape(-1, xs.shape[-1]))[0].reshape(out["pos_samples"].shape)
    e = np.abs(out["pos_samples"] - want).max()
    tol = 1e-13 * max(1.0, np.abs(want).max())
    print(f"{name}: pos_samples against the oracle's FK of x_samples {e:.2e} (tolerance {tol:.2e}); "
          f"spread of the samples' poses {out['pos_samples'].std(axis=0).max():.3e} m")
    assert e <= tol
    assert "pos_samples" not in build.model_samples([c["model"]], [c["x"]], n_samples=2, positions=False)[0]


def test_monte_carlo_variance(gpu_lib, golden_dir):
    """S = 4096 from ``seed`` on slice40: the per-variable sample variance of delta against diag(inv(A)) of the dense inverse,
    within 5 sqrt(2 / S) relative (five standard deviations of a chi-square mean) on the variables whose reference variance is
    above the median.  The band is applied FIRST to the CPU reference's delta from the same z: a failure of the band is then
    told apart from a failure of the kernel."""
    from acinoset_amd import build
    c = scases.case(golden_dir, "slice40")
    S, seed = 4096, 9
    N, P = c["fixed"].shape
    var_ref = np.diagonal(cref.dense_blocks(c["ab"], c["fixed"]), axis1=1, axis2=2)
    big = var_ref > np.median(var_ref)
    band = 5.0 * np.sqrt(2.0 / S)
    z = np.random.default_rng(seed).standard_normal((1, S, N, P))
    d_cpu = sref.banded_map(c["ab"], c["fixed"], z[0])
    e_cpu = np.abs(d_cpu.var(axis=0)[big] / var_ref[big] - 1.0).max()
    print(f"slice40, S {S}: band {band:.3f}; CPU reference's sample variance off by {e_cpu:.3f}")
    assert e_cpu <= band
    out = build.model_samples([c["model"]], [c["x"]], n_samples=S, seed=seed, positions=False)[0]
    delta = _delta(out, c)
    e_gpu = np.abs(delta.var(axis=0)[big] / var_ref[big] - 1.0).max()
    e_map = sref.map_err(delta, d_cpu)
    print(f"  GPU sample variance off by {e_gpu:.3f}; the map against the CPU's on the same z {e_map:.2e}")
    assert e_gpu <= band
    again = build.model_samples([c["model"]], [c["x"]], n_samples=S, seed=seed, positions=False)[0]
    other = build.model_samples([c["model"]], [c["x"]], n_samples=S, seed=seed + 1, positions=False)[0]
    assert np.array_equal(again["x_samples"], out["x_samples"])
    assert not np.array_equal(other["x_samples"], out["x_samples"])


def test_nothing_else_moved(gpu_lib, golden_dir):
    """The n_samples keyword leaves x, positions and info of the solve as they were; model_covariance stays within its bar of the
    dense inverse (PT 48 and PT 64) and returns the same bits before and after a model_samples call in the same process."""
    from acinoset_amd import build
    c = scases.case(golden_dir, "slice40")
    r0, i0 = build.solve_model(c["model"], x0=c["x"], max_iter=6)
    r1, i1 = build.solve_model(c["model"], x0=c["x"], max_iter=6, n_samples=4, sample_seed=1)
    assert i0 == i1 and sorted(r0) == ["ddx", "dx", "positions", "x"]
    assert sorted(r1) == ["ddx", "dx", "pos_samples", "positions", "x", "x_samples"]
    assert all(np.array_equal(r0[k], r1[k]) for k in r0)
    assert r1["x_samples"].shape == (4,) + r0["x"].shape and r1["pos_samples"].shape == (4,) + r0["positions"].shape
    draw = build.model_samples([c["model"]], [r1["x"]], n_samples=4, seed=1)[0]
    assert np.array_equal(draw["x_samples"], r1["x_samples"]) and np.array_equal(draw["pos_samples"], r1["pos_samples"])
    for name in ("slice40", "p51"):
        c = scases.case(golden_dir, name)
        act = c["prob"].ACT
        before = build.model_covariance([c["model"]], [c["x"]])[0]
        build.model_samples([c["model"]], [c["x"]], n_samples=3)
        after = build.model_covariance([c["model"]], [c["x"]])[0]
        for key in ("cov_x", "cov_pos", "std_pos"):
            assert np.array_equal(before[key], after[key]), (name, key)
        Sa = cref.dense_blocks(c["ab"], c["fixed"])
        Sb = cref.probe_blocks(c["ab"], c["fixed"], np.arange(c["fixed"].shape[0]))
        d0 = cref.rel_err(Sb, Sa)
        e = cref.rel_err(before["cov_x"][:, act[:, None], act[None, :]], Sa)
        print(f"{name}: model_covariance against the dense inverse {e:.2e} (d0 {d0:.2e}, bar {cref.bar(d0):.2e})")
        assert before["status"] == 0 and e <= cref.bar(d0)
