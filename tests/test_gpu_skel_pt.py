"""GPU (-m gpu): the PT = 16 and PT = 32 instantiations of the skeleton kernels (k_skel_solve2, k_skel_selinv, k_skel_factor,
k_skel_sample_back), which the human skeleton (PT 48) and its 51-state extension (PT 64) never launch.  Inputs: connected
sub-trees of ``generic_skeleton`` on 12 frames (tests/skel_cov_cases.py SUB_TREES, tests/skel_sample_cases.py SUB_TREE_CASES;
tests/test_skel_cov_host.py checks on the CPU that they are observed and that the references accept them).  Every check uses
the bar of the test it is taken from: tests/test_gpu_skel_cov.py, test_gpu_skel_sample.py, test_gpu_skel_reproj.py and
tests/test_skel_fte.py::test_gpu_solve_walks_the_oracle_lm_path."""
import numpy as np
import pytest

import skel_cov_ref as ref
import skel_reproj_ref as rref
import skel_sample_cases as scases
import skel_sample_ref as sref
from test_gpu_skel_reproj import _compare

from oracle import skel_fte as osf

pytestmark = pytest.mark.gpu

CASES = ["pt16", "pt16pin", "pt32"]
_REF = {}


def _case(golden_dir, name):
    """The case, asserted to have the PT it is named for, with the covariance reference (once per input)."""
    c = scases.case(golden_dir, name)
    n_act = len(c["model"].active)
    assert (n_act + 15) // 16 * 16 == scases.SUB_TREE_CASES[name][0], n_act
    if name not in _REF:
        _REF[name] = ref.reference(c["prob"], c["x"][:, c["prob"].ACT])
    return c, _REF[name]


@pytest.mark.parametrize("name", CASES)
def test_covariance(gpu_lib, golden_dir, name):
    from acinoset_amd import build
    c, r = _case(golden_dir, name)
    model, act = c["model"], c["prob"].ACT
    out = build.model_covariance([model], [c["x"]])[0]
    cov = out["cov_x"][:, act[:, None], act[None, :]]
    tol = ref.bar(r["d0"])
    e_a, e_b = ref.rel_err(cov, r["Sa"]), ref.rel_err(cov[r["frames"]], r["Sb"])
    e_p = ref.rel_err(out["cov_pos"].reshape(model.N, -1), r["cov_pos"].reshape(model.N, -1))
    e_s = float(np.max(np.abs(out["std_pos"] - r["std_pos"]) / r["std_pos"]))
    print(f"{name}: d0 {r['d0']:.2e}, bar {tol:.2e}; cov_x vs (a) {e_a:.2e}, vs (b) {e_b:.2e}; cov_pos {e_p:.2e}; std_pos {e_s:.2e}")
    assert out["status"] == 0
    assert e_a <= tol and e_b <= tol and e_p <= tol and e_s <= tol


@pytest.mark.parametrize("name", CASES)
def test_samples(gpu_lib, golden_dir, name):
    from acinoset_amd import build
    c, _r = _case(golden_dir, name)
    act = c["prob"].ACT
    z = scases.normal_z(c, 3)
    db, dd = sref.banded_map(c["ab"], c["fixed"], z), sref.dense_map(c["ab"], c["fixed"], z)
    d0 = sref.map_err(db, dd)
    assert d0 <= sref.D0_REFUSED
    tol = sref.bar(d0)
    out = build.model_samples([c["model"]], [c["x"]], z=z[None])[0]
    delta = out["x_samples"][:, :, act] - c["x"][None, :, act]
    e_d, e_b = sref.map_err(delta, dd), sref.map_err(delta, db)
    print(f"{name}: d0 {d0:.2e}, bar {tol:.2e}; vs dense {e_d:.2e}, vs banded {e_b:.2e}")
    assert out["status"] == 0 and e_d <= tol and e_b <= tol


@pytest.mark.parametrize("name", CASES)
def test_reprojection(gpu_lib, golden_dir, name):
    from acinoset_amd import build
    c, r = _case(golden_dir, name)
    model, cam = c["model"], c["cam"]
    got = build.model_reprojection([model], [c["x"]], cov_pos=[r["cov_pos"]])[0]
    want = rref.reprojection(c["sk"], c["x"], model.meas, model.weights, c["scene"], cam, cov_pos=r["cov_pos"],
                             gate_w=float(np.asarray(model.weights).max()))
    _compare(name, got, want, cam)


@pytest.mark.parametrize("name", CASES)
def test_solve_walks_the_oracle_lm_path(gpu_lib, golden_dir, name):
    from acinoset_amd import build
    c, _r = _case(golden_dir, name)
    model, prob, x0 = c["model"], c["prob"], c["x"]
    act = prob.ACT
    F0 = prob.evaluate(x0[:, act], need_jac=False)[0]
    for k in (0, 1, 2, 5):
        res, info = build.solve_model(model, x0=x0, max_iter=k, ftol=0.0, xtol=0.0, gtol=0.0)
        xo, oinfo = osf.lm_solve(prob, x0[:, act], max_iter=k, ftol=0.0, xtol=0.0, gtol=0.0) if k else (x0[:, act], dict(cost=F0, accepted=0))
        print(f"{name}, {k} iterations: cost {info['cost_final']:.12f} against {oinfo['cost']:.12f}, "
              f"max |dx| {float(np.abs(res['x'][:, act] - xo).max()):.2e}")
        assert abs(info["cost_initial"] - F0) < 1e-12 * abs(F0)
        assert info["accepted"] == oinfo["accepted"], (k, info, oinfo)
        assert abs(info["cost_final"] - oinfo["cost"]) < 1e-10 * abs(oinfo["cost"]), (k, info["cost_final"], oinfo["cost"])
        assert np.abs(res["x"][:, act] - xo).max() < 1e-8
        assert np.abs(res["positions"] - prob.outputs(xo)["positions"]).max() < 1e-8


def test_batch_of_three_equals_the_clips_one_by_one(gpu_lib, golden_dir):
    """PT = 16, two different clips (the second one twice): every array of the solve, the covariance and the samples."""
    from acinoset_amd import build
    cs = [_case(golden_dir, n)[0] for n in ("pt16", "pt16b", "pt16b")]
    models, xs = [c["model"] for c in cs], [c["x"] for c in cs]
    z = np.stack([scases.normal_z(c, 3, seed=7 + i) for i, c in enumerate(cs)])
    many = (build.solve_models(models, xs, max_iter=5), build.model_covariance(models, xs), build.model_samples(models, xs, z=z))
    for k in range(3):
        one = (build.solve_models([models[k]], [xs[k]], max_iter=5), build.model_covariance([models[k]], [xs[k]]),
               build.model_samples([models[k]], [xs[k]], z=z[k:k + 1]))
        assert many[0][k][1] == one[0][0][1]
        for got, want in ((many[0][k][0], one[0][0][0]), (many[1][k], one[1][0]), (many[2][k], one[2][0])):
            assert sorted(got) == sorted(want)
            for key in want:
                assert np.array_equal(got[key], want[key]), (k, key)
