"""Host side of the skeleton-FTE covariance (no GPU): the ABI entries, the three CPU references of tests/skel_cov_ref.py against
each other, and the argument checks of build.model_covariance.  Inputs: tests/skel_cov_cases.py (the fixture's detections, 8
frames, and the 40-frame windows of human_dlc_slice.npz starting at frames 60 and 300; every active state observed - asserted)."""
import copy
import ctypes as C
import os
import re

import numpy as np
import pytest

import skel_cov_cases as cases
import skel_cov_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("acino_skel_fte_covariance_workspace_bytes", "acino_skel_fte_covariance")


@pytest.fixture(scope="module")
def fx(golden_dir):
    g, sk = cases.load(golden_dir)
    det = np.load(os.path.join(golden_dir, "human_dlc_slice.npz"))["det"].astype(np.float64)
    return g, cases.generic_skeleton(sk), det


def test_header_library_and_binding_carry_the_two_entries():
    from acinoset_amd import _lib
    header = open(os.path.join(ROOT, "include", "acinoset_hip.h")).read()
    handle = C.CDLL(_lib.SO_PATH)
    for name in SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert hasattr(handle, name) and name in _lib.SIGNATURES
    assert re.search(r"#define ACINO_ABI_VERSION 3\b", header) and _lib.ABI_VERSION == 3 and _lib.lib().acino_abi_version() == 3
    p = _lib.SkelFteParams()
    p.n_frames, p.n_cams, p.n_pose, p.n_ops, p.n_angles, p.n_active = 100, 2, 15, 14, 15, 36
    one, many = (_lib.lib().acino_skel_fte_covariance_workspace_bytes(C.byref(p), b) for b in (1, 8))
    assert 0 < one < many and one % 256 == 0
    p.n_active = 65
    assert _lib.lib().acino_skel_fte_covariance_workspace_bytes(C.byref(p), 1) == 0


@pytest.fixture(scope="module")
def refs(fx):
    g, sk, det = fx
    scene = (g["K"], g["D"], g["R"], g["t"])
    out = {}
    for name, src, n, sf in (("golden", g["det"], int(g["n_frames"]), int(g["start_frame"])), ("slice60", det, 40, cases.SLICE_STARTS[0]),
                             ("slice300", det, 40, cases.SLICE_STARTS[1])):
        model = cases.make_model(g, sk, src, n, sf)
        x = cases.iterate(g, model, seed=len(out))
        prob = cases.problem(sk, model, scene)
        cases.assert_observed(prob, x[:, prob.ACT])
        out[name] = (model, x, prob, ref.reference(prob, x[:, prob.ACT]))
    return out


@pytest.mark.parametrize("name", ["golden", "slice60", "slice300"])
def test_the_three_references_agree(refs, name):
    _model, _x, _prob, r = refs[name]
    tol = ref.bar(r["d0"])
    Sc = ref.takahashi_blocks(r["ab"], r["fixed"])
    e = ref.rel_err(Sc, r["Sa"])
    print(f"{name}: d0 {r['d0']:.2e}, bar {tol:.2e}, recursion vs dense inverse {e:.2e}")
    assert e <= tol and ref.rel_err(Sc[r["frames"]], r["Sb"]) <= tol
    Sa = r["Sa"]
    assert np.abs(Sa - np.swapaxes(Sa, 1, 2)).max() <= 1e-9 * np.abs(Sa).max()
    assert (np.linalg.eigvalsh(0.5 * (Sa + np.swapaxes(Sa, 1, 2))) >= -1e-9 * np.abs(Sa).max()).all()
    assert np.all(r["std_pos"] > 0) and np.all(r["std_pos"] < 1.0)


def test_pinned_variables_give_zero_rows_and_columns(fx, refs):
    g, sk, _det = fx
    model, x, prob0, _r = refs["slice60"]
    act = prob0.ACT
    which = np.zeros((model.N, prob0.P), dtype=bool)
    which.reshape(-1)[::3] = True
    lo, hi = model.lo.copy(), model.hi.copy()
    la, ha = lo[:, act], hi[:, act]
    la[which], ha[which] = x[:, act][which], x[:, act][which] + 1.0
    lo[:, act], hi[:, act] = la, ha
    prob = cases.problem(sk, model, (g["K"], g["D"], g["R"], g["t"]), lo=lo, hi=hi)
    r = ref.reference(prob, x[:, act])
    fixed = r["fixed"]
    assert 0 < fixed.sum() < which.sum()
    pin = fixed[:, :, None] | fixed[:, None, :]
    Sc = ref.takahashi_blocks(r["ab"], fixed)
    assert np.all(r["Sa"][pin] == 0) and np.all(r["Sb"][pin] == 0) and np.all(Sc[pin] == 0)
    assert ref.rel_err(Sc, r["Sa"]) <= ref.bar(r["d0"])


def test_python_argument_checks_come_before_the_gpu(fx, refs):
    import torch
    from acinoset_amd import build
    model, x, _prob, _r = refs["slice60"]
    other = copy.copy(model)
    other.h = 2 * model.h
    with pytest.raises(ValueError, match="share h"):
        build.model_covariance([model, other], [x, x])
    pin = copy.copy(model)
    pin.camera_model = "pinhole"
    with pytest.raises(ValueError, match="camera model"):
        build.model_covariance([model, pin], [x, x])
    with pytest.raises(ValueError, match="must be"):
        build.model_covariance([model], [x[:, :-1]])
    with pytest.raises(ValueError, match="iterates"):
        build.model_covariance([model], [x, x])
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="GPU"):
            build.model_covariance([model], [x])


@pytest.mark.parametrize("name", ["pt16", "pt16b", "pt16pin", "pt32"])
def test_sub_tree_inputs_have_the_size_they_are_for_and_the_references_accept_them(golden_dir, name):
    """The inputs of tests/test_gpu_skel_pt.py, on the CPU: PT as named, every active state observed (``case`` asserts it), and
    both references' own disagreement below the 1e-8 at which their bars refuse an input."""
    import skel_sample_cases as scases
    import skel_sample_ref as sref
    c = scases.case(golden_dir, name)
    pt = scases.SUB_TREE_CASES[name][0]
    n_act = len(c["model"].active)
    assert {16: 4 <= n_act <= 16, 32: 17 <= n_act <= 32}[pt] and c["model"].N == 12 and c["fixed"].shape == (12, n_act)
    xa = c["x"][:, c["prob"].ACT]
    ref.bar(ref.reference(c["prob"], xa)["d0"])                 # (asserts d0 <= 1e-8)
    z = scases.normal_z(c, 3)
    assert sref.map_err(sref.banded_map(c["ab"], c["fixed"], z), sref.dense_map(c["ab"], c["fixed"], z)) <= sref.D0_REFUSED
