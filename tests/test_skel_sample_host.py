"""Host side of the skeleton-FTE posterior samples (no GPU): the two CPU references of tests/skel_sample_ref.py against each
other on the inputs of tests/skel_sample_cases.py, the ABI entries, the argument checks that come before any device call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import skel_cov_ref as cref
import skel_sample_cases as scases
import skel_sample_ref as sref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("acino_skel_fte_sample_workspace_bytes", "acino_skel_fte_sample")


@pytest.mark.parametrize("name", scases.NAMES)
def test_the_two_references_agree(golden_dir, name):
    """8 standard-normal samples (seed 5): banded Cholesky + banded solve against dense Cholesky + triangular solve."""
    c = scases.case(golden_dir, name)
    z = scases.normal_z(c, 8)
    db, dd = sref.banded_map(c["ab"], c["fixed"], z), sref.dense_map(c["ab"], c["fixed"], z)
    d0 = sref.map_err(db, dd)
    print(f"{name}: N {c['fixed'].shape[0]}, P {c['fixed'].shape[1]}, d0 {d0:.2e}")
    assert d0 <= 1e-8
    assert np.all(db[:, c["fixed"]] == 0) and np.all(dd[:, c["fixed"]] == 0)


def test_identity_z_gives_the_diagonal_blocks_of_the_dense_inverse(golden_dir):
    c = scases.case(golden_dir, "slice12")
    N, P = c["fixed"].shape
    delta = sref.banded_map(c["ab"], c["fixed"], sref.identity_z(N, P))
    Ai = np.linalg.inv(cref.dense(c["ab"]))
    e = sref.block_err(sref.cross_blocks(delta, 0), sref.inverse_blocks(Ai, c["fixed"], 0))
    print(f"slice12: sum_s delta_n delta_n^T against the dense inverse's diagonal blocks {e:.2e}")
    assert e <= 1e-8


def test_header_library_and_binding_carry_the_two_entries():
    from acinoset_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "acinoset_hip.h")).read()
    handle = C.CDLL(_lib.SO_PATH)
    for name in SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert hasattr(handle, name) and name in _lib.SIGNATURES
    assert re.search(r"#define ACINO_ABI_VERSION 3\b", header) and _lib.ABI_VERSION == 3 and _lib.lib().acino_abi_version() == 3
    assert "skel_sample.hip" in _lib.SOURCES and callable(build.model_samples)


def _params(n_active=36):
    from acinoset_amd import _lib
    p = _lib.SkelFteParams()
    p.n_frames, p.n_cams, p.n_pose, p.n_ops, p.n_angles, p.n_active = 100, 2, 15, 14, 15, n_active
    p.h, p.model_weight, p.l1_eps, p.lam0 = 1.0 / 120.0, 0.002, 1e-2, 1e-3
    return p


def test_workspace_bytes_is_zero_outside_the_limits():
    from acinoset_amd import _lib
    wsb = _lib.lib().acino_skel_fte_sample_workspace_bytes
    p = _params()
    one, many = wsb(C.byref(p), 1, 16), wsb(C.byref(p), 8, 16)
    assert 0 < one < many and one % 256 == 0
    assert wsb(C.byref(p), 1, 0) == 0 and wsb(C.byref(p), 1, -4) == 0 and wsb(C.byref(p), 0, 16) == 0 and wsb(None, 1, 16) == 0
    assert wsb(C.byref(_params(65)), 1, 16) == 0 and wsb(C.byref(_params(2)), 1, 16) == 0


def test_invalid_arguments_are_refused_without_a_device():
    from acinoset_amd import _lib
    fn = _lib.lib().acino_skel_fte_sample
    p = _params()
    ops, act = (_lib.SkelOp * 14)(), (C.c_int32 * 36)()
    status = (C.c_int32 * 2)()
    rows = 2 * 4 * 100                                      # clips x samples x frames
    z, xs, pos = 1 << 30, (1 << 30) + 8 * rows * 36, (1 << 30) + 16 * rows * 36           # three arrays back to back
    fake = C.c_void_p(1 << 20)

    def call(n_samples=4, d_z=z, d_xs=xs, d_pos=pos, prm=p, n_clips=2):
        return fn(C.byref(prm), n_clips, 0, ops, act, fake, fake, fake, fake, fake, fake, n_samples, C.c_void_p(d_z), C.c_void_p(d_xs),
                  C.c_void_p(d_pos), status, fake, 0, None)

    assert call() == -3                                     # (valid up to the workspace of 0 bytes: ACINO_ERR_WORKSPACE, no device call)
    for kw, what in ((dict(n_samples=0), b"n_samples"), (dict(n_samples=-3), b"n_samples"), (dict(d_z=None), b"d_z"),
                     (dict(d_xs=None), b"d_x_samples"), (dict(d_z=xs), b"overlaps d_x_samples"),
                     (dict(d_z=xs - 8), b"overlaps d_x_samples"), (dict(d_z=xs + 8 * rows * 36 - 8), b"overlaps d_x_samples"),
                     (dict(d_z=pos), b"overlaps d_pos_samples"), (dict(d_z=pos + 8 * rows * 45 - 8, d_xs=z), b"overlaps d_pos_samples"),
                     (dict(prm=_params(65)), b"n_active"), (dict(n_clips=0), b"n_clips")):
        assert call(**kw) == -1, kw
        assert what in _lib.lib().acino_last_error_string(), (kw, _lib.lib().acino_last_error_string())


def test_python_argument_checks_come_before_the_gpu(golden_dir):
    import torch
    from acinoset_amd import build
    c = scases.case(golden_dir, "slice12")
    model, x = c["model"], c["x"]
    n_act = len(model.active)
    with pytest.raises(ValueError, match="n_samples"):
        build.model_samples([model], [x])
    with pytest.raises(ValueError, match="n_samples"):
        build.model_samples([model], [x], n_samples=0)
    with pytest.raises(ValueError, match="z must be"):
        build.model_samples([model], [x], z=np.zeros((1, 2, model.N, n_act + 1)))
    with pytest.raises(ValueError, match="z must be"):
        build.model_samples([model], [x], z=np.zeros((2, 2, model.N, n_act)))
    with pytest.raises(ValueError, match="holds"):
        build.model_samples([model], [x], n_samples=3, z=np.zeros((1, 2, model.N, n_act)))
    with pytest.raises(ValueError, match="finite"):
        build.model_samples([model], [x], z=np.full((1, 2, model.N, n_act), np.nan))
    with pytest.raises(ValueError, match="iterates"):
        build.model_samples([model], [x, x], n_samples=2)
    with pytest.raises(TypeError, match="not one posterior"):
        build.solve_video(c["sk"], scene=c["scene"], dlc_tables=[], n_samples=4)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="GPU"):
            build.model_samples([model], [x], n_samples=2)
