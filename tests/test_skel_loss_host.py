"""The redescending loss of the skeleton FTE, the part that needs no GPU: the CPU reference tests/skel_loss_ref.py (its gradient
against central differences of its own cost, its curvature weights), the C ABI (the params block carries ``loss`` at an
unchanged size; the new entry is declared, exported and bound; refusals that come before any device call) and the Python
interface's host-side refusals (build.build_model / solve_models / model_calibration_sensitivity / solve_video).
Every test fails without the feature."""
import ctypes as C
import inspect
import json
import os
import re

import numpy as np
import pytest

from oracle import loss as oloss

import skel_loss_ref as lref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx(golden_dir):
    g = np.load(os.path.join(golden_dir, "skel_fte_model.npz"))
    return g, json.loads(str(g["skeleton_json"]))


def _problem(g, sk):
    return lref.RobustSkelFTEProblem(sk, g["meas"], g["meas_err_weight"], g["K"], g["D"], g["R"], g["t"], float(g["h"]))


def test_reference_gradient_equals_central_differences_of_its_cost(fx):
    """The 8-frame fixture at its straight-line start (every residual far out: the saturated zone) and at the fixture's own
    gradient iterate: the measurement gradient against central differences (step 1e-6) of the per-frame measurement cost - the
    term the reference overrides; smoothness is the oracle's - to 4e-9 of the largest entry."""
    g, sk = fx
    prob = _problem(g, sk)
    act = prob.ACT
    for X in (g["init_x"], g["case_x"][int(g["grad_case"])]):
        x = np.asarray(X[:, act], dtype=np.float64)
        cost, grad, H, _nb = prob.measurement_terms(x)
        assert abs(cost - prob.measurement_terms(x, need_jac=False, per_frame=True)[0].sum()) < 1e-12 * cost
        fd = np.zeros_like(grad)
        for p in range(x.shape[1]):
            xp, xm = x.copy(), x.copy()
            xp[:, p] += 1e-6
            xm[:, p] -= 1e-6
            fd[:, p] = (prob.measurement_terms(xp, need_jac=False, per_frame=True)[0]
                        - prob.measurement_terms(xm, need_jac=False, per_frame=True)[0]) / 2e-6
        err = float(np.abs(grad - fd).max() / np.abs(fd).max())
        print(f"gradient against central differences: {err:.2e} of the largest entry {np.abs(fd).max():.1f}")
        assert err < 4e-9
        assert np.abs(H - np.swapaxes(H, 1, 2)).max() <= 1e-12 * np.abs(H).max()
        assert (np.linalg.eigvalsh(H) > -1e-9 * np.abs(H).max()).all()          # h >= 0: every block is positive semidefinite


def test_curvature_weight_lies_in_the_unit_interval_and_dropped_rows_count_for_nothing(fx):
    e = np.concatenate([[0.0, 1e-13, 1e-9], np.linspace(-60.0, 60.0, 4001), np.logspace(-8, 3, 200)])
    rho, drho, h = oloss.redescending_dloss(e, *lref.ABC)
    assert (h >= 0).all() and (h <= 1).all() and h[np.abs(e) < 1.0].min() > 0.9 and h[np.abs(e) > 25.0].max() < 0.05
    assert abs(rho[0]) > 1e-3                    # rho(0) != 0: why the reference masks the rows without a weight
    g, sk = fx
    prob = _problem(g, sk)
    x = g["init_x"][:, prob.ACT]
    c0 = prob.measurement_terms(x, need_jac=False)[0]
    fewer = lref.RobustSkelFTEProblem(sk, g["meas"], np.where(np.arange(g["meas"].shape[2])[None, None, :] == 3, 0.0, g["meas_err_weight"]),
                                      g["K"], g["D"], g["R"], g["t"], float(g["h"]))
    c1 = fewer.measurement_terms(x, need_jac=False, per_frame=True)[0].sum()
    rep = lref.report(sk, g["init_x"], g["meas"], g["meas_err_weight"], (g["K"], g["D"], g["R"], g["t"]), gate_w=1.0 / 3.0)
    on3 = ((rep["flags"] & 1) != 0) & (np.arange(g["meas"].shape[2])[None, None, :] == 3)
    rho3 = oloss.redescending_dloss(rep["e"], *lref.ABC)[0][on3].sum()
    assert on3.any() and abs((c0 - c1) - rho3) < 1e-10 * c0
    assert (rep["weight"] >= 0).all() and (rep["weight"] <= 1).all() and np.all(rep["weight"][(rep["flags"] & 1) == 0] == 0)


def test_header_binding_and_params_carry_the_loss_at_an_unchanged_size():
    from acinoset_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "acinoset_hip.h")).read()
    assert re.search(r"#define ACINO_SKEL_LOSS_L1 0\b", header) and re.search(r"#define ACINO_SKEL_LOSS_REDESCENDING 1\b", header)
    block = header[header.index("typedef struct acino_skel_fte_params"):header.index("} acino_skel_fte_params;")]
    assert re.search(r"int32_t loss;", block) and "pad0" not in block
    assert re.search(r"#define ACINO_ABI_VERSION 3\b", header) and _lib.ABI_VERSION == 3 and _lib.lib().acino_abi_version() == 3
    fields = dict((f[0], f[1]) for f in _lib.SkelFteParams._fields_)
    assert "loss" in fields and "pad0" not in fields and _lib.SkelFteParams.loss.offset == 28
    assert C.sizeof(_lib.SkelFteParams) == 96 == _lib.lib().acino_sizeof_skel_fte_params()
    assert _lib.SkelFteParams().loss == 0                          # a block that never heard of the field states L1
    assert build.LOSSES == {"l1": 0, "redescending": 1}
    name = "acino_skel_fte_reprojection_weights"
    assert re.search(r"\b" + name + r"\s*\(", header) and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES[name][1]) == len(_lib.SIGNATURES["acino_skel_fte_reprojection"][1]) + 1
    assert hasattr(C.CDLL(_lib.SO_PATH), name) and hasattr(_lib.lib(), name)
    assert "l1_start" in inspect.signature(build.solve_models).parameters
    assert inspect.signature(build.build_model).parameters["loss"].default == "l1"
    assert inspect.signature(build.solve_video).parameters["loss"].default == "l1"
    assert "weight" in build.REPROJ_KEYS


def _valid_params():
    from acinoset_amd import _lib
    p = _lib.SkelFteParams()
    p.n_frames, p.n_cams, p.n_pose, p.n_ops, p.n_angles, p.n_active = 10, 2, 3, 2, 3, 5
    p.max_iter, p.h, p.model_weight, p.l1_eps, p.lam0 = 0, 1.0 / 120, 0.002, 1e-2, 1e-3
    ops = (_lib.SkelOp * 2)()
    for k, (child, parent, angle, flags) in enumerate(((1, 0, 0, 1 | 8), (2, 1, 1, 2))):
        ops[k].child, ops[k].parent, ops[k].angle, ops[k].flags = child, parent, angle, flags
        ops[k].off[0], ops[k].off[1], ops[k].off[2] = 0.1, 0.2, 0.3
    act = (C.c_int32 * 5)(0, 1, 2, 3, 3 + 3 + 1)
    return p, ops, act


def test_the_library_refuses_an_unknown_loss_and_the_calibration_of_a_robust_problem():
    """Before any device call: the device pointers below are never dereferenced."""
    from acinoset_amd import _lib
    h = _lib.lib()
    fake = C.c_void_p(256)
    last = lambda: h.acino_last_error_string().decode()          # noqa: E731
    p, ops, act = _valid_params()
    for bad in (2, -1, 7):
        p.loss = bad
        assert h.acino_skel_fte_workspace_bytes_batch(C.byref(p), 1) > 0
        rc = h.acino_skel_fte_reprojection(C.byref(p), 1, 0, ops, act, fake, fake, fake, fake, None, 1.0, fake, None, None, None, None, None)
        assert rc == -1 and "loss" in last(), (bad, rc, last())
        rc = h.acino_skel_fte_solve_batch(C.byref(p), 1, ops, act, fake, fake, fake, fake, fake, fake, None, fake, 1 << 30, None, None)
        assert rc == -1 and "loss" in last(), (bad, rc, last())
    for loss, want in ((0, "workspace"), (1, "loss")):             # (loss 0 passes on to the next check, the workspace's size)
        p.loss = loss
        rc = h.acino_skel_fte_calibration_sensitivity(C.byref(p), 1, 0, ops, act, fake, fake, fake, fake, fake, fake, None, fake, None,
                                                      None, None, None, fake, 0, None, 0, None)
        assert rc != 0 and want in last(), (loss, rc, last())
    assert rc == -1 and "redescending" in last()


def _models(fx):
    from acinoset_amd import build
    g, sk = fx
    tabs = [(list(g["parts"]), g["det"][:, c]) for c in range(g["det"].shape[1])]
    kw = dict(scene=(g["K"], g["D"], g["R"], g["t"]), dlc_tables=tabs, n_frames=8, start_frame=60, initial_line=False)
    return build, sk, kw


def test_the_python_layer_refuses_on_the_host(fx):
    build, sk, kw = _models(fx)
    with pytest.raises(ValueError, match="loss"):
        build.build_model(sk, loss="huber", **kw)
    l1, _ = build.build_model(sk, **kw)
    rob, _ = build.build_model(sk, loss="redescending", **kw)
    assert l1.loss == "l1" and rob.loss == "redescending" and build.model_loss(rob) == "redescending"
    del l1.__dict__["loss"]
    assert build.model_loss(l1) == "l1"                          # a model built before the attribute existed
    assert build._skel_params(l1, len(l1.active)).loss == 0 and build._skel_params(rob, len(rob.active)).loss == 1
    for call in (lambda: build.solve_models([l1, rob]), lambda: build.solve_models([rob, l1], l1_start=False),
                 lambda: build.model_covariance([l1, rob], [l1.init_x, rob.init_x]),
                 lambda: build.model_reprojection([rob, l1], [l1.init_x, rob.init_x], cov=False)):
        with pytest.raises(ValueError, match="share the loss"):
            call()
    rob.loss = "cauchy"
    with pytest.raises(ValueError, match="loss"):
        build.solve_models([rob])
    rob.loss = "redescending"
    sigma = np.eye(6 * rob.meas.shape[1]) * 1e-6
    for call in (lambda: build.model_calibration_sensitivity([rob], [rob.init_x]),
                 lambda: build.model_calibration_sensitivity([rob], [rob.init_x], cov_cams=sigma),
                 lambda: build.solve_models([rob], cov_cams=sigma), lambda: build.solve_model(rob, cov_cams=sigma),
                 lambda: build.solve_video(sk, scene=kw["scene"], dlc_tables=kw["dlc_tables"], window=8, first_frame=60, last_frame=75,
                                           loss="redescending", cov_cams=sigma)):
        with pytest.raises(ValueError, match="redescending"):
            call()
    with pytest.raises(ValueError, match="loss"):
        build.solve_video(sk, scene=kw["scene"], dlc_tables=kw["dlc_tables"], window=8, first_frame=60, last_frame=75, loss="l2")


def test_detection_report_counts_what_the_weights_reject():
    from acinoset_amd import build
    flags = np.array([[[1, 1, 0]], [[1, 0, 1]]], dtype=np.uint8)                        # [N = 2, C = 1, L = 3]
    weight = np.array([[[[1.0, 1.0], [0.02, 0.9], [0.0, 0.0]]], [[[0.5, 0.09], [0.0, 0.0], [1.0, 1.0]]]])
    rep = dict(res=np.ones((2, 1, 3, 2)), flags=flags, weight=weight, mahal2=np.ones((2, 1, 3)))
    out = build.detection_report(rep)
    assert out["n_rejected"].tolist() == [[1, 1, 0]] and build.detection_report(rep, reject=0.01)["n_rejected"].sum() == 0
    assert np.allclose(out["mean_weight"], [[(1 + 1 + 0.5 + 0.09) / 4, (0.02 + 0.9) / 2, 1.0]])
    assert "n_rejected" not in build.detection_report(dict(res=rep["res"], flags=flags))
