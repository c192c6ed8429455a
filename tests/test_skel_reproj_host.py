"""The skeleton FTE in image space, the part that needs no GPU: the C ABI of acino_skel_fte_reprojection (header, export,
signature, every argument check before any device call), the Python interface (build.model_reprojection, return_reprojection,
build.detection_report) and the CPU reference tests/skel_reproj_ref.py pinned to itself.  Inputs: tests/skel_cov_cases.py."""
import copy
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import skel_cov_cases as cases
import skel_cov_ref as ref
import skel_reproj_ref as rref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "acino_skel_fte_reprojection"


def test_header_library_and_binding_carry_the_entry():
    """Fails without the feature: declared, exported, bound; the ABI version stays 3."""
    from acinoset_amd import _lib
    header = open(os.path.join(ROOT, "include", "acinoset_hip.h")).read()
    assert re.search(r"\b" + NAME + r"\s*\(", header), f"{NAME} not declared in acinoset_hip.h"
    assert "skel_reproj.hip" in _lib.SOURCES
    assert NAME in _lib.SIGNATURES and len(_lib.SIGNATURES[NAME][1]) == 17
    assert hasattr(C.CDLL(_lib.SO_PATH), NAME) and hasattr(_lib.lib(), NAME)
    assert re.search(r"#define ACINO_ABI_VERSION 3\b", header) and _lib.ABI_VERSION == 3 and _lib.lib().acino_abi_version() == 3
    assert "NOT an exact chi-square" in header                   # the header must say what mahal2 is not


def _valid_call():
    """A call that would pass every check (3 pose slots in a chain, 2 cameras, 5 active states); the device pointers are never
    dereferenced, the argument checks come first."""
    from acinoset_amd import _lib
    p = _lib.SkelFteParams()
    p.n_frames, p.n_cams, p.n_pose, p.n_ops, p.n_angles, p.n_active = 10, 2, 3, 2, 3, 5
    p.max_iter, p.h, p.model_weight, p.l1_eps, p.lam0 = 0, 1.0 / 120, 0.002, 1e-2, 1e-3
    ops = (_lib.SkelOp * 2)()
    for k, (child, parent, angle, flags) in enumerate(((1, 0, 0, 1 | 8), (2, 1, 1, 2))):
        ops[k].child, ops[k].parent, ops[k].angle, ops[k].flags = child, parent, angle, flags
        ops[k].off[0], ops[k].off[1], ops[k].off[2] = 0.1, 0.2, 0.3
    act = (C.c_int32 * 5)(0, 1, 2, 3, 3 + 3 + 1)                 # x y z, phi of part 0, theta of part 1
    fake = C.c_void_p(256)
    args = dict(p=C.byref(p), n_clips=1, camera_model=0, h_ops=ops, h_active=act, d_meas=fake, d_w=fake, d_cams=fake, d_x=fake,
                d_cov_pos=fake, gate_w=1.0 / 3.0, d_uv=fake, d_cov_uv=fake, d_res=fake, d_mahal2=fake, d_flags=fake, stream=None)
    return p, ops, act, args


def test_every_invalid_argument_is_refused_before_any_device_call():
    from acinoset_amd import _lib
    h = _lib.lib()
    fn = getattr(h, NAME)

    def refused(what, **change):
        p, ops, act, args = _valid_call()
        for k, v in change.items():
            if k.startswith("p_"):
                setattr(p, k[2:], v)
            elif k.startswith("act_"):
                act[int(k[4:])] = v
            elif k.startswith("op0_"):
                setattr(ops[0], k[4:], v)
            else:
                args[k] = v
        rc = fn(*args.values())
        msg = h.acino_last_error_string().decode()
        assert rc == -1 and "invalid argument" in msg, (change, rc, msg)
        assert what in msg, (change, msg)

    refused("params", p=None)
    refused("n_clips", n_clips=0)
    refused("camera_model", camera_model=2)
    refused("camera_model", camera_model=-1)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        refused("gate_w", gate_w=bad)
    for name in ("h_ops", "h_active", "d_meas", "d_w", "d_cams", "d_x"):
        refused("null buffer", **{name: None})
    refused("no output", d_uv=None, d_cov_uv=None, d_res=None, d_mahal2=None, d_flags=None)
    refused("d_cov_pos", d_cov_pos=None)                         # d_cov_uv asked for without d_cov_pos
    # skel_validate
    refused("n_frames", p_n_frames=0)
    refused("n_cams", p_n_cams=17)
    refused("n_active", p_n_active=65)
    refused("n_ops", p_n_ops=65)
    refused("256", p_n_pose=65, p_n_cams=2)
    # skel_program
    refused("first three active states", act_0=1)
    refused("increasing", act_4=3)
    refused("op slot out of range", op0_child=3)
    refused("op angle index out of range", op0_angle=3)
    refused("missing from the active states", op0_flags=4 | 8)    # psi of part 0 enabled but not active
    # and without d_cov_uv a NULL d_cov_pos is fine as far as the checks go: nothing to assert without a device


def test_python_interface_defaults_off_and_checks_come_before_the_gpu(golden_dir):
    import torch
    from acinoset_amd import build
    sig = inspect.signature(build.model_reprojection).parameters
    assert list(sig)[:5] == ["models", "xs", "cov", "cov_pos", "r_gate"]
    assert sig["cov"].default is True and sig["cov_pos"].default is None and sig["r_gate"].default is None
    for fn in (build.solve_models, build.solve_model, build.solve_video):
        assert inspect.signature(fn).parameters["return_reprojection"].default is False
    assert inspect.signature(build.solve_video).parameters["gate"].default is None
    g, sk = cases.load(golden_dir)
    det = np.load(os.path.join(golden_dir, "human_dlc_slice.npz"))["det"].astype(np.float64)
    model = cases.make_model(g, cases.generic_skeleton(sk), det, 8, 60)
    x = cases.iterate(g, model)
    other = copy.copy(model)
    other.h = 2 * model.h
    with pytest.raises(ValueError, match="share h"):
        build.model_reprojection([model, other], [x, x], cov=False)
    with pytest.raises(ValueError, match="must be"):
        build.model_reprojection([model], [x[:, :-1]], cov=False)
    with pytest.raises(ValueError, match="iterates"):
        build.model_reprojection([model], [x, x], cov=False)
    with pytest.raises(ValueError, match="cov_pos"):
        build.model_reprojection([model], [x], cov_pos=[np.zeros((8, 2, 3, 3))])
    blind = copy.copy(model)
    blind.weights = np.zeros_like(model.weights)
    with pytest.raises(ValueError, match="r_gate"):
        build.model_reprojection([blind], [x], cov=False)
    with pytest.raises(ValueError, match="r_gate"):
        build.model_reprojection([model], [x], cov=False, r_gate=0.0)
    with pytest.raises(ValueError, match="gate needs"):
        build.solve_video(sk, scene=(g["K"], g["D"], g["R"], g["t"]), dlc_tables=cases.tables(det, g["parts"]), gate=9.21)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="GPU"):
            build.model_reprojection([model], [x], cov=False)
        with pytest.raises(RuntimeError, match="GPU"):
            build.model_reprojection([blind], [x], cov=False, r_gate=3.0)


def test_detection_report_on_a_hand_made_report():
    """3 frames, 1 camera, 3 pose slots.  Slot 0: two weighted detections, residuals (3, -4) inside and (60, 1) outside the gate;
    slot 1: one weighted detection inside, one unweighted finite detection inside, one unweighted outside; slot 2: nothing."""
    from acinoset_amd import build
    res = np.full((3, 1, 3, 2), np.nan)
    flags = np.zeros((3, 1, 3), dtype=np.uint8)
    mahal2 = np.full((3, 1, 3), np.nan)
    res[0, 0, 0], flags[0, 0, 0], mahal2[0, 0, 0] = (3.0, -4.0), 1, 1.0
    res[1, 0, 0], flags[1, 0, 0], mahal2[1, 0, 0] = (60.0, 1.0), 1, 144.0
    res[0, 0, 1], flags[0, 0, 1], mahal2[0, 0, 1] = (1.0, -2.0), 3, 0.08
    res[1, 0, 1], flags[1, 0, 1], mahal2[1, 0, 1] = (2.0, 0.0), 0, 0.16
    res[2, 0, 1], flags[2, 0, 1], mahal2[2, 0, 1] = (90.0, 0.0), 2, 300.0
    flags[:, 0, 2] = 4
    rep = dict(res=res, flags=flags, mahal2=mahal2)
    out = build.detection_report(rep)
    assert set(out) == {"n_weighted", "mean_abs_res_px", "max_abs_res_px"}
    assert out["n_weighted"].shape == (1, 3) and out["n_weighted"][0].tolist() == [2, 1, 0]
    assert out["mean_abs_res_px"][0, 0] == (3 + 4 + 60 + 1) / 4 and out["mean_abs_res_px"][0, 1] == 1.5
    assert out["max_abs_res_px"][0, 0] == 60.0 and out["max_abs_res_px"][0, 1] == 2.0
    assert np.isnan(out["mean_abs_res_px"][0, 2]) and np.isnan(out["max_abs_res_px"][0, 2])
    out = build.detection_report(rep, gate=9.21)
    assert out["n_weighted_inside"][0].tolist() == [1, 1, 0] and out["n_weighted_outside"][0].tolist() == [1, 0, 0]
    assert out["n_unweighted_inside"][0].tolist() == [0, 1, 0] and out["n_unweighted_outside"][0].tolist() == [0, 1, 0]


# ---- the reference pinned to itself ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case(golden_dir):
    g, sk = cases.load(golden_dir)
    sk = cases.generic_skeleton(sk)
    det = np.load(os.path.join(golden_dir, "human_dlc_slice.npz"))["det"].astype(np.float64)
    scene = (g["K"], g["D"], g["R"], g["t"])
    model = cases.make_model(g, sk, det, 40, cases.SLICE_STARTS[0])
    x = cases.iterate(g, model)
    prob = cases.problem(sk, model, scene)
    cov_pos = ref.reference(prob, x[:, prob.ACT])["cov_pos"]
    return sk, scene, model, x, prob, cov_pos


def test_reference_pixel_covariance_is_symmetric_and_positive_semidefinite(case):
    sk, scene, model, x, _prob, cov_pos = case
    r = rref.reprojection(sk, x, model.meas, model.weights, scene, cov_pos=cov_pos, gate_w=float(model.weights.max()))
    S = r["cov_uv"].reshape(-1, 2, 2)
    assert np.isfinite(S).all() and np.array_equal(S[:, 0, 1], S[:, 1, 0])
    ev = np.linalg.eigvalsh(S)
    assert np.all(ev[:, 0] >= -1e-12 * ev[:, 1]) and np.all(ev[:, 1] > 0)
    assert np.array_equal(r["std_uv"].reshape(-1), np.sqrt(S[:, 0, 0] + S[:, 1, 1]))
    # missing detections exist on this input (the slot paired with no marker): their residual and distance are NaN, the pixel is not
    gone = ~np.isfinite(model.meas).all(-1)
    assert 0 < gone.sum() < gone.size
    assert np.isnan(r["res"][gone]).all() and np.isnan(r["mahal2"][gone]).all() and np.isfinite(r["uv"]).all()
    assert np.isfinite(r["res"][~gone]).all() and np.isfinite(r["mahal2"][~gone]).all()


def test_reference_distance_without_covariance_is_the_scaled_squared_residual(case):
    """cov_pos = 0: the 2 x 2 form must give res^T res wg^2 / 2, the form used without cov_pos (a few roundings apart).  Every
    third frame loses its weights and is gated with gate_w = 1 / 5 instead."""
    sk, scene, model, x, _prob, cov_pos = case
    gw = 0.2
    weights = model.weights.copy()
    weights[::3] = 0.0
    a = rref.reprojection(sk, x, model.meas, weights, scene, cov_pos=np.zeros_like(cov_pos), gate_w=gw)
    b = rref.reprojection(sk, x, model.meas, weights, scene, cov_pos=None, gate_w=gw)
    assert b["cov_uv"] is None and b["std_uv"] is None
    ok = np.isfinite(b["mahal2"])
    assert np.array_equal(ok, np.isfinite(a["mahal2"])) and ok.any()
    assert np.all(np.abs(a["mahal2"][ok] - b["mahal2"][ok]) <= 8 * np.finfo(float).eps * b["mahal2"][ok])
    want = (b["res"] ** 2).sum(-1) * np.where(weights > 0, weights, gw) ** 2 / 2
    assert np.all(np.abs(want[ok] - b["mahal2"][ok]) <= 8 * np.finfo(float).eps * want[ok])
    unweighted = ok & ~(weights > 0)
    assert unweighted.any() and np.all((a["flags"][unweighted] & 1) == 0)


def test_reference_flags_are_the_rows_the_fisher_blocks_keep(case):
    """Bit 0 is where the oracle problem has a weight (finite detection, w != 0) off the singular plane; the Fisher blocks of a
    problem whose weights are masked by bit 0 are those of the problem itself, bit for bit; and the L1 cost from the report is
    the oracle's measurement cost."""
    sk, scene, model, x, prob, _cov_pos = case
    r = rref.reprojection(sk, x, model.meas, model.weights, scene, gate_w=1.0)
    on = (r["flags"] & 1) != 0
    assert np.array_equal(on, (prob.w != 0) & (np.abs(r["z_cam"]) >= 1e-9)) and 0 < on.sum() < on.size
    assert np.all((r["flags"] & 6) == 0)
    masked = copy.copy(model)
    masked.weights = np.where(on, model.weights, 0.0)
    prob_m = cases.problem(sk, masked, scene)
    xa = x[:, prob.ACT]
    assert np.array_equal(ref.fisher_blocks(prob_m, xa), ref.fisher_blocks(prob, xa))
    want = prob.measurement_terms(xa, need_jac=False)[0]
    got = rref.measurement_cost(r, model.weights)
    assert abs(got - want) <= 1e-12 * abs(want)
