"""Which camera model every public entry resolves, host side (no GPU needed): the accepted camera_model / project_func /
triangulate_func / precision combinations, the model they select, and the refusals with their exception types - all
before any device work.  The first device step of every entry is stubbed to raise ``Reached`` (with the model it was
given where one is passed): ``_lib.require_gpu``, ``calib.triangulate_pairs_dense`` and the sparse SBA solver ``sba._solve``.

The entries keep four different rules (calib.camera_model_of): FTE / EKF / skeleton match ``project_func`` by identity,
the sparse SBA entries by name, dense SBA takes the ``camera_model`` string, get_pairwise_3d_points_from_df matches
``triangulate_func`` by identity."""
import json
import os

import numpy as np
import pytest

from oracle import camera as ocam


class Reached(Exception):
    """The entry got past its camera-model checks to its first device step."""

    def __init__(self, model=None):
        super().__init__(model)
        self.model = model


def my_fisheye_projection(*a):
    return None


@pytest.fixture
def stubs(monkeypatch):
    from acinoset_amd import _lib, calib, sba

    def require_gpu():
        raise Reached()

    def triangulate_pairs_dense(*a, model="fisheye", **kw):
        raise Reached(model)

    def solve(*a, model, **kw):
        raise Reached({0: "fisheye", 1: "pinhole"}.get(model, model))     # (a name, or its acino_sba_params code)

    monkeypatch.setattr(_lib, "require_gpu", require_gpu)
    monkeypatch.setattr(calib, "triangulate_pairs_dense", triangulate_pairs_dense)
    monkeypatch.setattr(sba, "_solve", solve)


def _outcome(call):
    """("ok", model) - the model None where the entry's first device step does not take it - or the exception type."""
    try:
        out = call()
    except Reached as r:
        return "ok", r.model
    except (ValueError, NotImplementedError) as e:
        return type(e)
    return "ok", out


def _check(call, want, seen=False):
    """``want``: the model the call resolves to, or the exception type.  ``seen``: the entry hands the model to its first
    device step, so it must be reported."""
    got = _outcome(call)
    if isinstance(want, str):
        assert got[0] == "ok" and got[1] in ((want,) if seen else (None, want)), got
    else:
        assert got == want, got


def _rig(n=6):
    from acinoset_amd import synth
    K, D, R, t = synth.make_rig(n)
    return K, D, R, t


# (camera_model, project_func) -> the model, or the exception; the identity rule of FTE, EKF and the skeleton solve
def _identity_cases():
    from acinoset_amd import calib
    return [
        (None, None, "fisheye"),
        ("fisheye", None, "fisheye"),
        ("pinhole", None, "pinhole"),
        (None, calib.project_points_fisheye, "fisheye"),
        (None, calib.project_points, "pinhole"),
        ("fisheye", calib.project_points_fisheye, "fisheye"),
        ("pinhole", calib.project_points, "pinhole"),
        ("fisheye", calib.project_points, ValueError),
        ("pinhole", calib.project_points_fisheye, ValueError),
        ("kannala", None, ValueError),
        ("kannala", calib.project_points, ValueError),
        (None, ocam.project_points, NotImplementedError),          # the same name, not this package's function
        (None, ocam.project_points_fisheye, NotImplementedError),
        (None, my_fisheye_projection, NotImplementedError),
        ("fisheye", lambda *a: None, NotImplementedError),
    ]


def _fte_entries():
    from acinoset_amd import fte
    K, _, R, t = _rig()
    D = np.zeros((6, 5))                      # (valid for both models' distortion checks)
    det = np.zeros((12, 6, 20, 3))
    Ts = 1 / 120.0
    return {
        "FTEContext": lambda **kw: fte.FTEContext(det, K, D, R, t, Ts, **kw),
        "fte_solve": lambda **kw: fte.fte_solve(det[..., :2], det[..., 2], K, D, R, t, Ts, **kw),
        "fte_solve_clips": lambda **kw: fte.fte_solve_clips([det, det], K, D, R, t, Ts, **kw),
        "fte_solve_batch": lambda **kw: fte.fte_solve_batch([det], K, D, R, t, Ts, **kw),
    }


@pytest.mark.parametrize("entry", ["FTEContext", "fte_solve", "fte_solve_clips", "fte_solve_batch"])
def test_fte_entries(stubs, entry):
    from acinoset_amd import calib
    call = _fte_entries()[entry]
    for cm, pf, want in _identity_cases():
        for precision in ("f64", "bf16", "bf16_residuals"):
            # the pinhole model is fp64 only: refused in the other precisions (the fisheye model is not)
            w = ValueError if want == "pinhole" and precision != "f64" else want
            _check(lambda: call(camera_model=cm, project_func=pf, precision=precision), w, seen=entry == "fte_solve_clips")
    with pytest.raises(ValueError, match="pinhole"):
        call(camera_model="pinhole", precision="bf16")
    with pytest.raises(ValueError, match="contradicts"):
        call(camera_model="fisheye", project_func=calib.project_points)
    with pytest.raises(ValueError, match="camera_model"):
        call(camera_model="kannala")


@pytest.mark.parametrize("entry", ["ekf", "ekf_batch", "initial_state"])
def test_ekf_entries(stubs, entry):
    from acinoset_amd import ekf
    K, D, R, t = _rig()
    det = np.zeros((5, 6, 20, 3))
    s0 = np.zeros(75)
    call = dict(
        ekf=lambda **kw: ekf.ekf(det, K, D, R, t, 120.0, 0.5, (2704, 1520), states0=s0, **kw),
        ekf_batch=lambda **kw: ekf.ekf_batch([det], K, D, R, t, 120.0, 0.5, (2704, 1520), **kw),
        initial_state=lambda **kw: ekf.initial_state(det, K, D, R, t, 120.0, 0.5, **kw))[entry]
    for cm, pf, want in _identity_cases():
        _check(lambda: call(camera_model=cm, project_func=pf), want, seen=entry == "initial_state")


@pytest.fixture(scope="module")
def skel(golden_dir):
    g = np.load(os.path.join(golden_dir, "skel_fte_model.npz"))
    return g, json.loads(str(g["skeleton_json"]))


@pytest.mark.parametrize("entry", ["build_model", "solve_video"])
def test_skeleton_entries(stubs, skel, entry):
    from acinoset_amd import build
    g, sk = skel
    tables = [(list(g["parts"]), g["det"][:, c]) for c in range(g["det"].shape[1])]
    scene = (g["K"], g["D"], g["R"], g["t"])
    n = int(g["n_frames"])
    if entry == "build_model":
        def call(**kw):
            return build.build_model(sk, scene=scene, dlc_tables=tables, n_frames=n, start_frame=int(g["start_frame"]),
                                     initial_line=False, **kw)[0].camera_model
    else:
        def call(**kw):
            return build.solve_video(sk, scene=scene, dlc_tables=tables, window=n, overlap=2, **kw)
    for cm, pf, want in _identity_cases():
        _check(lambda: call(camera_model=cm, project_func=pf), want, seen=True)


def test_sparse_sba_entries_match_project_func_by_name(stubs):
    from acinoset_amd import calib, sba
    K, D, R, t = _rig(2)
    data = (np.zeros((0, 2)), np.zeros((0, 3)), np.zeros(0, int), np.zeros(0, int))
    board = ([[], []], [[], []], (2, 2))             # no board seen twice: no triangulation
    entries = {
        "points_only": lambda pf, **kw: sba.bundle_adjust_points_only(*data, K, D, R, t, pf, **kw),
        "points_and_extrinsics": lambda pf, **kw: sba.bundle_adjust_points_and_extrinsics(*data, K, D, R, t, pf, **kw),
        "sharded": lambda pf, **kw: sba.bundle_adjust_points_and_extrinsics_sharded(*data, K, D, R, t, pf, **kw),
        "board_points_only": lambda pf: sba.bundle_adjust_board_points_only(*board, K, D, R, t, None, pf),
        "board_points_and_extrinsics":
            lambda pf: sba.bundle_adjust_board_points_and_extrinsics(*board, K, D, R, t, None, pf),
    }
    cases = [
        (None, "fisheye"),
        (calib.project_points_fisheye, "fisheye"),
        (calib.project_points, "pinhole"),
        (ocam.project_points_fisheye, "fisheye"),       # the reference package's own functions, by name
        (ocam.project_points, "pinhole"),
        (my_fisheye_projection, "fisheye"),
        (lambda *a: None, NotImplementedError),
        (np.dot, NotImplementedError),
    ]
    for name, call in entries.items():
        for pf, want in cases:
            _check(lambda: call(pf), want, seen=True)
    for name in ("points_and_extrinsics", "sharded"):          # no precision rule: bf16 with pinhole reaches the solver
        _check(lambda: entries[name](calib.project_points, precision="bf16"), "pinhole", seen=True)


def test_dense_sba_entries_take_the_camera_model_string(stubs):
    from acinoset_amd import sba
    K, D, R, t = _rig()
    det = np.zeros((4, 6, 20, 3))
    pts = np.zeros((4, 20, 3))
    cases = [(None, "fisheye"), ("fisheye", "fisheye"), ("pinhole", "pinhole"), ("kannala", ValueError)]
    for cm, want in cases:
        for precision in ("f64", "bf16"):
            w = ValueError if want == "pinhole" and precision != "f64" else want
            _check(lambda: sba.bundle_adjust_dense_points_and_extrinsics(det, pts, K, D, R, t, precision=precision,
                                                                         camera_model=cm), w)
            _check(lambda: sba.refine_extrinsics_from_clips([det], K, D, R, t, 1 / 120.0, precision=precision,
                                                            camera_model=cm), w, seen=True)
        _check(lambda: sba.refine_extrinsics_from_clips([det], K, D, R, t, 1 / 120.0, camera_model=cm),   # default: bf16
               ValueError if want == "pinhole" else want, seen=True)
    with pytest.raises(ValueError, match="pinhole"):
        sba.bundle_adjust_dense_points_and_extrinsics(det, pts, K, D, R, t, precision="bf16", camera_model="pinhole")
    with pytest.raises(ValueError, match="camera_model"):
        sba.refine_extrinsics_from_clips([det], K, D, R, t, 1 / 120.0, camera_model="kannala")


def test_pairwise_triangulation_matches_triangulate_func_by_identity(stubs):
    import pandas as pd
    from acinoset_amd import calib
    K, D, R, t = _rig(2)
    df = pd.DataFrame([dict(frame=0, camera=c, marker="nose", x=1.0, y=2.0) for c in (0, 1)])
    cases = [
        (None, "fisheye"),
        (calib.triangulate_points_fisheye, "fisheye"),
        (calib.triangulate_points, "pinhole"),
        (ocam.triangulate_points_fisheye, NotImplementedError),
        (ocam.triangulate_points, NotImplementedError),
        (calib.project_points, NotImplementedError),
        (lambda *a: None, NotImplementedError),
    ]
    for tf, want in cases:
        _check(lambda: calib.get_pairwise_3d_points_from_df(df, K, D, R, t, tf), want, seen=True)
