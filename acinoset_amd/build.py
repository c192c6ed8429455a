"""Skeleton-driven Full Trajectory Estimation: the drop-in for the reference's ``src/build.py``.

Reference: ``load_skeleton`` (build.py:18-26), ``build_model(skel_dict, project_dir)`` (:28-304: sympy poses from the
skeleton dictionary, the shipped scene / DeepLabCut tables, a Pyomo NLP), ``solve_optimisation(model, exe_path,
project_dir, poses)`` (:306-335: IPOPT, then ``save_data`` -> ``data/results/traj_results.pickle``), ``convert_to_dict``
(:343-365), ``save_data`` (:367-378).  Same names, same argument meaning, same files read and written; the model object is
a plain container of arrays instead of a Pyomo model, and the solve is the projected Levenberg-Marquardt of
``csrc/skel_fte.hip`` on the GPU (``exe_path`` - the IPOPT binary - is accepted and ignored).  What is solved, with the
reference's own index quirks, is written down in oracle/skel_fte.py and DESIGN.md section 8.  The cameras are the reference's
fisheye model by default; ``camera_model="pinhole"`` (or ``project_func=calib.project_points``) on ``build_model`` /
``solve_video`` selects cv2.projectPoints (rational / tangential / thin-prism distortion), kept on the model for the solve.
"""
import ctypes as C
import glob
import os
import pickle

import numpy as np
import torch

from . import _lib, calib, fte, io, skeleton
from ._lib import MAX_CAMS, PoseFitPxParams, SkelFteInfo, SkelFteParams, SkelOp, check, lib, ptr, stream_ptr

MODEL_WEIGHT = 0.002        # build.py:186-191
R_MEAS = 3.0                # :142
LIK_THRESH = 0.4            # :145, :187
H_STEP = 1.0 / 120.0        # :131
START_FRAME, N_FRAMES = 60, 100     # :132-133
LOSSES = {"l1": 0, "redescending": 1}      # ACINO_SKEL_LOSS_L1 / ACINO_SKEL_LOSS_REDESCENDING (include/acinoset_hip.h)


def load_skeleton(skel_file):
    """build.py:18-26."""
    with open(skel_file, "rb") as handle:
        return pickle.load(handle)


def active_states(skel):
    """Indices (in the full state [x y z | phi | theta | psi], build.py:68) of the states a pose depends on: x, y, z and the
    enabled angles of every part that is the PARENT of a link (a part's own rotation only moves its children, :77)."""
    dofs = {k: list(v) for k, v in skel["dofs"].items()}
    for joint in skel["markers"]:
        dofs[joint] = [1, 1, 1]
    parts = list(dofs.keys())
    L = len(skel["positions"])
    parents = {link[0] for link in skel["links"] if len(link) == 2}
    act = [0, 1, 2]
    for axis in range(3):
        for i, part in enumerate(parts):
            if part in parents and dofs[part][axis]:
                act.append(3 + axis * L + i)
    return np.array(sorted(act), dtype=np.int32)


def bounds_table(skel, n_frames):
    """The ConstraintList of build.py:263-266, as written: |x[n, i]| <= pi/2 for the frames n = 1 .. N-1 and the 1-based state
    index i = 3 .. 3 len(positions) - 1 (the z coordinate is in, the last four angles and the last frame are out)."""
    L = len(skel["positions"])
    lo = np.full((n_frames, 3 + 3 * L), -np.inf)
    hi = np.full((n_frames, 3 + 3 * L), np.inf)
    lo[:n_frames - 1, 2:3 * L - 1] = -np.pi / 2
    hi[:n_frames - 1, 2:3 * L - 1] = np.pi / 2
    return lo, hi


def marker_pairing(skel, names, how="reference"):
    """Which detections feed pose slot l.  "reference": the marker at the same POSITION in the skeleton's marker list
    (``get_meas_from_df(n, c, l, d)`` looks up ``markers[l-1]`` while the projection uses ``pos_funcs[l-1]``, build.py:113-128
    with :288-292) - for the shipped skeletons that is NOT the part of the same name; "name": the part of the same name.
    The marker called "neck" carries no measurement (:120-121, :289)."""
    markers = list(skel["markers"])
    if how == "reference":
        return [(markers[l] if l < len(markers) and markers[l] != "neck" else None) for l in range(len(names))]
    if how == "name":
        return [n if n in markers and n != "neck" else None for n in names]
    raise ValueError("pairing must be 'reference' or 'name'")


class SkeletonModel:
    """What ``build_model`` returns in place of the Pyomo ConcreteModel: the arrays of the NLP."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def N(self):
        return int(self.meas.shape[0])

    @property
    def P(self):
        return 3 + 3 * self.prog["n_angles"]


def _rows_by_frame_value(idx, want):
    """Rows of a detection table (frame index ``idx``, one distinct value per row) that hold the frames ``want`` - looked up by
    VALUE, as the reference does (utils.py:105-120 -> ``frame == n - 1``).  A wanted frame that the table does not hold is an
    error, never the next frame's row."""
    idx = np.asarray(idx, dtype=np.int64)
    want = np.asarray(want, dtype=np.int64)
    order = np.argsort(idx)
    pos = np.searchsorted(idx[order], want)
    if idx.size == 0 or (pos >= idx.size).any() or (idx[order][np.minimum(pos, idx.size - 1)] != want).any():
        raise ValueError("frame window outside the detection tables")
    return order[pos]


def _forehead_union(tabs, lik_thresh, k_arr, d_arr, r_arr, t_arr, camera_model="fisheye"):
    """The triangulated forehead over every frame that AT LEAST TWO cameras hold (the reference's pairwise triangulation uses
    every frame a camera pair shares, calib.py:394-423) - frames, points [F, 3] (NaN where no pair sees it).  A camera without
    the frame contributes a row of likelihood 0."""
    frames = np.unique(np.concatenate([idx for _p, _v, idx in tabs]))
    held = np.stack([np.isin(frames, idx) for _p, _v, idx in tabs], axis=1)
    frames, held = frames[held.sum(1) >= 2], held[held.sum(1) >= 2]
    cols = []
    for c, (parts, vals, idx) in enumerate(tabs):
        col = np.zeros((frames.size, 1, 3))
        col[held[:, c], 0] = vals[_rows_by_frame_value(idx, frames[held[:, c]]), parts.index("forehead")]
        cols.append(col)
    tri = calib.triangulate_pairs_dense(np.stack(cols, axis=1), lik_thresh, k_arr, d_arr, r_arr, t_arr, return_masks=False,
                                        model=camera_model)
    return frames, np.asarray(tri.cpu().numpy() if isinstance(tri, torch.Tensor) else tri)[:, 0]


def _load_scene(project_dir):
    """``(k_arr, d_arr, r_arr, t_arr)`` of the reference's scene file (build.py:97-100)."""
    return io.load_scene(os.path.join(project_dir, "data", "4_cam_scene_static_sba.json"))[:4]


def _scene_distortion(camera_model, k_arr, d_arr, r_arr, t_arr):
    """The rig's distortion vectors as the model reads them: fisheye k1..k4 (the reference's ``reshape((-1, 4))``, :100), or
    the whole OpenCV pinhole vector of every camera (4, 5, 8, 12 or 14 entries; calib.pinhole_record refuses the others and
    the tilted model)."""
    if camera_model == "fisheye":
        return d_arr.reshape((-1, 4))
    d_arr = d_arr.reshape((len(k_arr), -1))
    calib.pinhole_records(k_arr, d_arr, r_arr, t_arr)
    return d_arr


def build_model(skel_dict, project_dir=None, *, scene=None, dlc_tables=None, n_frames=N_FRAMES, start_frame=START_FRAME,
                h=H_STEP, pairing="reference", lik_thresh=LIK_THRESH, r_meas=R_MEAS, model_weight=MODEL_WEIGHT, initial_line=True,
                camera_model=None, project_func=None, loss="l1", link_scales=None):
    """build.py:28-304.  ``project_dir`` is the reference's: ``data/4_cam_scene_static_sba.json`` and ``data/*.h5`` are read
    from it (:97-109); alternatively pass ``scene = (k_arr, d_arr, r_arr, t_arr)`` and ``dlc_tables`` = one
    ``(bodyparts, values[frames, K, 3])`` per camera.  ``camera_model`` "fisheye" (the default) or "pinhole", or
    ``project_func`` = calib.project_points_fisheye / calib.project_points, as calib.camera_model_of; the model keeps it as
    ``camera_model`` and every triangulation here uses it.  ``loss``: the measurement loss the model states, kept as
    ``model.loss`` and read by every call on the model - "l1" (the reference's, :299) or "redescending" (its
    ``redescending_loss`` with a, b, c = 3, 10, 20 on the residuals scaled by 1 / ``r_meas``, commented out at :307; see
    ``solve_models``).  ``link_scales`` = (groups, scales): ``scale_links`` is applied to the compiled program (the result of
    ``fit_link_scales`` for another subject than the one the skeleton file was measured on); None changes nothing.
    Returns ``(model, pose_to_3d)`` as the reference does."""
    _loss_kind(loss)
    cam_model = calib.camera_model_of(camera_model, project_func)
    prog = skeleton.compile_skeleton(skel_dict)
    names = prog["names"]
    if scene is None:
        scene = _load_scene(project_dir)
    k_arr, d_arr, r_arr, t_arr = (np.asarray(a, dtype=np.float64) for a in scene)
    d_arr = _scene_distortion(cam_model, k_arr, d_arr, r_arr, t_arr)
    if dlc_tables is None:
        paths = sorted(glob.glob(os.path.join(project_dir, "data", "*.h5")))  # :106
        dlc_tables = [io.read_dlc_table(p) for p in paths]
    C_ = len(k_arr)
    if len(dlc_tables) != C_:
        raise ValueError(f"{len(dlc_tables)} detection tables for {C_} cameras")
    # a table is (bodyparts, values[rows, K, 3]) or (bodyparts, values, frame index[rows]): the reference looks a detection up by
    # the VALUE of its frame index (utils.py:105-120 -> `frame == n - 1`), not by its row number, and every table by its own
    # body-part order
    tabs = []
    for tb in dlc_tables:
        parts, vals = list(tb[0]), np.asarray(tb[1], dtype=np.float64)
        idx = np.arange(vals.shape[0], dtype=np.int64) if len(tb) < 3 or tb[2] is None else np.asarray(tb[2], dtype=np.int64)
        if idx.shape != (vals.shape[0],) or np.unique(idx).size != idx.size:
            raise ValueError("a detection table needs one distinct frame index per row")
        tabs.append((parts, vals, idx))
    want = np.arange(start_frame, start_frame + n_frames, dtype=np.int64)
    rows = [_rows_by_frame_value(idx, want) for _parts, _vals, idx in tabs]
    # ---- measurements and weights per pose slot (:113-128, :184-206)
    pair = marker_pairing(skel_dict, names, pairing)
    Lp = len(names)
    meas = np.full((n_frames, C_, Lp, 2), np.nan)
    w = np.zeros((n_frames, C_, Lp))
    for c, (parts, vals, _idx) in enumerate(tabs):
        for l, mk in enumerate(pair):
            if mk is None or mk not in parts:
                continue
            sl = vals[rows[c], parts.index(mk)]
            meas[:, c, l] = sl[:, :2]
            w[:, c, l] = np.where(sl[:, 2] > lik_thresh, 1.0 / r_meas, 0.0)
    # ---- initial point: line through the triangulated "forehead" over ALL frames that a camera pair shares (:143-166), a
    #      regression against the frame VALUE, evaluated at 0 .. N-1 (:157)
    init_x = np.zeros((n_frames, 3 + 3 * prog["n_angles"]))
    if initial_line and all("forehead" in parts for parts, _v, _i in tabs) and C_ >= 2:   # (initial_line=False: the caller brings x0)
        common, tri = _forehead_union(tabs, lik_thresh, k_arr, d_arr, r_arr, t_arr, cam_model)
        ok = np.isfinite(tri).all(1)
        if ok.sum() >= 2:
            f = common.astype(np.float64)[ok]
            coef, *_ = np.linalg.lstsq(np.stack([f, np.ones_like(f)], 1), tri[ok], rcond=None)
            fe = np.arange(n_frames, dtype=np.float64)
            init_x[:, 0:3] = fe[:, None] * coef[0][None, :] + coef[1][None, :]
    lo, hi = bounds_table(skel_dict, n_frames)
    model = SkeletonModel(skel=skel_dict, prog=prog, names=names, active=active_states(skel_dict), meas=meas, weights=w,
                          K=k_arr, D=d_arr, R=r_arr, t=t_arr, h=float(h), lo=lo, hi=hi, init_x=init_x,
                          start_frame=int(start_frame), model_weight=float(model_weight), pairing=pair, camera_model=cam_model,
                          loss=loss, x=None, info=None)
    if link_scales is not None:
        model = scale_links(model, link_scales[1], link_scales[0])

    def pose_to_3d(*states):
        return np.asarray(skeleton.skeleton_fk(model.prog, np.asarray(states, dtype=np.float64)[None, :]))[0]
    return model, pose_to_3d


def _ops_array(prog):
    ops = (SkelOp * max(len(prog["ops"]), 1))()
    for i, (child, parent, angle, mask, untransposed, off) in enumerate(prog["ops"]):
        ops[i].child, ops[i].parent, ops[i].angle = child, parent, angle
        ops[i].flags = mask | (8 if untransposed else 0)
        ops[i].off[0], ops[i].off[1], ops[i].off[2] = off
    return ops


def _finite_diff_states(x_full, hh):
    """dx / ddx of convert_to_dict (build.py:343-365 takes them from the model's backward-Euler variables)."""
    N = x_full.shape[0]
    dx, ddx = np.zeros_like(x_full), np.zeros_like(x_full)
    if N >= 2:
        dx[1:] = (x_full[1:] - x_full[:-1]) / hh
    if N >= 3:
        ddx[2:] = (dx[2:] - dx[1:-1]) / hh
        ddx[1] = ddx[0] = ddx[2]
        dx[0] = dx[1] - hh * ddx[1]
    return dx, ddx


def _batch_camera_model(models):
    cam_models = {getattr(m, "camera_model", "fisheye") for m in models}
    if len(cam_models) > 1:
        raise ValueError("the models of one batch share the camera model (got " + " and ".join(sorted(cam_models)) + ")")
    cam_model = cam_models.pop()
    if cam_model not in calib.CAMERAS:
        raise ValueError(f"camera_model must be one of {calib.CAMERA_MODELS}")
    return cam_model


def _loss_kind(loss):
    if loss not in LOSSES:
        raise ValueError(f"loss must be one of {tuple(LOSSES)} (got {loss!r})")
    return LOSSES[loss]


def model_loss(model):
    """The measurement loss a model states: ``model.loss``, "l1" for a model without the attribute."""
    loss = getattr(model, "loss", "l1")
    _loss_kind(loss)
    return loss


def _with_loss(model, loss):
    return SkeletonModel(**{**model.__dict__, "loss": loss})


def _batch_check(models):
    m0 = models[0]
    losses = {model_loss(m) for m in models}
    if len(losses) > 1:
        raise ValueError("the models of one batch share the loss (got " + " and ".join(sorted(losses)) + ")")
    for m in models:
        if ((m.N, m.P) != (m0.N, m0.P) or repr(m.prog["ops"]) != repr(m0.prog["ops"]) or list(m.active) != list(m0.active)
                or m.meas.shape != m0.meas.shape):
            raise ValueError("the models of one batch share skeleton, active states, cameras and length")
        if not all(np.array_equal(np.asarray(getattr(m, k)), np.asarray(getattr(m0, k))) for k in ("K", "D", "R", "t")):
            raise ValueError("the models of one batch share the cameras")
        if (m.h, m.model_weight) != (m0.h, m0.model_weight):
            raise ValueError("the models of one batch share h and the model weight")


def _skel_params(m0, n_act, max_iter=0, lam0=1e-3, ftol=0.0, xtol=0.0, gtol=0.0, l1_eps=1e-2, lam_max=1e16):
    p = SkelFteParams()
    p.n_frames, p.n_cams, p.n_pose, p.n_ops = m0.N, int(m0.meas.shape[1]), len(m0.names), len(m0.prog["ops"])
    p.n_angles, p.n_active, p.max_iter = m0.prog["n_angles"], int(n_act), int(max_iter)
    p.h, p.model_weight, p.l1_eps = float(m0.h), float(m0.model_weight), float(l1_eps)
    p.lam0, p.ftol, p.xtol, p.gtol, p.lam_max = float(lam0), float(ftol), float(xtol), float(gtol), float(lam_max)
    p.loss = _loss_kind(model_loss(m0))
    return p


def _skel_inputs(models, xs, workspace_bytes=None, raw=False, start=False, **params):
    """What every batched skeleton call shares: the batch checks, the checks on ``xs`` (one [N, P] array per model), the
    parameter block (``params``: keywords of ``_skel_params``), the device arrays of the models and of ``xs`` and a workspace of
    ``workspace_bytes(p, B)`` bytes (None: the call has none).  ``raw`` (model_reprojection): the measurements and weights go to
    the device as they are, NaN kept, and there are no bounds.  ``start`` (the solve): ``xs`` are starting points - the caller's
    own copies, states outside ``model.active`` must be 0 - not iterates, which must be finite."""
    if len(models) == 0:
        raise ValueError("no models")
    cam_model = _batch_camera_model(models)
    _batch_check(models)
    m0 = models[0]
    B, N, P = len(models), m0.N, m0.P
    act = np.asarray(m0.active, dtype=np.int32)
    if len(xs) != B:
        raise ValueError(f"{len(xs)} iterates for {B} models")
    xs = [np.asarray(xf, dtype=np.float64) for xf in xs]
    inactive = np.setdiff1d(np.arange(P), act)
    for xf in xs:
        if xf.shape != (N, P):
            raise ValueError(f"x0 must be [{N}, {P}]" if start else
                             f"every x must be [{N}, {P}] (the full-state layout of results['x'])")
        if start and np.any(xf[:, inactive] != 0):
            raise ValueError("states that move no pose must start (and stay) at 0")
        if not start and not np.isfinite(xf[:, act]).all():
            raise ValueError("x must be finite")
    _lib.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    p = _skel_params(m0, len(act), **params)
    ws, tail = None, (stream_ptr(),)
    if workspace_bytes is not None:
        nbytes = workspace_bytes(p, B)
        if nbytes == 0:
            raise ValueError("problem outside the kernel limits (n_active <= 64)")
        ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=dev)
        tail = (C.c_void_p((ws.data_ptr() + 255) // 256 * 256), nbytes, stream_ptr())
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=dev)   # noqa: E731
    if raw:                                                               # a NaN detection gives a NaN residual
        meas, w, bounds = t(np.stack([m.meas for m in models])), t(np.stack([m.weights for m in models])), ()
    else:
        meas = t(np.stack([np.nan_to_num(m.meas, nan=0.0) for m in models]))
        w = t(np.stack([np.where(np.isfinite(m.meas).all(-1), m.weights, 0.0) for m in models]))
        bounds = (t(np.stack([m.lo[:, act] for m in models])), t(np.stack([m.hi[:, act] for m in models])))
    cams = torch.as_tensor(calib.camera_records(cam_model, m0.K, m0.D, m0.R, m0.t), device=dev)
    x = t(np.stack([xf[:, act] for xf in xs]))
    act_c = (C.c_int32 * len(act))(*[int(a) for a in act])
    head = (C.byref(p), B, 1 if cam_model == "pinhole" else 0, _ops_array(m0.prog), act_c, ptr(meas), ptr(w), ptr(cams),
            *[ptr(b) for b in bounds], ptr(x))
    keep = (p, ws, meas, w, cams, bounds, act_c)
    return dict(xs=xs, act=act, dev=dev, cam_model=cam_model, x=x, head=head, tail=tail, keep=keep)


def _attach(out, extras, keys, total=False):
    """Every ``results`` of ``out`` (the (results, info) pairs of a solve) takes ``keys`` from its clip's dict in ``extras``; a
    key the extras do not carry (``unobserved`` without ``pin_unobserved``) is left out.  ``total``: the extras are a share of the
    error bars (the cameras', the links') and ``std_pos_total`` is set beside the ``std_pos`` that is already there."""
    for (res, _info), ex in zip(out, extras):
        res.update({k: ex[k] for k in keys if k in ex})
        if total:
            res["std_pos_total"] = _total_std(res)


def _full_state(block, act, P, cols=False):
    """A device block over the active states, [N, n_active, ...], in the full-state layout [N, P, ...], zero outside ``act``;
    ``cols``: a square block [N, n_active, n_active], rows and columns."""
    if cols:
        full = np.zeros((block.shape[0], P, P))
        full[:, act[:, None], act[None, :]] = block
    else:
        full = np.zeros(block.shape[:1] + (P,) + block.shape[2:])
        full[:, act] = block
    return full


def _unobserved_lists(mask, act):
    """Per clip, the sorted full-state indices of the states a [B, n_active] device mask marks."""
    mh = mask.cpu().numpy()
    return [[int(a) for a in np.asarray(act)[np.nonzero(row)[0]]] for row in mh]


RATE_KEYS = ("cov_dx", "cov_ddx", "std_dx", "std_ddx", "cov_vel", "std_vel")


def _covariance(models, xs, l1_eps, want, raise_numeric=True, pin_unobserved=False):
    """model_covariance with the outputs chosen by name (``want``: a subset of cov_x, cov_pos, std_pos and of RATE_KEYS).
    ``raise_numeric=False``: a singular single clip is reported in its ``status`` like a clip of a batch.  ``pin_unobserved``: the
    _pinned entry, and ``unobserved`` in every dict.  Any of RATE_KEYS in ``want``: acino_skel_fte_covariance_rates (one
    factorisation for everything); without them the entries and their arguments are what they were."""
    pin = bool(pin_unobserved)
    rates = any(k in want for k in RATE_KEYS)
    io_ = _skel_inputs(models, xs, (lambda p, B: lib().acino_skel_fte_covariance_rates_workspace_bytes(C.byref(p), B, int(pin))) if rates else
                       (lambda p, B: lib().acino_skel_fte_covariance_pinned_workspace_bytes(C.byref(p), B, 1)) if pin else
                       (lambda p, B: lib().acino_skel_fte_covariance_workspace_bytes(C.byref(p), B)), l1_eps=l1_eps)
    m0, act, dev = models[0], io_["act"], io_["dev"]
    B, N, P = len(models), m0.N, m0.P
    Pa, Lp = len(act), len(m0.names)
    empty = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)   # noqa: E731
    cov_x = empty(B, N, Pa, Pa) if "cov_x" in want else None
    cov_pos = empty(B, N, Lp, 3, 3) if "cov_pos" in want else None
    std_pos = empty(B, N, Lp) if "std_pos" in want else None
    status = (C.c_int32 * B)()
    need_dx, need_ddx = "cov_dx" in want or "std_dx" in want, "cov_ddx" in want or "std_ddx" in want
    cov_dx = empty(B, N, Pa, Pa) if need_dx else None
    cov_ddx = empty(B, N, Pa, Pa) if need_ddx else None
    cov_vel = empty(B, N, Lp, 3, 3) if "cov_vel" in want else None
    std_vel = empty(B, N, Lp) if "std_vel" in want else None
    mask = torch.zeros((B, Pa), dtype=torch.uint8, device=dev) if pin else None
    if rates:
        rc = lib().acino_skel_fte_covariance_rates(*io_["head"], ptr(cov_x), ptr(cov_pos), ptr(std_pos), ptr(cov_dx), ptr(cov_ddx),
                                                   ptr(cov_vel), ptr(std_vel), status, *io_["tail"], int(pin), ptr(mask))
    elif pin:
        rc = lib().acino_skel_fte_covariance_pinned(*io_["head"], ptr(cov_x), ptr(cov_pos), ptr(std_pos), status, *io_["tail"], 1,
                                                    ptr(mask))
    else:
        rc = lib().acino_skel_fte_covariance(*io_["head"], ptr(cov_x), ptr(cov_pos), ptr(std_pos), status, *io_["tail"])
    if raise_numeric or rc != -6:                  # (ACINO_ERR_NUMERIC: one clip, singular - its status word and NaN arrays are set)
        check(rc)
    out = [dict(status=int(status[i])) for i in range(B)]
    if pin:
        for o, un in zip(out, _unobserved_lists(mask, act)):
            o["unobserved"] = un
    for key, std_key, arr in (("cov_x", None, cov_x), ("cov_dx", "std_dx", cov_dx), ("cov_ddx", "std_ddx", cov_ddx)):
        if arr is None:
            continue
        if key not in want:                                   # the bars alone: only the diagonals leave the device
            dg = arr.diagonal(dim1=-2, dim2=-1).contiguous().cpu().numpy()
            for i in range(B):
                out[i][std_key] = _full_state(np.sqrt(np.maximum(dg[i], 0.0)), act, P)
            continue
        ch = arr.cpu().numpy()
        for i in range(B):
            full = _full_state(ch[i], act, P, cols=True)
            if key in want:
                out[i][key] = full
            if std_key is not None and std_key in want:
                out[i][std_key] = np.sqrt(np.maximum(np.einsum("npp->np", full), 0.0))
    for key, arr in (("cov_pos", cov_pos), ("std_pos", std_pos), ("cov_vel", cov_vel), ("std_vel", std_vel)):
        if arr is not None:
            for i, c in enumerate(arr.cpu().numpy()):
                out[i][key] = c
    return out


def model_observability(models, xs, l1_eps=1e-2):
    """Which active states the detections of each clip say anything about, at the iterates ``xs`` (one [N, P] array per model):
    acino_skel_fte_observability - the Fisher assembly of ``model_covariance`` and one small reduction, no factorisation.  Returns
    one dict per model: ``info`` [P], the Fisher information sum_n H_F[n][p][p] of every state over the clip's frames (the prior
    is not in it), ``n_seen`` [P], the number of frames whose own term is above 1e-24 of the clip's largest ``info`` - both in the
    full-state layout, 0 outside ``model.active`` - and ``unobserved``, the sorted full-state indices of the ACTIVE states with
    ``info`` <= 1e-24 of the largest: no frame of the clip moves a weighted pixel with them.  The shipped human skeleton has two
    on every clip (the psi angles of "chin" and "hip2"); a limb no camera detects in the clip adds its joints.  Any such state
    makes the clip's covariance singular (status 5) unless ``pin_unobserved=True``.  A clip that is singular with an empty
    ``unobserved`` has a state with ``n_seen`` < 3: the prior's quadratic drift needs three informative frames, and such states are
    not pinned."""
    io_ = _skel_inputs(models, xs, lambda p, B: lib().acino_skel_fte_observability_workspace_bytes(C.byref(p), B), l1_eps=l1_eps)
    m0, act, dev = models[0], io_["act"], io_["dev"]
    B, P, Pa = len(models), m0.P, len(io_["act"])
    info = torch.empty((B, Pa), dtype=torch.float64, device=dev)
    seen = torch.empty((B, Pa), dtype=torch.int32, device=dev)
    mask = torch.empty((B, Pa), dtype=torch.uint8, device=dev)
    check(lib().acino_skel_fte_observability(*io_["head"], ptr(info), ptr(seen), ptr(mask), *io_["tail"]))
    ih, sh = info.cpu().numpy(), seen.cpu().numpy()
    out = []
    for i, un in enumerate(_unobserved_lists(mask, act)):
        fi, fs = np.zeros(P), np.zeros(P, dtype=np.int32)
        fi[act], fs[act] = ih[i], sh[i]
        out.append(dict(info=fi, n_seen=fs, unobserved=un))
    return out


def model_covariance(models, xs, std_only=False, l1_eps=1e-2, pin_unobserved=False, rates=False):
    """Error bars of the skeleton solve at the iterates ``xs`` (one [N, P] array per model, the layout of ``results["x"]``;
    normally the solutions): acino_skel_fte_covariance, all models in one batched call (one workgroup per clip).  Returns one
    dict per model: ``cov_x`` [N, P, P] - the frame's diagonal block of A^-1 in the full-state layout, zero rows and columns
    for the states outside ``model.active`` -, ``cov_pos`` [N, n_pose, 3, 3], ``std_pos`` [N, n_pose] (metres) and ``status``
    (0, or 5: the clip's matrix is singular - a state observed in no frame - and its arrays are NaN; for ONE model that is a
    RuntimeError, as in the solve).  ``std_only`` leaves cov_x and cov_pos out.

    A is the Fisher information of the stated model plus the smoothness prior: every weighted detection enters with w^2 (the
    L1 objective is the likelihood of Laplace noise of scale 1 / w), whatever its residual - neither the solver's IRLS curvature
    nor ``l1_eps`` enter the matrix, and outliers above the likelihood threshold are not discounted.  Variables the solver would
    hold at a bound at ``x`` are pinned (zero rows and columns; ``l1_eps`` only enters this rule, through the solver's diagonal).
    The same batch checks and camera-model selection as ``solve_models``.

    Models whose ``loss`` is "redescending": the blocks are sum w^2 h(e) J^T J, the Gauss-Newton curvature of the stated objective
    at ``x`` (the definition of ``fte.FTEContext.covariance``) - the loss is e^2 / 2 in its core, i.e. Gaussian noise of scale
    1 / w, and a detection the solve has rejected (h ~ 0, ``model_reprojection``'s ``weight``) adds no information, so a wrong
    detection no longer SHRINKS the bars.  Unlike the L1 Fisher matrix this one depends on the residuals: ``x`` should be the robust
    solution.  Pins, ``pin_unobserved`` (which goes by w^2: a row is observed whatever its h), ``rates``, ``model_samples`` and
    ``model_observability`` follow through the same build; ``model_calibration_sensitivity`` is L1 only.

    ``pin_unobserved=True`` (acino_skel_fte_covariance_pinned): the states of ``model_observability``'s ``unobserved`` are pinned
    in every frame of their clip, like bound pins and in addition to them - what the shipped human skeleton needs to get bars at
    all.  Every dict then carries ``unobserved`` (sorted full-state indices): ``cov_x`` has zero rows and columns there, and the
    list says which zeros mean "undetermined".  A pose slot whose position depends on such a state (a nonzero entry of its
    Jacobian in that column - the hand of an arm no camera detected) has ``std_pos`` = +inf and NaN ``cov_pos``; every other slot
    is G cov_x G^T as before; on the shipped skeleton no pose depends on the two psi states and every bar is finite.  The
    factorisation still decides: a state seen in one or two frames is not pinned and the clip stays status 5
    (``model_observability``'s ``n_seen`` says which).  The default keeps the definition above unchanged.

    ``rates=True`` (acino_skel_fte_covariance_rates: the same factorisation, one more streaming kernel): every dict gains the
    error bars of what a solve returns beside ``x`` - ``cov_dx`` and ``cov_ddx`` [N, P, P] in the full-state layout (zero outside
    ``model.active``; (unit/s)^2 and (unit/s^2)^2), ``std_dx`` and ``std_ddx`` [N, P], the square roots of their diagonals - and of
    the pose velocities (pose_l(x_n) - pose_l(x_n-1)) / h, frame 0 repeating frame 1: ``cov_vel`` [N, n_pose, 3, 3] in (m/s)^2
    and ``std_vel`` [N, n_pose] in m/s.  dx and ddx are exactly ``_finite_diff_states``' (the start-up rows included; N = 2:
    dx_0 = 0, ddx = 0).  sqrt(2 diag cov_x) / h is NOT that bar: the smoothness prior correlates neighbouring frames almost
    perfectly, and the exact answer uses the cross-frame blocks of A^-1 inside the 3-frame window.  Pinned variables contribute
    nothing from the frame they are pinned in; with ``pin_unobserved`` the rows and columns of the unobserved states are 0 and
    a pose that depends on one in either frame has ``std_vel`` = +inf and NaN ``cov_vel``; a singular clip has NaN everywhere.
    With ``std_only`` only ``std_dx``, ``std_ddx`` and ``std_vel`` are added, and only the diagonals of cov_dx and cov_ddx leave the
    device."""
    want = ("std_pos",) if std_only else ("cov_x", "cov_pos", "std_pos")
    if rates:
        want += ("std_dx", "std_ddx", "std_vel") if std_only else RATE_KEYS
    return _covariance(models, xs, l1_eps, want, pin_unobserved=pin_unobserved)


def model_samples(models, xs, n_samples=None, z=None, seed=0, positions=True, l1_eps=1e-2, pin_unobserved=False):
    """Joint draws of the whole trajectory from the Laplace posterior of the skeleton solve at the iterates ``xs`` (one [N, P]
    array per model, the layout of ``results["x"]``): acino_skel_fte_sample, all models in ONE batched call.  With A the matrix
    of ``model_covariance`` (Fisher blocks, smoothness prior, bound-active variables pinned) and A = L L^T,
    ``x_samples[s] = x + L^-T z[s]``: for standard-normal z the draws have covariance A^-1 with every cross-frame block - what
    step length, mean speed over a stride or the range of a joint angle over the clip need, and what the per-frame blocks of
    ``model_covariance`` cannot give.  ``z``: an optional [B][S][N][n_active] array (the map is deterministic; sample s depends
    on z[:, s] alone); otherwise ``np.random.default_rng(seed).standard_normal`` of that shape with S = ``n_samples`` is drawn
    on the host.  Returns one dict per model: ``x_samples`` [S, N, P] in the full-state layout (states outside ``model.active``
    keep ``x``'s values; pinned variables equal ``x`` exactly), ``pos_samples`` [S, N, n_pose, 3] - the forward kinematics of
    every sample, not a linearisation - unless ``positions=False``, and ``status`` (0, or 5: singular, NaN samples; for ONE
    model that is a RuntimeError, as in ``model_covariance``).  Samples are NOT clipped to the limits: the Laplace posterior is
    a Gaussian and only the pinned variables are held (``np.clip`` to ``model.lo`` / ``model.hi`` if the box matters).

    ``pin_unobserved=True`` (acino_skel_fte_sample_pinned): the clip's unobserved states (``model_observability``) are pinned in
    every frame as in ``model_covariance``; the samples equal ``x`` exactly there whatever z holds, and every dict carries
    ``unobserved``.  ``pos_samples`` of a pose that depends on an unobserved state show NO spread from that state, because it is
    held at ``x`` - where ``model_covariance`` reports std_pos = +inf; the caller finds out through ``unobserved``."""
    B = len(models)
    n_act = len(models[0].active) if B else 0
    N = models[0].N if B else 0
    if z is None:
        if n_samples is None or int(n_samples) < 1:
            raise ValueError("n_samples >= 1 (or pass z)")
        z = np.random.default_rng(seed).standard_normal((B, int(n_samples), N, n_act))
    z = np.ascontiguousarray(z, dtype=np.float64)
    if z.ndim != 4 or z.shape[0] != B or z.shape[1] < 1 or z.shape[2:] != (N, n_act):
        raise ValueError(f"z must be [{B}][S][{N}][{n_act}] (models, samples, frames, active states), S >= 1")
    if n_samples is not None and int(n_samples) != z.shape[1]:
        raise ValueError(f"n_samples = {n_samples}, z holds {z.shape[1]} samples")
    if not np.isfinite(z).all():
        raise ValueError("z must be finite")
    S = z.shape[1]
    pin = bool(pin_unobserved)
    io_ = _skel_inputs(models, xs, (lambda p, nb: lib().acino_skel_fte_sample_pinned_workspace_bytes(C.byref(p), nb, S, 1)) if pin else
                       (lambda p, nb: lib().acino_skel_fte_sample_workspace_bytes(C.byref(p), nb, S)), l1_eps=l1_eps)
    m0, act, dev = models[0], io_["act"], io_["dev"]
    zd = torch.as_tensor(z, device=dev)
    xs_d = torch.empty((B, S, N, n_act), dtype=torch.float64, device=dev)
    pos_d = torch.empty((B, S, N, len(m0.names), 3), dtype=torch.float64, device=dev) if positions else None
    status = (C.c_int32 * B)()
    if pin:
        mask = torch.zeros((B, n_act), dtype=torch.uint8, device=dev)
        check(lib().acino_skel_fte_sample_pinned(*io_["head"], S, ptr(zd), ptr(xs_d), ptr(pos_d), status, *io_["tail"], 1, ptr(mask)))
        unobs = _unobserved_lists(mask, act)
    else:
        check(lib().acino_skel_fte_sample(*io_["head"], S, ptr(zd), ptr(xs_d), ptr(pos_d), status, *io_["tail"]))
    xh = xs_d.cpu().numpy()
    ph = pos_d.cpu().numpy() if positions else None
    out = []
    for i, xf in enumerate(io_["xs"]):
        full = np.broadcast_to(xf, (S,) + xf.shape).copy()
        full[:, :, act] = xh[i]
        o = dict(x_samples=full, status=int(status[i]))
        if positions:
            o["pos_samples"] = ph[i]
        if pin:
            o["unobserved"] = unobs[i]
        out.append(o)
    return out


CALIB_KEYS = ("sens_cams", "cov_x_calib", "cov_pos_calib", "std_pos_calib")


def model_calibration_sensitivity(models, xs, cov_cams=None, l1_eps=1e-2, pin_unobserved=False):
    """The calibration's share of the skeleton solve's error bars at the iterates ``xs`` (one [N, P] array per model, the layout of
    ``results["x"]``): acino_skel_fte_calibration_sensitivity, all models in ONE batched call.  With A the matrix of
    ``model_covariance`` (Fisher blocks with w^2, smoothness prior, bound pins; ``pin_unobserved`` as there),
    ``sens_cams`` [N, P, 6C] = S = -A^-1 G is the shift of the minimiser of the expected (Fisher) quadratic model per unit change
    of c = [dw_0, dt_0, ..., dw_C-1, dt_C-1] with R_c <- exp([dw]x) R_c, t_c <- t_c + dt - the order and units of
    ``sba.covariance`` and ``calib.extrinsic_cov``.  It is consistent with the A^-1 the covariance reports (weights w^2, neither
    the residuals nor ``l1_eps`` enter G); it is not a derivative of the L1 / LM end point.  ``cov_cams``: a [6C, 6C] array or
    tensor, or the dict ``sba.covariance`` returns (its ``"cov_cams"`` is used); a wrong shape, a non-finite entry or an
    asymmetric matrix is a ValueError before any launch (``calib.cov_cams_matrix``, the validator of the cheetah path).
    Returns one dict per model: ``sens_cams``, ``cov_x_calib`` [N, P, P] = S_n cov_cams S_n^T - both in the full-state layout,
    zero rows (and columns) outside ``model.active`` and, exactly, at pinned variables -, ``cov_pos_calib`` [N, n_pose, 3, 3] =
    G_l cov_x_calib G_l^T, ``std_pos_calib`` [N, n_pose] = sqrt(trace) in metres - the last three None without ``cov_cams`` - and
    ``status`` (0, or 5: singular clip, NaN arrays; for ONE model a RuntimeError, as ``model_covariance``).  With
    ``pin_unobserved`` every dict carries ``unobserved`` and a pose slot that depends on such a state has ``std_pos_calib`` = +inf
    and NaN ``cov_pos_calib``.

    The total is ``cov + cov_calib`` (``std_pos_total = sqrt(std_pos^2 + std_pos_calib^2)``) ONLY for a calibration obtained from
    other data than the clips being solved; for extrinsics refined on the same clips the two errors are correlated and the sum
    is not valid.  The calibration term is perfectly correlated across frames: smoothing does not average it out."""
    return _calibration(models, xs, cov_cams, l1_eps, pin_unobserved)


def _refuse_robust(models, what):
    """``what``: "calibration sensitivity (cov_cams)" or "link sensitivity (cov_links)"."""
    for m in models:
        if model_loss(m) != "l1":
            raise ValueError(f"the {what} is defined for the l1 loss only; the model's loss is {model_loss(m)!r}")


def _sensitivity(models, xs, entry, cols, keys, sigma, l1_eps, pin_unobserved, raise_numeric, groups=(), unknown=None):
    """The one driver of ``_calibration`` and ``_links``: S = -A^-1 G with ``cols`` columns and the covariances ``sigma`` (a checked
    [cols, cols] matrix, or None) gives.  ``entry``: acino_skel_fte_<entry>_sensitivity with its ..._workspace_bytes; ``keys``: the
    names of S, cov_x, cov_pos, std_pos in the dicts returned - or, with the link entry's ``groups`` = (h_group, K) and ``unknown``
    ([K] uint8 or None), of S, T_l, cov_x, cov_pos, std_pos."""
    pin = bool(pin_unobserved)
    query = getattr(lib(), f"acino_skel_fte_{entry}_workspace_bytes")
    io_ = _skel_inputs(models, xs, lambda p, B: query(C.byref(p), B, int(pin)), l1_eps=l1_eps)
    m0, act, dev = models[0], io_["act"], io_["dev"]
    B, N, P = len(models), m0.N, m0.P
    Pa, Lp = len(act), len(m0.names)
    empty = lambda *shape: torch.empty((B, N) + shape, dtype=torch.float64, device=dev)   # noqa: E731
    sig_d = None if sigma is None else torch.as_tensor(sigma, dtype=torch.float64, device=dev).contiguous()
    unk_d = None if unknown is None else torch.as_tensor(unknown, device=dev).contiguous()
    arrays = [empty(Pa, cols)] + ([empty(Lp, 3, cols)] if groups else [])
    arrays += [None, None, None] if sigma is None else [empty(Pa, Pa), empty(Lp, 3, 3), empty(Lp)]
    status = (C.c_int32 * B)()
    mask = torch.zeros((B, Pa), dtype=torch.uint8, device=dev) if pin else None
    rc = getattr(lib(), f"acino_skel_fte_{entry}_sensitivity")(*io_["head"], *groups, ptr(sig_d), *((ptr(unk_d),) if groups else ()),
                                                                *[ptr(a) for a in arrays], status, *io_["tail"], int(pin), ptr(mask))
    if raise_numeric or rc != -6:                  # (ACINO_ERR_NUMERIC: one clip, singular - its status word and NaN arrays are set)
        check(rc)
    host = [None if a is None else a.cpu().numpy() for a in arrays]
    out = []
    for i in range(B):
        o = dict(zip(keys, (None if h is None else h[i] for h in host)), status=int(status[i]))
        o[keys[0]] = _full_state(o[keys[0]], act, P)
        if sigma is not None:
            o[keys[-3]] = _full_state(o[keys[-3]], act, P, cols=True)
        out.append(o)
    if pin:
        for o, un in zip(out, _unobserved_lists(mask, act)):
            o["unobserved"] = un
    return out


def _calibration(models, xs, cov_cams, l1_eps, pin_unobserved, raise_numeric=True):
    """model_calibration_sensitivity.  ``raise_numeric=False``: a singular single clip is reported in its ``status`` like a clip
    of a batch (solve_video's one-window case)."""
    if len(models) == 0:
        raise ValueError("no models")
    _refuse_robust(models, "calibration sensitivity (cov_cams)")
    Cn = int(models[0].meas.shape[1])
    return _sensitivity(models, xs, "calibration", 6 * Cn, CALIB_KEYS, calib.cov_cams_matrix(cov_cams, Cn), l1_eps, pin_unobserved,
                        raise_numeric)


LINK_KEYS = ("sens_links", "dpos_links", "cov_x_links", "cov_pos_links", "std_pos_links")


def link_cov_matrix(cov, K):
    """A covariance of the K link log-scales as ``(sigma, unknown)``: a checked float64 numpy [K, K] matrix and a bool [K] mask of
    the groups whose length nothing bounds (None, None for None).  ``cov``: a [K, K] array or tensor - a wrong shape, a
    non-finite entry or an asymmetric matrix is a ValueError, ``unknown`` is all False - or the dict ``fit_link_scales`` /
    ``fit_link_scales_pixels`` return: its ``cov_log_scales`` is used, and every group with ``observed`` False gets zero rows and
    columns and is flagged ``unknown`` (the fit left it at scale 1 with an infinite bar).  Host arithmetic, no launch."""
    if cov is None:
        return None, None
    unknown = np.zeros(int(K), dtype=bool)
    if isinstance(cov, dict):
        if "cov_log_scales" not in cov or "observed" not in cov:
            raise ValueError('cov_links given as a dict must hold "cov_log_scales" and "observed" (the dict of fit_link_scales)')
        obs = np.asarray(cov["observed"], dtype=bool)
        if obs.shape != (int(K),):
            raise ValueError(f"cov_links: observed must be [{int(K)}] (one flag per group), got {tuple(obs.shape)}")
        unknown = ~obs
        cov = cov["cov_log_scales"]
    a = cov.detach().cpu().numpy() if isinstance(cov, torch.Tensor) else np.asarray(cov)
    a = np.array(a, dtype=np.float64)
    if a.shape != (int(K), int(K)):
        raise ValueError(f"cov_links must be [{int(K)}, {int(K)}] (one log-scale per group of links), got {tuple(a.shape)}")
    a[unknown, :] = 0.0
    a[:, unknown] = 0.0
    if not np.isfinite(a).all():
        raise ValueError("cov_links has a non-finite entry")
    if not np.allclose(a, a.T, rtol=1e-12, atol=1e-12 * max(float(np.abs(a).max()), 1e-300)):
        raise ValueError("cov_links is not symmetric")
    return np.ascontiguousarray(a), unknown


def _link_inputs(model, groups, cov_links):
    """(grp [n_ops], K, sigma, unknown) of a link-sensitivity call, checked on the host.  ``groups`` None: those the dict of a
    length fit carries, else "links"."""
    if groups is None:
        groups = cov_links["groups"] if isinstance(cov_links, dict) and "groups" in cov_links else "links"
    grp, K = link_groups(model.prog, groups)
    return (grp, K) + link_cov_matrix(cov_links, K)


def model_link_sensitivity(models, xs, groups="links", cov_links=None, l1_eps=1e-2, pin_unobserved=False):
    """The link lengths' share of the skeleton solve's error bars at the iterates ``xs`` (one [N, P] array per model, the layout of
    ``results["x"]``): acino_skel_fte_link_sensitivity, all models in ONE batched call.  theta_g is the log-scale of group g of
    the link program's ops (``groups`` as ``link_groups``: "links", "global" or one index per op), theta = 0 the offsets the
    models carry - e.g. the scaled copy a length fit returns.  With A the matrix of ``model_covariance`` (Fisher blocks with w^2,
    smoothness prior, bound pins; ``pin_unobserved`` as there), ``sens_links`` [N, P, K] = S = -A^-1 G is the shift of the minimiser
    of the expected (Fisher) quadratic model per unit log-scale (weights w^2: neither the residuals nor ``l1_eps`` enter G; not a
    derivative of the L1 / LM end point), and ``dpos_links`` [N, n_pose, 3, K] = T_l = G_l S_n + D_l is what a pose does: it moves
    through the states AND directly, D_l[:, g] the sum of the rotated link vectors of group g on the slot's path.
    ``cov_links``: whatever ``link_cov_matrix`` takes - a [K, K] covariance of the log-scales, or the dict of ``fit_link_scales`` /
    ``fit_link_scales_pixels``, whose unobserved groups are flagged unknown; a malformed one is a ValueError before any launch.
    Returns one dict per model: ``sens_links``, ``cov_x_links`` [N, P, P] = S_n Sigma S_n^T - both in the full-state layout, zero
    rows (and columns) outside ``model.active`` and, exactly, at pinned variables -, ``dpos_links``, ``cov_pos_links``
    [N, n_pose, 3, 3] = T_l Sigma T_l^T, ``std_pos_links`` [N, n_pose] = sqrt(trace) in metres - the three covariance keys None
    without ``cov_links`` -, ``groups`` [n_ops] and ``status`` (0, or 5: singular clip, NaN arrays; for ONE model a RuntimeError, as
    ``model_covariance``).  A pose slot below an unknown group has ``std_pos_links`` = +inf and NaN ``cov_pos_links``; its column of
    ``sens_links`` is reported all the same.  With ``pin_unobserved`` every dict carries ``unobserved`` and a pose slot that depends
    on such a state has ``std_pos_links`` = +inf and NaN ``cov_pos_links``.

    The total is ``cov + cov_links`` (``std_pos_total = sqrt(std_pos^2 + std_pos_links^2)``) ONLY for a length covariance that came
    from other data than the clips being solved, or for an honest prior; lengths fitted to the same clip have errors correlated
    with the trajectory's and the sum is not valid - except for the dict of ``fit_link_scales_fte`` on these clips: its
    ``cov_log_scales`` is the Schur complement of the joint posterior over (trajectory, log-scales), and with it the sums ARE that
    posterior's marginals, the correlation included.  The term is perfectly correlated across frames: smoothing does not average
    it out."""
    return _links(models, xs, groups, cov_links, l1_eps, pin_unobserved)


def _links(models, xs, groups, cov_links, l1_eps, pin_unobserved, raise_numeric=True):
    """model_link_sensitivity.  ``raise_numeric=False``: a singular single clip is reported in its ``status`` like a clip of a
    batch (solve_video's one-window case)."""
    if len(models) == 0:
        raise ValueError("no models")
    _refuse_robust(models, "link sensitivity (cov_links)")
    grp, K, sigma, unknown = _link_inputs(models[0], groups, cov_links)
    grp_c = (C.c_int32 * max(len(grp), 1))(*[int(g) for g in grp])
    out = _sensitivity(models, xs, "link", K, LINK_KEYS, sigma, l1_eps, pin_unobserved, raise_numeric, groups=(grp_c, K),
                       unknown=None if sigma is None or not unknown.any() else unknown.astype(np.uint8))
    for o in out:
        o["groups"] = grp.copy()
    return out


def _check_links(models, cov_links, groups):
    """What a solve entry checks of ``cov_links`` / ``link_groups`` before it solves; True when either keyword is in use."""
    if cov_links is None and groups is None:
        return False
    if len(models):
        _refuse_robust(models, "link sensitivity (cov_links)")
        _link_inputs(models[0], groups, cov_links)
    return True


def link_fit_system(models, xs, groups="links", l1_eps=1e-2, pin_unobserved=False, return_sens=False):
    """The reduced system of the links' log-scales with the FTE trajectory eliminated, at the iterates ``xs`` (one [N, P] array per
    model, the layout of ``results["x"]``): acino_skel_fte_link_fit_system, all models in ONE batched call.  theta, ``groups``, A
    and G are those of ``model_link_sensitivity``; C = sum w^2 J_theta^T J_theta is the theta-theta block under the same Fisher
    weights and [[A, G], [G^T, C]] the information of the joint posterior over (trajectory, log-scales).  Returns one dict per
    model: ``S`` [K, K] = C - G^T A^-1 G, the information of theta with the trajectory eliminated; ``r`` [K] = c - G^T A^-1 g_x,
    the gradient of min_x F(x, theta) to first order (g_x: the solver's gradient at x, so r is right also where the solve
    stopped short of a stationary point); ``C``; ``c`` [K] = dF/dtheta at fixed x; ``cost`` = F(x, 0), the solver's own objective;
    ``status`` (0, or 5: singular clip, NaN arrays; for ONE model a RuntimeError, as ``model_covariance``) and ``groups`` [n_ops].
    S and C are symmetric to the bit; a group on no weighted slot's path has exact zeros.  Clips that share theta add their S and
    r.  ``return_sens``: ``sens_links`` [N, P, K] - the bits of ``model_link_sensitivity`` - and ``newton`` [N, P] = -A^-1 g_x, the
    Fisher-scoring step of the trajectory, both in the full-state layout.  ``pin_unobserved`` as ``model_covariance``; every dict
    then carries ``unobserved``.  Refused for models of the redescending loss."""
    return _link_fit_system(models, xs, groups, l1_eps, pin_unobserved, return_sens)


def _link_fit_system(models, xs, groups, l1_eps, pin_unobserved, return_sens, raise_numeric=True):
    """link_fit_system.  ``raise_numeric=False``: a singular single clip is reported in its ``status`` like a clip of a batch."""
    if len(models) == 0:
        raise ValueError("no models")
    _refuse_robust(models, "link fit (link_fit_system)")
    grp, K, _sigma, _unknown = _link_inputs(models[0], groups, None)
    grp_c = (C.c_int32 * max(len(grp), 1))(*[int(g) for g in grp])
    pin = bool(pin_unobserved)
    io_ = _skel_inputs(models, xs, lambda p, B: lib().acino_skel_fte_link_fit_workspace_bytes(C.byref(p), B, int(pin)), l1_eps=l1_eps)
    m0, act, dev = models[0], io_["act"], io_["dev"]
    B, N, P, Pa = len(models), m0.N, m0.P, len(act)
    empty = lambda *shape: torch.empty((B,) + shape, dtype=torch.float64, device=dev)   # noqa: E731
    arrays = dict(S=empty(K, K), r=empty(K), C=empty(K, K), c=empty(K), cost=empty())
    sens, newton = (empty(N, Pa, K), empty(N, Pa)) if return_sens else (None, None)
    status = (C.c_int32 * B)()
    mask = torch.zeros((B, Pa), dtype=torch.uint8, device=dev) if pin else None
    rc = lib().acino_skel_fte_link_fit_system(*io_["head"], grp_c, K, *[ptr(a) for a in arrays.values()], ptr(sens), ptr(newton), status,
                                              *io_["tail"], int(pin), ptr(mask))
    if raise_numeric or rc != -6:                  # (ACINO_ERR_NUMERIC: one clip, singular - its status word and NaN arrays are set)
        check(rc)
    host = {k: a.cpu().numpy() for k, a in arrays.items()}
    out = [dict({k: (float(h[i]) if k == "cost" else h[i]) for k, h in host.items()}, status=int(status[i]), groups=grp.copy())
           for i in range(B)]
    if return_sens:
        sh, nh = sens.cpu().numpy(), newton.cpu().numpy()
        for i, o in enumerate(out):
            o["sens_links"], o["newton"] = _full_state(sh[i], act, P), _full_state(nh[i], act, P)
    if pin:
        for o, un in zip(out, _unobserved_lists(mask, act)):
            o["unobserved"] = un
    return out


def _total_std(res):
    """std_pos_total of a ``results`` that holds ``std_pos``: the shares that are there (``std_pos_links``, ``std_pos_calib``), in
    quadrature."""
    var = res["std_pos"] ** 2
    for key in ("std_pos_links", "std_pos_calib"):
        if res.get(key) is not None:
            var = var + res[key] ** 2
    return np.sqrt(var)


REPROJ_KEYS = ("uv", "cov_uv", "std_uv", "res", "mahal2", "flags", "weight")


def model_reprojection(models, xs, cov=True, cov_pos=None, r_gate=None, l1_eps=1e-2, pin_unobserved=False):
    """The skeleton solve seen in the images at the iterates ``xs`` (one [N, P] array per model, the layout of ``results["x"]``):
    acino_skel_fte_reprojection, all models in ONE batched call of one streaming kernel.  Returns one dict per model, every
    array indexed [N, C, n_pose] like ``model.meas`` / ``model.weights``:

    ``uv`` [.., 2] the predicted pixel (NaN on a camera's singular plane); ``cov_uv`` [.., 2, 2] = J_pi cov_pos J_pi^T in px^2
    and ``std_uv`` = sqrt(trace); ``res`` [.., 2] = uv - detection for every FINITE detection whatever its weight (NaN for a
    missing one: the measurements go to the device raw); ``mahal2`` = res^T (cov_uv + (2 r^2) I)^-1 res with r = 1 / w for a
    weighted detection and ``r_gate`` (px; default 1 / max(model.weights): the R of the weighted ones) for the others, so that
    a low-likelihood detection can be asked whether it agrees with the trajectory all the same; ``flags`` (uint8) bit 0: the
    solve weights this detection, bit 1: behind the camera, bit 2: singular plane.

    The objective is plain L1 - every weighted detection pulls with the same force however wrong it is - so ``mahal2`` is the
    one number that says which detections the trajectory contradicts.  2 r^2 is the variance of the stated Laplace noise:
    a moment-matched gating distance, not an exact chi-square.

    ``cov=True`` without ``cov_pos`` (one [N, n_pose, 3, 3] array per model, normally ``model_covariance``'s at the same x)
    computes it first; a clip whose covariance is singular then gets NaN ``cov_uv`` / ``std_uv`` / ``mahal2`` and
    ``cov_status`` 5 in its dict (else 0) - nothing is raised, ``uv`` / ``res`` / ``flags`` stand.  ``cov=False``: ``cov_uv`` and
    ``std_uv`` are None and ``mahal2`` is res^T res / (2 r^2); no factorisation at all, so this also serves the shipped human
    skeleton, whose covariance is singular by definition.  Batch checks and camera-model selection as ``model_covariance``.

    ``pin_unobserved=True`` reaches the covariance this call computes itself (``cov=True`` without ``cov_pos``): the shipped
    skeleton then gets ``cov_status`` 0 and finite ``cov_uv`` / ``mahal2``; a pose slot that depends on an unobserved state has NaN
    ``cov_pos`` and therefore NaN ``cov_uv`` / ``std_uv`` / ``mahal2``, and the dict carries ``unobserved`` beside ``cov_status``.

    ``weight`` [.., 2] (acino_skel_fte_reprojection_weights): what each component of a detection counts for in the curvature of
    the model's loss at ``x``.  A "redescending" model: h(w res_d) in [0, 1] for a weighted detection - 1: it counts fully, ~0: the
    solve has rejected it - and 0 for the others; the covariance of such a model uses exactly w^2 h.  An "l1" model: 1 for a
    weighted detection (L1 rejects nothing), 0 otherwise.  For a "redescending" model ``mahal2`` uses the noise variance r^2 in place
    of 2 r^2 (the loss is e^2 / 2 in its core: Gaussian noise of scale r), ``cov=False``: res^T res / r^2."""
    if len(models) == 0:
        raise ValueError("no models")
    m0 = models[0]
    B, N = len(models), m0.N
    Cn, Lp = int(m0.meas.shape[1]), len(m0.names)
    if r_gate is None:
        w_max = max(float(np.nanmax(np.asarray(m.weights), initial=0.0)) for m in models)
        if not w_max > 0:
            raise ValueError("no positive weight in the models: pass r_gate (px), the noise scale of an unweighted detection")
        r_gate = 1.0 / w_max
    r_gate = float(r_gate)
    if not (r_gate > 0 and np.isfinite(r_gate)):
        raise ValueError("r_gate must be positive and finite (px)")
    if cov_pos is not None:
        if not cov:
            raise ValueError("cov_pos given with cov=False")
        if len(cov_pos) != B:
            raise ValueError(f"{len(cov_pos)} cov_pos arrays for {B} models")
        cov_pos = [np.asarray(cp, dtype=np.float64) for cp in cov_pos]
        for cp in cov_pos:
            if cp.shape != (N, Lp, 3, 3):
                raise ValueError(f"every cov_pos must be [{N}, {Lp}, 3, 3]")
    cov_status = cov_unobs = None
    if cov and cov_pos is None:
        covs = _covariance(models, xs, l1_eps, ("cov_pos",), raise_numeric=False, pin_unobserved=pin_unobserved)
        cov_pos, cov_status = [cv["cov_pos"] for cv in covs], [cv["status"] for cv in covs]
        if pin_unobserved:
            cov_unobs = [cv["unobserved"] for cv in covs]
    io_ = _skel_inputs(models, xs, raw=True, l1_eps=l1_eps)
    dev = io_["dev"]
    cp_d = torch.as_tensor(np.ascontiguousarray(np.stack(cov_pos), dtype=np.float64), device=dev) if cov else None
    empty = lambda *shape: torch.empty((B, N, Cn, Lp) + shape, dtype=torch.float64, device=dev)   # noqa: E731
    uv, res, m2 = empty(2), empty(2), empty()
    cuv = empty(2, 2) if cov else None
    flags = torch.empty((B, N, Cn, Lp), dtype=torch.uint8, device=dev)
    wt = empty(2)
    check(lib().acino_skel_fte_reprojection_weights(*io_["head"], ptr(cp_d), 1.0 / r_gate, ptr(uv), ptr(cuv), ptr(res), ptr(m2),
                                                    ptr(flags), ptr(wt), *io_["tail"]))
    uv, res, m2, flags, wt = uv.cpu().numpy(), res.cpu().numpy(), m2.cpu().numpy(), flags.cpu().numpy(), wt.cpu().numpy()
    cuv = cuv.cpu().numpy() if cov else None
    out = []
    for i in range(B):
        o = dict(uv=uv[i], cov_uv=None, std_uv=None, res=res[i], mahal2=m2[i], flags=flags[i], weight=wt[i])
        if cov:
            o["cov_uv"] = cuv[i]
            o["std_uv"] = np.sqrt(np.maximum(cuv[i][..., 0, 0] + cuv[i][..., 1, 1], 0.0))
        if cov_status is not None:
            o["cov_status"] = cov_status[i]
        if cov_unobs is not None:
            o["unobserved"] = cov_unobs[i]
        out.append(o)
    return out


def detection_report(reproj, gate=None, reject=0.1):
    """Summary of one dict of ``model_reprojection`` (or of the ``uv`` ... ``flags`` entries of a solve's results) per (camera,
    pose slot), as a dict of numpy arrays [C, n_pose]: ``n_weighted`` the detections the solve weighted (bit 0 of the flags),
    ``mean_abs_res_px`` the mean of |res| over their components - the quantity the L1 objective sums, and what
    ``window_residual_px`` averages per window - and ``max_abs_res_px`` (both NaN where nothing is weighted).  With ``gate`` - a
    chi-square quantile with 2 degrees of freedom the caller picks, e.g. 9.21 - also the finite detections inside / outside
    ``mahal2 <= gate``, split by bit 0: ``n_weighted_inside``, ``n_weighted_outside``, ``n_unweighted_inside`` (low-likelihood
    detections that agree with the trajectory all the same) and ``n_unweighted_outside``, as ``fte.detection_report`` counts
    them.  With ``weight`` in the dict (``model_reprojection`` returns it for every model) also ``mean_weight``, the mean of the
    curvature weights over the components of the weighted detections (NaN where nothing is weighted; 1 for an "l1" model), and
    ``n_rejected``, the weighted detections with a component below ``reject``: what a "redescending" solve has switched off.
    Host arithmetic on the arrays given; no kernel."""
    res, flags = np.asarray(reproj["res"]), np.asarray(reproj["flags"])
    weighted = (flags & 1) != 0
    n_w = weighted.sum(axis=0)
    ar = np.abs(np.where(weighted[..., None], res, 0.0))
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = np.where(n_w > 0, ar.sum(axis=(0, -1)) / (2 * np.maximum(n_w, 1)), np.nan)
    out = dict(n_weighted=n_w, mean_abs_res_px=mean, max_abs_res_px=np.where(n_w > 0, ar.max(axis=(0, -1), initial=0.0), np.nan))
    if gate is not None:
        m2 = np.asarray(reproj["mahal2"])
        finite = np.isfinite(m2)
        inside = finite & (np.where(finite, m2, np.inf) <= float(gate))
        outside = finite & ~inside
        out.update(n_weighted_inside=(inside & weighted).sum(axis=0), n_weighted_outside=(outside & weighted).sum(axis=0),
                   n_unweighted_inside=(inside & ~weighted).sum(axis=0),
                   n_unweighted_outside=(outside & ~weighted).sum(axis=0))
    if reproj.get("weight") is not None:
        wt = np.asarray(reproj["weight"])
        with np.errstate(divide="ignore", invalid="ignore"):
            out["mean_weight"] = np.where(n_w > 0, np.where(weighted[..., None], wt, 0.0).sum(axis=(0, -1)) / (2 * np.maximum(n_w, 1)),
                                          np.nan)
        out["n_rejected"] = (weighted & (wt.min(axis=-1) < float(reject))).sum(axis=0)
    return out


INITS = ("line", "pose_fit")


def _check_init(init):
    if init not in INITS:
        raise ValueError(f"init must be 'line' or 'pose_fit' (got {init!r})")


def _skel_workspace(model, act, workspace_bytes):
    """The params block of a per-frame fit and the bytes ``workspace_bytes`` asks for it; ValueError when it refuses the shape."""
    p = _skel_params(model, len(act))
    nbytes = workspace_bytes(C.byref(p))
    if nbytes == 0:
        raise ValueError("problem outside the kernel limits (n_active <= 64)")
    return p, nbytes


def _skel_fit_call(model, act, dev, sized, call, box=True):
    """The skeleton's side of a per-frame fit's library call: the boxes at the columns ``act`` on the device, ``sized`` (the pair
    of ``_skel_workspace``), the workspace aligned to 256 bytes, the active states as int32.  ``call(skel, box, ws)`` returns the
    status: ``skel`` = (params, ops, active), ``box`` = (lo, hi) - () with ``box=False``, for an entry that reads no box -,
    ``ws`` = (workspace, its bytes, stream)."""
    p, nbytes = sized
    lo_hi = [calib._to_dev(b[:, act], dev) for b in (model.lo, model.hi)] if box else []
    ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=dev)      # (it goes back to the allocator of this very stream)
    act_c = (C.c_int32 * len(act))(*[int(a) for a in act])
    check(call((C.byref(p), _ops_array(model.prog), act_c), tuple(ptr(b) for b in lo_hi),
               (C.c_void_p((ws.data_ptr() + 255) // 256 * 256), nbytes, stream_ptr())))


def pose_fit(model, points, cov=None, x0=None, prior_sigma=np.pi, sigma_iso=0.01, min_markers=1, max_iter=100, ftol=1e-10,
             xtol=1e-10, lam0=1e-3, return_cov=True):
    """Per-frame pose of a ``SkeletonModel`` from 3-D points with a covariance each (include/acinoset_hip.h:
    acino_skel_pose_fit; ``fte.pose_fit`` for a skeleton): per frame the minimiser over the ``model.active`` states, inside the
    frame's box ``model.lo`` / ``model.hi``, of

        F(x) = 1/2 sum_{l enters} (FK_l(x) - y_l)^T W_l (FK_l(x) - y_l) + 1/2 sum_{p >= 3} (x_p - m_p)^2 / prior_sigma^2

    by one projected Levenberg-Marquardt per frame in one launch: one frame, a frame range or a clip too short for the
    smoothness prior gets a pose.  ``points`` [N, n_pose, 3] in metres (slot l is pose slot l, ``model.names``; N =
    ``model.N``) and ``cov`` [N, n_pose, 3, 3] are the ``points`` / ``cov`` of ``calib.triangulate_multiview_dense`` -
    ``model_triangulation(model)`` -, whose dict is accepted in place of ``points``; a slot enters when its values are finite
    and its covariance positive definite (W = cov^-1), and with ``cov=None`` every finite point enters with
    W = I / sigma_iso^2.  ``x0`` [N, n_active] is the start and, clipped to the box, the centre m of the ridge on the angles
    (``prior_sigma`` rad; never on x, y, z): it gives a state that moves no pose - the psi angles of "chin" and "hip2" of the
    shipped human skeleton - the value m and the variance prior_sigma^2; default: every angle 0 and the root at the mean of
    (point - rest pose) over the entering slots.  The valley along a poorly observed angle is flat under the default
    ``prior_sigma`` = pi: a quarter of such frames is still descending after the default 100 trials (status 1; README), and
    ``prior_sigma=1.0, max_iter=255`` finishes most of them.  Returns a dict:

      x [N, n_active], x_full [N, 3 + 3 L] (0 outside ``model.active``), positions [N, n_pose, 3], cost [N]; n_markers,
      status, iters uint8 [N] (status 0 stopped on ``ftol`` / ``xtol``, 1 ``max_iter`` reached or lam overflowed, 2 fewer than
      ``min_markers`` enter, 3 numeric; every floating-point output of a frame is NaN for 2 and 3); pinned uint8
      [N, n_active], the bound-active states at x; and with ``return_cov`` cov_x [N, n_active, n_active] = A_free^-1 (rows and
      columns of pinned states exactly 0), cov_positions [N, n_pose, 3, 3] = G cov_x G^T for every slot and std_positions
      [N, n_pose] in metres.

    numpy in, numpy out; CUDA tensors in, CUDA tensors out with no host copy."""
    act = np.asarray(model.active, dtype=np.int32)
    N, Pa, Lp = model.N, len(act), len(model.names)

    def launch(prm, dev, N, ins, outs):
        _skel_fit_call(model, act, dev, _skel_workspace(model, act, lib().acino_skel_pose_fit_workspace_bytes),
                       lambda skel, box, ws: lib().acino_skel_pose_fit(prm, *skel, *ins, *box, N, *outs, *ws))

    return fte._pose_fit(launch, points, cov, x0, N, Lp, act, model.P,
                         (f"points must be [{N}, {Lp}, 3] (model.N frames, one slot per pose)", f"cov must be [{N}, {Lp}, 3, 3]",
                          f"x0 must be [{N}, {Pa}] (the active states)"),
                         prior_sigma, sigma_iso, min_markers, max_iter, ftol, xtol, lam0, return_cov)


def _model_detections(model):
    """The model's own per-slot detections as det [N, C, n_pose, 3] (x, y, likelihood): ``model.meas`` with the likelihood 1
    where ``model.weights`` > 0 and 0 elsewhere, so that a weighted detection is the valid one at threshold 0.5."""
    w = np.asarray(model.weights, dtype=np.float64)
    return np.ascontiguousarray(np.concatenate([np.asarray(model.meas, dtype=np.float64), (w > 0).astype(np.float64)[..., None]],
                                               axis=-1))


def _model_sigma_px(model):
    """1 / max(``model.weights``), the model's r_meas; ValueError when no weight is positive."""
    w_max = float(np.nanmax(np.asarray(model.weights, dtype=np.float64), initial=0.0))
    if not w_max > 0:
        raise ValueError("no positive weight in the model: pass sigma_px (px), the noise scale of a detection")
    return 1.0 / w_max


def model_triangulation(model, f_scale=5.0, sigma_px=None, **kw):
    """``calib.triangulate_multiview_dense`` of the model's own per-slot detections: det = [``model.meas``,
    ``model.weights`` > 0] with threshold 0.5 (a weighted detection is a valid one), the model's cameras and camera model.
    ``sigma_px`` defaults to 1 / max(``model.weights``), the model's r_meas, so that the covariances are those of the noise the
    solve states.  ``kw`` goes to the triangulation (``max_iter``, ``xtol``).  The detections go to the device as a tensor:
    the dict holds CUDA tensors (points [N, n_pose, 3], cov [N, n_pose, 3, 3], ...), what ``pose_fit`` takes."""
    if sigma_px is None:
        sigma_px = _model_sigma_px(model)
    det = _model_detections(model)
    dev = calib._dev()
    return calib.triangulate_multiview_dense(torch.as_tensor(det, device=dev), 0.5, model.K, model.D, model.R,
                                             model.t, model=getattr(model, "camera_model", "fisheye"), f_scale=f_scale,
                                             sigma_px=float(sigma_px), **kw)


def pose_fit_start(model, **fit_kw):
    """A starting point of the solve from a pose fit of every frame, ``init_x`` [N, 3 + 3 L]: ``model_triangulation``, then
    ``pose_fit`` of its points with their covariances (``fit_kw`` goes to ``pose_fit``); the frames without a fit (status >= 2)
    are filled by ``fte.fill_unfitted_frames`` (interpolated over the fitted frames, the psi angles unwrapped first; ValueError
    when no frame has a fit) and the result is clipped to the box.  Every active state starts near the detections instead of
    at 0 - the redescending loss gives a detection further than c = 20 from its prediction neither gradient nor curvature."""
    init_x = _pose_fit_start(model, fit_kw)
    if init_x is None:
        raise ValueError("no frame has a pose fit: no slot was triangulated in the whole clip")
    return init_x


def _pose_fit_start(model, fit_kw):
    """``pose_fit_start``; None when no frame of the model has a fit."""
    act = np.asarray(model.active, dtype=np.int64)
    if not (np.asarray(model.weights) > 0).any():              # (no weighted detection: nothing to triangulate)
        return None
    fit = pose_fit(model, model_triangulation(model), return_cov=False, **fit_kw)
    fitted = fit["status"].cpu().numpy() < 2
    if not fitted.any():
        return None
    L = model.prog["n_angles"]
    xa = fte.fill_unfitted_frames(fit["x"].cpu().numpy(), fitted, psi_columns=[int(c) for c in np.nonzero(act >= 3 + 2 * L)[0]])
    init_x = np.zeros((model.N, model.P))
    init_x[:, act] = np.clip(xa, model.lo[:, act], model.hi[:, act])
    return init_x


MAX_LINK_GROUPS = 16        # LSC_MAXK of csrc/link_scale_dev.hpp


def link_groups(prog, groups="links"):
    """The group of every op of a link program as int32 [n_ops], -1 for an op whose offset stays fixed, and their number K.
    ``groups``: "links" - one group per op with a non-zero offset, in program order (ValueError above 16: pass explicit
    groups); "global" - one scale for every such op; or a sequence of n_ops ints in -1 .. K-1."""
    ops = prog["ops"]
    moving = [bool(np.any(np.asarray(op[5], dtype=np.float64) != 0.0)) for op in ops]
    if isinstance(groups, str):
        if groups == "links":
            grp = np.full(len(ops), -1, dtype=np.int32)
            grp[moving] = np.arange(sum(moving))
            if sum(moving) > MAX_LINK_GROUPS:
                raise ValueError(f"the skeleton has {sum(moving)} links with an offset; one scale per link is limited to "
                                 f"{MAX_LINK_GROUPS}: pass explicit groups")
        elif groups == "global":
            grp = np.where(moving, 0, -1).astype(np.int32)
        else:
            raise ValueError("groups must be 'links', 'global' or one group index per op")
    else:
        grp = np.asarray(groups)
        if grp.shape != (len(ops),) or not np.issubdtype(grp.dtype, np.integer):
            raise ValueError(f"groups must hold one int per op of the link program ({len(ops)}), -1 for a fixed op")
        grp = grp.astype(np.int32)
    K = int(grp.max()) + 1 if grp.size else 0
    if grp.size and grp.min() < -1 or not 1 <= K <= MAX_LINK_GROUPS:
        raise ValueError(f"group indices must be -1 .. K-1 with K in 1..{MAX_LINK_GROUPS}")
    return grp, K


def scale_links(model, scales, groups="links"):
    """A copy of ``model`` whose link program carries ``scales[group(k)] * off_k`` (``groups`` as ``link_groups``; an op of
    group -1 keeps its offset).  The copy records ``link_groups`` and ``link_scales``; ``model`` is left as it is.  Scales are
    applied to the program, not to ``skel["positions"]``: a skeleton that defines a part twice has no positions that give
    every op its scaled offset."""
    grp, K = link_groups(model.prog, groups)
    s = np.asarray(scales, dtype=np.float64)
    if s.shape != (K,) or not (np.isfinite(s).all() and (s > 0).all()):
        raise ValueError(f"scales must be {K} finite positive numbers, one per group")
    ops = [op[:5] + (np.asarray(op[5], dtype=np.float64) * (s[g] if g >= 0 else 1.0),) for op, g in zip(model.prog["ops"], grp)]
    return SkeletonModel(**{**model.__dict__, "prog": dict(model.prog, ops=ops), "link_groups": grp.copy(), "link_scales": s.copy()})


def _pose_fit_centre(model, points, cov, x0, sigma_iso):
    """m [N, n_active] of a ``pose_fit`` call: ``x0`` clipped to the box, or the kernel's own default start - what a call
    whose single trial is refused returns; 0 in the frames without a point."""
    act = np.asarray(model.active, dtype=np.int64)
    if x0 is not None:
        return np.clip(np.asarray(x0, dtype=np.float64), model.lo[:, act], model.hi[:, act])
    start = pose_fit(model, points, cov, sigma_iso=sigma_iso, lam0=1e300, max_iter=1, return_cov=False)["x"]
    return np.nan_to_num(calib._host(start), nan=0.0)


def link_scale_system(model, points, cov, fit, groups="links", prior_sigma=np.pi, sigma_iso=0.01, m=None, return_sens=True):
    """The Gauss-Newton system of the log-scales of ``model``'s links at the poses of ``fit`` = ``pose_fit(model, points, cov,
    prior_sigma=..., sigma_iso=...)``, every frame's pose eliminated (include/acinoset_hip.h: acino_skel_link_scale; one launch
    and a summing one).  ``model`` carries the current offsets (``scale_links``); ``groups`` as ``link_groups``; ``m``
    [N, n_active] is the ridge centre of the fit - its ``x0`` clipped to the box; None: the fit's default start.  Returns a dict
    of numpy arrays: S [K, K], r [K], cost and n_used (sums over the used frames, in frame order); S_frames [N, K, K],
    r_frames [N, K], cost_frames [N], used [N] bool, status [N] (the fit's, 3 where a frame's matrix has no factor) and, with
    ``return_sens``, sens [N, n_active, K] = d x / d theta (NaN for an unused frame)."""
    points, cov = _points_and_cov(points, cov)
    grp, K = link_groups(model.prog, groups)
    act = np.asarray(model.active, dtype=np.int32)
    N, Lp = model.N, len(model.names)
    if fte._shape(points) != (N, Lp, 3):
        raise ValueError(f"points must be [{N}, {Lp}, 3] (model.N frames, one slot per pose)")
    if cov is not None and fte._shape(cov) != (N, Lp, 3, 3):
        raise ValueError(f"cov must be [{N}, {Lp}, 3, 3]")
    _check_fit(fit, m, N, len(act), "pose_fit")
    for name, val in (("prior_sigma", prior_sigma), ("sigma_iso", sigma_iso)):
        if not (np.isfinite(val) and val > 0):
            raise ValueError(f"{name} must be finite and > 0")
    sized = _skel_workspace(model, act, lib().acino_skel_link_scale_workspace_bytes)
    dev = calib._dev()
    if m is None:
        m = _pose_fit_centre(model, points, cov, None, sigma_iso)
    pts, cv = calib._to_dev(points, dev), None if cov is None else calib._to_dev(cov, dev)
    return _link_scale_call(model, act, grp, K, fit, m, return_sens, dev, sized,
                            lambda skel, g, f, outs, ws: lib().acino_skel_link_scale(
                                *skel, *g, float(prior_sigma), float(sigma_iso), ptr(pts), ptr(cv), *f, N, *outs, *ws))


def _points_and_cov(points, cov):
    """``points`` may be the triangulation's dict: its points and its cov then, and ValueError when ``cov`` is given beside it."""
    if isinstance(points, dict):
        if cov is not None:
            raise ValueError("cov comes with the dict of triangulate_multiview_dense: pass one or the other")
        return points["points"], points["cov"]
    return points, cov


def _check_fit(fit, m, N, Pa, fit_name):
    """The shapes of ``fit[...]`` (``fit_name``: the pose fit the message names) and of ``m``."""
    for key, shape in (("x", (N, Pa)), ("pinned", (N, Pa)), ("status", (N,))):
        if fte._shape(fit[key]) != shape:
            raise ValueError(f"fit['{key}'] must be {list(shape)}: the result of {fit_name} on this model")
    if m is not None and fte._shape(m) != (N, Pa):
        raise ValueError(f"m must be [{N}, {Pa}] (the active states)")


def _link_scale_call(model, act, grp, K, fit, m, return_sens, dev, sized, call):
    """What ``link_scale_system`` and ``link_scale_system_pixels`` do once their checks are through and their measurement is on
    the device: the fit and ``m`` to the device, the outputs, the library call through ``_skel_fit_call`` - ``call(skel, grp, fit,
    outs, ws)`` with ``grp`` = (groups, K), ``fit`` = (x, m, pinned, status), ``outs`` = (S, r, F, used, frame_status, sens,
    total) - and the dict read back."""
    N, Pa = model.N, len(act)
    x, mc = calib._to_dev(fit["x"], dev), calib._to_dev(m, dev)
    u8 = lambda a: torch.as_tensor(a, device=dev).to(torch.uint8).contiguous()      # noqa: E731
    pinned, status = u8(fit["pinned"]), u8(fit["status"])
    f64, b8 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.uint8, device=dev)
    S, r, F = torch.empty((N, K, K), **f64), torch.empty((N, K), **f64), torch.empty((N,), **f64)
    used, fst = torch.empty((N,), **b8), torch.empty((N,), **b8)
    sens = torch.empty((N, Pa, K), **f64) if return_sens else None
    total = torch.zeros((K * K + K + 2,), **f64)
    grp_c = (C.c_int32 * max(len(grp), 1))(*[int(g) for g in grp])
    _skel_fit_call(model, act, dev, sized, lambda skel, _box, ws: call(
        skel, (grp_c, K), (ptr(x), ptr(mc), ptr(pinned), ptr(status)),
        (ptr(S), ptr(r), ptr(F), ptr(used), ptr(fst), ptr(sens), ptr(total)), ws), box=False)
    tot = total.cpu().numpy()
    return dict(S=tot[:K * K].reshape(K, K), r=tot[K * K:K * K + K], cost=float(tot[K * K + K]), n_used=int(tot[K * K + K + 1]),
                S_frames=S.cpu().numpy(), r_frames=r.cpu().numpy(), cost_frames=F.cpu().numpy(), used=used.cpu().numpy().astype(bool),
                status=fst.cpu().numpy(), groups=grp, sens=sens.cpu().numpy() if return_sens else None)


def link_scale_step(S, r, theta, lam, prior_prec=0.0):
    """One damped step on the observed groups: d = -(S_oo + lam I + prior_prec I)^-1 (r_o + prior_prec theta_o), 0 for a group
    whose diagonal entry of S is 0 (no frame observes it).  Returns d [K] and observed [K]."""
    obs = np.diag(S) > 0
    d = np.zeros(len(r))
    if obs.any():
        Soo = S[np.ix_(obs, obs)] + (lam + prior_prec) * np.eye(int(obs.sum()))
        d[obs] = -np.linalg.solve(Soo, r[obs] + prior_prec * theta[obs])
    return d, obs


def fit_link_scales(model, points=None, cov=None, groups="links", x0=None, scale_prior_sigma=None, max_outer=30, tol=1e-6,
                    prior_sigma=1.0, max_iter=255, **fit_kw):
    """The link lengths of ``model``'s skeleton from the 3-D points of a clip, with an error bar each: one scale s_g = exp(theta_g)
    per group of links (``groups`` as ``link_groups``), the minimiser over all poses and theta of the summed ``pose_fit``
    objective (plus theta^2 / (2 ``scale_prior_sigma``^2) per group when given).  ``points`` / ``cov`` as ``pose_fit`` takes
    them; None: ``model_triangulation(model)``.  The points are metric - the cameras are calibrated - so scales are observable.

    Outer Gauss-Newton on theta: ``pose_fit`` at the current scales (``prior_sigma``, ``max_iter``, ``fit_kw``), then
    ``link_scale_system`` and the step -(S + lam I + prior)^-1 (r + prior); a step is accepted when the cost summed over the
    frames both points use falls, otherwise lam is raised and the step tried again; stop on max |dtheta| < ``tol``.  The ridge
    centre m of every pose fit is the first start (``x0`` clipped to the box, or the default start at the scales 1), so that
    the objective does not move; every pose fit starts there.  A group with a zero diagonal entry of S - no frame has a point
    below it - stays at 1 with ``observed`` False and ``std`` inf; the others are solved without it.

    Returns a dict: scales [K]; cov_log_scales [K, K] = S_obs^-1 at the end point (zero rows and columns for unobserved
    groups); std_scales = s sqrt(diag) (inf where unobserved); observed [K]; groups [n_ops]; model - the scaled copy, ready for
    ``solve_models`` / ``pose_fit*``; fit - the pose fit at the end point; system - ``link_scale_system`` there; history - one
    dict per outer step (cost, max_dtheta, lam, n_used, accepted); status "ok", "max_outer" or "no_frames"."""
    grp, K = link_groups(model.prog, groups)
    _check_outer(scale_prior_sigma, max_outer, tol)
    if points is None:
        points = model_triangulation(model)
    points, cov = _points_and_cov(points, cov)
    sigma_iso = fit_kw.get("sigma_iso", 0.01)
    m = _pose_fit_centre(model, points, cov, x0, sigma_iso)

    def evaluate(theta):
        mdl = scale_links(model, np.exp(theta), grp)
        fit = _host_fit(pose_fit(mdl, points, cov, x0=m, prior_sigma=prior_sigma, max_iter=max_iter, return_cov=False, **fit_kw))
        return mdl, fit, link_scale_system(mdl, points, cov, fit, grp, prior_sigma=prior_sigma, sigma_iso=sigma_iso, m=m)

    return _fit_link_scales(evaluate, grp, K, scale_prior_sigma, max_outer, tol)


def _host_fit(fit):
    """The dict of a per-frame fit on the host: the floating-point outputs through ``calib._host``, the rest as numpy."""
    return {k: calib._host(v) if k in ("x", "x_full", "positions", "cost") else np.asarray(v.cpu() if isinstance(v, torch.Tensor) else v)
            for k, v in fit.items()}


def _check_outer(scale_prior_sigma, max_outer, tol):
    if scale_prior_sigma is not None and not (np.isfinite(scale_prior_sigma) and scale_prior_sigma > 0):
        raise ValueError("scale_prior_sigma must be finite and > 0")
    if int(max_outer) != max_outer or max_outer < 1 or not (np.isfinite(tol) and tol > 0):
        raise ValueError("max_outer must be an integer >= 1 and tol > 0")


def _fit_link_scales(evaluate, grp, K, scale_prior_sigma, max_outer, tol):
    """The outer loop of ``fit_link_scales`` and ``fit_link_scales_pixels``: ``evaluate(theta)`` returns (scaled model, pose fit,
    system) at the log-scales theta - the system the dict of ``link_scale_system``.  The damped step on the observed groups,
    the acceptance on the frames both points use, the lam rule, the stop on max |dtheta| < ``tol``, ``observed``,
    ``cov_log_scales``, the history and the returned dict."""
    prec = 0.0 if scale_prior_sigma is None else 1.0 / float(scale_prior_sigma) ** 2

    def cost_on(sys_, theta, frames):
        return float(np.add.reduce(sys_["cost_frames"][frames])) + 0.5 * prec * float(theta @ theta)

    theta = np.zeros(K)
    cur = evaluate(theta)
    lam, history, status = 0.0, [], "max_outer"
    if cur[2]["n_used"] == 0:
        status = "no_frames"
    for _ in range(int(max_outer) if status != "no_frames" else 0):
        sys_ = cur[2]
        top = float(np.diag(sys_["S"]).max())
        accepted = False
        while True:
            d, _obs = link_scale_step(sys_["S"], sys_["r"], theta, lam, prec)
            step = float(np.abs(d).max())
            if step < tol:
                break
            trial = evaluate(theta + d)
            both = sys_["used"] & trial[2]["used"]
            if both.any() and cost_on(trial[2], theta + d, both) < cost_on(sys_, theta, both):
                theta, cur, accepted = theta + d, trial, True
                lam = lam / 10.0 if lam > 1e-12 * top else 0.0
                break
            lam = max(10.0 * lam, 1e-3 * top)
        history.append(dict(cost=cost_on(cur[2], theta, cur[2]["used"]), max_dtheta=step, lam=lam, n_used=cur[2]["n_used"],
                            accepted=accepted))
        if not accepted:
            status = "ok"
            break
    mdl, fit, sys_ = cur
    obs = np.diag(sys_["S"]) > 0
    cov_t = np.zeros((K, K))
    if obs.any():
        cov_t[np.ix_(obs, obs)] = np.linalg.inv(sys_["S"][np.ix_(obs, obs)] + prec * np.eye(int(obs.sum())))
    scales = np.exp(theta)
    with np.errstate(invalid="ignore"):
        std = np.where(obs, scales * np.sqrt(np.diag(cov_t)), np.inf)
    return dict(scales=scales, cov_log_scales=cov_t, std_scales=std, observed=obs, groups=grp, model=mdl, fit=fit, system=sys_,
                history=history, status=status)


def _pixel_start(model, x0):
    """The start of ``pose_fit_pixels`` on ``model`` clipped to the box, [N, n_active]: ``x0``, or the chain of its default."""
    act = np.asarray(model.active, dtype=np.int64)
    if x0 is None:
        x0 = _default_pixel_start(model)
    return np.clip(np.asarray(calib._host(x0), dtype=np.float64), model.lo[:, act], model.hi[:, act])


def _default_pixel_start(model):
    """The default start of ``pose_fit_pixels``, [N, n_active]: the chain of ``pose_fit_start``; ValueError without a fit."""
    init_x = _pose_fit_start(model, {})
    if init_x is None:
        raise ValueError("no frame has a pose fit to start from (no slot was triangulated in the whole clip): pass x0")
    return init_x[:, np.asarray(model.active, dtype=np.int64)]


def link_scale_system_pixels(model, fit, groups="links", det=None, thresh=0.5, f_scale=5.0, sigma_px=None, prior_sigma=np.pi,
                             m=None, return_sens=True):
    """``link_scale_system`` for the objective of ``pose_fit_pixels``: the Gauss-Newton system of the log-scales of ``model``'s
    links at the poses of ``fit`` = ``pose_fit_pixels(model, det=..., thresh=..., f_scale=..., sigma_px=..., prior_sigma=...)``,
    every frame's pose eliminated (include/acinoset_hip.h: acino_skel_link_scale_px; one launch and a summing one).  No
    triangulation stands between a detection and a length: a link whose far end one camera sees at a time is constrained in
    every such frame.  The residuals carry the IRLS weights w = 1 / (1 + r^2 / f^2) at the fit's x: r is the exact gradient of
    the summed Cauchy cost in theta at the minimising poses, S its Gauss-Newton curvature.  ``model`` carries the current offsets
    (``scale_links``); ``groups`` as ``link_groups``; ``det``, ``thresh``, ``f_scale``, ``sigma_px`` and their defaults as
    ``pose_fit_pixels``; ``m`` [N, n_active] is the ridge centre of the fit - its ``x0`` clipped to the box; None: the chain of
    the fit's default start.  Works on a rig of any size; on one camera a global scale is a null direction (S = 0 for
    ``groups="global"``).  Returns the dict of ``link_scale_system``."""
    grp, K = link_groups(model.prog, groups)
    act = np.asarray(model.active, dtype=np.int32)
    N, Lp, Cn = model.N, len(model.names), int(np.shape(model.meas)[1])
    camera_model = getattr(model, "camera_model", "fisheye")
    if camera_model not in calib.CAMERAS:
        raise ValueError(f"the model's camera_model must be one of {calib.CAMERA_MODELS}")
    if det is not None and fte._shape(det) != (N, Cn, Lp, 3):
        raise ValueError(f"det must be [{N}, {Cn}, {Lp}, 3] (model.N frames, the model's cameras, one slot per pose)")
    if not 1 <= Cn <= MAX_CAMS:
        raise ValueError(f"the model holds {Cn} cameras: 1..{MAX_CAMS} are supported")
    _check_fit(fit, m, N, len(act), "pose_fit_pixels")
    if sigma_px is None:
        sigma_px = _model_sigma_px(model)
    for name, val in (("prior_sigma", prior_sigma), ("f_scale", f_scale), ("sigma_px", sigma_px)):
        if not (np.isfinite(val) and val > 0):
            raise ValueError(f"{name} must be finite and > 0")
    if np.isnan(thresh):
        raise ValueError("thresh must not be NaN")
    recs = calib.camera_records(camera_model, model.K, model.D, model.R, model.t)
    sized = _skel_workspace(model, act, lib().acino_skel_link_scale_px_workspace_bytes)
    dev = calib._dev()
    if m is None:
        m = _pixel_start(model, None)
    d, cams = calib._to_dev(_model_detections(model) if det is None else det, dev), torch.as_tensor(recs, device=dev)
    prm = PoseFitPxParams(calib.CAMERAS[camera_model].code, 1, 1, 0, 1e-3, 1e-10, 1e-10, float(prior_sigma), float(thresh),
                          float(f_scale), float(sigma_px))
    return _link_scale_call(model, act, grp, K, fit, m, return_sens, dev, sized,
                            lambda skel, g, f, outs, ws: lib().acino_skel_link_scale_px(
                                C.byref(prm), *skel, *g, ptr(d), N, Cn, ptr(cams), *f, *outs, *ws))


def fit_link_scales_pixels(model, groups="links", x0=None, det=None, thresh=0.5, f_scale=5.0, sigma_px=None,
                           scale_prior_sigma=None, max_outer=30, tol=1e-6, prior_sigma=1.0, max_iter=255, **fit_kw):
    """``fit_link_scales`` on the detections themselves: the link lengths of ``model``'s skeleton as the minimiser, over all poses
    and one log-scale per group of links (``groups`` as ``link_groups``), of the summed ``pose_fit_pixels`` objective (plus
    theta^2 / (2 ``scale_prior_sigma``^2) per group when given), with an error bar each.  ``det``, ``thresh``, ``f_scale``,
    ``sigma_px`` and their defaults as ``pose_fit_pixels``; ``fit_kw`` goes to it (``min_detections``, ``ftol``, ...).

    The outer loop is that of ``fit_link_scales``: ``pose_fit_pixels`` at the current scales (``prior_sigma``, ``max_iter``), then
    ``link_scale_system_pixels`` and the damped step.  ``x0`` [N, n_active] is the first start; None: the chain of
    ``pose_fit_pixels`` at the scales 1.  The ridge centre of every pose fit is that first start clipped to the box, and every
    pose fit starts there, so that the objective does not move.

    One camera cannot tell a larger animal further away from a smaller one nearer: on a model of one camera this raises
    ValueError unless ``scale_prior_sigma`` is given.  Returns the dict of ``fit_link_scales``."""
    grp, K = link_groups(model.prog, groups)
    _check_outer(scale_prior_sigma, max_outer, tol)
    if int(np.shape(model.meas)[1]) == 1 and scale_prior_sigma is None:
        raise ValueError("one camera does not determine the size of the skeleton (a larger animal further away gives the same "
                         "pixels): pass scale_prior_sigma")
    if sigma_px is None:
        sigma_px = _model_sigma_px(model)
    if det is None:
        det = _model_detections(model)
    m = _pixel_start(model, x0)
    px = dict(det=det, thresh=thresh, f_scale=f_scale, sigma_px=sigma_px, prior_sigma=prior_sigma)

    def evaluate(theta):
        mdl = scale_links(model, np.exp(theta), grp)
        fit = _host_fit(pose_fit_pixels(mdl, x0=m, max_iter=max_iter, return_cov=False, **px, **fit_kw))
        return mdl, fit, link_scale_system_pixels(mdl, fit, grp, m=m, **px)

    return _fit_link_scales(evaluate, grp, K, scale_prior_sigma, max_outer, tol)


def fit_link_scales_fte(models, groups="links", x0=None, scale_prior_sigma=None, max_outer=30, tol=1e-6, pin_unobserved=False,
                        **solve_kw):
    """The link lengths of a skeleton fitted JOINTLY with the FTE trajectory: one scale s_g = exp(theta_g) per group of links
    (``groups`` as ``link_groups``), the minimiser over theta of sum_b min_x F_b(x, theta) - F_b the objective ``solve_models``
    minimises on clip b, data term and smoothness prior - plus theta^2 / (2 ``scale_prior_sigma``^2) per group when given.
    ``models``: one ``SkeletonModel`` or a list of clips of the same skeleton, cameras and length, e.g. the windows of a video: the
    lengths belong to the animal, so all clips share one theta and their reduced systems add.  ``x0``: None or one [N, P] start
    per clip (a single array for a single model); ``solve_kw`` goes to ``solve_models`` (``max_iter``, ``ftol``, ``l1_eps``, ...).

    The outer loop is that of ``fit_link_scales``.  Every evaluation at a theta is ``scale_links`` on every model, ONE
    ``solve_models`` over all clips - started from the iterates of the accepted evaluation moved by ``sens_links`` dtheta and
    clipped to the box; ``x0`` the first time - and ONE ``link_fit_system`` at the solutions: S = sum_b S_b and r = sum_b r_b over
    the clips whose solve and system both succeeded.  The Fisher-scoring step ``newton`` is NOT added to the start: at the end
    point of an L1 solve the gradient does not vanish (the signs of the residuals near zero keep flipping), and -A^-1 g_x
    amplifies it along the directions two cameras see worst - measured on the 12-frame test windows: steps of 8 to 700 m or rad,
    a start whose cost is 3e8 against 4e3, and solves that end in a worse local minimum at better scales.  A step is accepted when the cost summed over the clips both
    points use falls.  A group with a zero diagonal entry of S stays at 1 with ``observed`` False and ``std`` inf.  One camera does
    not determine the size of the skeleton: a model of one camera raises ValueError unless ``scale_prior_sigma`` is given.
    ``pin_unobserved`` goes to ``link_fit_system``.  Refused for models of the redescending loss.

    Returns the dict of ``fit_link_scales`` with ``models`` (the scaled copies) and ``results`` (the ``[(results, info), ...]`` of
    the solve at the end point) in the place of ``model`` and ``fit``; ``system`` carries S, r, ``cost_frames`` (the clips' costs),
    ``used``, ``n_used`` and ``clips`` (the dicts of ``link_fit_system``); ``joint`` is True.

    ``cov_log_scales`` = S^-1 is the marginal covariance of theta under the joint posterior over (trajectories, log-scales), whose
    information is [[A, G], [G^T, C]] per clip.  By the block inverse, cov(x) = A^-1 + S_x Sigma S_x^T and
    cov(pos_l) = G_l A^-1 G_l^T + T_l Sigma T_l^T with S_x = -A^-1 G and T_l = G_l S_x + D_l: the sums ``cov_x + cov_x_links``,
    ``cov_pos + cov_pos_links`` and ``std_pos_total`` that ``solve_models(result["models"], ..., return_cov=True,
    cov_links=result)`` returns ARE the marginals of that joint posterior, the correlation between the lengths' errors and the
    trajectory's included.  This is the valid total for lengths fitted on the same clips."""
    single = isinstance(models, SkeletonModel)
    models = [models] if single else list(models)
    if len(models) == 0:
        raise ValueError("no models")
    if x0 is not None:
        x0 = [x0] if single else list(x0)
    grp, K = link_groups(models[0].prog, groups)
    _check_outer(scale_prior_sigma, max_outer, tol)
    _refuse_robust(models, "link fit (fit_link_scales_fte)")
    if int(np.shape(models[0].meas)[1]) == 1 and scale_prior_sigma is None:
        raise ValueError("one camera does not determine the size of the skeleton (a larger animal further away gives the same "
                         "pixels): pass scale_prior_sigma")
    prec = 0.0 if scale_prior_sigma is None else 1.0 / float(scale_prior_sigma) ** 2
    l1_eps = solve_kw.get("l1_eps", 1e-2)
    seen = []                                                  # the evaluations so far that can still be the accepted one: at most two

    def total(ev, both):
        return float(np.add.reduce(ev["cost"][both])) + 0.5 * prec * float(ev["theta"] @ ev["theta"])

    def base():
        """The accepted evaluation by the loop's own rule: the later of two wins when its cost on the clips both use is lower."""
        if len(seen) == 2:
            both = seen[0]["used"] & seen[1]["used"]
            if both.any() and total(seen[1], both) < total(seen[0], both):
                del seen[0]
            else:
                del seen[1]
        return seen[0]

    def evaluate(theta):
        mdls = [scale_links(m, np.exp(theta), grp) for m in models]
        start = x0
        if seen:
            b0 = base()
            start = []
            for m, xb, sb in zip(mdls, b0["xs"], b0["clips"]):
                act = np.asarray(m.active, dtype=np.int64)
                x = xb.copy()
                if sb["status"] == 0:
                    x = x + sb["sens_links"] @ (theta - b0["theta"])
                x[:, act] = np.clip(x[:, act], m.lo[:, act], m.hi[:, act])
                start.append(x)
        out = solve_models(mdls, start, **solve_kw)
        xs = [r["x"] for r, _i in out]
        clips = _link_fit_system(mdls, xs, grp, l1_eps, pin_unobserved, True, raise_numeric=False)      # (with sens_links)
        used = np.array([s["status"] == 0 and i["status_name"] != "numeric" for s, (_r, i) in zip(clips, out)], dtype=bool)
        S, r = np.zeros((K, K)), np.zeros(K)
        for s, u in zip(clips, used):                          # the clips in their order
            if u:
                S, r = S + s["S"], r + s["r"]
        cost = np.array([s["cost"] for s in clips])
        seen.append(dict(theta=np.array(theta, copy=True), xs=xs, clips=clips, used=used, cost=cost))
        return mdls, out, dict(S=S, r=r, cost_frames=cost, used=used, n_used=int(used.sum()), clips=clips)

    fit = _fit_link_scales(evaluate, grp, K, scale_prior_sigma, max_outer, tol)
    fit["models"], fit["results"], fit["joint"] = fit.pop("model"), fit.pop("fit"), True
    return fit


def pose_fit_pixels(model, x0=None, det=None, thresh=0.5, f_scale=5.0, sigma_px=None, prior_sigma=np.pi, min_detections=2,
                    max_iter=100, ftol=1e-10, xtol=1e-10, lam0=1e-3, return_cov=True):
    """Per-frame pose of a ``SkeletonModel`` from the detections of every camera (include/acinoset_hip.h:
    acino_skel_pose_fit_px; ``fte.pose_fit_pixels`` for a skeleton): per frame the minimiser over the ``model.active`` states,
    inside the frame's box ``model.lo`` / ``model.hi``, of

        F(x) = 1/sigma_px^2 sum_{(c,l) valid} sum_{k in (u,v)} 1/2 f^2 log1p(r_k^2 / f^2)
             + 1/2 sum_{p >= 3} (x_p - m_p)^2 / prior_sigma^2,        r = pi_c(FK_l(x)) - det[n, c, l, :2],  f = f_scale

    by the projected Levenberg-Marquardt of ``pose_fit``, one launch.  No triangulation stands between a detection and the
    skeleton: a slot one camera sees enters, a frame without any triangulated slot has a pose, and a wrong detection is
    down-weighted frame by frame (w = 1 / (1 + r^2 / f^2)).  ``det`` [N, C, n_pose, 3] (x, y, likelihood; N = ``model.N``, slot
    l is pose slot l) is valid where its likelihood is above ``thresh`` and both pixel values are finite; default: the model's
    own detections as ``model_triangulation`` takes them, [``model.meas``, ``model.weights`` > 0].  ``sigma_px`` defaults to
    1 / max(``model.weights``).  The rig and the camera model are the model's.  ``x0`` [N, n_active] is the start and, clipped
    to the box, the centre m of the ridge on the angles; default: the chain of ``pose_fit_start`` on the model's own
    detections - ``model_triangulation``, ``pose_fit`` without covariances, ``fte.fill_unfitted_frames`` with the skeleton's
    psi columns, the clip to the box - and ValueError when no frame has a fit (a clip of one camera: pass ``x0``).

    Returns the dict of ``pose_fit`` with n_detections uint16 [N] (the valid detections; status 2: fewer than
    ``min_detections``) in place of n_markers, plus weight [N, C, n_pose, 2]: the weight every coordinate ended with, exactly 0
    for an invalid detection, NaN for status 2 and 3.  cov_x = A_free^-1 with A = sum w J^T J / sigma_px^2 + the ridge.

    numpy in, numpy out; a CUDA tensor as ``det`` or ``x0`` gives CUDA tensors out, with no host copy when ``x0`` is given."""
    act = np.asarray(model.active, dtype=np.int32)
    N, Pa, Lp, Cn = model.N, len(act), len(model.names), int(np.shape(model.meas)[1])

    sized = []

    def ready(dev):                                          # (the workspace's refusal comes before anything is staged)
        sized.append(_skel_workspace(model, act, lib().acino_skel_pose_fit_px_workspace_bytes))

    def launch(prm, dev, N, Cn, ins, outs):
        _skel_fit_call(model, act, dev, sized[0],
                       lambda skel, box, ws: lib().acino_skel_pose_fit_px(prm, *skel, ins[0], N, Cn, *ins[1:], *box, *outs, *ws))

    texts = dict(camera_model=f"the model's camera_model must be one of {calib.CAMERA_MODELS}",
                 det=f"det must be [{N}, {Cn}, {Lp}, 3] (model.N frames, the model's cameras, one slot per pose)",
                 cams="the model holds {} cameras: 1..{} are supported", x0=f"x0 must be [{N}, {Pa}] (the active states)")
    return fte._pose_fit_px(launch, (lambda: _model_detections(model)) if det is None else det, x0,
                            lambda d: _default_pixel_start(model), shape=(N, Cn, Lp),
                            active=act, n_full=model.P, camera_model=getattr(model, "camera_model", "fisheye"),
                            rig=(model.K, model.D, model.R, model.t), texts=texts, ready=ready,
                            tensors=isinstance(det, torch.Tensor) or isinstance(x0, torch.Tensor), thresh=thresh, f_scale=f_scale,
                            sigma_px=(lambda: _model_sigma_px(model)) if sigma_px is None else sigma_px, prior_sigma=prior_sigma,
                            min_detections=min_detections, max_iter=max_iter, ftol=ftol, xtol=xtol, lam0=lam0,
                            return_cov=return_cov)


def solve_models(models, x0=None, max_iter=200, lam0=1e-3, ftol=1e-10, xtol=1e-10, gtol=1e-8, l1_eps=1e-2, lam_max=1e16,
                 return_cov=False, n_samples=0, sample_seed=0, return_reprojection=False, pin_unobserved=False,
                 return_rate_cov=False, cov_cams=None, l1_start=True, init="line", cov_links=None, link_groups=None):
    """The GPU solve of SEVERAL ``SkeletonModel`` s of the same skeleton, cameras and length in one call
    (acino_skel_fte_solve_batch: one workgroup per clip in the banded factorisation, a Levenberg-Marquardt controller per clip
    on the device).  ``x0``: None or one [N, P] array per model.  Returns ``[(results, info), ...]`` in the order of ``models``.
    In a batch a clip that fails numerically does not fail the call: its ``info["status_name"]`` is "numeric" (its results are
    the last accepted iterate) and the other clips' results stand.  The models' ``camera_model`` (fisheye or pinhole) selects
    the assembly kernel; a batch that mixes the two is refused.  ``return_cov``: ``cov_x``, ``cov_pos`` and ``std_pos`` of
    ``model_covariance`` at the returned ``x`` are added to every ``results`` (one more batched call; a clip whose covariance
    is singular gets NaN arrays).  ``n_samples`` > 0: ``x_samples`` [S, N, P] and ``pos_samples`` [S, N, n_pose, 3] of
    ``model_samples(models, xs, n_samples, seed=sample_seed)`` at the returned ``x`` join every ``results`` the same way.
    ``return_reprojection``: ``uv``, ``cov_uv``, ``std_uv``, ``res``, ``mahal2`` and ``flags`` of ``model_reprojection`` at the
    returned ``x`` join every ``results`` (one more batched call); with ``return_cov`` the covariance runs once and its ``cov_pos``
    is passed on, without it the report runs with ``cov=False`` (``cov_uv`` and ``std_uv`` are None).
    ``pin_unobserved``: passed to ``model_covariance`` / ``model_samples`` (it acts only together with ``return_cov`` or
    ``n_samples``, and through ``return_cov`` on the report; the solve itself never changes); ``results`` then carries
    ``unobserved``.  ``pos_samples`` of a pose that depends on an unobserved state show no spread from it.
    ``return_rate_cov``: the six arrays of ``model_covariance(rates=True)`` (``cov_dx``, ``cov_ddx``, ``std_dx``, ``std_ddx``,
    ``cov_vel``, ``std_vel`` - the bars of the returned ``dx`` / ``ddx`` and of the pose velocities) join every ``results``; with
    ``return_cov`` both come from one call and one factorisation.
    ``cov_cams`` (a [6C, 6C] covariance of the extrinsics, or the dict of ``sba.covariance``; a malformed one is a ValueError
    before the solve): ``sens_cams``, ``cov_x_calib``, ``cov_pos_calib`` and ``std_pos_calib`` of
    ``model_calibration_sensitivity`` at the returned ``x`` join every ``results`` (one more batched call), and with
    ``return_cov`` also ``std_pos_total`` = sqrt(std_pos^2 + std_pos_calib^2) - valid only for a calibration that came from other
    data than these clips.  Without ``cov_cams`` the keys are what they were.
    ``cov_links`` (whatever ``link_cov_matrix`` takes: a [K, K] covariance of the links' log-scales, or the dict of a length fit; a
    malformed one is a ValueError before the solve) and ``link_groups`` (``groups`` of ``model_link_sensitivity``; None: those of
    the dict, else "links"): ``sens_links``, ``dpos_links``, ``cov_x_links``, ``cov_pos_links`` and ``std_pos_links`` of
    ``model_link_sensitivity`` at the returned ``x`` join every ``results`` (one more batched call), and with ``return_cov``
    ``std_pos_total`` = sqrt(std_pos^2 + std_pos_links^2 [+ std_pos_calib^2 when ``cov_cams`` is given too]) - valid only for
    lengths that came from other data than these clips, or an honest prior.  ``link_groups`` without ``cov_links`` gives
    ``sens_links`` and ``dpos_links`` alone (the three covariance keys None): there is no Sigma of the links, and ``std_pos_total``
    stays what it is without them - absent, or with ``cov_cams`` the two-term calibration total.  Refused for models of the
    redescending loss.
    Without the two keywords the keys are what they were.

    Models whose ``loss`` is "redescending" (``build_model(loss=...)``; one batch, one loss) are solved under the redescending
    measurement loss - a wrong detection above the likelihood threshold stops pulling once it is far enough off (beyond c = 20
    scaled units its force is ~0) - in two stages: ``l1_start=True`` (read for such models only) first runs the L1 solve of the
    same models from ``x0`` with the same tolerances and ``max_iter``, then the robust solve from its result; ``info["l1"]`` holds
    the first stage's info.  The first stage is part of the method: from the straight-line start every residual lies beyond c,
    where the loss is constant and its curvature 0, and Levenberg-Marquardt crawls.  A clip whose L1 stage ends "numeric" keeps
    that result and status.  ``l1_start=False`` starts the robust solve at ``x0`` directly (for a caller who brings the L1 end
    point).  Everything attached afterwards is evaluated under the model's loss: the covariance, rates and samples are those
    of the Gauss-Newton curvature sum w^2 h J^T J (``model_covariance``), the report carries the weights h; ``cov_cams`` is
    refused for such models (ValueError before any device call).

    ``init``: where a model without an ``x0`` starts - "line" (the default): its ``init_x``, the reference's line through the
    triangulated forehead with every angle 0; "pose_fit": ``pose_fit_start(model)`` and nothing else, a pose fit of every
    frame of the model's own detections (README: what that start was measured to be worth).  Any other value is a ValueError."""
    _check_init(init)
    if init == "pose_fit":
        x0 = [pose_fit_start(m) if x0 is None or x0[i] is None else x0[i] for i, m in enumerate(models)]
    if len(models) and cov_cams is not None:
        _refuse_robust(models, "calibration sensitivity (cov_cams)")
        calib.cov_cams_matrix(cov_cams, int(models[0].meas.shape[1]))      # (a malformed matrix fails before the solve, not after)
    with_links = _check_links(models, cov_links, link_groups)
    lm = dict(max_iter=max_iter, lam0=lam0, ftol=ftol, xtol=xtol, gtol=gtol, l1_eps=l1_eps, lam_max=lam_max)
    if len(models) and l1_start and all(model_loss(m) != "l1" for m in models):
        first = _lm_solve([_with_loss(m, "l1") for m in models], x0, **lm)
        out = _lm_solve(models, [r["x"] for r, _i in first], **lm)
        for i, (res1, info1) in enumerate(first):
            out[i] = (res1, dict(info1, l1=info1)) if info1["status_name"] == "numeric" else (out[i][0], dict(out[i][1], l1=info1))
    else:
        out = _lm_solve(models, x0, **lm)
    xs_out = [r["x"] for r, _i in out]
    if return_cov or return_rate_cov:
        keys = (("cov_x", "cov_pos", "std_pos") if return_cov else ()) + (RATE_KEYS if return_rate_cov else ())
        _attach(out, _covariance(models, xs_out, l1_eps, keys, pin_unobserved=pin_unobserved), keys + ("unobserved",))
    if n_samples:
        _attach(out, model_samples(models, xs_out, n_samples=n_samples, seed=sample_seed, l1_eps=l1_eps, pin_unobserved=pin_unobserved),
                ("x_samples", "pos_samples", "unobserved"))
    if return_reprojection:
        _attach(out, model_reprojection(models, xs_out, cov=bool(return_cov),
                                        cov_pos=[r["cov_pos"] for r, _i in out] if return_cov else None, l1_eps=l1_eps), REPROJ_KEYS)
    if cov_cams is not None:
        _attach(out, model_calibration_sensitivity(models, xs_out, cov_cams, l1_eps=l1_eps, pin_unobserved=pin_unobserved),
                CALIB_KEYS + ("unobserved",), total=bool(return_cov))
    if with_links:
        _attach(out, _links(models, xs_out, link_groups, cov_links, l1_eps, pin_unobserved), LINK_KEYS + ("unobserved",),
                total=bool(return_cov) and cov_links is not None)
    return out


def _lm_solve(models, x0, **lm):
    """One batched Levenberg-Marquardt call (acino_skel_fte_solve_batch*) under the models' loss: ``[(results, info), ...]``."""
    xs = [np.array(m.init_x if x0 is None or x0[i] is None else x0[i], dtype=np.float64, copy=True) for i, m in enumerate(models)]
    io_ = _skel_inputs(models, xs, lambda p, B: lib().acino_skel_fte_workspace_bytes_batch(C.byref(p), B), start=True,
                       **lm)
    m0, act, x = models[0], io_["act"], io_["x"]
    B = len(models)
    pos = torch.empty((B, m0.N, len(m0.names), 3), dtype=torch.float64, device=io_["dev"])
    infos = (SkelFteInfo * B)()
    solve = getattr(lib(), calib.CAMERAS[io_["cam_model"]].skel_fte_solve_batch)
    head = io_["head"]
    check(solve(*head[:2], *head[3:], ptr(pos), *io_["tail"][:2], infos, io_["tail"][2]))      # (the camera model is in the entry's name)
    xh, ph = x.cpu().numpy(), pos.cpu().numpy()
    out = []
    for i, (m, xf) in enumerate(zip(models, xs)):
        xf[:, act] = xh[i]
        dx, ddx = _finite_diff_states(xf, float(m.h))
        out.append((dict(positions=ph[i], x=xf, dx=dx, ddx=ddx), infos[i].as_dict()))
    return out


def solve_model(model, x0=None, max_iter=200, lam0=1e-3, ftol=1e-10, xtol=1e-10, gtol=1e-8, l1_eps=1e-2, lam_max=1e16,
                return_cov=False, n_samples=0, sample_seed=0, return_reprojection=False, pin_unobserved=False,
                return_rate_cov=False, cov_cams=None, l1_start=True, init="line", cov_links=None, link_groups=None):
    """The GPU solve of a ``SkeletonModel`` (acino_skel_fte_solve).  Returns (results, info): ``results`` has the layout of
    ``convert_to_dict`` (positions [N, n_pose, 3], x / dx / ddx [N, P]); states outside ``model.active`` keep their initial
    values - which must be 0, as in the reference's initialisation (:215-222).  A numeric failure raises (one clip: the
    failure is the call's).  ``return_cov``: ``cov_x`` / ``cov_pos`` / ``std_pos`` at the returned ``x`` (``model_covariance``)
    join ``results``; ``n_samples`` > 0: ``x_samples`` / ``pos_samples`` (``model_samples`` with ``seed=sample_seed``) do;
    ``return_reprojection``: the six arrays of ``model_reprojection`` do (``cov_uv`` / ``std_uv`` None without ``return_cov``).
    ``pin_unobserved``: as ``solve_models`` (only together with ``return_cov`` or ``n_samples``; ``results["unobserved"]``).
    ``return_rate_cov``: the bars of ``dx``, ``ddx`` and the pose velocities (``model_covariance(rates=True)``) join ``results``.
    ``cov_cams``: the calibration's share (``model_calibration_sensitivity``; ``std_pos_total`` with ``return_cov``), as
    ``solve_models``.  ``cov_links`` / ``link_groups``: the link lengths' share (``model_link_sensitivity``; it joins
    ``std_pos_total``), as ``solve_models``.  A model whose ``loss`` is "redescending" is solved in two stages, L1 first
    (``l1_start``, ``info["l1"]``), as ``solve_models`` describes.  ``init``: "line" or "pose_fit", as ``solve_models``."""
    return solve_models([model], None if x0 is None else [x0], max_iter=max_iter, lam0=lam0, ftol=ftol, xtol=xtol, gtol=gtol,
                        l1_eps=l1_eps, lam_max=lam_max, return_cov=return_cov, n_samples=n_samples, sample_seed=sample_seed,
                        return_reprojection=return_reprojection, pin_unobserved=pin_unobserved,
                        return_rate_cov=return_rate_cov, cov_cams=cov_cams, l1_start=l1_start, init=init, cov_links=cov_links,
                        link_groups=link_groups)[0]


def solve_model_parallel(model, x0=None, window=N_FRAMES, outer_max=40, xtol_outer=1e-7, first_max_iter=30, later_max_iter=30,
                         **solver_kw):
    """ONE long clip solved with every compute unit: alternating Schwarz on the nonlinear problem.  The clip is covered by
    windows of ``window`` frames that overlap by half; an outer iteration solves ALL windows in one batched call
    (``solve_models``: one workgroup and one controller per window) with the three frames at either inner end of a window
    PINNED (lo = hi) to the current global iterate - three frames are what the third-difference term reaches across - and
    every frame then takes its value from the window in which it lies deepest.  A free frame of a window sees exactly the
    residual rows and smoothness rows it sees in the whole-clip problem, so a fixed point of the outer iteration is a
    stationary point of the whole-clip objective; the error of the boundary values decays over the half-window overlap
    from one outer iteration to the next.  Each outer iteration reports the whole-clip cost and projected-gradient norm
    (one assembly of the full model).  Returns ``(results, info)`` as ``solve_model``; ``info`` carries the outer history.
    (The single-workgroup solve of the same clip, ``solve_model``, walks the banded factorisation frame by frame - 34 us
    per frame and iteration whatever the GPU's size.)  Windows are solved only ``first_max_iter`` / ``later_max_iter`` LM
    iterations per outer iteration: boundary values that are still wrong are not worth converging against.  Measured
    (MI355X, the shipped detections): 400 frames in 10 outer iterations, 1.1 s against 1.9 s for ``solve_model``, ending at
    a LOWER cost (an L1 objective on real detections has many stationary points); the whole 6 240-frame video does NOT
    reach ``xtol_outer`` in 40 outer iterations (9 s; the cost still falls by ~0.4 % per outer iteration): where a stretch of
    the video has no detections the trajectory is held by the smoothness term alone (weight 0.002 / h^4 = 4e5) and
    information crosses it half a window per outer iteration - ``solve_video`` (free windows) is the practical entry for that.
    The windows and the whole-clip evaluation follow ``model.loss``: a "redescending" model's windows are solved in two stages
    (``solve_models``; pass ``l1_start=False`` in ``solver_kw`` when ``x0`` is an L1 end point already)."""
    if "max_iter" in solver_kw:
        raise TypeError("solve_model_parallel: the inner iteration budget is first_max_iter / later_max_iter (and outer_max), not max_iter")
    N, P = model.N, model.P
    act = np.asarray(model.active, dtype=np.int64)
    if N < 2 * window:
        return solve_model(model, x0=x0, **solver_kw)
    starts = video_windows(0, N - 1, window, window // 2)
    x = np.array(model.init_x if x0 is None else x0, dtype=np.float64, copy=True)
    x[:, act] = np.clip(x[:, act], model.lo[:, act], model.hi[:, act])
    owner = _window_owner(starts, window, 0, N)
    history = []
    res_full, info_full = None, None
    for outer in range(outer_max):
        subs = []
        for st in starts:
            lo, hi = model.lo[st:st + window].copy(), model.hi[st:st + window].copy()
            if st > 0:
                lo[:3, act] = hi[:3, act] = x[st:st + 3, act]
            if st + window < N:
                lo[-3:, act] = hi[-3:, act] = x[st + window - 3:st + window, act]
            subs.append(SkeletonModel(**{**model.__dict__, "meas": model.meas[st:st + window], "weights": model.weights[st:st + window],
                                         "lo": lo, "hi": hi, "init_x": x[st:st + window].copy(), "x": None, "info": None}))
        solved = solve_models(subs, max_iter=first_max_iter if outer == 0 else later_max_iter, **solver_kw)
        xn = _stitch(owner, starts, 0, [res for res, _i in solved], ("x",))["x"]
        change = float(np.abs(xn - x).max())
        x = xn
        res_full, info_full = solve_model(model, x0=x, max_iter=0, **solver_kw)      # whole-clip cost and gradient norm at x
        history.append(dict(outer=outer + 1, change=change, cost=info_full["cost_final"], gnorm_inf=info_full["gnorm_inf"],
                            window_iterations=int(sum(i["iterations"] for _r, i in solved))))
        if change <= xtol_outer:
            break
    info = dict(info_full)
    info.update(outer_iterations=len(history), history=history, windows=len(starts), window_frames=window,
                status_name="outer_xtol" if history[-1]["change"] <= xtol_outer else "outer_max")
    return res_full, info


def video_windows(first_frame, last_frame, window, overlap):
    """First frames of the windows ``solve_video`` cuts first_frame .. last_frame into: ``window`` frames each, consecutive
    windows ``overlap`` frames apart from abutting, the last one pulled back so that it ends on ``last_frame``."""
    if not 0 <= overlap < window:
        raise ValueError("0 <= overlap < window")
    if last_frame - first_frame + 1 < window:
        raise ValueError(f"{last_frame - first_frame + 1} frames, windows of {window}")
    starts = list(range(first_frame, last_frame - window + 2, window - overlap))
    if starts[-1] + window - 1 < last_frame:
        starts.append(last_frame - window + 1)
    return starts


def window_residual_px(model, info):
    """Mean absolute reprojection residual (px) at the end state of a solved window: the L1 objective is sum w |e| with w = 1 / R
    on every detection above the threshold (x and y are two rows each), plus a smoothness term that is small beside it."""
    n_rows = 2 * int((np.asarray(model.weights) > 0).sum())
    return float(info["cost_final"]) * R_MEAS / max(n_rows, 1)


def _window_owner(starts, window, first_frame, total):
    """The depth rule, owner[total]: every frame belongs to the window in which it lies deepest, the earlier window wins a tie.
    Window w covers frames ``starts[w] - first_frame ... + window`` (relative to first_frame), its row r has depth
    min(r, window - 1 - r), and a frame changes owner only for a strictly greater depth."""
    d = np.minimum(np.arange(window), window - 1 - np.arange(window))
    depth, owner = np.full(total, -1), np.full(total, -1)
    for w, st in enumerate(starts):
        sl = slice(st - first_frame, st - first_frame + window)
        take = d > depth[sl]
        owner[sl][take] = w
        depth[sl] = np.maximum(depth[sl], d)
    assert (owner >= 0).all(), "the windows do not cover every frame"
    return owner


def _stitch(owner, starts, first_frame, per_window, keys, fill=0.0):
    """The gather by owner: for every key of ``keys`` frame n takes row n - (starts[w] - first_frame) of its owner window w's
    array ``per_window[w][key]``.  The stitched arrays have the per-window arrays' trailing shape and dtype (``fill``: what a
    frame without an owner would keep)."""
    out = {k: np.full((len(owner),) + per_window[0][k].shape[1:], fill, dtype=per_window[0][k].dtype) for k in keys}
    for w, (st, arrays) in enumerate(zip(starts, per_window)):
        mine = np.nonzero(owner == w)[0]
        for k in keys:
            out[k][mine] = arrays[k][mine - (st - first_frame)]
    return out


def _warm_pairs(px, warm_px):
    """Which window is retried from which neighbour, ``[(i, j), ...]``: window i when ``px[i] > warm_px`` (a NaN is not), from
    the neighbour j of i - 1, i + 1 with ``px[j] < px[i]`` and ``px[j] <= warm_px`` - the one with the smaller px, i - 1 on a tie."""
    pairs = []
    for i in range(len(px)):
        if not (px[i] > warm_px):
            continue
        cand = [j for j in (i - 1, i + 1) if 0 <= j < len(px) and px[j] < px[i] and px[j] <= warm_px]
        if cand:
            pairs.append((i, min(cand, key=lambda q: px[q])))
    return pairs


def _warm_x0(x0_own, st, x_donor, st_donor, window, act, lo, hi):
    """The initial point of the window at ``st`` retried from a donor window's end state ``x_donor`` (at ``st_donor``; the two
    share frames): the window's own first initial point, then the donor's joint angles (active states >= 3) at the shared frame
    nearest to the rest of the window - the last shared frame of a donor that starts earlier, the first of a later one - held
    over all rows, then the shared frames as the donor left them (whole rows), then the active states clipped to ``lo`` / ``hi``."""
    lo_g, hi_g = max(st, st_donor), min(st, st_donor) + window            # shared frames [lo_g, hi_g) (global numbering)
    x0 = x0_own.copy()
    edge = x_donor[(hi_g - 1 if st_donor < st else lo_g) - st_donor]      # the donor's state at the shared frame nearest to the rest
    x0[:, act[act >= 3]] = edge[act[act >= 3]][None, :]                   # its joint angles held over the window ...
    x0[lo_g - st:hi_g - st] = x_donor[lo_g - st_donor:hi_g - st_donor]    # ... and the shared frames as the donor left them
    x0[:, act] = np.clip(x0[:, act], lo[:, act], hi[:, act])
    return x0


def _warm_passes(models, x0s, starts, window, solved, px, warm_px, passes, kw):
    """solve_video's warm starts, on ``solved`` and ``px`` in place: up to ``passes`` times, one batched solve of the windows
    of ``_warm_pairs`` that share frames with their donor from ``_warm_x0``, the better of the two end states kept; it ends
    with the first pass that retries or improves nothing.  Returns the donor every window's kept state was started from (or None)."""
    warm_from = [None] * len(starts)
    act = np.asarray(models[0].active, dtype=np.int64)
    for _pass in range(int(passes)):
        redo = [(i, j) for i, j in _warm_pairs(px, warm_px) if abs(starts[i] - starts[j]) < window]
        if not redo:
            break
        x0r = [_warm_x0(x0s[i], starts[i], solved[j][0]["x"], starts[j], window, act, models[i].lo, models[i].hi) for i, j in redo]
        again = solve_models([models[i] for i, _j in redo], x0r, **kw)
        improved = False
        for (i, j), (res, info) in zip(redo, again):
            p_new = window_residual_px(models[i], info)
            if info["status_name"] != "numeric" and p_new < px[i]:
                solved[i], px[i], warm_from[i], improved = (res, info), p_new, j, True
        if not improved:
            break
    return warm_from


def _video_forehead(dlc_tables, idx, f0, f1, scene, lik_thresh, cam_model):
    """The forehead of frames f0 .. f1, triangulated once and its gaps interpolated, [frames, 3] (the reference's initial point
    uses the same marker, build.py:143-166) - or None without the marker, a second camera or two frames that see it.  Every
    table must hold f0 .. f1 (ValueError)."""
    tabs3 = [(list(tb[0]), np.asarray(tb[1], dtype=np.float64), ix) for tb, ix in zip(dlc_tables, idx)]
    rows3 = [_rows_by_frame_value(ix, np.arange(f0, f1 + 1)) for _parts, _vals, ix in tabs3]
    if not all("forehead" in parts for parts, _v, _i in tabs3) or len(tabs3) < 2:
        return None
    k_arr, d_arr, r_arr, t_arr = (np.asarray(a, dtype=np.float64) for a in scene)
    cols = [vals[rw, parts.index("forehead")][:, None, :] for (parts, vals, _ix), rw in zip(tabs3, rows3)]
    tri = calib.triangulate_pairs_dense(np.stack(cols, axis=1), lik_thresh, k_arr, _scene_distortion(cam_model, k_arr, d_arr, r_arr, t_arr),
                                        r_arr, t_arr, return_masks=False, model=cam_model)
    tri = np.asarray(tri.cpu().numpy() if isinstance(tri, torch.Tensor) else tri)[:, 0]
    ok = np.isfinite(tri).all(1)
    if ok.sum() < 2:
        return None
    fr = np.arange(f1 - f0 + 1, dtype=np.float64)
    return np.stack([np.interp(fr, fr[ok], tri[ok, j]) for j in range(3)], axis=1)


def solve_video(skel_dict, project_dir=None, *, scene=None, dlc_tables=None, first_frame=None, last_frame=None, window=N_FRAMES,
                overlap=20, warm_px=15.0, warm_passes=3, return_cov=False, return_reprojection=False, gate=None, pin_unobserved=False,
                return_rate_cov=False, cov_cams=None, loss="l1", init="line", link_scales=None, cov_links=None, link_groups=None, **kw):
    """A whole video as the reference would have to do it - windows of ``window`` frames (build.py:131-133: N = 100), here
    ALL of them in one batched GPU solve: consecutive windows overlap by ``overlap`` frames and every frame is taken from
    the window in which it lies deepest.  An extension (the reference solves one window per run): the initial point of a
    window is the triangulated forehead of its OWN frames, gaps interpolated (the reference fits one straight line through the
    forehead of the whole video and evaluates it at 0 .. N-1 whatever ``start_frame`` is, :143-166 - fine for its one window
    near the start, metres away for a window later in a video in which the subject turns round).

    Warm starts: a window that starts with all joint angles 0 can settle in a wrong local minimum of the L1 objective (the
    body facing the other way: mean residuals of 20 .. 140 px where its neighbours end at 2 .. 6).  After the first batched solve
    every window whose mean absolute residual exceeds ``warm_px`` is solved AGAIN from its better neighbour's end state - the
    shared ``overlap`` frames copied, the neighbour's joint angles at the nearest shared frame held over the rest, positions
    from the triangulated forehead - and the better of the two end states is kept; up to ``warm_passes`` passes, each one
    batched call over the windows concerned (a repaired window can repair its other neighbour in the next pass).

    ``dx`` / ``ddx`` are taken per window and selected with the same depth rule as ``x``: at a seam between two windows the
    stitched ``x`` jumps between two independently converged solutions, and differences ACROSS a seam would read as spikes of
    jump / h and jump / h^2.  ``kw``: build_model's (``pairing``, ``h``, ``camera_model``, ``project_func``, ...) and
    solve_models' (``max_iter``, ...) keywords.
    Returns ``(results, infos, starts)``: ``results`` as convert_to_dict over frames first_frame .. last_frame (plus
    ``start_frame`` and ``seams``: the first frame, relative to first_frame, of every stretch taken from a new window), one
    info per window (with ``mean_abs_residual_px`` and ``warm_started_from``).

    ``return_cov``: after the final stitching ONE batched ``model_covariance`` call over all windows at their final iterates;
    ``results`` gains ``std_pos`` [frames, n_pose] and ``cov_pos`` [frames, n_pose, 3, 3], every frame from the same window that
    supplied its ``positions``, and every info ``cov_status``.  A window's covariance ignores the frames outside it, so its bars
    grow towards the window's ends - which is why the stitch takes each frame from the window in which it is most interior.  A
    window whose covariance is singular (``cov_status`` 5: a state observed in none of its frames) gives NaN bars for its frames;
    such windows are listed in ``results["cov_singular_windows"]`` and nothing is raised (``owner``: the window every frame was
    taken from; ``window_std_pos``: every window's own bars).  ``pin_unobserved=True`` (acts only with ``return_cov``): every
    window's unobserved states (``model_observability``) are pinned, ``results["cov_unobserved"]`` lists them per window
    (full-state indices; [33, 43] for the shipped human skeleton) and ``cov_singular_windows`` keeps its meaning - the windows
    that are singular all the same, e.g. a limb seen in one or two frames only.  Bars of a pose that depends on an unobserved
    state are +inf.

    ``return_reprojection``: ONE ``model_reprojection`` call over the stitched trajectory - one clip of all the frames at
    ``results["x"]``, the measurements and weights of every frame gathered from the window that owns it - adds ``uv``, ``cov_uv``,
    ``std_uv``, ``res``, ``mahal2`` and ``flags`` [frames, C, n_pose, ...] to ``results``; with ``return_cov`` the stitched ``cov_pos``
    is used (NaN bars of a singular window carry over), without it ``cov_uv`` and ``std_uv`` are None.  With ``gate`` (a chi-square
    quantile with 2 degrees of freedom, e.g. 9.21; needs ``return_reprojection``) also ``outlier_frames``: the frames, relative to
    first_frame, in which any weighted detection lies outside ``mahal2 <= gate``.  A per-frame report of a stitched trajectory is
    sound where joint samples are not: every frame's pixels, residuals and bars are those of the window that supplied it.

    ``return_rate_cov``: ONE batched ``model_covariance(rates=True)`` call over all windows (the same call as ``return_cov``'s when
    both are set); ``results`` gains ``std_dx``, ``std_ddx`` [frames, P], ``cov_dx``, ``cov_ddx`` [frames, P, P], ``std_vel``
    [frames, n_pose] and ``cov_vel`` [frames, n_pose, 3, 3], every frame from the window that supplied its ``dx`` and ``ddx`` (the
    same depth rule: the bars are those of the window's own differences, never of a difference across a seam); ``cov_status``,
    ``cov_singular_windows``, ``owner`` and ``cov_unobserved`` as with ``return_cov``.

    ``cov_cams`` (as ``solve_models``; checked before the solve): ONE batched ``model_calibration_sensitivity`` call over all
    windows at their final iterates; ``results`` gains ``sens_cams`` [frames, P, 6C], ``cov_x_calib`` [frames, P, P],
    ``cov_pos_calib`` [frames, n_pose, 3, 3] and ``std_pos_calib`` [frames, n_pose], every frame from the window that supplied its
    ``positions``, and with ``return_cov`` ``std_pos_total`` = sqrt(std_pos^2 + std_pos_calib^2).  A singular window gives NaN
    for its frames, as with ``return_cov``.  It is NOT passed on to the windows' solves.

    ``cov_links`` / ``link_groups`` (as ``solve_models``; checked before the solve, refused with ``loss="redescending"``): ONE batched
    ``model_link_sensitivity`` call over all windows at their final iterates; ``results`` gains ``sens_links`` [frames, P, K],
    ``dpos_links`` [frames, n_pose, 3, K], ``cov_x_links``, ``cov_pos_links`` and ``std_pos_links`` (None without ``cov_links``), every
    frame from the window that supplied its ``positions``, and with ``return_cov`` ``std_pos_total`` = sqrt(std_pos^2 +
    std_pos_links^2 [+ std_pos_calib^2]).  A singular window gives NaN for its frames.  Not passed on to the windows' solves.

    ``loss="redescending"``: the windows are built, solved, retried and warm-started exactly as above under L1 - which window
    is kept and ``mean_abs_residual_px`` are the L1 stage's - then ONE batched robust call (``solve_models`` on the same windows
    with ``loss="redescending"``, ``l1_start=False``) runs from the windows' L1 end states before the stitching, and everything
    after it (the stitch, the covariance, the report with its ``weight``) is the robust models'.  Every info is the robust
    stage's with the L1 stage's under ``"l1"``; a window that fails numerically there keeps its L1 result and info and is listed
    in ``results["robust_failed_windows"]``.  ``cov_cams`` is refused (ValueError).

    ``init``: "line" (the default) - every window starts from the triangulated forehead of its own frames, all angles 0, as
    above - or "pose_fit": every window starts from ``pose_fit_start`` of its model, a pose fit of each of its frames; a
    window none of whose frames has a triangulated point keeps the forehead start, and every info says which start its window
    had (``init``).  The warm starts, the stages of the robust loss and everything after the solve are the same.  Any other
    value is a ValueError.

    ``link_scales`` = (groups, scales): every window's model is built with them (``build_model``; None changes nothing).

    There is no ``n_samples`` here: a stitched video is not one posterior (every window has its own, and draws of neighbouring
    windows are independent); call ``model_samples`` on the windows' models."""
    _check_init(init)
    if "n_samples" in kw or "sample_seed" in kw:
        raise TypeError("solve_video takes no n_samples: a stitched video is not one posterior (use model_samples per window)")
    if gate is not None and not return_reprojection:
        raise ValueError("gate needs return_reprojection=True")
    _loss_kind(loss)
    if loss != "l1" and cov_cams is not None:
        raise ValueError(f"the calibration sensitivity (cov_cams) is defined for the l1 loss only; loss is {loss!r}")
    if loss != "l1" and (cov_links is not None or link_groups is not None):
        raise ValueError(f"the link sensitivity (cov_links) is defined for the l1 loss only; loss is {loss!r}")
    kw.pop("l1_start", None)                                  # (the stages are this function's own)
    build_kw = {k: kw.pop(k) for k in ("h", "pairing", "lik_thresh", "r_meas", "model_weight") if k in kw}
    cam_model = calib.camera_model_of(kw.pop("camera_model", None), kw.pop("project_func", None))
    build_kw["camera_model"] = cam_model
    if link_scales is not None:
        build_kw["link_scales"] = link_scales
    l1_eps = kw.get("l1_eps", 1e-2)
    if scene is None:
        scene = _load_scene(project_dir)
    if cov_cams is not None:                                  # (a malformed matrix fails before the solve, not after)
        calib.cov_cams_matrix(cov_cams, len(scene[0]))
    if dlc_tables is None:
        dlc_tables = [io.read_dlc_table(p) for p in sorted(glob.glob(os.path.join(project_dir, "data", "*.h5")))]
    idx = [np.arange(np.asarray(tb[1]).shape[0]) if len(tb) < 3 or tb[2] is None else np.asarray(tb[2]) for tb in dlc_tables]
    f0 = max(int(i.min()) for i in idx) if first_frame is None else int(first_frame)
    f1 = min(int(i.max()) for i in idx) if last_frame is None else int(last_frame)
    total = f1 - f0 + 1
    if total < window:
        raise ValueError(f"{total} frames, windows of {window}")
    starts = video_windows(f0, f1, window, overlap)
    head = _video_forehead(dlc_tables, idx, f0, f1, scene, build_kw.get("lik_thresh", LIK_THRESH), cam_model)
    models = [build_model(skel_dict, project_dir, scene=scene, dlc_tables=dlc_tables, n_frames=window, start_frame=st,
                          initial_line=head is None, **build_kw)[0] for st in starts]
    with_links = _check_links(models, cov_links, link_groups)   # (a malformed matrix fails before the solve, not after)
    x0s = [m.init_x.copy() for m in models]
    for st, x0 in zip(starts, x0s if head is not None else []):
        x0[:, :3] = head[st - f0:st - f0 + window]
    started = ["line"] * len(models)
    if init == "pose_fit":
        for i, m in enumerate(models):
            fitted = _pose_fit_start(m, {})
            if fitted is not None:                            # (None: no frame of the window has a triangulated point)
                x0s[i], started[i] = fitted, "pose_fit"
    solved = solve_models(models, x0s, **kw)
    px = [window_residual_px(m, i) for m, (_r, i) in zip(models, solved)]
    warm_from = _warm_passes(models, x0s, starts, window, solved, px, warm_px, warm_passes, kw)
    robust_failed = []
    if loss != "l1":                                          # the robust stage: one batched call from the L1 end states
        models = [_with_loss(m, loss) for m in models]
        for i, (res2, info2) in enumerate(solve_models(models, [res["x"] for res, _info in solved], l1_start=False, **kw)):
            if info2["status_name"] == "numeric":
                robust_failed.append(i)
            else:
                solved[i] = (res2, dict(info2, l1=solved[i][1]))
    xs_final = [res["x"] for res, _info in solved]
    owner = _window_owner(starts, window, f0, total)
    results = _stitch(owner, starts, f0, [res for res, _info in solved], ("positions", "x", "dx", "ddx"))
    results.update(start_frame=f0, seams=[int(n) for n in np.nonzero(np.diff(owner) != 0)[0] + 1])
    infos = [dict(info, mean_abs_residual_px=px[i], warm_started_from=warm_from[i]) for i, (_r, info) in enumerate(solved)]
    if init == "pose_fit":
        for info, how in zip(infos, started):
            info["init"] = how
    if loss != "l1":
        results["robust_failed_windows"] = robust_failed
    if return_cov or return_rate_cov:
        keys = (("cov_pos", "std_pos") if return_cov else ()) + (RATE_KEYS if return_rate_cov else ())
        covs = _covariance(models, xs_final, l1_eps, keys, raise_numeric=False, pin_unobserved=pin_unobserved)
        for info, cv in zip(infos, covs):
            info["cov_status"] = cv["status"]
        results.update(_stitch(owner, starts, f0, covs, keys, fill=np.nan), owner=owner.copy(),
                       cov_singular_windows=[i for i, cv in enumerate(covs) if cv["status"] == 5])
        if return_cov:
            results["window_std_pos"] = [cv["std_pos"] for cv in covs]
        if pin_unobserved:
            results["cov_unobserved"] = [cv["unobserved"] for cv in covs]
    def attach_share(rows, keys, total):                      # (the keys a share leaves None - no Sigma - stay None)
        given = tuple(k for k in keys if rows[0][k] is not None)
        stitched = dict({k: None for k in keys}, **_stitch(owner, starts, f0, rows, given, fill=np.nan))
        _attach([(results, None)], [stitched], keys, total=bool(return_cov) and total)
    if cov_cams is not None:
        attach_share(_calibration(models, xs_final, cov_cams, l1_eps, pin_unobserved, raise_numeric=False), CALIB_KEYS, True)
    if with_links:
        attach_share(_links(models, xs_final, link_groups, cov_links, l1_eps, pin_unobserved, raise_numeric=False), LINK_KEYS,
                     cov_links is not None)
    if return_reprojection:                                   # one clip of all the frames, every frame's detections its owner's
        lo_t, hi_t = bounds_table(skel_dict, total)
        seen = _stitch(owner, starts, f0, [m.__dict__ for m in models], ("meas", "weights"))
        whole = SkeletonModel(**{**models[0].__dict__, **seen, "lo": lo_t, "hi": hi_t, "init_x": results["x"].copy(), "start_frame": f0,
                                 "x": None, "info": None})
        rep = model_reprojection([whole], [results["x"]], cov=bool(return_cov), cov_pos=[results["cov_pos"]] if return_cov else None,
                                 l1_eps=l1_eps)[0]
        results.update({k: rep[k] for k in REPROJ_KEYS})
        if gate is not None:
            finite = np.isfinite(rep["mahal2"])
            out_w = finite & (np.where(finite, rep["mahal2"], 0.0) > float(gate)) & ((rep["flags"] & 1) != 0)
            results["outlier_frames"] = [int(n) for n in np.nonzero(out_w.any(axis=(1, 2)))[0]]
    return results, infos, starts


def convert_to_dict(m, poses=None):
    """build.py:343-365: the result dictionary of a solved model."""
    if m.x is None:
        raise ValueError("the model has not been solved")
    return dict(positions=m.x["positions"], x=m.x["x"], dx=m.x["dx"], ddx=m.x["ddx"])


def save_data(file_data, file_path, poses=None, dict=True):
    """build.py:367-378."""
    if dict:
        file_data = convert_to_dict(file_data, poses)
    os.makedirs(os.path.dirname(file_path), exist_ok=True)
    with open(file_path, "wb") as f:
        pickle.dump(file_data, f)
    print(f"save {file_path}")


def solve_optimisation(model, exe_path=None, project_dir=None, poses=None, **solver_kw):
    """build.py:306-335: solve, then save ``data/results/traj_results.pickle`` under ``project_dir`` (when given).
    ``exe_path`` named the IPOPT executable; there is none here.  ``return_cov=True`` (a ``solve_model`` keyword) adds the
    covariance arrays to the returned ``results``, ``n_samples=S`` (with ``sample_seed``) the posterior samples,
    ``return_reprojection=True`` the image-space report of ``model_reprojection``, ``return_rate_cov=True`` the error bars of
    ``dx``, ``ddx`` and the pose velocities (``model_covariance(rates=True)``), ``pin_unobserved=True`` pins the unobserved
    states in those (``results["unobserved"]``), ``cov_cams=Sigma`` adds the calibration's share of the bars
    (``model_calibration_sensitivity``), ``cov_links=Sigma`` (with ``link_groups``) the link lengths' share
    (``model_link_sensitivity``); the saved pickle keeps the reference's four entries.  A model built with
    ``loss="redescending"`` is solved in two stages (``solve_models``: ``l1_start``, ``info["l1"]``)."""
    results, info = solve_model(model, **solver_kw)
    model.x, model.info = results, info
    if project_dir is not None:
        save_data(model, file_path=os.path.join(project_dir, "data", "results", "traj_results.pickle"), poses=poses)
    return results, info
