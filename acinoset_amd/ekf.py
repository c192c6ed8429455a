"""Extended Kalman filter + RTS smoother on the GPU - the array-level drop-in for ``ekf`` of
src/all_optimizations.py:569-865.

The reference function reads the videos' fps / resolution, the scene file and the DLC tables, then runs the filter
frame by frame (finite-difference Jacobian: 26 FK + 156 projection calls per frame, a 240 x 240 inverse) and pickles
``dict(x, dx, ddx, smoothed_x, smoothed_dx, smoothed_ddx)`` (:848-856).  ``ekf`` here takes the same information as
arrays and returns that dictionary (25 columns, pose parameters in the order of ``qb_list`` :734-746 = ``POSE_PARAMS``),
plus the gated-outlier count and the marker positions of both state sequences.  All model constants are the
reference's literals; the arithmetic runs in csrc/ekf.hip (one workgroup per sequence, covariance resident in LDS).
Several clips are filtered by one launch with ``ekf_batch`` (the filter is sequential in frames, parallel in clips).
The camera model is the reference's fisheye by default; ``camera_model="pinhole"`` (or ``project_func=calib.project_points``)
projects with cv2.projectPoints (rational / tangential / thin-prism distortion) instead, in fp64 as the fisheye path.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib, calib, fte
from ._lib import EkfParams, check, lib, ptr, stream_ptr

N_POSE, N_EKF_STATES = 25, 75
POSE_PARAMS = ["x_0", "y_0", "z_0", "phi_0", "theta_0", "psi_0", "phi_1", "theta_1", "psi_1", "theta_2",
               "phi_3", "theta_3", "psi_3", "theta_4", "psi_4", "theta_5", "psi_5", "theta_6", "theta_7",
               "theta_8", "theta_9", "theta_10", "theta_11", "theta_12", "theta_13"]
_BASE = dict(phi=fte.PHI, theta=fte.THETA, psi=fte.PSI)
# index of every pose parameter in the 45-state vector [x y z | phi_0..13 | theta_0..13 | psi_0..13]
EKF_ORDER = np.array([0, 1, 2] + [_BASE[n.split("_")[0]] + int(n.split("_")[1]) for n in POSE_PARAMS[3:]])


def get_pose_params():
    """``misc.get_pose_params()`` (:581): state name -> index."""
    return {name: i for i, name in enumerate(POSE_PARAMS)}


def get_3d_marker_coords(x):
    """``misc.get_3d_marker_coords`` (:617): pose parameters [..., 25] -> marker positions [..., 20, 3]."""
    x = np.asarray(x, dtype=np.float64)
    q = np.zeros(x.shape[:-1] + (fte.N_STATES,))
    q[..., EKF_ORDER] = x
    return fte.cheetah_fk(q.reshape(-1, fte.N_STATES)).reshape(x.shape[:-1] + (20, 3))


def initial_state(det, k_arr, d_arr, r_arr, t_arr, fps, dlc_thresh, start_frame=0, camera_model=None, project_func=None):
    """:700-711 - nose position and heading from two regressions of the triangulated nose on the frame number.  The nose is
    triangulated with the camera model of ``camera_model`` / ``project_func`` (calib.camera_model_of)."""
    model = calib.camera_model_of(camera_model, project_func)
    tri = calib.triangulate_pairs_dense(det, dlc_thresh, k_arr, d_arr, r_arr, t_arr, return_masks=False, model=model)
    nose = tri[:, 2] if isinstance(tri, np.ndarray) else tri[:, 2].cpu().numpy()
    ok = np.isfinite(nose).all(1)
    if ok.sum() < 2:
        raise ValueError("fewer than two triangulated nose points: cannot initialise the filter")
    f = np.arange(nose.shape[0], dtype=np.float64)[ok] + start_frame
    A = np.stack([f, np.ones_like(f)], 1)
    (xs, xi), (ys, yi) = (np.linalg.lstsq(A, nose[ok, j], rcond=None)[0] for j in (0, 1))
    sT = 1.0 / fps
    s = np.zeros(N_EKF_STATES)
    s[[0, 1, 5]] = [start_frame * xs + xi, start_frame * ys + yi, np.arctan2(ys, xs)]
    s[[N_POSE + 0, N_POSE + 1]] = [xs / sT, ys / sT]
    return s


def _a256(v):
    return (v + 255) // 256 * 256


def workspace_layout(n_frames, n_seq):
    """The read-back contract of the workspace after a successful ``acino_ekf_run`` (include/acinoset_hip.h, EKF section):
    name -> (byte offset, shape) of the three float64 arrays the kernels leave there, each rounded up to 256 bytes -
    ``P_est`` [n_seq, N, 75, 75], ``rts_gain_T`` [n_seq, N, 75, 75] (the smoother gains, stored TRANSPOSED, written for the
    frames 1 .. N-2 only) and ``x_pred`` [n_seq, N, 75].  ``private`` is the offset at which the library's own part begins
    (a second state-sized slot, then 1024 bytes of flags); ``end`` + 1024 = ``acino_ekf_workspace_bytes``."""
    n = int(n_frames) * int(n_seq)
    if n_frames < 1 or n_seq < 1:
        raise ValueError("n_frames and n_seq must be at least 1")
    mat, vec = _a256(n * N_EKF_STATES * N_EKF_STATES * 8), _a256(n * N_EKF_STATES * 8)
    shape = (int(n_seq), int(n_frames), N_EKF_STATES)
    return dict(P_est=(0, shape + (N_EKF_STATES,)), rts_gain_T=(mat, shape + (N_EKF_STATES,)), x_pred=(2 * mat, shape),
                private=2 * mat + vec, end=2 * mat + 2 * vec)


def _read_internals(ws, base, n_frames, n_seq):
    """x_pred, P_est and the un-transposed smoother gains of one launch from its workspace (``workspace_layout``).  The
    kernel writes no gain for the frames 0 and N-1 (none at all when N < 3): those are NaN here."""
    lay = workspace_layout(n_frames, n_seq)
    arr = {}
    for name in ("P_est", "rts_gain_T", "x_pred"):
        off, shape = lay[name]
        arr[name] = ws[base + off:base + off + int(np.prod(shape)) * 8].cpu().numpy().view(np.float64).reshape(shape)
    gain = np.ascontiguousarray(np.swapaxes(arr["rts_gain_T"], 2, 3))
    gain[:, :1] = np.nan
    gain[:, max(n_frames - 1, 1):] = np.nan
    return arr["x_pred"], arr["P_est"], gain


def _check_return_cov(return_cov):
    """False, "bars" or True -> None, "bars" or "full"; anything else is a ValueError (before any device work)."""
    if isinstance(return_cov, (bool, np.bool_)):
        return "full" if return_cov else None
    if isinstance(return_cov, str) and return_cov == "bars":
        return "bars"
    raise ValueError(f'return_cov must be False, True or "bars", not {return_cov!r}')


def _covariances(prm, ws_ptr, nbytes, est, smo, full):
    """The covariance pass of one launch (csrc/ekf_cov.hip) on the workspace ``acino_ekf_run`` has just filled: the smoothed
    covariances by the second half of Rauch-Tung-Striebel, then the marker bars of (est, P_est) and (smo, P_s).  Returns
    host arrays keyed as the result dictionary, each with the leading axis of the launch's sequences."""
    n_seq, n_frames = est.shape[0], est.shape[1]
    ps = torch.empty((n_seq, n_frames, N_EKF_STATES, N_EKF_STATES), dtype=torch.float64, device=est.device)
    check(lib().acino_ekf_smoothed_covariance(C.byref(prm), C.c_void_p(ws_ptr), nbytes, ptr(ps), stream_ptr()))
    out = {}
    for prefix, states, cov_ptr in (("", est, C.c_void_p(ws_ptr)), ("smoothed_", smo, ptr(ps))):
        cov_pos = torch.empty((n_seq, n_frames, 20, 3, 3), dtype=torch.float64, device=est.device)
        std_pos = torch.empty((n_seq, n_frames, 20), dtype=torch.float64, device=est.device)
        std_state = torch.empty((n_seq, n_frames, N_EKF_STATES), dtype=torch.float64, device=est.device)
        check(lib().acino_ekf_marker_covariance(C.byref(prm), ptr(states), cov_ptr, ptr(cov_pos), ptr(std_pos), ptr(std_state),
                                                stream_ptr()))
        std_h = std_state.cpu().numpy()
        out[prefix + "std_x"], out[prefix + "std_dx"], out[prefix + "std_ddx"] = (
            std_h[..., :N_POSE], std_h[..., N_POSE:2 * N_POSE], std_h[..., 2 * N_POSE:])
        out[prefix + "cov_positions"], out[prefix + "std_positions"] = cov_pos.cpu().numpy(), std_pos.cpu().numpy()
    if full:
        out["smoothed_cov"] = ps.cpu().numpy()
    return out


def ekf_batch(dets, k_arr, d_arr, r_arr, t_arr, fps, dlc_thresh, camera_resolution, start_frames=None, states0=None,
              with_positions=True, smoother_pivoting=False, camera_model=None, project_func=None, return_internals=False,
              return_cov=False):
    """Filter + smooth several clips of the same rig.  ``dets``: list of det[N_b, C, 20, 3] (x, y, likelihood);
    clips of equal length share one launch.  Returns one result dictionary per clip.  ``camera_model`` "fisheye" (the
    default) or "pinhole", or ``project_func`` = calib.project_points_fisheye / calib.project_points (calib.camera_model_of:
    a contradiction is a ValueError, any other function NotImplementedError, both before any device work).
    ``return_internals`` adds what the kernels left in the workspace (``workspace_layout``): ``x_pred`` [N, 75] the float32-
    rounded predictions, ``P_est`` [N, 75, 75] the filtered covariances and ``rts_gain`` [N, 75, 75] the smoother gains
    A_i = P_est[i] F^T inv(P_pred[i+1]) (NaN where the kernel writes none: frames 0 and N-1, every frame when N < 3).  The
    same launches either way; the internals cost three more read-backs.

    ``return_cov`` = "bars" adds the error bars of both state sequences (csrc/ekf_cov.hip, one more pass over the same
    workspace; everything above is bit for bit what it is without the flag): ``std_x``, ``std_dx``, ``std_ddx`` [N, 25] =
    sqrt(diag) of the filtered covariance, ``cov_positions`` [N, 20, 3, 3] = J P[:25, :25] J^T with J the analytic Jacobian
    of the marker positions at ``x`` and ``std_positions`` [N, 20] = sqrt(trace) of it (metres; the definition of the FTE's
    ``std_positions``), and the same five with the prefix ``smoothed_`` from the smoothed covariance
    P_s[i] = P_est[i] + A_i (P_s[i+1] - P_pred[i+1]) A_i^T at ``smoothed_x``.  ``return_cov=True`` adds ``cov`` and
    ``smoothed_cov`` [N, 75, 75] on top.  Any other value is a ValueError.  Three things to know about these bars:

    * they are the filter's OWN belief under the reference's literal constants - a measurement sigma of 25 px per
      coordinate (R = 25^2 px^2), ``camera_resolution[0]`` px under the likelihood threshold, the process noise of
      ``qb_list`` - not a calibrated detector noise;
    * the 3-sigma gate does not change them: a gated pair has its residual zeroed, the gain and (I - K H) P keep its rows;
    * frames 0 and N-1 carry the filtered covariance (``smoothed_cov[i]`` == ``cov[i]`` there, every frame when N < 3),
      because the reference's smoother returns the filtered state at both ends.

    Bars of the marker velocities are not computed."""
    cov_mode = _check_return_cov(return_cov)
    model = calib.camera_model_of(camera_model, project_func)
    _lib.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    B = len(dets)
    start_frames = list(start_frames) if start_frames is not None else [0] * B
    dets_d = [calib._to_dev(d, dev) for d in dets]
    for d in dets_d:
        if d.dim() != 4 or d.shape[2] != 20 or d.shape[3] != 3:
            raise ValueError("det must be [N, C, 20, 3] = (x, y, likelihood)")
    cams = torch.as_tensor(calib.camera_records(model, k_arr, d_arr, r_arr, t_arr), device=dev)
    n_cams = int(cams.shape[0])
    if any(int(d.shape[1]) != n_cams for d in dets_d):
        raise ValueError("camera count mismatch between det and the rig")
    if n_cams > 6:
        raise NotImplementedError("the EKF kernel holds the measurement Jacobian of at most 6 cameras in LDS")
    s0 = []
    for b in range(B):
        if states0 is not None and states0[b] is not None:
            s = np.asarray(states0[b], dtype=np.float64).reshape(-1)
            if s.size != N_EKF_STATES:
                raise ValueError("states0 must have 75 entries (pose, velocity, acceleration)")
        else:
            s = initial_state(dets_d[b], k_arr, d_arr, r_arr, t_arr, fps, dlc_thresh, start_frames[b], camera_model=model)
        s0.append(s)
    out = [None] * B
    groups = {}
    for b, d in enumerate(dets_d):
        groups.setdefault(int(d.shape[0]), []).append(b)
    for n_frames, members in groups.items():
        if n_frames < 1:
            raise ValueError("empty sequence")
        det = torch.stack([dets_d[b] for b in members]).contiguous()
        st0 = torch.as_tensor(np.stack([s0[b] for b in members]), device=dev)
        prm = EkfParams(n_frames=n_frames, n_seq=len(members), n_cams=n_cams, fps=float(fps), dlc_thresh=float(dlc_thresh),
                        cam_width=float(camera_resolution[0]), smoother_pivoting=int(bool(smoother_pivoting)))
        nbytes = lib().acino_ekf_workspace_bytes(n_frames, len(members))
        ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=dev)
        ws_ptr = (ws.data_ptr() + 255) // 256 * 256
        est = torch.empty((len(members), n_frames, N_EKF_STATES), dtype=torch.float64, device=dev)
        smo = torch.empty_like(est)
        outl = torch.zeros(len(members), dtype=torch.int32, device=dev)
        run = getattr(lib(), calib.CAMERAS[model].ekf_run)
        check(run(C.byref(prm), ptr(det), ptr(cams), ptr(st0), C.c_void_p(ws_ptr), nbytes, ptr(est), ptr(smo),
                  C.c_void_p(outl.data_ptr()), stream_ptr()))
        est_h, smo_h, outl_h = est.cpu().numpy(), smo.cpu().numpy(), outl.cpu().numpy()
        if return_internals:
            xp_h, pe_h, gain_h = _read_internals(ws, ws_ptr - ws.data_ptr(), n_frames, len(members))
        if cov_mode:
            cov_h = _covariances(prm, ws_ptr, nbytes, est, smo, cov_mode == "full")
            if cov_mode == "full":
                base, (off, shape) = ws_ptr - ws.data_ptr(), workspace_layout(n_frames, len(members))["P_est"]
                cov_h["cov"] = ws[base + off:base + off + int(np.prod(shape)) * 8].cpu().numpy().view(np.float64).reshape(shape)
        for j, b in enumerate(members):
            r = dict(x=est_h[j, :, :N_POSE], dx=est_h[j, :, N_POSE:2 * N_POSE], ddx=est_h[j, :, 2 * N_POSE:],
                     smoothed_x=smo_h[j, :, :N_POSE], smoothed_dx=smo_h[j, :, N_POSE:2 * N_POSE],
                     smoothed_ddx=smo_h[j, :, 2 * N_POSE:], outliers_ignored=int(outl_h[j]), start_frame=start_frames[b])
            if with_positions:
                r["positions"] = get_3d_marker_coords(r["x"])
                r["smoothed_positions"] = get_3d_marker_coords(r["smoothed_x"])
            if return_internals:
                r.update(x_pred=xp_h[j], P_est=pe_h[j], rts_gain=gain_h[j])
            if cov_mode:
                r.update({key: val[j] for key, val in cov_h.items()})
            out[b] = r
    return out


def ekf(det, k_arr, d_arr, r_arr, t_arr, fps, dlc_thresh, camera_resolution, start_frame=0, states0=None,
        with_positions=True, smoother_pivoting=False, camera_model=None, project_func=None, return_internals=False,
        return_cov=False):
    """One clip: det[N, C, 20, 3] for the frames start_frame .. start_frame + N - 1 (camera model, ``return_internals`` and
    ``return_cov`` - False, "bars" or True: the error bars and covariances of both state sequences - as ``ekf_batch``)."""
    _check_return_cov(return_cov)
    return ekf_batch([det], k_arr, d_arr, r_arr, t_arr, fps, dlc_thresh, camera_resolution, [start_frame],
                     None if states0 is None else [states0], with_positions, smoother_pivoting, camera_model=camera_model,
                     project_func=project_func, return_internals=return_internals, return_cov=return_cov)[0]
