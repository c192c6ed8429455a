"""Drop-in replacements for the camera-model entry points of AcinoSet's ``src/calib/calib.py``.

Same names, argument order and array conventions as the reference:

    triangulate_points_fisheye(img_pts_1, img_pts_2, k1, d1, r1, t1, k2, d2, r2, t2) -> (M,3)   calib.py:121-130
    triangulate_points(...)                                                          -> (M,3)   calib.py:52-61
    project_points_fisheye(obj_pts, k, d, r, t)                                      -> (M,2)   calib.py:132-136
    project_points(obj_pts, k, d, r, t)                                              -> (M,2)   calib.py:64-66
    get_pairwise_3d_points_from_df(points_2d_df, k_arr, d_arr, r_arr, t_arr, triangulate_func)  calib.py:394-423

Inputs may be numpy arrays (returned as numpy, like cv2 does) or torch CUDA tensors (returned as CUDA
tensors, no host round trip).  All arithmetic runs in hand-written HIP kernels through the C ABI of
libacinoset_hip.so; there is no CPU path - a missing library or GPU raises RuntimeError.
"""
from typing import Callable, NamedTuple

import numpy as np
import torch

from . import _lib
from ._lib import CAM_STRIDE, PINHOLE_STRIDE, check, lib, ptr, stream_ptr


def _dev():
    _lib.require_gpu()
    return torch.device("cuda", torch.cuda.current_device())


def _to_dev(a, dev):
    if isinstance(a, torch.Tensor):
        return a.to(device=dev, dtype=torch.float64).contiguous()
    return torch.as_tensor(np.ascontiguousarray(np.asarray(a, dtype=np.float64)), device=dev)


def _ret(t, like):
    return t if isinstance(like, torch.Tensor) else t.cpu().numpy()


def _host(a):
    if isinstance(a, torch.Tensor):
        return a.detach().cpu().numpy().astype(np.float64)
    return np.asarray(a, dtype=np.float64)


def _rodrigues(rvec):
    """cv2.Rodrigues for an rvec handed to project_points (calib.py:65 passes `r` straight through)."""
    rvec = rvec.reshape(3)
    th = np.linalg.norm(rvec)
    if th < np.finfo(float).eps:
        return np.eye(3)
    kx, ky, kz = rvec / th
    K = np.array([[0, -kz, ky], [kz, 0, -kx], [-ky, kx, 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def fisheye_record(k, d, r, t):
    """One 24-double camera record [fx fy cx cy | k1..k4 | R | t | alpha 0 0 0] (include/acinoset_hip.h)."""
    k, d, r, t = _host(k), _host(d).reshape(-1), _host(r), _host(t).reshape(-1)
    if k.shape != (3, 3) or d.size != 4 or t.size != 3:
        raise ValueError("fisheye camera needs k (3,3), d (4,) or (4,1), t (3,) or (3,1)")
    if r.size == 3:
        r = _rodrigues(r)
    if r.shape != (3, 3):
        raise ValueError("r must be a 3x3 rotation matrix (or an rvec)")
    rec = np.zeros(CAM_STRIDE)
    rec[0:4] = k[0, 0], k[1, 1], k[0, 2], k[1, 2]
    rec[4:8] = d
    rec[8:17] = r.reshape(-1)
    rec[17:20] = t
    rec[20] = k[0, 1] / k[0, 0]
    return rec


def fisheye_records(k_arr, d_arr, r_arr, t_arr):
    k_arr, r_arr = _host(k_arr), _host(r_arr)
    d_arr = _host(d_arr).reshape(len(k_arr), -1)
    t_arr = _host(t_arr).reshape(len(k_arr), -1)
    return np.stack([fisheye_record(k_arr[i], d_arr[i], r_arr[i], t_arr[i]) for i in range(len(k_arr))])


def pinhole_record(k, d, r, t):
    k, d, r, t = _host(k), _host(d).reshape(-1), _host(r), _host(t).reshape(-1)
    if d.size not in (4, 5, 8, 12, 14):
        raise ValueError("OpenCV pinhole distortion vectors have 4, 5, 8, 12 or 14 entries")
    if d.size == 14 and (d[12] != 0 or d[13] != 0):
        raise ValueError("tilted sensor model (tau_x, tau_y) is not supported")
    if r.size == 3:
        r = _rodrigues(r)
    rec = np.zeros(PINHOLE_STRIDE)
    rec[0:4] = k[0, 0], k[1, 1], k[0, 2], k[1, 2]
    rec[4:4 + d.size] = d
    rec[18:27] = r.reshape(-1)
    rec[27:30] = t
    return rec


def pinhole_records(k_arr, d_arr, r_arr, t_arr):
    k_arr, r_arr = _host(k_arr), _host(r_arr)
    d_arr = _host(d_arr).reshape(len(k_arr), -1)
    t_arr = _host(t_arr).reshape(len(k_arr), -1)
    return np.stack([pinhole_record(k_arr[i], d_arr[i], r_arr[i], t_arr[i]) for i in range(len(k_arr))])


def _triangulate(fn_name, rec_fn, img_pts_1, img_pts_2, cam_a, cam_b):
    dev = _dev()
    p1 = _to_dev(img_pts_1, dev).reshape(-1, 2)
    p2 = _to_dev(img_pts_2, dev).reshape(-1, 2)
    if p1.shape != p2.shape:
        raise ValueError("img_pts_1 and img_pts_2 must hold the same number of points")
    ca = torch.as_tensor(rec_fn(*cam_a), device=dev)
    cb = torch.as_tensor(rec_fn(*cam_b), device=dev)
    out = torch.empty((p1.shape[0], 3), dtype=torch.float64, device=dev)
    check(getattr(lib(), fn_name)(ptr(p1), ptr(p2), p1.shape[0], ptr(ca), ptr(cb), ptr(out), stream_ptr()))
    return _ret(out, img_pts_1)


def triangulate_points_fisheye(img_pts_1, img_pts_2, k1, d1, r1, t1, k2, d2, r2, t2):
    """Two-view fisheye triangulation (calib.py:121-130): undistort both views, 4x4 DLT, dehomogenise."""
    return _triangulate("acino_triangulate_fisheye", fisheye_record, img_pts_1, img_pts_2, (k1, d1, r1, t1),
                        (k2, d2, r2, t2))


def triangulate_points(img_pts_1, img_pts_2, k1, d1, r1, t1, k2, d2, r2, t2):
    """Two-view pinhole triangulation (calib.py:52-61)."""
    return _triangulate("acino_triangulate_pinhole", pinhole_record, img_pts_1, img_pts_2, (k1, d1, r1, t1),
                        (k2, d2, r2, t2))


def _project(fn_name, rec_fn, obj_pts, k, d, r, t):
    dev = _dev()
    X = _to_dev(obj_pts, dev).reshape(-1, 3)
    cam = torch.as_tensor(rec_fn(k, d, r, t), device=dev)
    out = torch.empty((X.shape[0], 2), dtype=torch.float64, device=dev)
    check(getattr(lib(), fn_name)(ptr(X), X.shape[0], ptr(cam), ptr(out), stream_ptr()))
    return _ret(out, obj_pts)


def project_points_fisheye(obj_pts, k, d, r, t):
    """Fisheye projection (calib.py:132-136)."""
    return _project("acino_project_fisheye", fisheye_record, obj_pts, k, d, r, t)


def project_points(obj_pts, k, d, r, t):
    """Pinhole / rational-model projection (calib.py:64-66); `r` may be a matrix or an rvec."""
    return _project("acino_project_pinhole", pinhole_record, obj_pts, k, d, r, t)


def undistort_points_fisheye(pts, k, d, max_iter=10, eps=1e-8):
    """cv2.fisheye.undistortPoints(pts, k, d) -> normalised coordinates (calib.py:124-125)."""
    dev = _dev()
    p = _to_dev(pts, dev).reshape(-1, 2)
    cam = torch.as_tensor(fisheye_record(k, d, np.eye(3), np.zeros(3)), device=dev)
    out = torch.empty_like(p)
    check(lib().acino_undistort_fisheye(ptr(p), p.shape[0], ptr(cam), ptr(out), int(max_iter), float(eps),
                                        stream_ptr()))
    return _ret(out, pts)


# --------------------------------------------------------------------------- camera models
class CameraModel(NamedTuple):
    """One camera model as the library knows it (include/acinoset_hip.h): code in FteConst and acino_sba_params, record
    stride and builder, whether its kernels are fp64 only, and the names of the C entry points that exist once per model."""
    code: int
    stride: int
    records: Callable
    fp64_only: bool
    fte_create: str
    ekf_run: str
    skel_fte_solve_batch: str
    triangulate_pairs: str


CAMERAS = {
    "fisheye": CameraModel(0, CAM_STRIDE, fisheye_records, False, "acino_fte_create", "acino_ekf_run",
                           "acino_skel_fte_solve_batch", "acino_triangulate_pairs"),
    "pinhole": CameraModel(1, PINHOLE_STRIDE, pinhole_records, True, "acino_fte_create_pinhole", "acino_ekf_run_pinhole",
                           "acino_skel_fte_solve_batch_pinhole", "acino_triangulate_pairs_pinhole"),
}
CAMERA_MODELS = tuple(CAMERAS)


def camera_model_of(camera_model=None, project_func=None, precision="f64", by_name=False,
                    seams=(project_points_fisheye, project_points)):
    """The camera model of a problem, a name in CAMERAS: ``camera_model``, or the one the reference's injection seam
    ``project_func`` selects, or "fisheye" (the reference's default).  Raises before any device work."""
    # The entries keep different rules.  FTE, EKF, skeleton: project_func by identity with ``seams``, any other callable is
    # NotImplementedError.  get_pairwise_3d_points_from_df: its triangulate_func the same way, with the triangulations as
    # ``seams``.  Sparse SBA (by_name): project_func by __name__ - None or a name containing "fisheye" is fisheye,
    # "project_points" pinhole -, so the reference package's own functions select a model too.  Dense SBA: camera_model
    # alone.  Only the FTE and dense SBA entries pass a precision: only they refuse bf16 with the fp64-only pinhole model.
    if project_func is None:
        seam = None
    elif by_name:
        name = getattr(project_func, "__name__", "")
        seam = "fisheye" if "fisheye" in name else "pinhole" if name == "project_points" else None
    else:
        seam = "fisheye" if project_func is seams[0] else "pinhole" if project_func is seams[1] else None
    if project_func is not None and seam is None:
        raise NotImplementedError(f"no HIP kernel for {getattr(project_func, '__name__', project_func)!r}: pass "
                                  f"acinoset_amd.calib.{seams[0].__name__} or .{seams[1].__name__}")
    if camera_model is not None and camera_model not in CAMERAS:
        raise ValueError(f"camera_model must be one of {CAMERA_MODELS}")
    if camera_model is not None and seam is not None and camera_model != seam:
        raise ValueError(f"camera_model={camera_model!r} contradicts project_func (the {seam} model)")
    model = camera_model or seam or "fisheye"
    if CAMERAS[model].fp64_only and precision != "f64":
        raise ValueError(f"the {model} camera model is fp64 only (precision 'f64', got {precision!r})")
    return model


def camera_records(model, k_arr, d_arr, r_arr, t_arr):
    """The rig as the library's camera records of ``model``: [C, 24] fisheye or [C, 32] pinhole (include/acinoset_hip.h)."""
    return CAMERAS[model].records(k_arr, d_arr, r_arr, t_arr)


# --------------------------------------------------------------------------- dense index path
def triangulate_pairs_dense(det, thresh, k_arr, d_arr, r_arr, t_arr, return_masks=True, model="fisheye"):
    """det[N,C,L,3] (x, y, likelihood) -> tri[N,L,3] (NaN where no adjacent pair), npairs[N,L] u8,
    pairmask[N,L] u8.  The dense form of get_pairwise_3d_points_from_df (adjacent pairs, mean).
    ``model``: "fisheye" (triangulate_points_fisheye, calib.py:121-130) or "pinhole" (triangulate_points,
    calib.py:52-61) - the two functions the reference injects through ``triangulate_func`` (app.py:215-223)."""
    dev = _dev()
    d = _to_dev(det, dev)
    if d.dim() != 4 or d.shape[-1] != 3:
        raise ValueError("det must be [N, C, L, 3]")
    if model not in CAMERAS:
        raise ValueError("model must be 'fisheye' or 'pinhole'")
    N, Cn, L, _ = d.shape
    cams = torch.as_tensor(camera_records(model, k_arr, d_arr, r_arr, t_arr), device=dev)
    if cams.shape[0] != Cn:
        raise ValueError("camera count mismatch")
    tri = torch.empty((N, L, 3), dtype=torch.float64, device=dev)
    npairs = torch.empty((N, L), dtype=torch.uint8, device=dev)
    mask = torch.empty((N, L), dtype=torch.uint8, device=dev)
    fn = getattr(lib(), CAMERAS[model].triangulate_pairs)
    check(fn(ptr(d), N, Cn, L, float(thresh), ptr(cams), ptr(tri), ptr(npairs), ptr(mask), stream_ptr()))
    if not return_masks:
        return _ret(tri, det)
    return _ret(tri, det), _ret(npairs, det), _ret(mask, det)


R_MEAS = 5.0        # the FTE's measurement sigma in pixels (fte.R_MEAS, asserted equal by the tests): default sigma_px


def triangulate_multiview_dense(det, thresh, k_arr, d_arr, r_arr, t_arr, model="fisheye", f_scale=5.0, sigma_px=R_MEAS,
                                max_iter=60, xtol=1e-10, cov_cams=None, return_sens=False):
    """Robust N-view triangulation of det[N,C,L,3] (x, y, likelihood) with an error bar per point: per (frame, marker) the
    minimiser of the per-coordinate Cauchy cost (scale ``f_scale`` px) of the calibration-level reprojection residuals over
    ALL cameras with a valid detection (likelihood > thresh, finite pixel, undistortion succeeded) - not only adjacent pairs -,
    from the N-view ray midpoint, by one damped Gauss-Newton solver per point in one launch (include/acinoset_hip.h:
    acino_triangulate_multiview).  ``model``: "fisheye" (project_points_fisheye, with the skew) or "pinhole"
    (project_points).  Returns a dict:

      points [N,L,3]; cov [N,L,3,3] = sigma_px^2 (sum J^T W J)^-1, W the Cauchy IRLS weights at the point - the matrix of
      ``sba.covariance(optimize_cameras=False)``; std [N,L] = sqrt(trace cov) in metres; n_views, status, iters uint8 [N,L]
      (status 0 stopped on ``xtol``, 1 ``max_iter`` reached, 2 fewer than two views, 3 numeric; points / cov / std / wssr are
      NaN for 2 and 3); wssr [N,L] = sum w r^2; sigma2_hat = sum wssr / (2 sum n_views - 3 P) over the P points returned.

    The default ``sigma_px`` is the FTE's R_MEAS, so the bars compare with ``fte_solve(..., return_cov=True)``.  With
    ``cov_cams`` (the forms ``fte_solve`` takes: [6C,6C] per camera (dw, dt), or the dict of ``sba.covariance``) or
    ``return_sens``: sens_cams [N,L,3,6C], the derivative of the point with respect to every camera's extrinsics (exact zeros
    for the cameras that do not see it), and with ``cov_cams`` cov_calib = S Sigma S^T [N,L,3,3], std_calib and std_total =
    sqrt(std^2 + std_calib^2).  numpy in, numpy out; CUDA tensors in, CUDA tensors out with no host copy."""
    if model not in CAMERAS:
        raise ValueError(f"model must be one of {CAMERA_MODELS}")
    shape = tuple(det.shape) if hasattr(det, "shape") else np.shape(det)
    if len(shape) != 4 or shape[-1] != 3:
        raise ValueError("det must be [N, C, L, 3]")
    N, Cn, L, _ = shape
    if not 1 <= Cn <= _lib.MAX_CAMS:
        raise ValueError(f"det holds {Cn} cameras: 1..{_lib.MAX_CAMS} are supported")
    if len(k_arr) != Cn:
        raise ValueError("camera count mismatch")
    for name, val in (("f_scale", f_scale), ("sigma_px", sigma_px), ("xtol", xtol)):
        if not (np.isfinite(val) and val > 0):
            raise ValueError(f"{name} must be finite and > 0")
    if int(max_iter) != max_iter or not 1 <= max_iter <= 255:
        raise ValueError("max_iter must be an integer in 1..255")
    if np.isnan(thresh):
        raise ValueError("thresh must not be NaN")
    sigma_c = cov_cams_matrix(cov_cams, Cn)
    recs = camera_records(model, k_arr, d_arr, r_arr, t_arr)
    want_sens = return_sens or sigma_c is not None
    dev = _dev()
    d = _to_dev(det, dev)
    cams = torch.as_tensor(recs, device=dev)
    f64 = dict(dtype=torch.float64, device=dev)
    u8 = dict(dtype=torch.uint8, device=dev)
    pts, cov, wssr = torch.empty((N, L, 3), **f64), torch.empty((N, L, 3, 3), **f64), torch.empty((N, L), **f64)
    nviews, status, iters = torch.empty((N, L), **u8), torch.empty((N, L), **u8), torch.empty((N, L), **u8)
    sens = torch.empty((N, L, 3, 6 * Cn), **f64) if want_sens else None
    prm = _lib.TriMvParams(CAMERAS[model].code, int(max_iter), float(thresh), float(f_scale), float(sigma_px), float(xtol))
    check(lib().acino_triangulate_multiview(prm, ptr(d), N, Cn, L, ptr(cams), ptr(pts), ptr(cov), ptr(wssr), ptr(nviews),
                                            ptr(status), ptr(iters), ptr(sens), stream_ptr()))
    var = (cov[..., 0, 0] + cov[..., 1, 1]) + cov[..., 2, 2]
    got = status < 2
    dof = 2 * (nviews * got).sum(dtype=torch.float64) - 3 * got.sum(dtype=torch.float64)
    sigma2 = torch.where(got, wssr, torch.zeros_like(wssr)).sum() / dof
    out = dict(points=pts, cov=cov, std=torch.sqrt(var), n_views=nviews, status=status, iters=iters, wssr=wssr,
               sigma2_hat=sigma2)
    if want_sens:
        out["sens_cams"] = sens
    if sigma_c is not None:
        cc = torch.einsum("nlia,ab,nljb->nlij", sens, torch.as_tensor(sigma_c, device=dev), sens)
        cc = 0.5 * (cc + cc.transpose(-1, -2))
        vc = (cc[..., 0, 0] + cc[..., 1, 1]) + cc[..., 2, 2]
        out.update(cov_calib=cc, std_calib=torch.sqrt(vc), std_total=torch.sqrt(var + vc))
    if isinstance(det, torch.Tensor):
        return out
    out = {k: v.cpu().numpy() for k, v in out.items()}
    out["sigma2_hat"] = float(out["sigma2_hat"])
    return out


def reproject_residuals(pts3, det, thresh, k_arr, d_arr, r_arr, t_arr):
    """pts3[N,L,3], det[N,C,L,3] -> residuals[N,C,L,2] (NaN where invalid) and
    sums = (count, sum r, sum r^2, 0.5*sum log1p(r^2))."""
    dev = _dev()
    p = _to_dev(pts3, dev)
    d = _to_dev(det, dev)
    N, Cn, L, _ = d.shape
    cams = torch.as_tensor(fisheye_records(k_arr, d_arr, r_arr, t_arr), device=dev)
    res = torch.empty((N, Cn, L, 2), dtype=torch.float64, device=dev)
    sums = torch.zeros(4, dtype=torch.float64, device=dev)
    check(lib().acino_reproject_residuals(ptr(p), ptr(d), N, Cn, L, float(thresh), ptr(cams), ptr(res), ptr(sums),
                                          stream_ptr()))
    return _ret(res, det), _ret(sums, det)


def triangulate_reproject_dense(det, thresh, k_arr, d_arr, r_arr, t_arr):
    """``triangulate_pairs_dense`` followed by ``reproject_residuals`` of the triangulated points, in ONE pass over
    the detections (BASELINE config 2): returns tri[N,L,3], npairs, pairmask, residuals[N,C,L,2], sums[4]."""
    dev = _dev()
    d = _to_dev(det, dev)
    if d.dim() != 4 or d.shape[-1] != 3:
        raise ValueError("det must be [N, C, L, 3]")
    N, Cn, L, _ = d.shape
    cams = torch.as_tensor(fisheye_records(k_arr, d_arr, r_arr, t_arr), device=dev)
    if cams.shape[0] != Cn:
        raise ValueError("camera count mismatch")
    tri = torch.empty((N, L, 3), dtype=torch.float64, device=dev)
    npairs = torch.empty((N, L), dtype=torch.uint8, device=dev)
    mask = torch.empty((N, L), dtype=torch.uint8, device=dev)
    res = torch.empty((N, Cn, L, 2), dtype=torch.float64, device=dev)
    sums = torch.zeros(4, dtype=torch.float64, device=dev)
    check(lib().acino_triangulate_reproject(ptr(d), N, Cn, L, float(thresh), ptr(cams), ptr(tri), ptr(npairs), ptr(mask),
                                            ptr(res), ptr(sums), stream_ptr()))
    return _ret(tri, det), _ret(npairs, det), _ret(mask, det), _ret(res, det), _ret(sums, det)


def extrinsic_cov(n_cams, std_rot_deg, std_t_m, fixed=()):
    """A diagonal covariance of the extrinsics of ``n_cams`` cameras for ``FTEContext.calibration_sensitivity`` /
    ``fte_solve(cov_cams=...)`` when no bundle-adjustment covariance is at hand: [6 n_cams, 6 n_cams] float64 in the order
    and units of ``sba.covariance``'s ``cov_cams`` - per camera (dw [rad], dt [m]) with R <- exp([dw]x) R, t <- t + dt -,
    ``std_rot_deg`` degrees per rotation axis and ``std_t_m`` metres per translation axis, uncorrelated.  The cameras
    listed in ``fixed`` (held by the gauge, e.g. ``(0,)``) get zero rows and columns."""
    n_cams = int(n_cams)
    if n_cams < 1:
        raise ValueError("n_cams must be >= 1")
    if not (np.isfinite(std_rot_deg) and np.isfinite(std_t_m)) or std_rot_deg < 0 or std_t_m < 0:
        raise ValueError("std_rot_deg and std_t_m must be finite and >= 0")
    fixed = [int(c) for c in fixed]
    if any(c < 0 or c >= n_cams for c in fixed):
        raise ValueError(f"fixed cameras must lie in 0..{n_cams - 1}")
    var = np.tile(np.r_[np.full(3, np.deg2rad(float(std_rot_deg)) ** 2), np.full(3, float(std_t_m) ** 2)], n_cams)
    for c in fixed:
        var[6 * c:6 * c + 6] = 0.0
    return np.diag(var)


def cov_cams_matrix(cov_cams, n_cams):
    """``cov_cams`` as a checked float64 numpy [6C, 6C] matrix (None stays None): host arithmetic, no launch."""
    if cov_cams is None:
        return None
    if isinstance(cov_cams, dict):
        if "cov_cams" not in cov_cams:
            raise ValueError('cov_cams given as a dict must hold "cov_cams" (the dict of sba.covariance)')
        cov_cams = cov_cams["cov_cams"]
    a = cov_cams.detach().cpu().numpy() if isinstance(cov_cams, torch.Tensor) else np.asarray(cov_cams)
    a = np.asarray(a, dtype=np.float64)
    W = 6 * int(n_cams)
    if a.shape != (W, W):
        raise ValueError(f"cov_cams must be [{W}, {W}] (6 per camera: dw, dt), got {tuple(a.shape)}")
    if not np.isfinite(a).all():
        raise ValueError("cov_cams has a non-finite entry")
    if not np.allclose(a, a.T, rtol=1e-12, atol=1e-12 * max(float(np.abs(a).max()), 1e-300)):
        raise ValueError("cov_cams is not symmetric")
    return np.ascontiguousarray(a)


def dataframe_to_dense(points_2d_df, n_cameras):
    """Long DataFrame [frame, camera, marker, x, y, (likelihood)] -> dense det[N,C,L,3] plus the sorted
    frame and marker keys.  Rows absent from the frame get likelihood -inf (never valid)."""
    df = points_2d_df
    frames = np.sort(df["frame"].unique())
    markers = np.array(sorted(df["marker"].unique()), dtype=object)
    fi = np.searchsorted(frames, df["frame"].to_numpy())
    mi = np.searchsorted(markers.astype(str), df["marker"].to_numpy().astype(str))
    ci = df["camera"].to_numpy().astype(np.int64)
    if ci.size and (ci.min() < 0 or ci.max() >= n_cameras):
        raise ValueError("camera index outside the rig")
    det = np.zeros((len(frames), n_cameras, len(markers), 3))
    det[..., 2] = -np.inf
    det[fi, ci, mi, 0] = df["x"].to_numpy(dtype=np.float64)
    det[fi, ci, mi, 1] = df["y"].to_numpy(dtype=np.float64)
    det[fi, ci, mi, 2] = df["likelihood"].to_numpy(dtype=np.float64) if "likelihood" in df else 1.0
    return det, frames, markers


def get_pairwise_3d_points_from_df(points_2d_df, k_arr, d_arr, r_arr, t_arr, triangulate_func=None):
    """Adjacent-pair triangulation of a long detections DataFrame (calib.py:394-423).

    Output rows are sorted by (frame, marker) with ``frame`` as float64, exactly as the reference's
    groupby().mean().reset_index().  The caller pre-filters by likelihood (all_optimizations.py:262-263),
    so every row present is valid.  ``triangulate_func`` is the reference's injection seam (calib.py:394,
    412-413; app.py:215-223 injects either pair function): ``triangulate_points_fisheye`` (default) and
    ``triangulate_points`` select the fused dense HIP kernel of that camera model; any other callable raises
    (there is no CPU path here to run foreign Python per pair).
    Like the reference, raises KeyError when no adjacent pair exists at all.
    """
    import pandas as pd
    model = camera_model_of(project_func=triangulate_func, seams=(triangulate_points_fisheye, triangulate_points))
    n_cam = len(k_arr)
    det, frames, markers = dataframe_to_dense(points_2d_df, n_cam)
    det[..., 2] = np.where(np.isfinite(det[..., 2]), np.inf, -np.inf)   # presence == valid
    tri, cnt, _ = triangulate_pairs_dense(det, 0.0, k_arr, d_arr, r_arr, t_arr, model=model)
    has = cnt > 0
    if not has.any():
        raise KeyError("['frame', 'marker'] not in index")
    n_i, l_i = np.nonzero(has)
    return pd.DataFrame({"frame": np.asarray(frames, dtype=np.float64)[n_i], "marker": markers[l_i],
                         "x": tri[n_i, l_i, 0], "y": tri[n_i, l_i, 1], "z": tri[n_i, l_i, 2]})


def get_multiview_3d_points_from_df(points_2d_df, k_arr, d_arr, r_arr, t_arr, triangulate_func=None, **kw):
    """``triangulate_multiview_dense`` of a long detections DataFrame, with the conventions of
    ``get_pairwise_3d_points_from_df``: every row present is valid, the rows of the result are sorted by (frame, marker),
    ``frame`` is float64, and ``triangulate_func`` (``triangulate_points_fisheye``, the default, or ``triangulate_points``)
    selects the camera model.  Columns frame, marker, x, y, z, std, n_views, for the points with status 0 or 1 - every marker
    seen by two or more cameras, adjacent or not.  ``kw``: the keywords of ``triangulate_multiview_dense`` (f_scale, sigma_px,
    max_iter, xtol).  Raises KeyError when there is no such point."""
    import pandas as pd
    model = camera_model_of(project_func=triangulate_func, seams=(triangulate_points_fisheye, triangulate_points))
    det, frames, markers = dataframe_to_dense(points_2d_df, len(k_arr))
    det[..., 2] = np.where(np.isfinite(det[..., 2]), np.inf, -np.inf)   # presence == valid
    out = triangulate_multiview_dense(det, 0.0, k_arr, d_arr, r_arr, t_arr, model=model, **kw)
    has = out["status"] < 2
    if not has.any():
        raise KeyError("['frame', 'marker'] not in index")
    n_i, l_i = np.nonzero(has)
    pts = out["points"]
    return pd.DataFrame({"frame": np.asarray(frames, dtype=np.float64)[n_i], "marker": markers[l_i],
                         "x": pts[n_i, l_i, 0], "y": pts[n_i, l_i, 1], "z": pts[n_i, l_i, 2], "std": out["std"][n_i, l_i],
                         "n_views": out["n_views"][n_i, l_i]})
