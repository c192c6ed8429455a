"""Sparse bundle adjustment on the GPU - drop-ins for the SBA entry points of ``src/calib/calib.py``.

    prepare_calib_board_data_for_bundle_adjustment(...)            calib.py:210-263
    prepare_manual_points_for_bundle_adjustment(...)               calib.py:266-304
    bundle_adjust_points_only(..., project_func, f_scale=50)       calib.py:327-341
    bundle_adjust_board_points_only(...)                           calib.py:319-324
    bundle_adjust_points_and_extrinsics(..., project_func)         calib.py:369-390
    bundle_adjust_board_points_and_extrinsics(...)                 calib.py:362-366

Same argument order and return values (``obj_pts[, r_arr, t_arr], residuals`` with ``residuals = dict(before=,
after=)`` flat ``(reprojected - points_2d).ravel()`` vectors).  ``project_func`` selects the camera model exactly as
the reference's two call sites do (app.py:215-223): ``project_points_fisheye`` -> cv2.fisheye, ``project_points`` ->
cv2.projectPoints (rational / tangential / thin-prism pinhole); the arithmetic is the analytic-Jacobian Levenberg-Marquardt solver in csrc/sba.hip, which
minimises the SAME robust cost as scipy's ``least_squares(loss='cauchy', f_scale=...)``.  The last solve's
summary (costs, iterations, status) is kept in ``last_info``.

Error bars: ``covariance(...)`` evaluates the covariance of the extrinsics and of every point at a given iterate
(csrc/sba_cov.hip); ``return_cov=True`` on the entry points above and on the dense / clip refinements evaluates it at
the iterate they return.
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib, calib
from ._lib import SbaCovInfo, SbaInfo, SbaParams, check, lib, ptr, stream_ptr

last_info = None
# acino_sba_params::precision: fp64 throughout, or BASELINE config 5's "bf16 residuals with fp32 accumulate"
PRECISIONS = {"f64": 0, "bf16": 1}


def _csr_by_point(point_3d_indices, n_points):
    idx = np.asarray(point_3d_indices, dtype=np.int64)
    if idx.size and (idx.min() < 0 or idx.max() >= n_points):
        raise ValueError("point_3d_indices out of range")
    order = np.argsort(idx, kind="stable").astype(np.int32)
    start = np.zeros(n_points + 1, dtype=np.int32)
    np.cumsum(np.bincount(idx, minlength=n_points), out=start[1:])
    return start, order


class ReduceHook:
    """The callback of ``acino_sba_solve_sharded``: combines ``n`` doubles at an address inside the workspace tensor
    ``ws`` over all ranks, in place (op 0 sum, 1 max).  ``comm`` offers ``all_reduce(tensor, op)`` - by default
    torch.distributed (backend "nccl" = RCCL on the GPU node; with "gloo" device memory is staged through the host,
    which is how several ranks can share one GPU in the tests)."""

    def __init__(self, ws, group=None):
        self.ws, self.group, self.calls, self.error = ws, group, 0, None
        self.sizes = []                      # doubles per reduction, in call order
        self.fn = _lib.REDUCE_FN(self._call)

    def all_reduce(self, t, op):
        import torch.distributed as dist
        rop = dist.ReduceOp.MAX if op == 1 else dist.ReduceOp.SUM
        if t.is_cuda and dist.get_backend(self.group) == "gloo":
            h = t.cpu()
            dist.all_reduce(h, op=rop, group=self.group)
            t.copy_(h)
        else:
            dist.all_reduce(t, op=rop, group=self.group)
        if t.is_cuda:
            torch.cuda.current_stream().synchronize()

    def _call(self, _user, buf, n, op, _stream):
        try:
            off = int(buf) - self.ws.data_ptr()
            if off < 0 or off % 8 or off + 8 * n > self.ws.numel():
                raise ValueError("reduction buffer outside the workspace")
            self.all_reduce(self.ws[off:off + 8 * n].view(torch.float64), op)
            self.calls += 1
            self.sizes.append(int(n))
            return 0
        except Exception as e:      # an exception must not unwind through the C frames
            self.error = e
            return 1


GAUGES = {"baseline": 0, "free": 1, "custom": 2}     # ACINO_SBA_GAUGE_*
SCALES = {"residual": 0, "unit": 1}                  # ACINO_SBA_SCALE_*


def _cov_options(n_cams, optimize_cameras, gauge="baseline", ref_cam=0, scale_cam=1, scale="residual", group=None):
    """The checks of the covariance keywords that need no device; returns (gauge name, constraint matrix or None)."""
    if group is not None:
        raise ValueError("return_cov=True with group=: the covariance of a solve whose points are sharded over ranks is not "
                         "available (it needs one more all-reduce of the reduced camera system)")
    if scale not in SCALES:
        raise ValueError(f"scale must be one of {sorted(SCALES)}, not {scale!r}")
    if isinstance(gauge, str):
        if gauge not in ("baseline", "free"):
            raise ValueError(f"gauge must be 'baseline', 'free' or a [6C, 7] constraint matrix, not {gauge!r}")
        name, mat = gauge, None
    else:
        mat = np.ascontiguousarray(np.asarray(gauge, dtype=np.float64))
        if mat.shape != (6 * n_cams, 7):
            raise ValueError(f"a custom gauge is a [6C, 7] = {(6 * n_cams, 7)} constraint matrix, not {mat.shape}")
        name = "custom"
    if optimize_cameras:
        if n_cams < 2:
            raise ValueError("the covariance of the extrinsics needs at least two cameras")
        if name == "baseline":
            ref_cam, scale_cam = int(ref_cam), int(scale_cam)
            if not (0 <= ref_cam < n_cams and 0 <= scale_cam < n_cams):
                raise ValueError("ref_cam and scale_cam must be cameras of the rig")
            if ref_cam == scale_cam:
                raise ValueError("ref_cam and scale_cam must differ: the baseline between them fixes the scale")
    return name, mat


def _workspace(nbytes, dev):
    """``nbytes`` of device memory from a 256-byte boundary: (the tensor that owns them, the aligned address)."""
    ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=dev)
    return ws, C.c_void_p((ws.data_ptr() + 255) // 256 * 256)


def _device_problem(intr, Rt, pts, uv, cam_idx, start, order, model, optimize_cameras, f_scale, lam0=1e-3, ftol=0.0, gtol=0.0,
                    max_iter=0, precision="f64"):
    """The problem as the library takes it: the seven arrays on the current device (host arrays are uploaded, device tensors
    stay where they are), ``acino_sba_params`` and ``head``, the leading arguments of both library entries.  A solve updates
    ``Rt[C, 12]`` and ``pts[P, 3]`` in place; the covariance reads them (and none of the solver's keywords)."""
    dev = torch.device("cuda", torch.cuda.current_device())
    p = SimpleNamespace(model=model, optimize_cameras=bool(optimize_cameras), f_scale=float(f_scale), n_cams=len(intr), dev=dev)
    p.intr, p.Rt, p.pts, p.uv, p.cam, p.start, p.order = (torch.as_tensor(a, device=dev)
                                                          for a in (intr, Rt, pts, uv, cam_idx, start, order))
    p.n_points, p.n_obs = int(p.pts.shape[0]), int(p.uv.shape[0])
    p.prm = SbaParams(n_cams=p.n_cams, optimize_cameras=int(p.optimize_cameras), n_points=p.n_points, n_obs=p.n_obs,
                      f_scale=p.f_scale, lam0=float(lam0), ftol=float(ftol), gtol=float(gtol), max_iter=int(max_iter),
                      camera_model=calib.CAMERAS[model].code, precision=PRECISIONS[precision])
    p.head = (C.byref(p.prm), ptr(p.intr), ptr(p.Rt), ptr(p.pts), ptr(p.uv), ptr(p.cam), ptr(p.start), ptr(p.order))
    return p


def _covariance_device(p, gauge="baseline", ref_cam=0, scale_cam=1, scale="residual", points=True, raise_numeric=True):
    """acino_sba_covariance at the iterate of a device problem; returns the dict of ``covariance``."""
    n_cams, optimize_cameras, n_points, n = p.n_cams, p.optimize_cameras, p.n_points, 6 * p.n_cams
    name, mat = _cov_options(n_cams, optimize_cameras, gauge, ref_cam, scale_cam, scale)
    nbytes = lib().acino_sba_covariance_workspace_bytes(n_cams, n_points, p.n_obs)
    _ws, ws_ptr = _workspace(nbytes, p.dev)
    empty = lambda *shape: torch.empty(shape, dtype=torch.float64, device=p.dev)   # noqa: E731
    cov_cams = empty(n, n) if optimize_cameras else None
    cov_pts = empty(n_points, 6) if points else None
    std_pts = empty(n_points) if points else None
    info = SbaCovInfo()
    rc = lib().acino_sba_covariance(*p.head, GAUGES[name], int(ref_cam), int(scale_cam),
                                    mat.ctypes.data_as(C.c_void_p) if mat is not None else C.c_void_p(0), SCALES[scale],
                                    ws_ptr, nbytes, ptr(cov_cams), ptr(cov_pts), ptr(std_pts), C.byref(info), stream_ptr())
    if raise_numeric or rc != -6:                  # (ACINO_ERR_NUMERIC: the status word and NaN outputs are set)
        check(rc)
    torch.cuda.current_stream().synchronize()
    out = dict(cov_cams=None, cov_cam=None, std_rot_deg=None, cov_center=None, std_center=None, cov_points=None,
               std_points=None, sigma2=info.sigma2, dof=int(info.dof), n_points_excluded=int(info.n_points_excluded),
               n_obs_used=int(info.n_obs_used), sum_w_r2=info.sum_w_r2, min_pivot_ratio=info.min_pivot_ratio,
               gauge=name if optimize_cameras else None, scale=scale, status_name=info.as_dict()["status_name"])
    if optimize_cameras:
        cc = cov_cams.cpu().numpy()
        Rt = p.Rt.cpu().numpy()
        blocks = np.stack([cc[6 * c:6 * c + 6, 6 * c:6 * c + 6] for c in range(n_cams)])
        # camera centre c = -R^T t: dc = -R^T [t]x dw - R^T dt
        jac = np.zeros((n_cams, 3, 6))
        for c in range(n_cams):
            R, t = Rt[c, :9].reshape(3, 3), Rt[c, 9:]
            tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
            jac[c, :, :3] = -R.T @ tx
            jac[c, :, 3:] = -R.T
        cen = np.einsum("cia,cab,cjb->cij", jac, blocks, jac)
        # (a camera the gauge holds has zero variance up to rounding of either sign: np.maximum keeps NaN, clips -1e-40)
        out.update(cov_cams=cc, cov_cam=blocks, cov_center=cen,
                   std_rot_deg=np.degrees(np.sqrt(np.maximum(np.einsum("cii->c", blocks[:, :3, :3]), 0.0))),
                   std_center=np.sqrt(np.maximum(np.einsum("cii->c", cen), 0.0)))
    if points:
        pk = cov_pts.cpu().numpy()
        full = np.empty((n_points, 3, 3))
        for q, (i, j) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
            full[:, i, j] = full[:, j, i] = pk[:, q]
        out.update(cov_points=full, std_points=std_pts.cpu().numpy())
    return out


def _camera_tables(k_arr, d_arr, r_arr, t_arr, model, so3):
    """intr[C, 16] = fx fy cx cy | distortion, Rt[C, 12] = R row-major | t.  ``so3``: every rotation is projected onto SO(3),
    as cv2.Rodrigues does in calib.py:373 (scene files carry ~1e-8 of round-off)."""
    n_cams = len(k_arr)
    intr = np.zeros((n_cams, 16))
    Rt = np.zeros((n_cams, 12))
    for c in range(n_cams):
        k = np.asarray(k_arr[c], dtype=np.float64)
        dist = np.asarray(d_arr[c], dtype=np.float64).reshape(-1)
        if model == "fisheye":
            if abs(k[0, 1]) > 1e-12 * abs(k[0, 0]):
                raise NotImplementedError("skewed fisheye intrinsics are not supported by the GPU bundle adjustment "
                                          "(calib.py:78 calibrates with CALIB_FIX_SKEW)")
            if dist.size != 4:
                raise ValueError("fisheye cameras have 4 distortion coefficients")
        elif dist.size not in (4, 5, 8, 12):
            raise ValueError("pinhole distortion vector must have 4, 5, 8 or 12 entries (cv2.projectPoints)")
        intr[c, :4] = [k[0, 0], k[1, 1], k[0, 2], k[1, 2]]
        intr[c, 4:4 + dist.size] = dist
        r = np.asarray(r_arr[c], dtype=np.float64)
        r = calib._rodrigues(r) if r.size == 3 else r
        if so3:
            u, _s, vt = np.linalg.svd(r)
            r = u @ vt
        Rt[c, :9] = r.reshape(-1)
        Rt[c, 9:] = np.asarray(t_arr[c], dtype=np.float64).reshape(-1)
    return intr, Rt


def covariance(points_2d, points_3d, point_3d_indices, camera_indices, k_arr, d_arr, r_arr, t_arr, optimize_cameras=True,
               project_func=None, f_scale=1.0, gauge="baseline", ref_cam=0, scale_cam=1, scale="residual", points=True,
               raise_numeric=True):
    """Error bars of the bundle adjustment at the iterate (r_arr, t_arr, points_3d), independent of any solve: the inverse
    of A = J^T W J (J: Jacobian of (reprojected - points_2d) under R <- exp([dw]x) R, t <- t + dt; W: the Cauchy IRLS weights
    1 / (1 + (r / f_scale)^2); no damping; fp64).  With the cameras free A has a 7-dimensional null space (world translation,
    rotation, scale), so the covariance is taken under seven constraints on the CAMERA parameters:

      gauge="baseline"   the pose of ``ref_cam`` and the distance between the centres of ``ref_cam`` and ``scale_cam`` are held
                         (camera 0 as the world frame - the gauge of the reference's rigs)
      gauge="free"       the free-network covariance over the cameras: the Moore-Penrose inverse of the reduced camera system
      gauge=ndarray      a [6C, 7] constraint matrix of the caller

    ``scale="residual"`` multiplies every covariance by sigma2 = sum w r^2 / (2 M - dof), the noise level estimated from the
    residuals (the Cauchy cost is not a normalised likelihood); ``scale="unit"`` returns the unit-weight inverse.  A point with
    a single view is left out (NaN, counted in ``n_points_excluded``).  ``optimize_cameras=False``: points only, Sigma_p =
    V_p^-1 (``bundle_adjust_points_only`` uses f_scale=50).  Returns a dict: cov_cams[6C, 6C] (per camera [dw, dt]),
    cov_cam[C, 6, 6], std_rot_deg[C], cov_center[C, 3, 3], std_center[C] (m), cov_points[P, 3, 3], std_points[P] (sqrt of the
    trace, m), sigma2, dof, n_points_excluded, gauge, scale, status_name.  A singular problem (a camera no point sees, too few
    points, constraints that do not fix the gauge) raises RuntimeError, or with ``raise_numeric=False`` returns NaN arrays and
    status_name "numeric"."""
    _cov_options(len(k_arr), optimize_cameras, gauge, ref_cam, scale_cam, scale)
    model = calib.camera_model_of(None, project_func, by_name=True)
    p = _problem(points_2d, points_3d, point_3d_indices, camera_indices, k_arr, d_arr, r_arr, t_arr, optimize_cameras, f_scale,
                 model)
    return _covariance_device(p, gauge, ref_cam, scale_cam, scale, points, raise_numeric)


def _problem(points_2d, points_3d, point_3d_indices, camera_indices, k_arr, d_arr, r_arr, t_arr, optimize_cameras, f_scale,
             model, camera_range=True, duplicates=False, **solver_kw):
    """The device problem of the list-based entries: the arrays normalised, one entry per observation, the optional host checks,
    the observations grouped by point (CSR), the camera tables; everything that can be refused is refused before the device
    is asked for."""
    n_cams = len(k_arr)
    pts0 = np.ascontiguousarray(np.asarray(points_3d, dtype=np.float64).reshape(-1, 3))
    uv = np.ascontiguousarray(np.asarray(points_2d, dtype=np.float64).reshape(-1, 2))
    cam_idx = np.ascontiguousarray(np.asarray(camera_indices, dtype=np.int32).reshape(-1))
    n_obs = uv.shape[0]
    if cam_idx.size != n_obs or len(point_3d_indices) != n_obs:
        raise ValueError("points_2d, point_3d_indices and camera_indices must have one entry per observation")
    if camera_range and n_obs and (cam_idx.min() < 0 or cam_idx.max() >= n_cams):
        raise ValueError("camera_indices out of range")
    if duplicates and n_obs:
        # one GPU lane per (point, camera) slot (csrc/sba.hip): one observation per pair
        key = np.asarray(point_3d_indices, dtype=np.int64).reshape(-1) * n_cams + cam_idx
        if np.unique(key).size != key.size:
            raise ValueError("a point is observed twice by the same camera: merge the duplicate observations first")
    start, order = _csr_by_point(point_3d_indices, pts0.shape[0])
    intr, Rt = _camera_tables(k_arr, d_arr, r_arr, t_arr, model, bool(optimize_cameras))
    _lib.require_gpu()
    return _device_problem(intr, Rt, pts0, uv, cam_idx, start, order, model, optimize_cameras, f_scale, **solver_kw)


def _run_solve(p, sharded=False, group=None):
    """acino_sba_solve_sharded on a device problem, in place (``acino_sba_solve`` is this call with a null callback): the
    residuals before and after [M, 2] and the reduction hook (None unless ``sharded``); sets ``last_info``."""
    global last_info
    nbytes = lib().acino_sba_workspace_bytes(p.n_cams, p.n_points, p.n_obs)
    ws, ws_ptr = _workspace(nbytes, p.dev)
    res_b = torch.empty((p.n_obs, 2), dtype=torch.float64, device=p.dev)
    res_a = torch.empty((p.n_obs, 2), dtype=torch.float64, device=p.dev)
    info = SbaInfo()
    hook = ReduceHook(ws, group) if sharded else None
    status = lib().acino_sba_solve_sharded(*p.head, ws_ptr, nbytes, ptr(res_b), ptr(res_a), C.byref(info),
                                           hook.fn if hook else _lib.REDUCE_FN(0), None, stream_ptr())
    if hook is not None and hook.error is not None:
        raise hook.error
    check(status)
    torch.cuda.current_stream().synchronize()
    last_info = info.as_dict()
    return res_b, res_a, hook


def _solve(points_2d, points_3d, point_3d_indices, camera_indices, k_arr, d_arr, r_arr, t_arr, optimize_cameras,
           f_scale, max_iter, ftol, gtol, lam0=1e-3, model="fisheye", group=None, sharded=False, precision="f64", host_checks=True,
           cov_kw=None):
    """``cov_kw``: the keywords of ``_covariance_device`` - the covariance at the returned iterate is appended to the result.
    ``host_checks=False`` leaves the camera-range and duplicate tests to the library, which makes them itself on the device -
    the C ABI's own guard, exercised by the tests - and answers ACINO_ERR_INVALID_ARG = ValueError."""
    n_cams = len(k_arr)
    if cov_kw is not None:
        _cov_options(n_cams, optimize_cameras, group=group, **cov_kw)
    p = _problem(points_2d, points_3d, point_3d_indices, camera_indices, k_arr, d_arr, r_arr, t_arr, optimize_cameras, f_scale,
                 model, camera_range=host_checks, duplicates=host_checks, lam0=lam0, ftol=ftol, gtol=gtol, max_iter=max_iter,
                 precision=precision)
    res_b, res_a, _hook = _run_solve(p, sharded, group)
    Rt_o = p.Rt.cpu().numpy()
    out = (p.pts.cpu().numpy(), Rt_o[:, :9].reshape(n_cams, 3, 3).copy(), Rt_o[:, 9:].reshape(n_cams, 3, 1).copy(),
           dict(before=res_b.cpu().numpy().ravel(), after=res_a.cpu().numpy().ravel()))
    if cov_kw is not None:
        out += (_covariance_device(p, **cov_kw),)
    return out


def _cov_kw(return_cov, gauge, ref_cam, scale_cam, scale):
    return dict(gauge=gauge, ref_cam=ref_cam, scale_cam=scale_cam, scale=scale) if return_cov else None


def bundle_adjust_points_only(points_2d, points_3d, point_3d_indices, camera_indices, k_arr, d_arr, r_arr, t_arr,
                              project_func=None, f_scale=50, max_iter=200, ftol=1e-15, gtol=1e-10, return_cov=False,
                              gauge="baseline", ref_cam=0, scale_cam=1, scale="residual"):
    """calib.py:327-341: refine the 3-D points, cameras fixed; Cauchy loss with scale ``f_scale`` px.  ``return_cov=True``
    appends the covariance dict of ``covariance`` at the refined points (points only: no gauge; the same ``f_scale``)."""
    out = _solve(points_2d, points_3d, point_3d_indices, camera_indices, k_arr, d_arr, r_arr, t_arr,
                 False, f_scale, max_iter, ftol, gtol, model=calib.camera_model_of(None, project_func, by_name=True),
                 cov_kw=_cov_kw(return_cov, gauge, ref_cam, scale_cam, scale))
    return (out[0],) + out[3:]


def bundle_adjust_points_and_extrinsics(points_2d, points_3d, point_3d_indices, camera_indices, k_arr, d_arr, r_arr,
                                        t_arr, project_func=None, max_iter=300, ftol=1e-10, gtol=1e-10, precision="f64",
                                        return_cov=False, gauge="baseline", ref_cam=0, scale_cam=1, scale="residual"):
    """calib.py:369-390: refine the 3-D points and every camera's rotation + translation (Cauchy loss, scale 1).
    ``precision="bf16"``: BASELINE config 5's mixed mode (residual / Jacobian rows in bf16, blocks accumulated in fp32).
    ``return_cov=True`` appends the covariance dict of ``covariance`` at the returned iterate (always evaluated in fp64)."""
    return _solve(points_2d, points_3d, point_3d_indices, camera_indices, k_arr, d_arr, r_arr, t_arr, True, 1.0,
                  max_iter, ftol, gtol, model=calib.camera_model_of(None, project_func, by_name=True), precision=precision,
                  cov_kw=_cov_kw(return_cov, gauge, ref_cam, scale_cam, scale))


def bundle_adjust_points_and_extrinsics_sharded(points_2d, points_3d, point_3d_indices, camera_indices, k_arr, d_arr,
                                                r_arr, t_arr, project_func=None, max_iter=300, ftol=1e-10, gtol=1e-10,
                                                group=None, precision="f64"):
    """The same refinement with the POINTS spread over the ranks of a torch.distributed group (one process per GPU)
    and the cameras shared: every rank passes its own points / observations (``point_3d_indices`` local, 0-based) and
    the same initial poses; the reduced camera system is summed over the ranks each iteration (a 6C x 6C block + 6C
    vector - BASELINE config 5's extrinsic refinement over all sequences).  Returns this rank's refined points, the
    common poses and this rank's residuals; ``last_info`` carries the GLOBAL costs."""
    return _solve(points_2d, points_3d, point_3d_indices, camera_indices, k_arr, d_arr, r_arr, t_arr, True, 1.0,
                  max_iter, ftol, gtol, model=calib.camera_model_of(None, project_func, by_name=True), group=group,
                  sharded=True, precision=precision)


def prepare_calib_board_data_for_bundle_adjustment(img_pts_arr, fnames_arr, board_shape, k_arr, d_arr, r_arr, t_arr,
                                                   triangulate_func=None):
    """calib.py:210-263.  Boards seen by >= 2 cameras, in sorted file-name order (the reference iterates a
    set-built dict, i.e. an arbitrary order; the optimum does not depend on it).  Initial points from the first two
    cameras that see each board, all boards triangulated in one batched launch per camera pair."""
    triangulate_func = triangulate_func or calib.triangulate_points_fisheye
    n_cam = len(img_pts_arr)
    fnames_arr = [list(f) for f in fnames_arr]
    count = {}
    for fnames in fnames_arr:
        for f in set(fnames):
            count[f] = count.get(f, 0) + 1
    keep = sorted(f for f, v in count.items() if v >= 2)
    per_img = int(board_shape[0] * board_shape[1])
    lookup = [{f: i for i, f in reversed(list(enumerate(fnames)))} for fnames in fnames_arr]   # .index() = first hit
    points_2d, point_3d_indices, camera_indices = [], [], []
    pair_jobs = {}
    for b, fname in enumerate(keep):
        seen = [(cam, lookup[cam][fname]) for cam in range(n_cam) if fname in lookup[cam]]
        for cam, f_idx in seen:
            points_2d.append(np.asarray(img_pts_arr[cam][f_idx], dtype=np.float64).reshape(per_img, 2))
            point_3d_indices.append(np.arange(b * per_img, (b + 1) * per_img))
            camera_indices.append(np.full(per_img, cam))
        (ca, fa), (cb, fb) = seen[0], seen[1]
        pair_jobs.setdefault((ca, cb), []).append((b, fa, fb))
    points_3d = np.zeros((len(keep) * per_img, 3))
    for (ca, cb), jobs in pair_jobs.items():
        pa = np.concatenate([np.asarray(img_pts_arr[ca][fa], dtype=np.float64).reshape(per_img, 2) for _, fa, _ in jobs])
        pb = np.concatenate([np.asarray(img_pts_arr[cb][fb], dtype=np.float64).reshape(per_img, 2) for _, _, fb in jobs])
        est = np.asarray(triangulate_func(pa, pb, k_arr[ca], d_arr[ca], r_arr[ca], t_arr[ca],
                                          k_arr[cb], d_arr[cb], r_arr[cb], t_arr[cb])).reshape(-1, 3)
        for j, (b, _, _) in enumerate(jobs):
            points_3d[b * per_img:(b + 1) * per_img] = est[j * per_img:(j + 1) * per_img]
    if not keep:
        return (np.zeros((0, 2), np.float32), np.zeros((0, 3), np.float32), np.zeros(0, int), np.zeros(0, int))
    return (np.concatenate(points_2d).astype(np.float32), points_3d.astype(np.float32),
            np.concatenate(point_3d_indices).astype(int), np.concatenate(camera_indices).astype(int))


def prepare_manual_points_for_bundle_adjustment(img_pts_arr, k_arr, d_arr, r_arr, t_arr, triangulate_func=None):
    """calib.py:266-304: img_pts_arr[n_points, n_cameras, 2] with NaN where a camera does not see the point."""
    triangulate_func = triangulate_func or calib.triangulate_points_fisheye
    pts = np.asarray(img_pts_arr, dtype=np.float64).swapaxes(0, 1)
    n_cam, n_pts = pts.shape[0], pts.shape[1]
    points_2d, point_3d_indices, camera_indices, first_two = [], [], [], []
    p = 0
    for i in range(n_pts):
        cams = [c for c in range(n_cam) if not np.isnan(pts[c, i]).any()]
        if len(cams) > 1:
            points_2d.extend(pts[c, i] for c in cams)
            camera_indices.extend(cams)
            point_3d_indices.extend([p] * len(cams))
            first_two.append((cams[0], cams[1], i))
            p += 1
    points_3d = np.zeros((p, 1, 3))
    groups = {}
    for j, (a, b, i) in enumerate(first_two):
        groups.setdefault((a, b), []).append((j, i))
    for (a, b), items in groups.items():
        ia = np.array([i for _, i in items])
        est = np.asarray(triangulate_func(pts[a, ia], pts[b, ia], k_arr[a], d_arr[a], r_arr[a], t_arr[a],
                                          k_arr[b], d_arr[b], r_arr[b], t_arr[b])).reshape(-1, 3)
        points_3d[[j for j, _ in items], 0] = est
    return (np.array(points_2d, dtype=np.float32).reshape(-1, 2), points_3d.astype(np.float32),
            np.array(point_3d_indices, dtype=int), np.array(camera_indices, dtype=int))


def bundle_adjust_board_points_only(img_pts_arr, fnames_arr, board_shape, k_arr, d_arr, r_arr, t_arr,
                                    triangulate_func=None, project_func=None, return_cov=False, gauge="baseline",
                                    ref_cam=0, scale_cam=1, scale="residual"):
    """calib.py:319-324.  ``return_cov``: as ``bundle_adjust_points_only``."""
    data = prepare_calib_board_data_for_bundle_adjustment(img_pts_arr, fnames_arr, board_shape, k_arr, d_arr, r_arr,
                                                          t_arr, triangulate_func)
    return bundle_adjust_points_only(*data, k_arr, d_arr, r_arr, t_arr, project_func, return_cov=return_cov, gauge=gauge,
                                     ref_cam=ref_cam, scale_cam=scale_cam, scale=scale)


def bundle_adjust_board_points_and_extrinsics(img_pts_arr, fnames_arr, board_shape, k_arr, d_arr, r_arr, t_arr,
                                              triangulate_func=None, project_func=None, return_cov=False,
                                              gauge="baseline", ref_cam=0, scale_cam=1, scale="residual"):
    """calib.py:362-366.  ``return_cov``: as ``bundle_adjust_points_and_extrinsics``."""
    data = prepare_calib_board_data_for_bundle_adjustment(img_pts_arr, fnames_arr, board_shape, k_arr, d_arr, r_arr,
                                                          t_arr, triangulate_func)
    return bundle_adjust_points_and_extrinsics(*data, k_arr, d_arr, r_arr, t_arr, project_func, return_cov=return_cov,
                                               gauge=gauge, ref_cam=ref_cam, scale_cam=scale_cam, scale=scale)


# ---------------------------------------------------------------------------------------------------------------
# BASELINE config 5: extrinsic refinement over the marker trajectories of many sequences (app.py:201-223 feeds board
# corners or hand-picked points into calib.py:345-390; here the points are the FTE marker positions of every clip and
# the observations their above-threshold detections, the six extrinsics shared by all sequences)
# ---------------------------------------------------------------------------------------------------------------
def dense_observations(det, dlc_thresh, min_views=2):
    """Observation lists of dense detections det[N, C, L, 3] = (x, y, likelihood), built on the device: every (frame,
    marker) seen by >= min_views cameras above the threshold (calib.py:281 keeps points with > 1 view) becomes a point;
    observations are point-major, cameras ascending.  Returns (keep[N, L] bool, uv[M, 2], cam_idx[M] int32,
    pt_start[P + 1] int32, pt_obs[M] int32) as device tensors."""
    lik = det[..., 2].permute(0, 2, 1)                    # [N, L, C]
    seen = lik > dlc_thresh
    keep = seen.sum(-1) >= min_views                      # [N, L]
    sel = seen & keep[..., None]
    idx = torch.nonzero(sel)                              # rows sorted by (frame, marker, camera)
    uv = det.permute(0, 2, 1, 3)[idx[:, 0], idx[:, 1], idx[:, 2], :2].contiguous()
    cam_idx = idx[:, 2].to(torch.int32).contiguous()
    counts = sel.sum(-1)[keep]                            # observations per kept point, in point order
    pt_start = torch.zeros(counts.numel() + 1, dtype=torch.int32, device=det.device)
    pt_start[1:] = torch.cumsum(counts, 0).to(torch.int32)
    pt_obs = torch.arange(uv.shape[0], dtype=torch.int32, device=det.device)
    return keep, uv, cam_idx, pt_start, pt_obs


def bundle_adjust_dense_points_and_extrinsics(det, points_3d, k_arr, d_arr, r_arr, t_arr, dlc_thresh=0.5, precision="f64",
                                              max_iter=100, ftol=1e-10, gtol=1e-10, f_scale=1.0, lam0=1e-3, min_views=2,
                                              group=None, camera_model=None, return_cov=False, gauge="baseline", ref_cam=0,
                                              scale_cam=1, scale="residual"):
    """calib.py:369-390 on DENSE data, everything resident on the device: det[N, C, 20, 3] detections and
    points_3d[N, 20, 3] initial points (e.g. ``positions`` of an FTE solve, clips concatenated along N).  ``camera_model``:
    "fisheye" (the default) or "pinhole" (cv2.projectPoints, distortion vectors of 4, 5, 8 or 12 entries; fp64 only:
    ``precision="bf16"`` with pinhole is a ValueError before any device work).  Returns (points[N, 20, 3] - refined where a point had >= min_views views, input value elsewhere -, r_arr[C, 3, 3],
    t_arr[C, 3, 1], info) with info = the solver summary plus ``n_points``, ``n_obs`` and the rms residuals (px)
    before / after.  ``group``: a torch.distributed group whose ranks each hold their own sequences (points sharded,
    cameras replicated: the reduced camera system - (6C)^2 + 6C doubles - is all-reduced every iteration).
    ``return_cov=True``: info["cov"] = the covariance dict of ``covariance`` at the returned iterate (fp64, the same f_scale),
    with cov_points / std_points scattered back to [N, L, 3, 3] / [N, L] (NaN where a point was not kept); together with
    ``group`` it is a ValueError before any device work."""
    model = calib.camera_model_of(camera_model, precision=precision)
    n_cams = len(k_arr)
    if return_cov:
        _cov_options(n_cams, True, gauge, ref_cam, scale_cam, scale, group=group)
    intr, Rt = _camera_tables(k_arr, d_arr, r_arr, t_arr, model, True)
    _lib.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    det = calib._to_dev(det, dev)
    pts_all = calib._to_dev(points_3d, dev).to(torch.float64).contiguous().clone()
    if det.dim() != 4 or det.shape[1] != n_cams or tuple(pts_all.shape) != (det.shape[0], det.shape[2], 3):
        raise ValueError("det must be [N, C, L, 3] and points_3d [N, L, 3] for the C cameras of the rig")
    keep, uv, cam_idx, pt_start, pt_obs = dense_observations(det, float(dlc_thresh), min_views)
    if pt_start.numel() < 2:
        raise ValueError("no point is seen by enough cameras")
    p = _device_problem(intr, Rt, pts_all[keep].contiguous(), uv, cam_idx, pt_start, pt_obs, model, True, f_scale, lam0=lam0,
                        ftol=ftol, gtol=gtol, max_iter=max_iter, precision=precision)
    res_b, res_a, hook = _run_solve(p, group is not None, group)
    out = dict(last_info, n_points=p.n_points, n_obs=p.n_obs, precision=precision,
               rms_before=float(res_b.pow(2).mean().sqrt()), rms_after=float(res_a.pow(2).mean().sqrt()),
               reduce_calls=hook.calls if hook else 0, reduce_sizes=sorted(set(hook.sizes)) if hook else [])
    if return_cov:
        cov = _covariance_device(p, gauge, ref_cam, scale_cam, scale)
        keep_h = keep.cpu().numpy()
        for key, tail in (("cov_points", (3, 3)), ("std_points", ())):
            full = np.full(keep_h.shape + tail, np.nan)
            full[keep_h] = cov[key]
            cov[key] = full
        out["cov"] = cov
    pts_all[keep] = p.pts
    Rt_o = p.Rt.cpu().numpy()
    return pts_all, Rt_o[:, :9].reshape(n_cams, 3, 3).copy(), Rt_o[:, 9:].reshape(n_cams, 3, 1).copy(), out


def refine_extrinsics_from_clips(dets, k_arr, d_arr, r_arr, t_arr, Ts, dlc_thresh=0.5, precision="bf16", fte_iter=60,
                                 sba_iter=60, fte_kw=None, sba_kw=None, camera_model=None, return_cov=False, gauge="baseline",
                                 ref_cam=0, scale_cam=1, scale="residual"):
    """BASELINE config 5 end to end on one GPU: the clips' trajectories are estimated with the current rig (fte_solve_clips:
    all clips as one chain, ``precision`` = "bf16": bf16 residual / Jacobian rows, fp32 accumulation), then the marker
    positions of ALL clips and their above-threshold detections go through one bundle adjustment of points + the shared
    extrinsics in the same precision mode.  ``camera_model="pinhole"`` runs both stages on the OpenCV pinhole camera; that
    model is fp64 only, so it needs ``precision="f64"`` (bf16 with pinhole is a ValueError before any device work).
    Returns (r_arr, t_arr, info) with info = dict(fte=..., sba=...); ``return_cov=True`` adds info["cov"], the error bars of the
    refined extrinsics and points (``bundle_adjust_dense_points_and_extrinsics``)."""
    from . import fte
    calib.camera_model_of(camera_model, precision=precision)
    cov_kw = {}
    if return_cov:
        _cov_options(len(k_arr), True, gauge, ref_cam, scale_cam, scale, group=(sba_kw or {}).get("group"))
        cov_kw = dict(return_cov=True, gauge=gauge, ref_cam=ref_cam, scale_cam=scale_cam, scale=scale)
    cam_kw = {} if camera_model is None else dict(camera_model=camera_model)
    outs = fte.fte_solve_clips(dets, k_arr, d_arr, r_arr, t_arr, Ts, dlc_thresh=dlc_thresh, max_iter=fte_iter,
                               return_numpy=False, precision=precision, **cam_kw, **(fte_kw or {}))
    dev = torch.device("cuda", torch.cuda.current_device())
    pos = torch.cat([o[0]["positions"] for o in outs], 0)
    det_all = torch.cat([calib._to_dev(d, dev) for d in dets], 0)
    _pts, r_new, t_new, info = bundle_adjust_dense_points_and_extrinsics(det_all, pos, k_arr, d_arr, r_arr, t_arr, dlc_thresh,
                                                                         precision=precision, max_iter=sba_iter,
                                                                         **cam_kw, **(sba_kw or {}), **cov_kw)
    out = dict(fte=outs[0][1], sba=info)
    if return_cov:
        out["cov"] = info.pop("cov")
    return r_new, t_new, out
