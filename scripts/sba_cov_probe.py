"""Time of the bundle-adjustment covariance (acino_sba_covariance) at BASELINE config 5's size - 64 x 1 000 frames: 1.28 M
points, 6.5 M observations, six shared extrinsics - beside ONE Levenberg-Marquardt iteration of the existing solve
(acino_sba_solve, max_iter = 1, fp64) on the same data, both through the C ABI on device-resident inputs.  The iterate is
the one a 10-iteration refinement returns.  HIP events, median of 5 blocks of 3 calls after 2 warm-up calls.  The point
kernel's own time is the difference between the call with and without the point outputs; its flop count is computed from
the view counts (per point with k views: 108 k for Y, 216 k^2 for Z = Sigma Y^T, 72 k for Y^T Z).  Prints one JSON line."""
import ctypes as C
import json
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from acinoset_amd import _lib, calib, sba, synth
from acinoset_amd._lib import SbaCovInfo, SbaInfo, SbaParams, lib, ptr, stream_ptr


def median_ms(fn, warm=2, reps=5, inner=3):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / inner)
    return float(np.median(out)), float(np.min(out)), float(np.max(out))


def main(n_clips=64, n_frames=1000):
    dev = torch.device("cuda")
    seq = synth.make_sequence(n_frames, "trot")
    K, D, R, t = seq["K"], seq["D"], seq["R"], seq["t"]
    n_cams = len(K)
    det = torch.as_tensor(seq["det"], device=dev).repeat(n_clips, 1, 1, 1)
    gen = torch.Generator(device="cuda").manual_seed(3)
    pos = torch.as_tensor(seq["pos_true"], device=dev).repeat(n_clips, 1, 1)
    pos = pos + 0.005 * torch.randn(pos.shape, dtype=torch.float64, device=dev, generator=gen)
    rng = np.random.default_rng(7)
    Rp = np.array([calib._rodrigues(rng.normal(0, 1, 3) / np.sqrt(3) * np.radians(0.5)) @ R[c] for c in range(n_cams)])
    tp = np.asarray(t, dtype=np.float64).reshape(-1, 3, 1) + rng.normal(0, 1, (n_cams, 3, 1)) / np.sqrt(3) * 1e-2
    pts, r_new, t_new, info = sba.bundle_adjust_dense_points_and_extrinsics(det, pos, K, D, Rp, tp, 0.5, max_iter=10)
    keep, uv, cam_idx, pt_start, pt_obs = sba.dense_observations(det, 0.5)
    intr, Rt = sba._camera_tables(K, D, r_new, t_new, "fisheye", True)
    d_intr, d_Rt = torch.as_tensor(intr, device=dev), torch.as_tensor(Rt, device=dev)
    d_pts = pts[keep].contiguous()
    P, M = int(d_pts.shape[0]), int(uv.shape[0])
    prm = SbaParams(n_cams=n_cams, optimize_cameras=1, n_points=P, n_obs=M, f_scale=1.0, lam0=1e-3, ftol=0.0, gtol=0.0,
                    max_iter=1, camera_model=0, precision=0)

    def workspace(nbytes):
        ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=dev)
        return ws, C.c_void_p((ws.data_ptr() + 255) // 256 * 256), nbytes

    ws_s, ws_s_ptr, nb_s = workspace(lib().acino_sba_workspace_bytes(n_cams, P, M))
    ws_c, ws_c_ptr, nb_c = workspace(lib().acino_sba_covariance_workspace_bytes(n_cams, P, M))
    Rt_w, pts_w = d_Rt.clone(), d_pts.clone()
    sinfo, cinfo = SbaInfo(), SbaCovInfo()

    def lm_iteration():
        Rt_w.copy_(d_Rt)
        pts_w.copy_(d_pts)
        _lib.check(lib().acino_sba_solve(C.byref(prm), ptr(d_intr), ptr(Rt_w), ptr(pts_w), ptr(uv), ptr(cam_idx), ptr(pt_start),
                                         ptr(pt_obs), ws_s_ptr, nb_s, None, None, C.byref(sinfo), stream_ptr()))

    cov_cams = torch.empty((6 * n_cams, 6 * n_cams), dtype=torch.float64, device=dev)
    cov_pts = torch.empty((P, 6), dtype=torch.float64, device=dev)
    std_pts = torch.empty(P, dtype=torch.float64, device=dev)

    def covariance(points):
        _lib.check(lib().acino_sba_covariance(C.byref(prm), ptr(d_intr), ptr(d_Rt), ptr(d_pts), ptr(uv), ptr(cam_idx),
                                              ptr(pt_start), ptr(pt_obs), 0, 0, 1, None, 0, ws_c_ptr, nb_c, ptr(cov_cams),
                                              ptr(cov_pts) if points else None, ptr(std_pts) if points else None,
                                              C.byref(cinfo), stream_ptr()))

    lm = median_ms(lm_iteration)
    cov = median_ms(lambda: covariance(True))
    cams = median_ms(lambda: covariance(False))
    k = (pt_start[1:] - pt_start[:-1]).to(torch.float64)
    flop = float((108 * k + 216 * k * k + 72 * k).sum())
    kernel_ms = cov[0] - cams[0]
    peak = 78.6e12                                     # fp64 vector peak of the MI355X, flop / s
    covariance(True)
    first = cov_cams.clone()
    covariance(True)
    out = dict(probe="sba_covariance", device=torch.cuda.get_device_name(0), n_points=P, n_obs=M, n_cams=n_cams,
               lm_iteration_ms=round(lm[0], 3), lm_iteration_min_max_ms=[round(lm[1], 3), round(lm[2], 3)],
               covariance_ms=round(cov[0], 3), covariance_min_max_ms=[round(cov[1], 3), round(cov[2], 3)],
               covariance_without_points_ms=round(cams[0], 3), point_kernel_ms=round(kernel_ms, 3),
               point_kernel_gflop=round(flop / 1e9, 2), point_kernel_tflops=round(flop / (kernel_ms * 1e-3) / 1e12, 2),
               point_kernel_share_of_fp64_vector_peak=round(flop / (kernel_ms * 1e-3) / peak, 3),
               workspace_mb=round(nb_c / 2 ** 20, 1), sigma2=cinfo.sigma2, dof=int(cinfo.dof),
               n_points_excluded=int(cinfo.n_points_excluded), min_pivot_ratio=cinfo.min_pivot_ratio,
               std_rot_deg=[float(np.degrees(np.sqrt(max(float(cov_cams[6 * c:6 * c + 3, 6 * c:6 * c + 3].trace()), 0.0))))
                            for c in range(n_cams)],
               std_points_median_m=float(std_pts.median()), repeat_bit_identical=bool(torch.equal(first, cov_cams)),
               solve=dict(iterations=info["iterations"], rms_after=info["rms_after"]))
    print(json.dumps(out))


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:3]))
