"""Numpy reference of the EKF + RTS smoother on the OpenCV pinhole camera (cv2.projectPoints: k1 k2 p1 p2 k3 k4 k5 k6
s1 s2 s3 s4).

``ekf`` is oracle.ekf.ekf with its measurement function ``h_function`` swapped, for the duration of the call, for the
projection of the 20 FK markers through oracle.camera.project_points - the restatement of cv2.projectPoints the pinhole
model is pinned to.  Everything else (model matrices, float32 prediction, forward-difference Jacobian, gate, gain,
smoother) is the oracle's.  No cut behind the camera, as the fisheye measurement function.
"""
import contextlib

from oracle import camera as ocam
from oracle import ekf as oekf


def h_pinhole(pose25, k, d, r, t):
    """The measurement function on a pinhole camera: pixel coordinates [20, 2] of the markers of ``pose25``."""
    return ocam.project_points(oekf.marker_coords(pose25), k, d, r, t)


@contextlib.contextmanager
def _pinhole_measurement():
    saved = oekf.h_function
    oekf.h_function = h_pinhole
    try:
        yield
    finally:
        oekf.h_function = saved


def ekf(det, k_arr, d_arr, r_arr, t_arr, fps, dlc_thresh, cam_width, states0, **kw):
    """oracle.ekf.ekf on pinhole cameras: d_arr[C] are OpenCV distortion vectors (4, 5, 8 or 12 entries)."""
    with _pinhole_measurement():
        return oekf.ekf(det, k_arr, d_arr, r_arr, t_arr, fps, dlc_thresh, cam_width, states0, **kw)
