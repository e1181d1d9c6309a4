"""Lens undistortion of frames that share one calibration (csrc/dd_undistort.hip): the definition on the host in numpy
and the launch.  Stands in for `cv2.undistort(img, K, dist)` of the reference's Waymo preparation (prepare_data/waymo.py:10-27) with
the new camera matrix equal to K.  `intrinsic` is Waymo's (f_u, f_v, c_u, c_v, k1, k2, p1, p2, k3); for destination pixel (u, v), in
float64, one rounding per operation, in this order:

  x = (u - c_u) / f_u,  y = (v - c_v) / f_v,  xx = x * x,  yy = y * y,  r2 = xx + yy
  k = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
  x_d = (x * k + ((2 * p1) * x) * y) + p2 * (r2 + 2 * xx)
  y_d = (y * k + p1 * (r2 + 2 * yy)) + ((2 * p2) * x) * y
  m_x = f_u * x_d + c_u,  m_y = f_v * y_d + c_v
  i_x = rint(m_x * 32), i_y = rint(m_y * 32), halves to even; a value outside [-2^30, 2^30] or a NaN reads as -2^30

then in integers: taps at (i_x >> 5, i_y >> 5) and its right, lower and lower-right neighbours with the weights (32 - a)(32 - b),
a (32 - b), (32 - a) b, a b for a = i_x & 31, b = i_y & 31; a tap outside the image counts as 0; dst = (sum + 512) >> 10."""
import ctypes

import numpy as np

FAR = -(1 << 30)


def source_grid(intrinsic, height, width):
    """(i_x, i_y) int64 (height, width): the source position of every destination pixel in 1/32 pixels, as defined above."""
    fu, fv, cu, cv, k1, k2, p1, p2, k3 = (np.float64(v) for v in np.asarray(intrinsic, dtype=np.float64).reshape(9))
    with np.errstate(all="ignore"):
        x = ((np.arange(width, dtype=np.float64) - cu) / fu)[None, :]
        y = ((np.arange(height, dtype=np.float64) - cv) / fv)[:, None]
        xx, yy = x * x, y * y
        r2 = xx + yy
        k = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2
        xd = (x * k + ((2.0 * p1) * x) * y) + p2 * (r2 + 2.0 * xx)
        yd = (y * k + p1 * (r2 + 2.0 * yy)) + ((2.0 * p2) * x) * y
        out = []
        for m in (fu * xd + cu, fv * yd + cv):
            t = np.rint(m * 32.0)
            near = (t >= float(FAR)) & (t <= float(-FAR))
            out.append(np.where(near, t, float(FAR)).astype(np.int64))
    return out[0], out[1]


def undistort_host(frames, intrinsic):
    """The definition of dd_undistort: frames (n, H, W, 3) uint8 -> the same shape."""
    frames = np.asarray(frames)
    if frames.ndim != 4 or frames.shape[-1] != 3 or frames.dtype != np.uint8:
        raise ValueError("undistort takes (n, H, W, 3) uint8 frames")
    n, H, W = frames.shape[:3]
    ix, iy = source_grid(intrinsic, H, W)
    sx, sy, a, b = ix >> 5, iy >> 5, ix & 31, iy & 31
    acc = np.full((n, H, W, 3), 512, dtype=np.int64)
    for dy, dx, wt in ((0, 0, (32 - a) * (32 - b)), (0, 1, a * (32 - b)), (1, 0, (32 - a) * b), (1, 1, a * b)):
        tx, ty = sx + dx, sy + dy
        inside = (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
        tap = frames[:, np.clip(ty, 0, H - 1), np.clip(tx, 0, W - 1)].astype(np.int64)
        acc += tap * np.where(inside, wt, 0)[None, :, :, None]
    return (acc >> 10).astype(np.uint8)


def undistort_batch(frames, intrinsic):
    """frames (n, H, W, 3) uint8 on the GPU -> `undistort_host` of them on the device, one launch on the current stream."""
    import torch

    from . import abi
    from . import lib as L
    if not (torch.is_tensor(frames) and frames.is_cuda and frames.dtype == torch.uint8 and frames.dim() == 4 and frames.shape[-1] == 3 and frames.shape[0] >= 1):
        raise L.DynamoHipError("undistort_batch takes (n, H, W, 3) uint8 frames on the GPU")
    cal = np.ascontiguousarray(np.asarray(intrinsic, dtype=np.float64).reshape(-1))
    if cal.size != 9:
        raise L.DynamoHipError("undistort_batch takes the 9 intrinsic values f_u, f_v, c_u, c_v, k1, k2, p1, p2, k3")
    frames = frames.contiguous()
    out = torch.empty_like(frames)
    L.check(L.load().dd_undistort(abi.ptr(frames), int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2]),
                                  cal.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), abi.ptr(out), L.current_stream()), "dd_undistort")
    return out
