"""KITTI LiDAR depth lists (csrc/dd_lidar.hip): the definition on the host in numpy, the projection matrix from the two
calibration files, and the batched launch.

Replaces `generate_depth_map(calib_dir, velo_file, cam, vel_depth=True)` followed by the `np.where(depth > 0)` stacking of the
reference's data preparation (prepare_data/kitti.py:104-115, kitti_util.py:46-98).  For one scan `points` (float32 (n, 4), column 3
ignored), one matrix `P` (float64 3x4) and an image H x W with W >= 2:

  kept      point i with x_i >= 0 (false for NaN, true for -0.0)
  project   in float64, unfused, left to right: a_k = ((P[k,0] x + P[k,1] y) + P[k,2] z) + P[k,3] for k = 0, 1, 2;
            u = a_0 / a_2, v = a_1 / a_2 (IEEE division); c = rint(u) - 1, r = rint(v) - 1, half to even, still in float64
  valid     c >= 0 and r >= 0 and c < W and r < H, compared in float64 (NaN, +-inf and huge values fall out); the depth d is x_i,
            the float32 value (-0.0 read as 0), not a_2
  map       map[r, c] = d of the valid point with the highest i at that pixel, 0 where there is none
  buckets   b = r (W - 1) + c - 1, the reference's sub2ind, quirk included: it runs from -1 (pixel (0, 0)) to H (W - 1) - 1, and pixels
            (r, W - 1) and (r + 1, 0) share a bucket.  In every bucket that holds two or more valid points (an exact duplicate counts
            as two) the pixel of the LOWEST-index point gets the minimum d over all points of the bucket; every other pixel of the
            bucket keeps its map value
  rows      the pixels with map > 0 in row-major order as float64 rows [r, c, d]

`i` counts the kept points in file order."""
import ctypes
import os

import numpy as np


def depth_points_host(points, P, H, W):
    """(rows float64 (n, 3), map float32 (H, W)) of the definition above, for one scan and one camera."""
    H, W = int(H), int(W)
    if H < 1 or W < 2:
        raise ValueError("depth_points_host needs H >= 1 and W >= 2")
    pts = np.asarray(points, dtype=np.float32).reshape(-1, 4)
    P = np.asarray(P, dtype=np.float64).reshape(3, 4)
    kept = pts[pts[:, 0] >= 0]
    x, y, z = (kept[:, k].astype(np.float64) for k in range(3))
    with np.errstate(all="ignore"):
        a = [((P[k, 0] * x + P[k, 1] * y) + P[k, 2] * z) + P[k, 3] for k in range(3)]
        c, r = np.rint(a[0] / a[2]) - 1.0, np.rint(a[1] / a[2]) - 1.0
        valid = (c >= 0) & (r >= 0) & (c < W) & (r < H)
    c, r = c[valid].astype(np.int64), r[valid].astype(np.int64)
    d = kept[valid, 0]
    d = np.where(d == 0, np.float32(0), d)
    n = d.size
    index = np.arange(n, dtype=np.int64)
    depth = np.zeros(H * W, dtype=np.float32)
    last = np.full(H * W, -1, dtype=np.int64)
    np.maximum.at(last, r * W + c, index)
    hit = last >= 0
    depth[hit] = d[last[hit]]
    q = r * (W - 1) + c                                                     # bucket + 1
    nb = H * (W - 1) + 1
    first = np.full(nb, n, dtype=np.int64)
    np.minimum.at(first, q, index)
    nearest = np.full(nb, np.inf, dtype=np.float32)
    np.minimum.at(nearest, q, d)
    crowded = np.nonzero(np.bincount(q, minlength=nb) >= 2)[0]
    f = first[crowded]
    depth[r[f] * W + c[f]] = nearest[crowded]
    depth = depth.reshape(H, W)
    rr, cc = np.nonzero(depth > 0)
    rows = np.stack([rr.astype(np.float64), cc.astype(np.float64), depth[rr, cc].astype(np.float64)], axis=1)
    return rows, depth


def read_calib(path):
    """{key: float64 array} of a KITTI calibration file's `key: value` lines; values that are not numbers (calib_time) are skipped."""
    out = {}
    with open(path, "r") as fh:
        for line in fh:
            if ":" not in line:
                continue
            key, value = line.split(":", 1)
            try:
                out[key] = np.array([float(t) for t in value.split()], dtype=np.float64)
            except ValueError:
                pass
    return out


def projection(calib_dir, cam):
    """(P float64 (3, 4), H, W): velodyne -> pixel matrix of camera `cam` (2 or 3) from calib_cam_to_cam.txt and calib_velo_to_cam.txt,
    and the image size, the date's S_rect_02 for both cameras as in the reference."""
    cam2cam = read_calib(os.path.join(calib_dir, "calib_cam_to_cam.txt"))
    velo2cam = read_calib(os.path.join(calib_dir, "calib_velo_to_cam.txt"))
    T4 = np.hstack((velo2cam["R"].reshape(3, 3), velo2cam["T"][..., np.newaxis]))
    T4 = np.vstack((T4, np.array([0, 0, 0, 1.0])))
    W, H = cam2cam["S_rect_02"].astype(np.int32)
    R4 = np.eye(4)
    R4[:3, :3] = cam2cam["R_rect_00"].reshape(3, 3)
    P_rect = cam2cam["P_rect_0" + str(int(cam))].reshape(3, 4)
    return np.dot(np.dot(P_rect, R4), T4), int(H), int(W)


def depth_points(points, offsets, P, H, W, return_maps=False):
    """points (n_total, 4) float32 and P (C, 3, 4) float64 on the GPU, offsets the S + 1 scan boundaries (a host sequence: they are
    checked before the launch, so that the call never waits for the device) -> (rows, counts[, maps]): rows (C * n_total, 3) float64
    and counts (S, C) int32 on the GPU, laid out as include/dynamo_hip.h documents (`split_rows` cuts them up), and with
    return_maps the dense (S, C, H, W) float32 maps.  One call on the current stream, no host sync."""
    import torch

    from . import abi
    from . import lib as L
    if not (torch.is_tensor(points) and points.is_cuda and points.dtype == torch.float32 and points.dim() == 2 and points.shape[1] == 4):
        raise L.DynamoHipError("depth_points takes (n_total, 4) float32 points on the GPU")
    if not (torch.is_tensor(P) and P.is_cuda and P.dtype == torch.float64 and P.dim() == 3 and tuple(P.shape[1:]) == (3, 4)):
        raise L.DynamoHipError("depth_points takes (C, 3, 4) float64 matrices on the GPU")
    if torch.is_tensor(offsets) and offsets.is_cuda:
        raise L.DynamoHipError("depth_points takes the scan offsets on the host")
    off = np.ascontiguousarray(np.asarray(offsets, dtype=np.int64).reshape(-1))
    n_total, S, C = int(points.shape[0]), off.size - 1, int(P.shape[0])
    if S < 1 or off.min() < 0 or off.max() > 2 ** 31 - 1:
        raise L.DynamoHipError("depth_points: offsets must hold S + 1 >= 2 row numbers")
    off = off.astype(np.int32)
    lib = L.load()
    points, P = points.contiguous(), P.contiguous()
    dev = points.device
    src = points if n_total > 0 else torch.zeros((1, 4), dtype=torch.float32, device=dev)
    rows = torch.empty((max(C * n_total, 1), 3), dtype=torch.float64, device=dev)
    counts = torch.empty((S, C), dtype=torch.int32, device=dev)
    maps = torch.empty((S, C, H, W), dtype=torch.float32, device=dev) if return_maps else None
    need = int(lib.dd_lidar_depth_points_workspace_bytes(S, C, H, W))
    work = torch.empty(max(need, 4), dtype=torch.uint8, device=dev)
    L.check(lib.dd_lidar_depth_points(abi.ptr(src), n_total, off.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), S, abi.ptr(P), C, H, W, abi.ptr(counts),
                                      abi.ptr(rows), abi.ptr(maps), abi.ptr(work), need, L.current_stream()), "dd_lidar_depth_points")
    rows = rows[:C * n_total]
    return (rows, counts, maps) if return_maps else (rows, counts)


def split_rows(rows, counts, offsets):
    """The per-job arrays of one `depth_points` call: out[s][c] = float64 (counts[s, c], 3).  The two copies to the host are the only
    synchronisation."""
    off = np.asarray(offsets, dtype=np.int64).reshape(-1)
    S, C = int(counts.shape[0]), int(counts.shape[1])
    host, cnt = rows.cpu().numpy(), counts.cpu().numpy()
    out = []
    for s in range(S):
        n = int(off[s + 1] - off[s])
        out.append([host[C * off[s] + c * n:C * off[s] + c * n + int(cnt[s, c])].copy() for c in range(C)])
    return out
