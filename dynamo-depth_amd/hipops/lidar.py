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

`i` counts the kept points in file order.

Below the KITTI part: the nuScenes preparation's pose chain (`pose_points_host`, `pose_points`; csrc/dd_lidar.hip dd_lidar_pose_points) and
the key frames' box fit (`box_fit_host`, `box_fit`, `motion_labels`; dd_box_fit), DESIGN 4.22, with pyquaternion's rotation matrix and the
devkit's box corners written out.  Last the Waymo preparation's range images (`range_image_points_host`, `range_image_points`;
csrc/dd_range_image.hip) and upright box corners, DESIGN 4.23."""
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


POSE_STRIDE = 64        # doubles per scan of dd_lidar_pose_points' params
BOX_STRIDE = 16         # doubles per box of dd_box_fit


def quaternion_matrix(q):
    """float64 (3, 3) rotation matrix of the quaternion (w, x, y, z), normalised first: pyquaternion's `Quaternion(q).rotation_matrix`
    written out (the lower-right block of its left and conjugate-right product matrices)."""
    q = np.asarray(q, dtype=np.float64).reshape(4)
    norm = np.sqrt(np.dot(q, q))
    if norm > 0:
        q = q / norm
    w, x, y, z = q
    return np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]], dtype=np.float64)


def transform_matrix(translation, rotation):
    """The devkit's transform_matrix(translation, Quaternion(rotation)): float64 (4, 4)."""
    T = np.eye(4)
    T[:3, :3] = quaternion_matrix(rotation)
    T[:3, 3] = np.asarray(translation, dtype=np.float64)
    return T


def pose_params(lidar_cs, lidar_pose, cam_pose, cam_cs, K, W, H):
    """The POSE_STRIDE doubles of one scan from four records with `rotation` (w, x, y, z) and `translation`, the 3x3 intrinsics and
    the image size: the matrices as reference nuScenes.py:161-180 applies them (the last two transposed)."""
    out = np.zeros(POSE_STRIDE, dtype=np.float64)
    out[0:9] = quaternion_matrix(lidar_cs["rotation"]).reshape(-1)
    out[9:12] = lidar_cs["translation"]
    out[12:21] = quaternion_matrix(lidar_pose["rotation"]).reshape(-1)
    out[21:24] = lidar_pose["translation"]
    out[24:27] = cam_pose["translation"]
    out[27:36] = quaternion_matrix(cam_pose["rotation"]).T.reshape(-1)
    out[36:39] = cam_cs["translation"]
    out[39:48] = quaternion_matrix(cam_cs["rotation"]).T.reshape(-1)
    out[48:57] = np.asarray(K, dtype=np.float64).reshape(-1)
    out[57], out[58] = W, H
    return out


def _rotate(R, p):
    R = R.reshape(3, 3)
    return [(R[k, 0] * p[0] + R[k, 1] * p[1]) + R[k, 2] * p[2] for k in range(3)]


def pose_points_host(points, params):
    """The definition of dd_lidar_pose_points for one scan: points float32 (n, >= 3), params from `pose_params` -> (rows float64
    (m, 6) [u, v, depth, gx, gy, gz] of the kept points in scan order, all float64 (n, 6), kept bool (n,)).  float64 from the first
    step on, every dot product summed left to right: the devkit keeps its cloud in float32 between the steps, which is not
    reproduced."""
    q = np.asarray(params, dtype=np.float64).reshape(POSE_STRIDE)
    pts = np.asarray(points, dtype=np.float32)
    p = [pts[:, k].astype(np.float64) for k in range(3)]
    with np.errstate(all="ignore"):
        p = [c + t for c, t in zip(_rotate(q[0:9], p), q[9:12])]
        p = [c + t for c, t in zip(_rotate(q[12:21], p), q[21:24])]
        g = p
        p = _rotate(q[27:36], [c - t for c, t in zip(p, q[24:27])])
        p = _rotate(q[39:48], [c - t for c, t in zip(p, q[36:39])])
        depth = p[2]
        a = _rotate(q[48:57], p)
        u, v = a[0] / a[2], a[1] / a[2]
        kept = (depth > 1.0) & (u > 1.0) & (u < q[57] - 1.0) & (v > 1.0) & (v < q[58] - 1.0)
    full = np.stack([u, v, depth, g[0], g[1], g[2]], axis=1)
    return full[kept], full, kept


def pose_points(points, offsets, params):
    """points (n_total, 4) float32 and params (S, POSE_STRIDE) float64 on the GPU, offsets the S + 1 scan boundaries on the host ->
    (rows (n_total, 6) float64, counts (S, 1) int32) on the GPU, laid out for `split_rows`.  One call on the current stream."""
    import torch

    from . import abi
    from . import lib as L
    if not (torch.is_tensor(points) and points.is_cuda and points.dtype == torch.float32 and points.dim() == 2 and points.shape[1] == 4):
        raise L.DynamoHipError("pose_points takes (n_total, 4) float32 points on the GPU")
    if not (torch.is_tensor(params) and params.is_cuda and params.dtype == torch.float64 and params.dim() == 2 and params.shape[1] == POSE_STRIDE):
        raise L.DynamoHipError("pose_points takes (S, {}) float64 parameters on the GPU".format(POSE_STRIDE))
    off = np.ascontiguousarray(np.asarray(offsets, dtype=np.int64).reshape(-1))
    n_total, S = int(points.shape[0]), off.size - 1
    if S < 1 or S != int(params.shape[0]) or off.min() < 0 or off.max() > 2 ** 31 - 1:
        raise L.DynamoHipError("pose_points: offsets must hold S + 1 >= 2 row numbers, one parameter row per scan")
    longest = int(np.diff(off).max())
    off = off.astype(np.int32)
    lib = L.load()
    points, params = points.contiguous(), params.contiguous()
    dev = points.device
    src = points if n_total > 0 else torch.zeros((1, 4), dtype=torch.float32, device=dev)
    rows = torch.empty((max(n_total, 1), 6), dtype=torch.float64, device=dev)
    counts = torch.empty((S, 1), dtype=torch.int32, device=dev)
    need = int(lib.dd_lidar_pose_points_workspace_bytes(S, max(longest, 0)))
    work = torch.empty(max(need, 4), dtype=torch.uint8, device=dev)
    L.check(lib.dd_lidar_pose_points(abi.ptr(src), n_total, off.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), S, abi.ptr(params), abi.ptr(counts),
                                     abi.ptr(rows), abi.ptr(work), need, L.current_stream()), "dd_lidar_pose_points")
    return rows[:n_total], counts


def box_corners(center, wlh, rotation):
    """float64 (8, 3): the corners of an annotation box in the devkit's `Box.corners()` order (x forward, y left, z up; the first
    four have x > 0), transposed as the reference uses them."""
    w, l, h = (float(v) for v in wlh)
    x = l / 2 * np.array([1, 1, 1, 1, -1, -1, -1, -1], dtype=np.float64)
    y = w / 2 * np.array([1, -1, -1, 1, 1, -1, -1, 1], dtype=np.float64)
    z = h / 2 * np.array([1, 1, -1, -1, 1, 1, -1, -1], dtype=np.float64)
    corners = np.dot(quaternion_matrix(rotation), np.vstack((x, y, z)))
    return (corners + np.asarray(center, dtype=np.float64).reshape(3, 1)).T


def box_params(corners):
    """(B, 8, 3) corners -> (B, BOX_STRIDE) float64: p1, i = p2 - p1, j = p4 - p1, k = p5 - p1, i.i, j.j, k.k (sums left to right)."""
    c = np.asarray(corners, dtype=np.float64).reshape(-1, 8, 3)
    out = np.zeros((c.shape[0], BOX_STRIDE), dtype=np.float64)
    out[:, 0:3] = c[:, 0]
    for n, corner in enumerate((1, 3, 4)):
        e = c[:, corner] - c[:, 0]
        out[:, 3 + 3 * n:6 + 3 * n] = e
        out[:, 12 + n] = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
    return out


def box_fit_host(points, seg, label_cat, boxes, box_cat):
    """The definition of dd_box_fit: points float64 (n, 3) with label l at rows seg[l] .. seg[l + 1] - 1, boxes from `box_params` ->
    (counts int32 (L, B), -1 where the categories differ; best int32 (L, 2) [first box with the strictly greatest count or -1, count])."""
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    seg = np.asarray(seg, dtype=np.int64).reshape(-1)
    boxes = np.asarray(boxes, dtype=np.float64).reshape(-1, BOX_STRIDE)
    L, B = seg.size - 1, boxes.shape[0]
    counts = np.full((L, B), -1, dtype=np.int32)
    best = np.zeros((L, 2), dtype=np.int32)
    best[:, 0] = -1
    for l in range(L):
        p = pts[seg[l]:seg[l + 1]]
        for b in range(B):
            if int(box_cat[b]) != int(label_cat[l]):
                continue
            q = boxes[b]
            d = [p[:, k] - q[k] for k in range(3)]
            dots = [(d[0] * q[3 + 3 * n] + d[1] * q[4 + 3 * n]) + d[2] * q[5 + 3 * n] for n in range(3)]
            inside = np.ones(p.shape[0], dtype=bool)
            for n in range(3):
                inside &= (0.0 < dots[n]) & (dots[n] < q[12 + n])
            counts[l, b] = int(inside.sum())
            if counts[l, b] > best[l, 1]:
                best[l] = (b, counts[l, b])
    return counts, best


def box_fit(points, seg, label_cat, boxes, box_cat):
    """`box_fit_host` on the device from host arrays, one launch: (counts (L, B), best (L, 2)) as int32 numpy arrays."""
    import torch

    from . import abi
    from . import lib as L_
    pts = np.ascontiguousarray(np.asarray(points, dtype=np.float64).reshape(-1, 3))
    seg = np.ascontiguousarray(np.asarray(seg, dtype=np.int32).reshape(-1))
    boxes = np.ascontiguousarray(np.asarray(boxes, dtype=np.float64).reshape(-1, BOX_STRIDE))
    n_labels, B = seg.size - 1, boxes.shape[0]
    if n_labels < 0 or len(label_cat) != n_labels or len(box_cat) != B or (n_labels and (seg[0] != 0 or seg[-1] != pts.shape[0] or (np.diff(seg) < 0).any())):
        raise L_.DynamoHipError("box_fit: seg must run from 0 to the number of points, one category per label and per box")
    counts = torch.full((max(n_labels * B, 1),), -1, dtype=torch.int32, device="cuda")
    best = torch.zeros((max(n_labels, 1), 2), dtype=torch.int32, device="cuda")
    if n_labels:
        def up(a, dtype, fill):
            a = np.ascontiguousarray(np.asarray(a, dtype=dtype))
            return torch.from_numpy(a if a.size else np.full(fill, 0, dtype=dtype)).cuda()
        d_pts, d_boxes = up(pts, np.float64, (1, 3)), up(boxes, np.float64, (1, BOX_STRIDE))
        d_seg, d_lc, d_bc = up(seg, np.int32, 2), up(np.asarray(label_cat).reshape(-1), np.int32, 1), up(np.asarray(box_cat).reshape(-1), np.int32, 1)
        L_.check(L_.load().dd_box_fit(abi.ptr(d_pts), pts.shape[0], abi.ptr(d_seg), abi.ptr(d_lc), n_labels, abi.ptr(d_boxes), abi.ptr(d_bc), B,
                                      abi.ptr(counts), abi.ptr(best), L_.current_stream()), "dd_box_fit")
    return counts[:n_labels * B].cpu().numpy().reshape(n_labels, B), best[:n_labels].cpu().numpy()


def motion_labels(panoptic, points, boxes, movable_cats, fit=box_fit_host):
    """Reference nuScenes.py:218-243 for one key frame.  panoptic uint16 (n,) labels (category * 1000 + instance) and points float64
    (n, 3) of the kept points; boxes a list of (token, category index, corners (8, 3), moving bool) in the annotations' order ->
    (motion_label uint8 (n,): 0 not movable, 1 in motion, 2 static movable, 3 no box found; panoptic2ann {label: {token, fit}})."""
    panoptic = np.asarray(panoptic)
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    motion = np.full(panoptic.shape, 3, dtype=np.uint8)
    uniq = np.unique(panoptic)
    movable = [u for u in uniq if int(u) // 1000 in movable_cats]
    for u in uniq:
        if int(u) // 1000 not in movable_cats:
            motion[panoptic == u] = 0
    panoptic2ann = {}
    if movable:
        index = [np.nonzero(panoptic == u)[0] for u in movable]
        seg = np.concatenate([[0], np.cumsum([i.size for i in index])]).astype(np.int32)
        corners = np.array([b[2] for b in boxes], dtype=np.float64).reshape(-1, 8, 3)
        _, best = fit(points[np.concatenate(index)], seg, [int(u) // 1000 for u in movable], box_params(corners), [int(b[1]) for b in boxes])
        for l, u in enumerate(movable):
            b, count = int(best[l][0]), int(best[l][1])
            if b < 0:
                panoptic2ann[u] = {"token": None, "fit": 0}
                continue
            motion[index[l]] = 1 if boxes[b][3] else 2
            panoptic2ann[u] = {"token": boxes[b][0], "fit": np.float64(count) / np.float64(index[l].size)}
    return motion, panoptic2ann


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


RI_STRIDE = 64          # doubles per image of dd_range_image_points' params
AXIS_SWAP = np.array([[0, 0, 1, 0], [-1, 0, 0, 0], [0, -1, 0, 0], [0, 0, 0, 1]], dtype=np.float64)     # (x front, y left, z up) -> (x right, y down, z front)


def inclination_table(height, beam_inclinations, inclination_min, inclination_max):
    """float64 (height,) inclination of every row of a range image: the calibration's list where it has one, else uniform between the
    two bounds, (0.5 + i) / height * (max - min) + min; reversed, so that row 0 looks up."""
    height = int(height)
    if len(beam_inclinations):
        table = np.asarray(beam_inclinations, dtype=np.float64).reshape(-1)
        if table.size != height:
            raise ValueError("{} beam inclinations for a range image of {} rows".format(table.size, height))
    else:
        table = (0.5 + np.arange(height, dtype=np.float64)) / height * (float(inclination_max) - float(inclination_min)) + float(inclination_min)
    return np.ascontiguousarray(table[::-1])


def range_image_trig(inclinations, width, extrinsic):
    """float64 (2 H + 2 W,): cos incl, sin incl per row, then cos az, sin az per column with
    az = ((W - c - 0.5) / W * 2 - 1) * pi - atan2(E[1][0], E[0][0]).  The host and the device both read these values."""
    incl = np.asarray(inclinations, dtype=np.float64).reshape(-1)
    E = np.asarray(extrinsic, dtype=np.float64).reshape(4, 4)
    W = int(width)
    az = ((W - np.arange(W, dtype=np.float64) - 0.5) / W * 2.0 - 1.0) * np.pi - np.arctan2(E[1, 0], E[0, 0])
    return np.concatenate([np.cos(incl), np.sin(incl), np.cos(az), np.sin(az)])


def vehicle_to_camera(cam_extrinsic):
    """inv(extrinsic @ axis_swap) of reference waymo.py:216-220, float64 (4, 4)."""
    return np.linalg.inv(np.asarray(cam_extrinsic, dtype=np.float64).reshape(4, 4) @ AXIS_SWAP)


def range_image_params(extrinsic, frame_pose, e2c, K, width, height):
    """The RI_STRIDE doubles of one image: the laser's extrinsic, the inverse of the frame pose (inverted here in float64; None for
    an image without a per-pixel pose), the vehicle-to-camera matrix, the 3x3 intrinsics and the image size."""
    out = np.zeros(RI_STRIDE, dtype=np.float64)
    E = np.asarray(extrinsic, dtype=np.float64).reshape(4, 4)
    out[0:9], out[9:12] = E[:3, :3].reshape(-1), E[:3, 3]
    F = np.eye(4) if frame_pose is None else np.linalg.inv(np.asarray(frame_pose, dtype=np.float64).reshape(4, 4))
    out[13:22], out[22:25] = F[:3, :3].reshape(-1), F[:3, 3]
    C = np.asarray(e2c, dtype=np.float64).reshape(4, 4)
    out[25:34], out[34:37] = C[:3, :3].reshape(-1), C[:3, 3]
    out[37:46] = np.asarray(K, dtype=np.float64).reshape(-1)
    out[46], out[47] = width, height
    return out


def range_image_points_host(ranges, cps, poses, trigs, params):
    """The definition of dd_range_image_points.  Per image s: ranges[s] (H, W) float32, cps[s] (H, W, >= 3) int32, poses[s] (H, W, 6)
    float32 (roll, pitch, yaw, x, y, z) or None, trigs[s] from `range_image_trig`, params[s] from `range_image_params` -> a list of
    (points float64 (n, 3), cp int32 (n, 3), rows float64 (m, 3) [u, v, depth]) and counts int32 (S, 2): the valid pixels (range > 0)
    and of those the ones the camera keeps, both in row-major order.  float64, every dot product summed left to right; the
    library's float32 point is not reproduced."""
    out, counts = [], np.zeros((len(ranges), 2), dtype=np.int32)
    for s, (rng, cp, pose, trig) in enumerate(zip(ranges, cps, poses, trigs)):
        q = np.asarray(params[s], dtype=np.float64).reshape(RI_STRIDE)
        rng = np.asarray(rng, dtype=np.float32)
        H, W = rng.shape
        t = np.asarray(trig, dtype=np.float64).reshape(2 * H + 2 * W)
        ci, si, ca, sa = t[:H, None], t[H:2 * H, None], t[None, 2 * H:2 * H + W], t[None, 2 * H + W:]
        rho = rng.astype(np.float64)
        with np.errstate(all="ignore"):
            p = [(ca * ci) * rho, (sa * ci) * rho, si * rho]
            p = [c + k for c, k in zip(_rotate(q[0:9], p), q[9:12])]
            if pose is not None:
                e = [np.asarray(pose, dtype=np.float32)[:, :, k].astype(np.float64) for k in range(6)]
                cr, sr, cq, sq, cy, sy = np.cos(e[0]), np.sin(e[0]), np.cos(e[1]), np.sin(e[1]), np.cos(e[2]), np.sin(e[2])
                R = [cy * cq, (cy * sq) * sr - sy * cr, (cy * sq) * cr + sy * sr,
                     sy * cq, (sy * sq) * sr + cy * cr, (sy * sq) * cr - cy * sr,
                     -sq, cq * sr, cq * cr]
                p = [(R[3 * k] * p[0] + R[3 * k + 1] * p[1]) + R[3 * k + 2] * p[2] + e[3 + k] for k in range(3)]
                p = [c + k for c, k in zip(_rotate(q[13:22], p), q[22:25])]
            valid = rng > 0
            c = [c + k for c, k in zip(_rotate(q[25:34], p), q[34:37])]
            a = _rotate(q[37:46], c)
            u, v = a[0] / a[2], a[1] / a[2]
            keep = valid & (a[2] > 0) & (u >= 0) & (u < q[46]) & (v >= 0) & (v < q[47])
        points = np.stack([c[valid] for c in p], axis=1)
        rows = np.stack([u[keep], v[keep], a[2][keep]], axis=1)
        out.append((points, np.ascontiguousarray(np.asarray(cp)[:, :, :3][valid], dtype=np.int32), rows))
        counts[s] = (points.shape[0], rows.shape[0])
    return out, counts


def range_image_pack(ranges, cps, poses, trigs):
    """The flat host arrays of one dd_range_image_points call: (range float32 [n], cp int32 (n, 3), pose float32 (n_pose, 6), trig
    float64 [n_trig], desc int32 (S, 5))."""
    desc = np.zeros((len(ranges), 5), dtype=np.int32)
    pix = n_pose = n_trig = 0
    for s, (rng, pose, trig) in enumerate(zip(ranges, poses, trigs)):
        H, W = np.shape(rng)
        desc[s] = (pix, H, W, n_pose if pose is not None else -1, n_trig)
        pix, n_trig = pix + H * W, n_trig + len(trig)
        n_pose += H * W if pose is not None else 0
    flat_pose = [np.asarray(p, dtype=np.float32).reshape(-1, 6) for p in poses if p is not None]
    return (np.concatenate([np.asarray(r, dtype=np.float32).reshape(-1) for r in ranges]),
            np.concatenate([np.asarray(c)[:, :, :3].reshape(-1, 3) for c in cps]).astype(np.int32, copy=False),
            np.concatenate(flat_pose) if flat_pose else np.zeros((0, 6), dtype=np.float32),
            np.concatenate([np.asarray(t, dtype=np.float64).reshape(-1) for t in trigs]), desc)


def range_image_points_device(rng, cp, pose, trig, desc, params):
    """One dd_range_image_points call on the current stream, no host sync: rng [n] float32, cp (n, 3) int32, pose (n_pose, 6) float32,
    trig [n_trig] float64 and params (S, RI_STRIDE) float64 on the GPU, desc (S, 5) int32 on the host (`range_image_pack`) ->
    (points (n, 3) float64, cp_out (n, 3) int32, rows (n, 3) float64, counts (S, 2) int32) on the GPU, image s in the rows from
    desc[s, 0] on."""
    import torch

    from . import abi
    from . import lib as L
    ok = (torch.is_tensor(t) and t.is_cuda and t.dtype == d and t.dim() == n for t, d, n in
          ((rng, torch.float32, 1), (cp, torch.int32, 2), (pose, torch.float32, 2), (trig, torch.float64, 1), (params, torch.float64, 2)))
    if not all(ok) or cp.shape[1] != 3 or pose.shape[1] != 6 or params.shape[1] != RI_STRIDE or cp.shape[0] != rng.shape[0]:
        raise L.DynamoHipError("range_image_points takes float32 ranges, (n, 3) int32 projections, (n_pose, 6) float32 poses, float64 tables and "
                               "(S, {}) float64 parameters on the GPU".format(RI_STRIDE))
    desc = np.ascontiguousarray(np.asarray(desc, dtype=np.int32).reshape(-1, 5))
    S, n = desc.shape[0], int(rng.shape[0])
    if S < 1 or S != int(params.shape[0]) or n < 1:
        raise L.DynamoHipError("range_image_points: one descriptor and one parameter row per image, at least one pixel")
    lib = L.load()
    rng, cp, pose, trig, params = (t.contiguous() for t in (rng, cp, pose, trig, params))
    dev = rng.device
    points = torch.empty((n, 3), dtype=torch.float64, device=dev)
    cp_out = torch.empty((n, 3), dtype=torch.int32, device=dev)
    rows = torch.empty((n, 3), dtype=torch.float64, device=dev)
    counts = torch.empty((S, 2), dtype=torch.int32, device=dev)
    need = int(lib.dd_range_image_points_workspace_bytes(S, int((desc[:, 1].astype(np.int64) * desc[:, 2]).max())))
    work = torch.empty(max(need, 4), dtype=torch.uint8, device=dev)
    L.check(lib.dd_range_image_points(abi.ptr(rng), abi.ptr(cp), abi.ptr(pose) if pose.shape[0] else None, abi.ptr(trig), n, int(pose.shape[0]),
                                      int(trig.shape[0]), desc.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), S, abi.ptr(params), abi.ptr(counts),
                                      abi.ptr(points), abi.ptr(cp_out), abi.ptr(rows), abi.ptr(work), need, L.current_stream()),
            "dd_range_image_points")
    return points, cp_out, rows, counts


def range_image_points(ranges, cps, poses, trigs, params):
    """`range_image_points_host` on the device from host arrays, one call for all the images: the same (list, counts)."""
    import torch
    rng, cp, pose, trig, desc = range_image_pack(ranges, cps, poses, trigs)
    up = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (rng, cp, pose, trig, np.asarray(params, dtype=np.float64).reshape(-1, RI_STRIDE))]
    points, cp_out, rows, counts = (t.cpu().numpy() for t in range_image_points_device(up[0], up[1], up[2], up[3], desc, up[4]))
    out = []
    for s in range(desc.shape[0]):
        a, n, m = int(desc[s, 0]), int(counts[s, 0]), int(counts[s, 1])
        out.append((points[a:a + n].copy(), cp_out[a:a + n].copy(), rows[a:a + m].copy()))
    return out, counts


def upright_box_corners(box):
    """float64 (8, 3): the Waymo library's get_upright_3d_box_corners for [center_x, center_y, center_z, length, width, height,
    heading]: corner 0 at (+l/2, +w/2, -h/2), corners 1, 3 and 4 across the length, the width and the height from it, rotated by the
    heading about z and moved to the centre."""
    cx, cy, cz, l, w, h, heading = (float(v) for v in box)
    c, s = np.cos(heading), np.sin(heading)
    R = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    local = 0.5 * np.array([[l, w, -h], [-l, w, -h], [-l, -w, -h], [l, -w, -h], [l, w, h], [-l, w, h], [-l, -w, h], [l, -w, h]], dtype=np.float64)
    return local @ R.T + np.array([cx, cy, cz])
