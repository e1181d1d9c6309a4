"""Moving objects as labelled instances (csrc/dd_objects.hip): the definition on the host in numpy, the wrapper of the
five-launch entry point, the table's layout and what goes to JSON.

The network's motion mask, thresholded, falls into connected components; every component that is large enough is an object with a
number, a box, a position and a motion of its own.  Everything is at the NETWORK's resolution h x w; the camera convention is the
clouds' (hipops/cloud.py): x right, y down, z forward, integer pixel coordinates, intrinsics (fx, fy, cx, cy) in pixels of h x w.

  foreground  fg = motion_mask >= thresh, compared in fp32: false for NaN.
  components  the maximal sets of foreground pixels of ONE image connected through 4-neighbourhoods (W, E, N, S) or 8-neighbourhoods
              (the diagonals too).  A component's anchor is its smallest row-major index y * w + x.
  objects     the components of at least min_pixels pixels, numbered 1, 2, ... per image in increasing anchor order (the numbering
              scipy.ndimage.label gives).  With more than max_objects of them only the first max_objects by that order stay objects:
              count_found is the full number, truncated is set.
  labels      (B,h,w) int32: the object's number; 0 for background, for the components that are too small and for those the cap cut.
  per pixel   every operation in fp32 and none fused.  d = disp[y, x], or with `disp_flipped` hipops/export.py's fuse_host;
              s = lo + span * d with export.depth_params;  z = 1 / s (IEEE);  xc = ((float)x - cx) * ifx, yc = ((float)y - cy) * ify with
              cloud.inverse_focal;  p = (xc * z, yc * z, z);  with pose = [R | t] of frame 0 -> the neighbouring frame
              q_k = ((R[k,0] * p0 + R[k,1] * p1) + R[k,2] * p2) + t[k];  ego = q - p;  c = complete_flow * ts[b];  r = c - ego.
              r is the object's own motion between the two frames in frame 0's camera coordinates: Trainer.generate_images_pred's
              `residual` at scale 0 with `interp` the identity.
  table       one row per object, ROW_DTYPE (ROW = 22 32-bit words, include/dynamo_hip.h DD_OBJECTS_ROW):
              pixels, box = (x0, y0, x1, y1) inclusive, anchor: exact integers;
              z = (z_min, z_max): fminf / fmaxf of z over the object's pixels with 0 < z < inf -- a pixel whose z is NaN, infinite, zero
              or negative is left out of the two, and an object without any valid pixel has z_min = +inf and z_max = 0;
              sums = sum p[3], sum r[3], sum motion_mask: float64 sums of the fp32 per-pixel values, on the host added in row-major
              order, on the device in the order the atomics arrive.
              Such a pixel still BELONGS to its object (labels are a property of the mask alone) and enters the sums: the sums of that
              object become NaN or infinite, and no other row is touched -- the host sums per label (np.bincount), never across.
              Rows at and past the image's kept count are all zero.
  derived     on the host in float64: centroid = sum_p / pixels, motion = sum_r / pixels, speed = |motion|, confidence = sum_mask / pixels.
  box         `scale_box` takes a network box to the H x W source image as the extent of its pixels: x0' = floor(x0 * W / w),
              x1' = ceil((x1 + 1) * W / w) - 1, the same with H / h for y, in integer arithmetic.
  label image `labels_u16`: out[Y, X] = labels[min(h-1, (2Y+1)*h // (2H)), min(w-1, (2X+1)*w // (2W))], saturated at 65535."""
import numpy as np

from . import abi
from . import lib as L
from .cloud import inverse_focal
from .export import _device_planes, _planes, _size, _table, depth_params, fuse_host

_f32 = np.float32
ROW = abi.DD_OBJECTS_ROW
ROW_DTYPE = np.dtype([("pixels", "<i4"), ("box", "<i4", (4,)), ("anchor", "<i4"), ("z", "<f4", (2,)), ("sums", "<f8", (7,))])
MAX_OBJECTS = 65535             # a label fits the 16-bit image
MOTION_NOTE = "motion is the object's own 3-D motion over one frame gap (the network's flow times the gap's time step ts), ego-motion removed"
assert ROW_DTYPE.itemsize == 4 * ROW


def _check(connectivity, min_pixels, max_objects, error=ValueError):
    if int(connectivity) not in (4, 8):
        raise error("objects: connectivity is 4 or 8, not {}".format(connectivity))
    if int(min_pixels) < 1:
        raise error("objects: min_pixels is at least 1, not {}".format(min_pixels))
    if not 1 <= int(max_objects) <= MAX_OBJECTS:
        raise error("objects: max_objects is between 1 and {}, not {}".format(MAX_OBJECTS, max_objects))
    return int(connectivity), int(min_pixels), int(max_objects)


def _anchors(fg, connectivity):
    """(h,w) bool -> (h*w,) int64: the anchor of every foreground pixel's component, -1 for background.  Two-pass union-find over the
    row-major indices; a union hangs the larger root under the smaller, so a root is its set's smallest index."""
    h, w = fg.shape
    flat = fg.reshape(-1).tolist()
    parent = list(range(h * w))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    eight = connectivity == 8
    for i in np.flatnonzero(fg.reshape(-1)).tolist():
        y, x = divmod(i, w)
        near = []
        if x > 0:
            near.append(i - 1)
        if y > 0:
            near.append(i - w)
            if eight and x > 0:
                near.append(i - w - 1)
            if eight and x < w - 1:
                near.append(i - w + 1)
        for j in near:
            if flat[j]:
                a, b = find(i), find(j)
                if a != b:
                    parent[max(a, b)] = min(a, b)
    return np.array([find(i) if flat[i] else -1 for i in range(h * w)], dtype=np.int64)


def label_components_host(motion_mask, *, thresh=0.5, connectivity=8, min_pixels=16, max_objects=256):
    """The definition above: (labels (B,h,w) int32, count_found (B,) int32, truncated (B,) bool)."""
    connectivity, min_pixels, max_objects = _check(connectivity, min_pixels, max_objects)
    m = _planes(motion_mask, "motion_mask")
    B, h, w = m.shape
    with np.errstate(invalid="ignore"):
        fg = m >= _f32(thresh)
    labels = np.zeros((B, h, w), dtype=np.int32)
    found = np.zeros(B, dtype=np.int32)
    for b in range(B):
        root = _anchors(fg[b], connectivity)
        size = np.bincount(root[root >= 0], minlength=h * w)
        anchors = np.flatnonzero(size >= min_pixels)            # increasing: the numbering
        found[b] = len(anchors)
        number = np.zeros(h * w + 1, dtype=np.int32)            # the last entry serves the background's -1
        kept = anchors[:max_objects]
        number[kept] = np.arange(1, len(kept) + 1)
        labels[b] = number[root].reshape(h, w)
    return labels, found, found > max_objects


def pixel_quantities_host(motion_mask, disp, complete_flow, ts, pose, intrinsics, *, disp_flipped=None, min_depth, max_depth):
    """The per-pixel quantities of the definition: {"z": (B,h,w), "p": (B,3,h,w), "r": (B,3,h,w), "mask": (B,h,w)} float32."""
    m, d = _planes(motion_mask, "motion_mask"), _planes(disp, "disp")
    B, h, w = d.shape
    flow, ts, T = np.asarray(complete_flow, dtype=np.float32), np.asarray(ts, dtype=np.float32).reshape(-1), np.asarray(pose, dtype=np.float32)
    if m.shape != d.shape or flow.shape != (B, 3, h, w) or ts.shape != (B,) or T.shape != (B, 3, 4):
        raise ValueError("objects: motion_mask as disp, complete_flow (B, 3, h, w), ts (B,), pose (B, 3, 4)")
    fx, fy, cx, cy = (_f32(v) for v in intrinsics)
    with np.errstate(all="ignore"):
        if disp_flipped is not None:
            r = _planes(disp_flipped, "disp_flipped")
            if r.shape != d.shape:
                raise ValueError("disp_flipped must have disp's shape")
            d = fuse_host(d, r)
        lo, span = depth_params(min_depth, max_depth)
        z = (_f32(1) / (lo + span * d).astype(np.float32)).astype(np.float32)
        xc = ((np.arange(w).astype(np.float32)[None, None, :] - cx) * inverse_focal(fx)).astype(np.float32)
        yc = ((np.arange(h).astype(np.float32)[None, :, None] - cy) * inverse_focal(fy)).astype(np.float32)
        p = [(xc * z).astype(np.float32), (yc * z).astype(np.float32), z]
        T = T[:, :, :, None, None]
        q = [(((T[:, k, 0] * p[0] + T[:, k, 1] * p[1]) + T[:, k, 2] * p[2]) + T[:, k, 3]).astype(np.float32) for k in range(3)]
        c = (flow * ts[:, None, None, None]).astype(np.float32)
        res = [(c[:, k] - (q[k] - p[k]).astype(np.float32)).astype(np.float32) for k in range(3)]
    return {"z": z, "p": np.stack(p, axis=1), "r": np.stack(res, axis=1), "mask": m}


def object_table_host(labels, quantities, max_objects=256):
    """labels (B,h,w) and `pixel_quantities_host`'s result -> the table, (B, max_objects, ROW) int32 in the device's layout (view it
    with `rows`)."""
    labels = np.asarray(labels, dtype=np.int32)
    B, h, w = labels.shape
    table = np.zeros((B, int(max_objects)), dtype=ROW_DTYPE)
    ys, xs = np.divmod(np.arange(h * w), w)
    values = np.concatenate([quantities["p"], quantities["r"], quantities["mask"][:, None]], axis=1).reshape(B, 7, h * w).astype(np.float64)
    with np.errstate(all="ignore"):
        for b in range(B):
            lab = labels[b].reshape(-1)
            n = int(lab.max())
            if n == 0:
                continue
            row = table[b, :n]
            row["pixels"] = np.bincount(lab, minlength=n + 1)[1:]
            inside = lab > 0
            li, x, y, z = lab[inside] - 1, xs[inside], ys[inside], quantities["z"][b].reshape(-1)[inside]
            box = np.array([[w, h, -1, -1]] * n)
            np.minimum.at(box[:, 0], li, x), np.minimum.at(box[:, 1], li, y), np.maximum.at(box[:, 2], li, x), np.maximum.at(box[:, 3], li, y)
            row["box"] = box
            first = np.full(n, h * w)
            np.minimum.at(first, li, np.flatnonzero(inside))
            row["anchor"] = first
            ok = (z > 0) & np.isfinite(z)
            zr = np.stack([np.full(n, np.inf, dtype=np.float32), np.zeros(n, dtype=np.float32)], axis=1)
            np.minimum.at(zr[:, 0], li[ok], z[ok]), np.maximum.at(zr[:, 1], li[ok], z[ok])
            row["z"] = zr
            for k in range(7):          # bincount adds in index order, row-major, one accumulator per label: a NaN stays in its row
                row["sums"][:, k] = np.bincount(lab, weights=values[b, k], minlength=n + 1)[1:]
    return table.view(np.int32).reshape(B, int(max_objects), ROW)


def objects_host(motion_mask, disp, complete_flow, ts, pose, intrinsics, *, disp_flipped=None, min_depth, max_depth, thresh=0.5, connectivity=8,
                 min_pixels=16, max_objects=256):
    """The definition above in numpy: (labels (B,h,w) int32, table (B,max_objects,ROW) int32, counts (B,3) int32 = kept, found, truncated)."""
    labels, found, truncated = label_components_host(motion_mask, thresh=thresh, connectivity=connectivity, min_pixels=min_pixels, max_objects=max_objects)
    q = pixel_quantities_host(motion_mask, disp, complete_flow, ts, pose, intrinsics, disp_flipped=disp_flipped, min_depth=min_depth, max_depth=max_depth)
    counts = np.stack([np.minimum(found, int(max_objects)), found, truncated.astype(np.int32)], axis=1).astype(np.int32)
    return labels, object_table_host(labels, q, max_objects), counts


def rows(table):
    """(B, max_objects, ROW) int32, from the host or fetched from the device -> (B, max_objects) records of ROW_DTYPE."""
    t = np.ascontiguousarray(np.asarray(table, dtype=np.int32))
    if t.ndim != 3 or t.shape[2] != ROW:
        raise ValueError("an object table is (B, max_objects, {}) int32".format(ROW))
    return t.view(ROW_DTYPE).reshape(t.shape[:2])


def scale_box(box, h, w, H, W):
    """The inclusive network-resolution box (x0, y0, x1, y1) at the H x W source image: the extent of its pixels, low edges rounded
    down and high edges rounded up."""
    x0, y0, x1, y1 = (int(v) for v in box)
    return [x0 * W // w, y0 * H // h, -(-(x1 + 1) * W // w) - 1, -(-(y1 + 1) * H // h) - 1]


def _number(v):
    v = float(v)
    return v if np.isfinite(v) else None            # JSON has no NaN and no infinity


def unpack_table(table, counts, size=None):
    """table (B,max_objects,ROW) and counts (B,3) as arrays on the host -> per frame {"found", "truncated", "objects": [...]} of plain
    Python values: what goes to JSON.  Per object id, pixels, box (network pixels, or with size = (h, w, H, W) `scale_box`ed to the
    source image), anchor, centroid, motion, speed, confidence, z_min, z_max; a value that is not finite (an object with a pixel of
    undefined depth) is None."""
    t, counts = rows(table), np.asarray(counts).reshape(-1, 3)
    frames = []
    with np.errstate(all="ignore"):
        for b in range(t.shape[0]):
            objects = []
            for n in range(int(counts[b, 0])):
                row = t[b, n]
                pixels = int(row["pixels"])
                sums = row["sums"].astype(np.float64) / pixels
                motion = sums[3:6]
                box = [int(v) for v in row["box"]]
                objects.append({"id": n + 1, "pixels": pixels, "box": box if size is None else scale_box(box, *size), "anchor": int(row["anchor"]),
                                "centroid": [_number(v) for v in sums[:3]], "motion": [_number(v) for v in motion],
                                "speed": _number(np.sqrt((motion * motion).sum())), "confidence": _number(sums[6]),
                                "z_min": _number(row["z"][0]), "z_max": _number(row["z"][1]) if np.isfinite(row["z"][0]) else None})
            frames.append({"found": int(counts[b, 1]), "truncated": bool(counts[b, 2]), "objects": objects})
    return frames


def labels_u16_host(labels, H, W):
    """The label image at the source size in numpy: (B,H,W) uint16."""
    labels = np.asarray(labels)
    B, h, w = labels.shape
    y = np.minimum(h - 1, (2 * np.arange(int(H)) + 1) * h // (2 * int(H)))
    x = np.minimum(w - 1, (2 * np.arange(int(W)) + 1) * w // (2 * int(W)))
    return np.clip(labels[:, y][:, :, x], 0, 65535).astype(np.uint16)


# ---- device --------------------------------------------------------------------------------------------------------------------------
_workspaces = {}            # (B, h, w, max_objects, device) -> int64 tensor: one per shape, every call writes what it reads


def _workspace(B, h, w, max_objects, device):
    import torch
    key = (B, h, w, max_objects, str(device))
    if key not in _workspaces:
        need = L.load().dd_objects_workspace_bytes(B, h, w, max_objects)
        if need == 0:
            raise L.DynamoHipError("find_objects: {} x {} x {} with {} objects is more than one call takes".format(B, h, w, max_objects))
        _workspaces[key] = (torch.empty((need // 8,), dtype=torch.int64, device=device), need)
    return _workspaces[key]


def find_objects(motion_mask, disp, complete_flow, ts, pose, intrinsics, *, disp_flipped=None, min_depth, max_depth, thresh=0.5, connectivity=8,
                 min_pixels=16, max_objects=256):
    """motion_mask, disp (B,1,h,w) or (B,h,w), complete_flow (B,3,h,w), ts (B,) or (B,1), pose (B,3,4) or (B,4,4), optional disp_flipped,
    all fp32 on one GPU -> (labels (B,h,w) int32, table (B,max_objects,ROW) int32, counts (B,3) int32) on the GPU.  Five launches on
    the current stream, no host sync.  The workspace is shared by the calls of one shape: calls on different streams must not overlap."""
    import torch
    connectivity, min_pixels, max_objects = _check(connectivity, min_pixels, max_objects, L.DynamoHipError)
    m = _device_planes(motion_mask, "find_objects: motion_mask")
    d = _device_planes(disp, "find_objects: disp")
    B, h, w = m.shape
    if d.shape != m.shape or d.device != m.device:
        raise L.DynamoHipError("find_objects: disp must have motion_mask's shape and device")
    r = lmask = None
    if disp_flipped is not None:
        r = _device_planes(disp_flipped, "find_objects: disp_flipped")
        if r.shape != m.shape or r.device != m.device:
            raise L.DynamoHipError("find_objects: disp_flipped must have motion_mask's shape and device")
        lmask = _table("l_mask", w, m.device)

    def fp32(t, shapes, what):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.device == m.device and tuple(t.shape) in shapes):
            raise L.DynamoHipError("find_objects: {} must be an fp32 tensor of shape {} on motion_mask's device".format(what, " or ".join(str(s) for s in shapes)))
        return t

    flow = fp32(complete_flow, ((B, 3, h, w),), "complete_flow").contiguous()
    ts = fp32(ts, ((B,), (B, 1)), "ts").reshape(B).contiguous()
    T = fp32(pose, ((B, 3, 4), (B, 4, 4)), "pose")[:, :3].contiguous()
    fx, fy, cx, cy = (float(v) for v in intrinsics)
    if not (np.isfinite(fx) and np.isfinite(fy) and _f32(fx) != 0 and _f32(fy) != 0):
        raise L.DynamoHipError("find_objects: fx and fy are finite and not zero")
    if not (float(min_depth) > 0 and float(max_depth) > 0):
        raise L.DynamoHipError("find_objects: min_depth and max_depth are positive")
    lo, span = depth_params(min_depth, max_depth)
    lib = L.load()
    with torch.cuda.device(m.device):
        ws, need = _workspace(B, h, w, max_objects, m.device)
        labels = torch.empty((B, h, w), dtype=torch.int32, device=m.device)
        table = torch.empty((B, max_objects, ROW), dtype=torch.int32, device=m.device)
        counts = torch.empty((B, 3), dtype=torch.int32, device=m.device)
        L.check(lib.dd_objects(abi.ptr(m), abi.ptr(d), abi.ptr(r), abi.ptr(lmask), abi.ptr(flow), abi.ptr(ts), abi.ptr(T), B, h, w, fx, fy, cx, cy,
                               float(lo), float(span), float(thresh), connectivity, min_pixels, max_objects, abi.ptr(labels), abi.ptr(table),
                               abi.ptr(counts), abi.ptr(ws), need, L.current_stream()), "dd_objects")
    return labels, table, counts


def labels_u16(labels, H, W):
    """labels (B,h,w) int32 on the GPU -> (B,H,W) uint16 on the GPU, the nearest-neighbour label image at the source size: one launch."""
    import torch
    if not (torch.is_tensor(labels) and labels.is_cuda and labels.dtype == torch.int32 and labels.dim() == 3 and labels.numel() > 0):
        raise L.DynamoHipError("labels_u16: labels must be a (B, h, w) int32 tensor on the GPU")
    H, W = _size(H, W, "labels_u16")
    labels = labels.contiguous()
    B, h, w = labels.shape
    with torch.cuda.device(labels.device):
        out = torch.empty((B, H, W), dtype=torch.uint16, device=labels.device)
        L.check(L.load().dd_export_labels_u16(abi.ptr(labels), B, h, w, H, W, abi.ptr(out), L.current_stream()), "dd_export_labels_u16")
    return out
