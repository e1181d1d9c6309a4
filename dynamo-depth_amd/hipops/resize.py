"""Host side of the device bicubic resize (csrc/dd_resize.hip): Pillow's tap tables and the batch call.

Replaces `transforms.Resize((height, width), interpolation=BICUBIC)` on PIL frames in the loaders (reference
datasets/base_dataset.py:80,147) for frames that are not stored at the training resolution (KITTI's `original` image type: four
sizes around 1242x375): the workers hand over the compressed files, the GPU decodes (hipops.jpeg) and resizes -- the result is
Pillow's, bit for bit.

The tables follow Pillow's src/libImaging/Resample.c (public source; `precompute_coeffs` + `normalize_coeffs_8bpc`), restated:
output index xx looks at the input window [center - support, center + support) around center = (xx + 0.5) * scale with
support = 2 * max(scale, 1) (bicubic, stretched when down-scaling: the antialiasing), weights = Keys cubic (a = -0.5) of the
distances / max(scale, 1), normalised to sum 1, rounded half away from zero to 22-bit fixed point."""
import ctypes as C
import math

import numpy as np
import torch

from . import abi
from . import lib as L

PRECISION_BITS = 32 - 8 - 2
_tables = {}


def _cubic(x):
    x = np.abs(x)
    a = -0.5
    near = ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0
    far = (((x - 5.0) * x + 8.0) * x - 4.0) * a
    return np.where(x < 1.0, near, np.where(x < 2.0, far, 0.0))


def coefficients(in_size, out_size):
    """(bounds (out, 2) int32 [first input index, tap count], coef (out, ksize) int32) of one axis."""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    coef = np.zeros((out_size, ksize), dtype=np.int32)
    inv = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        count = min(int(center + support + 0.5), in_size) - xmin
        w = _cubic((np.arange(count, dtype=np.float64) + xmin - center + 0.5) * inv)
        total = 0.0
        for v in w:                      # (left-to-right sum in double, as the C loop accumulates it)
            total += float(v)
        if total != 0.0:
            w = w / total
        q = np.where(w < 0, (-0.5 + w * (1 << PRECISION_BITS)).astype(np.int64), (0.5 + w * (1 << PRECISION_BITS)).astype(np.int64))      # C casts truncate
        coef[xx, :count] = q
        bounds[xx] = (xmin, count)
    return bounds, coef


def _device_tables(in_size, out_size, device):
    key = (in_size, out_size, str(device))
    t = _tables.get(key)
    if t is None:
        b, k = coefficients(in_size, out_size)
        t = _tables[key] = (torch.from_numpy(b).to(device), torch.from_numpy(k).to(device), k.shape[1])
    return t


def area_table(in_size, out_size):
    """(start (out,) int32, count (out,) int32, weight (out, taps) float32 padded with zeros) of one axis of the area-weighted
    down-sample: OpenCV's computeResizeAreaTab (public source) restated.  Destination d covers [d scale, (d + 1) scale) with
    scale = in / out; cell = min(scale, in - d scale); the left partial pixel weighs (ceil(f1) - f1) / cell and the right one
    min(min(f2 - floor(f2), 1), cell) / cell, each only where its length exceeds 1e-3; whole pixels weigh 1 / cell.  float64
    arithmetic, every weight rounded to fp32 once."""
    in_size, out_size = int(in_size), int(out_size)
    if out_size < 1 or in_size < out_size:
        raise ValueError("area_table is a down-sample: 1 <= out <= in")
    scale = in_size / out_size
    rows = []
    for d in range(out_size):
        f1 = d * scale
        f2 = f1 + scale
        cell = min(scale, in_size - f1)
        s2 = min(int(math.floor(f2)), in_size - 1)
        s1 = min(int(math.ceil(f1)), s2)
        taps = []
        if s1 - f1 > 1e-3:
            taps.append((s1 - 1, (s1 - f1) / cell))
        taps.extend((s, 1.0 / cell) for s in range(s1, s2))
        if f2 - s2 > 1e-3:
            taps.append((s2, min(min(f2 - s2, 1.0), cell) / cell))
        rows.append(taps)
    width = max(len(t) for t in rows)
    start = np.array([t[0][0] for t in rows], dtype=np.int32)
    count = np.array([len(t) for t in rows], dtype=np.int32)
    weight = np.zeros((out_size, width), dtype=np.float32)
    for d, taps in enumerate(rows):
        assert [s for s, _ in taps] == list(range(taps[0][0], taps[0][0] + len(taps)))
        weight[d, :len(taps)] = [w for _, w in taps]
    return start, count, weight


def resize_area_sums(frames, height, width):
    """The float64 weighted sums of `resize_area_host` before rounding: (n, height, width, 3)."""
    frames = np.asarray(frames)
    if frames.ndim != 4 or frames.shape[-1] != 3 or frames.dtype != np.uint8:
        raise ValueError("resize_area takes (n, H, W, 3) uint8 frames")
    hs, _, hw = area_table(frames.shape[2], width)
    vs, _, vw = area_table(frames.shape[1], height)
    cols = np.zeros(frames.shape[:2] + (width, 3), dtype=np.float64)
    for k in range(hw.shape[1]):                     # a padded tap has weight 0: any pixel will do
        cols += frames[:, :, np.minimum(hs + k, frames.shape[2] - 1), :] * hw[:, k].astype(np.float64)[None, None, :, None]
    out = np.zeros((frames.shape[0], height, width, 3), dtype=np.float64)
    for k in range(vw.shape[1]):
        out += cols[:, np.minimum(vs + k, frames.shape[1] - 1)] * vw[:, k].astype(np.float64)[None, :, None, None]
    return out


def resize_area_host(frames, height, width):
    """The definition of dd_resize_area in numpy: frames (n, Hs, Ws, 3) uint8 -> (n, height, width, 3) uint8, the separable weighted
    sum of `area_table`'s fp32 weights in float64, rounded half to even, saturated.  What cv2.resize(frame, (width, height),
    interpolation=cv2.INTER_AREA) computes in fp32 at a non-integer scale."""
    return np.clip(np.rint(resize_area_sums(frames, height, width)), 0, 255).astype(np.uint8)


def _area_device_tables(in_size, out_size, device):
    key = ("area", in_size, out_size, str(device))
    t = _tables.get(key)
    if t is None:
        s, c, w = area_table(in_size, out_size)
        t = _tables[key] = (torch.from_numpy(s).to(device), torch.from_numpy(c).to(device), torch.from_numpy(w).to(device), w.shape[1])
    return t


def resize_area_batch(frames, height, width):
    """frames (n, Hs, Ws, 3) uint8 on the GPU -> (n, height, width, 3) uint8: `resize_area_host` on the device (fp32 sums), one launch."""
    if not (torch.is_tensor(frames) and frames.is_cuda and frames.dtype == torch.uint8 and frames.dim() == 4 and frames.shape[-1] == 3):
        raise L.DynamoHipError("resize_area_batch takes (n, H, W, 3) uint8 frames on the GPU")
    n, hs, ws = int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2])
    height, width = int(height), int(width)
    if n < 1 or height < 1 or width < 1 or height > hs or width > ws:
        raise L.DynamoHipError("resize_area_batch is a down-sample of at least one frame")
    lib = L.load()
    frames = frames.contiguous()
    out = torch.empty((n, height, width, 3), dtype=torch.uint8, device=frames.device)
    h_s, h_c, h_w, h_k = _area_device_tables(ws, width, frames.device)
    v_s, v_c, v_w, v_k = _area_device_tables(hs, height, frames.device)
    L.check(lib.dd_resize_area(abi.ptr(frames), n, hs, ws, abi.ptr(out), height, width, abi.ptr(h_s), abi.ptr(h_c), abi.ptr(h_w), h_k, abi.ptr(v_s),
                               abi.ptr(v_c), abi.ptr(v_w), v_k, L.current_stream()), "dd_resize_area")
    return out


def resize_batch(src, out_h, out_w, out=None, slots=None):
    """src (n, Hs, Ws, 3) uint8 on the GPU -> (n, out_h, out_w, 3) uint8 (or image i into out[slots[i]] of a caller's (m, out_h, out_w, 3)
    buffer): what `Image.fromarray(frame).resize((out_w, out_h), Image.BICUBIC)` holds for every frame."""
    if not src.is_cuda or src.dtype != torch.uint8 or src.dim() != 4 or src.shape[-1] != 3:
        raise L.DynamoHipError("resize_batch takes (n, H, W, 3) uint8 frames on the GPU")
    lib = L.load()
    src = src.contiguous()
    n, hs, ws = int(src.shape[0]), int(src.shape[1]), int(src.shape[2])
    if out is None:
        out = torch.empty((n, out_h, out_w, 3), dtype=torch.uint8, device=src.device)
    slot_t = None
    if slots is not None:
        slot_t = torch.as_tensor(slots, dtype=torch.int32).to(src.device).contiguous()
    if hs == out_h and ws == out_w:
        if slot_t is None:
            out.copy_(src)
        else:
            out[slot_t.long()] = src
        return out
    hb = hk = vb = vk = None
    hks = vks = 0
    if ws != out_w:
        hb, hk, hks = _device_tables(ws, out_w, src.device)
    if hs != out_h:
        vb, vk, vks = _device_tables(hs, out_h, src.device)
    need = int(lib.dd_resize_workspace_bytes(n, hs, ws, out_h, out_w))
    work = torch.empty(max(need, 1), dtype=torch.uint8, device=src.device)
    L.check(lib.dd_resize_bicubic(abi.ptr(src), n, hs, ws, abi.ptr(out), abi.ptr(slot_t), out_h, out_w, abi.ptr(hb), abi.ptr(hk), hks, abi.ptr(vb), abi.ptr(vk), vks,
                                  abi.ptr(work), need, L.current_stream()), "dd_resize_bicubic")
    return out
