"""Full-resolution depth export (csrc/dd_export.hip): the definition on the host in numpy and the one-launch wrappers.

What the depth metrics define at a LiDAR point -- reference tools.py:42 `F.interpolate(disp_scaled, gt size, mode="bilinear",
align_corners=False)` over tools.py:291-298 `disp_to_depth`, then `1 / x` -- at every pixel of the H x W source image.  Per output
pixel (b, Y, X), every operation in fp32 and none fused:

  fuse      only with `disp_flipped`, the network's disparity of the mirrored image, not mirrored back (the flip post-processing the
            monocular-depth literature reports as "PP").  For a source tap (y, x): l = disp[y, x], r = disp_flipped[y, w-1-x],
            m = 0.5 * (l + r), lm = l_mask[x], rm = l_mask[w-1-x], d = (rm*l + lm*r) + ((1 - lm) - rm) * m, in that order;
            l_mask = 1 - clip(20 * (linspace(0, 1, w) - 0.05), 0, 1) evaluated in float64 and rounded to fp32 (`l_mask_table`).
            Without `disp_flipped`, d = disp[y, x].
  scale     s = lo + span * d with lo = 1 / max_depth and span = 1 / min_depth - 1 / max_depth, both evaluated in float64 on the fp32
            bounds and rounded to fp32 once: tools.disp_to_depth as csrc/dd_ops.hip evaluates it.
  upsample  ATen's fp32 bilinear (csrc/dd_bilinear.h): scale = (float)in / (float)out, src = max(scale * (X + 0.5) - 0.5, 0),
            i0 = min((int)src, in - 1), i1 = i0 + (i0 < in - 1), w1 = src - i0;  top = (1 - wx) * a + wx * b, bot = (1 - wx) * c + wx * d,
            value = (1 - wy) * top + wy * bot.  u is the blend of the four s taps, d_up the same blend of the four d taps.
  outputs   depth = 1 / u (IEEE division);  depth16 = min(rint(depth * depth_scale), 65535) half to even, 0 where that is NaN or
            below 1;  rgb = table[entry of d_up] by matplotlib's Normalize(vmin, vmax) and 256-entry lookup on fp32 data (hipops.vis),
            black for NaN.

`export_plane_u8` is the same upsample of a plane followed by (uint8)(clamp(x, 0, 1) * 255): the motion mask."""
import numpy as np

from . import abi
from . import lib as L
from .vis import cmap_bytes

OUTPUTS = ("depth", "depth16", "rgb")
_f32 = np.float32


def l_mask_table(w):
    """[w] fp32: 1 - clip(20 * (linspace(0, 1, w) - 0.05), 0, 1), float64 rounded to fp32."""
    return (1.0 - np.clip(20.0 * (np.linspace(0.0, 1.0, int(w)) - 0.05), 0.0, 1.0)).astype(np.float32)


def depth_params(min_depth, max_depth):
    """(lo, span) of s = lo + span * d: csrc/dd_math.h depth_params."""
    lo, hi = 1.0 / float(_f32(max_depth)), 1.0 / float(_f32(min_depth))
    return _f32(lo), _f32(hi - lo)


def _taps(out_size, in_size):
    """dm_tap of csrc/dd_bilinear.h for every destination index: (i0, i1, w1)."""
    scale = _f32(in_size) / _f32(out_size)
    src = scale * (np.arange(out_size).astype(np.float32) + _f32(0.5)) - _f32(0.5)
    src = np.where(src < 0, _f32(0), src).astype(np.float32)
    i0 = np.minimum(src.astype(np.int64), in_size - 1)
    i1 = i0 + (i0 < in_size - 1)
    return i0, i1, (src - i0.astype(np.float32)).astype(np.float32)


def _blend(v, H, W):
    """dm_blend over (B, h, w) fp32 -> (B, H, W) fp32."""
    y0, y1, wy = _taps(H, v.shape[1])
    x0, x1, wx = _taps(W, v.shape[2])
    wy, wx = wy[None, :, None], wx[None, None, :]
    one = _f32(1)
    top = (one - wx) * v[:, y0][:, :, x0] + wx * v[:, y0][:, :, x1]
    bot = (one - wx) * v[:, y1][:, :, x0] + wx * v[:, y1][:, :, x1]
    return ((one - wy) * top + wy * bot).astype(np.float32)


def _planes(x, what):
    x = np.asarray(x, dtype=np.float32)
    if x.ndim == 4 and x.shape[1] == 1:
        x = x[:, 0]
    if x.ndim != 3 or x.size == 0:
        raise ValueError("{} must be (B, h, w) or (B, 1, h, w)".format(what))
    return x


def fuse_host(disp, disp_flipped):
    """The fuse step on (B, h, w) fp32."""
    w = disp.shape[2]
    l, r = disp, disp_flipped[:, :, ::-1]
    lm = l_mask_table(w)[None, None, :]
    rm = lm[:, :, ::-1]
    m = _f32(0.5) * (l + r)
    return ((rm * l + lm * r) + ((_f32(1) - lm) - rm) * m).astype(np.float32)


def export_depth_host(disp, H, W, *, disp_flipped=None, min_depth, max_depth, depth_scale=256.0, want=OUTPUTS, vmin=0.0, vmax=1.0):
    """The definition above in numpy: {"depth": (B,H,W) float32, "depth16": (B,H,W) uint16, "rgb": (B,H,W,3) uint8}, the requested ones."""
    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise ValueError("export_depth_host needs H, W >= 1")
    d = _planes(disp, "disp")
    with np.errstate(all="ignore"):
        if disp_flipped is not None:
            r = _planes(disp_flipped, "disp_flipped")
            if r.shape != d.shape:
                raise ValueError("disp_flipped must have disp's shape")
            d = fuse_host(d, r)
        lo, span = depth_params(min_depth, max_depth)
        depth = (_f32(1) / _blend((lo + span * d).astype(np.float32), H, W)).astype(np.float32)
        out = {}
        if "depth" in want:
            out["depth"] = depth
        if "depth16" in want:
            q = np.rint(depth * _f32(depth_scale))
            q = np.where(q >= 1, np.minimum(q, _f32(65535)), _f32(0))       # NaN compares false
            out["depth16"] = q.astype(np.uint16)
        if "rgb" in want:
            vmin, vmax = _f32(vmin), _f32(vmax)
            s = ((_blend(d, H, W) - vmin) / (vmax - vmin)) * _f32(256)
            nan = np.isnan(s)
            idx = np.clip(np.where(nan, _f32(0), s), 0, 255).astype(np.int64)      # below 0 -> 0, 256 and above -> 255, else truncated
            rgb = cmap_bytes("plasma")[idx]
            rgb[nan] = 0
            out["rgb"] = rgb
    return out


def export_plane_u8_host(plane, H, W):
    """(B, H, W) uint8 = (uint8)(clamp(bilinear(plane), 0, 1) * 255); a NaN clamps to 0 (fmaxf)."""
    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise ValueError("export_plane_u8_host needs H, W >= 1")
    with np.errstate(all="ignore"):
        v = _blend(_planes(plane, "plane"), H, W)
        return (np.fmin(np.fmax(v, _f32(0)), _f32(1)) * _f32(255)).astype(np.uint8)


# ---- device ------------------------------------------------------------------------------------------------------------------------
_tables = {}            # (what, w, device) -> device tensor: made once, so that a call copies nothing from the host


def _table(what, w, device):
    import torch
    key = (what, int(w), str(device))
    if key not in _tables:
        if what == "l_mask":
            host = torch.from_numpy(l_mask_table(w))
        else:
            t = cmap_bytes("plasma").astype(np.int32)
            host = torch.from_numpy(t[:, 0] | (t[:, 1] << 8) | (t[:, 2] << 16))
        _tables[key] = host.to(device)
    return _tables[key]


def _device_planes(t, what):
    import torch
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32):
        raise L.DynamoHipError("{} must be an fp32 tensor on the GPU".format(what))
    if t.dim() == 4 and t.shape[1] == 1:
        t = t[:, 0]
    if t.dim() != 3 or t.numel() == 0:
        raise L.DynamoHipError("{} must be (B, h, w) or (B, 1, h, w)".format(what))
    return t.contiguous()


def _size(H, W, what):
    H, W = int(H), int(W)
    if H < 1 or W < 1 or H * W > 2 ** 31 - 1:
        raise L.DynamoHipError("{}: H, W >= 1 and H * W <= 2**31 - 1, not {} x {}".format(what, H, W))
    return H, W


def export_depth(disp, H, W, *, disp_flipped=None, min_depth, max_depth, depth_scale=256.0, want=("depth16",), vmin=0.0, vmax=1.0):
    """disp (B,1,h,w) or (B,h,w) fp32 on the GPU -> {name: device tensor} for the names in `want` ("depth" (B,H,W) float32, "depth16"
    (B,H,W) uint16, "rgb" (B,H,W,3) uint8): one launch on the current stream, no host sync."""
    import torch
    want = tuple(want)
    if len(want) < 1 or any(name not in OUTPUTS for name in want):
        raise L.DynamoHipError("export_depth: `want` is a non-empty subset of {}, not {}".format(OUTPUTS, want))
    d = _device_planes(disp, "export_depth: disp")
    H, W = _size(H, W, "export_depth")
    r = mask = None
    if disp_flipped is not None:
        r = _device_planes(disp_flipped, "export_depth: disp_flipped")
        if r.shape != d.shape or r.device != d.device:
            raise L.DynamoHipError("export_depth: disp_flipped must have disp's shape and device")
        mask = _table("l_mask", d.shape[2], d.device)
    if not (float(min_depth) > 0 and float(max_depth) > 0):
        raise L.DynamoHipError("export_depth: min_depth and max_depth are positive")
    B, h, w = d.shape
    lib = L.load()
    dtypes = {"depth": ((B, H, W), torch.float32), "depth16": ((B, H, W), torch.uint16), "rgb": ((B, H, W, 3), torch.uint8)}
    with torch.cuda.device(d.device):
        out = {name: torch.empty(dtypes[name][0], dtype=dtypes[name][1], device=d.device) for name in want}
        lut = _table("lut", 0, d.device) if "rgb" in out else None
        L.check(lib.dd_export_depth(abi.ptr(d), abi.ptr(r), abi.ptr(mask), B, h, w, H, W, float(min_depth), float(max_depth), float(depth_scale),
                                    abi.ptr(lut), float(vmin), float(vmax), abi.ptr(out.get("depth")), abi.ptr(out.get("depth16")),
                                    abi.ptr(out.get("rgb")), L.current_stream()), "dd_export_depth")
    return out


def export_plane_u8(plane, H, W):
    """plane (B,1,h,w) or (B,h,w) fp32 on the GPU -> (B,H,W) uint8 on the GPU: one launch on the current stream, no host sync."""
    import torch
    p = _device_planes(plane, "export_plane_u8: plane")
    H, W = _size(H, W, "export_plane_u8")
    B, h, w = p.shape
    with torch.cuda.device(p.device):
        out = torch.empty((B, H, W), dtype=torch.uint8, device=p.device)
        L.check(L.load().dd_export_plane_u8(abi.ptr(p), B, h, w, H, W, abi.ptr(out), L.current_stream()), "dd_export_plane_u8")
    return out
