"""Coloured point clouds (csrc/dd_cloud.hip): the definition on the host in numpy, the three-launch wrapper, and the PLY
reader and writer.

The depth of `hipops.export` at the source image's H x W, back-projected through a pinhole camera, filtered, optionally moved by a
rigid pose and written as the 16-byte vertex records of a binary PLY file.  The camera convention is that of the reference's
tools.BackprojectDepth: x right, y down, z forward, integer pixel coordinates (the centre of the upper-left pixel is (0, 0)).
Geometry is at the SOURCE resolution; colours come from the NETWORK-resolution frame (B,3,h,w) that is on the device anyway, sampled
with the same bilinear taps -- a cloud's colours are as sharp as the network's input, not as the file the frame came from.

Candidates are the pixels (Y, X) of the H x W frame with Y % stride == 0 and X % stride == 0.  Per candidate of frame b, every
operation in fp32 and none fused:

  taps    dm_tap (csrc/dd_bilinear.h) of Y and of X exactly as `export_depth_host`: (y0, y1, wy), (x0, x1, wx).  The four disparity taps
          d are disp[y, x], or with `disp_flipped` the `fuse` step of hipops/export.py;  s = lo + span * d with `depth_params`.
  depth   u = dm_blend(wy, wx, s00, s01, s10, s11), depth = 1 / u (IEEE): the number dd_export_depth writes.
  keep    all of: depth > 0 && depth <= max_range (both false for NaN);
          with edge > 0: (smax - smin) <= edge * smin, smax = fmaxf and smin = fminf over the four s taps dm_tap names, whatever their
          weights -- it drops the "flying pixels" a bilinear blend across a depth discontinuity creates;
          with a motion mask: dm_blend(mask taps) < motion_thresh (false for NaN).
  point   xc = ((float)X - cx) * ifx, yc = ((float)Y - cy) * ify with ifx = 1 / fx, ify = 1 / fy evaluated in float64 on the fp32 value
          and rounded to fp32 once;  p = (xc * depth, yc * depth, depth).
  pose    only when given, (B,3,4) = [R | t] per frame: p'_k = ((R[k,0] * x + R[k,1] * y) + R[k,2] * z) + t[k], left to right.
  colour  per channel vis_unit_byte(dm_blend(colour taps)) = (uint8)(fminf(fmaxf(v, 0), 1) * 255).
  record  16 bytes: x, y, z as little-endian floats, then r, g, b, 255.
  order   the kept candidates of frame 0 in row-major (Y, X) order, then frame 1, ...; offsets (B+1) int64 are the prefix counts.

PLY files: `ply_header` is the header, byte for byte; `write_ply` / `read_ply` write and read the records; `ScenePly` appends
records and fills the count in at the end (its header's length does not depend on the count)."""
import numpy as np

from . import abi
from . import lib as L
from .export import _device_planes, _planes, _size, _table, _taps, depth_params, fuse_host

_f32 = np.float32
RECORD = 16
CONVENTION = "camera coordinates: x right, y down, z forward; depth is up to scale (one unknown factor per model)"
COUNT_DIGITS = 20           # a fixed-length header leaves room for every int64 count
PROPERTIES = ("property float x", "property float y", "property float z", "property uchar red", "property uchar green", "property uchar blue",
              "property uchar alpha")


def _blend_at(v, ty, tx):
    """dm_blend of (..., h, w) fp32 at the taps ty = (y0, y1, wy), tx = (x0, x1, wx) -> (..., len(y0), len(x0)) fp32."""
    (y0, y1, wy), (x0, x1, wx) = ty, tx
    wy, wx = wy[:, None], wx[None, :]
    one = _f32(1)
    top = (one - wx) * v[..., y0, :][..., x0] + wx * v[..., y0, :][..., x1]
    bot = (one - wx) * v[..., y1, :][..., x0] + wx * v[..., y1, :][..., x1]
    return ((one - wy) * top + wy * bot).astype(np.float32)


def inverse_focal(f):
    """1 / f in float64 on the fp32 value, rounded to fp32 once."""
    return _f32(1.0 / float(_f32(f)))


def cloud_candidates_host(disp, color, H, W, intrinsics, *, disp_flipped=None, motion_mask=None, pose=None, min_depth, max_depth, max_range=None,
                          edge=0.05, motion_thresh=0.5, stride=1):
    """The definition above per candidate, before the compaction: (keep (B,Hc,Wc) bool, xyz (B,Hc,Wc,3) float32, rgb (B,Hc,Wc,3) uint8)
    with Hc = ceil(H / stride), Wc = ceil(W / stride).  intrinsics = (fx, fy, cx, cy) in pixels of the H x W frame; max_range None:
    max_depth."""
    H, W, stride = int(H), int(W), int(stride)
    if H < 1 or W < 1 or stride < 1:
        raise ValueError("export_cloud_host needs H, W, stride >= 1")
    d = _planes(disp, "disp")
    B, h, w = d.shape
    color = np.asarray(color, dtype=np.float32)
    if color.shape != (B, 3, h, w):
        raise ValueError("color must be (B, 3, h, w) with disp's B, h, w")
    fx, fy, cx, cy = (_f32(v) for v in intrinsics)
    max_range = _f32(max_depth if max_range is None else max_range)
    edge, thresh = _f32(edge), _f32(motion_thresh)
    ty = tuple(a[::stride] for a in _taps(H, h))
    tx = tuple(a[::stride] for a in _taps(W, w))
    with np.errstate(all="ignore"):
        if disp_flipped is not None:
            r = _planes(disp_flipped, "disp_flipped")
            if r.shape != d.shape:
                raise ValueError("disp_flipped must have disp's shape")
            d = fuse_host(d, r)
        lo, span = depth_params(min_depth, max_depth)
        s = (lo + span * d).astype(np.float32)
        depth = (_f32(1) / _blend_at(s, ty, tx)).astype(np.float32)
        keep = (depth > 0) & (depth <= max_range)
        if edge > 0:
            taps = [s[:, yy, :][:, :, xx] for yy in ty[:2] for xx in tx[:2]]
            smax, smin = np.fmax.reduce(taps), np.fmin.reduce(taps)
            keep &= (smax - smin).astype(np.float32) <= (edge * smin).astype(np.float32)
        if motion_mask is not None:
            m = _planes(motion_mask, "motion_mask")
            if m.shape != d.shape:
                raise ValueError("motion_mask must have disp's shape")
            keep &= _blend_at(m, ty, tx) < thresh
        Y = (np.arange(H)[::stride]).astype(np.float32)[None, :, None]
        X = (np.arange(W)[::stride]).astype(np.float32)[None, None, :]
        xc = ((X - cx) * inverse_focal(fx)).astype(np.float32)
        yc = ((Y - cy) * inverse_focal(fy)).astype(np.float32)
        p = [(xc * depth).astype(np.float32), (yc * depth).astype(np.float32), depth]
        if pose is not None:
            T = np.asarray(pose, dtype=np.float32)
            if T.shape != (B, 3, 4):
                raise ValueError("pose must be (B, 3, 4)")
            T = T[:, :, :, None, None]
            p = [(((T[:, k, 0] * p[0] + T[:, k, 1] * p[1]) + T[:, k, 2] * p[2]) + T[:, k, 3]).astype(np.float32) for k in range(3)]
        rgb = _blend_at(color, ty, tx)
        rgb = (np.fmin(np.fmax(rgb, _f32(0)), _f32(1)) * _f32(255)).astype(np.uint8)
    return keep, np.stack(np.broadcast_arrays(*p), axis=-1), np.ascontiguousarray(np.moveaxis(rgb, 1, -1))


def export_cloud_host(disp, color, H, W, intrinsics, **kwargs):
    """The definition above in numpy, `cloud_candidates_host` compacted: (records (n,16) uint8, offsets (B+1,) int64)."""
    keep, xyz, rgb = cloud_candidates_host(disp, color, H, W, intrinsics, **kwargs)
    B = keep.shape[0]
    offsets = np.zeros(B + 1, dtype=np.int64)
    offsets[1:] = np.cumsum(keep.reshape(B, -1).sum(axis=1))
    records = np.empty((int(offsets[B]), RECORD), dtype=np.uint8)
    records[:, :12] = np.ascontiguousarray(xyz[keep].astype("<f4")).view(np.uint8).reshape(-1, 12)       # boolean indexing walks (b, Y, X) in row-major order
    records[:, 12:15] = rgb[keep]
    records[:, 15] = 255
    return records, offsets


# ---- the scene's poses --------------------------------------------------------------------------------------------------------------
def chain_poses(transforms, start=None):
    """transforms (n,4,4): frame i -> its predecessor (predict_batch's fp32 "cam_T_cam").  Returns (n,4,4) float64, frame i -> the first
    frame of the chain: G_i = G_{i-1} . T_i, accumulated in float64.  `start` None: frame 0 opens the chain, G_0 = I whatever T_0 says;
    otherwise `start` is the G of the frame in front of frame 0 (the last one of the previous batch)."""
    T = np.asarray(transforms, dtype=np.float64).reshape(-1, 4, 4)
    G = np.empty_like(T)
    prev = None if start is None else np.asarray(start, dtype=np.float64)
    for i in range(T.shape[0]):
        prev = np.eye(4) if prev is None else prev @ T[i]
        G[i] = prev
    return G


# ---- PLY -----------------------------------------------------------------------------------------------------------------------------
def ply_header(count, fixed=False):
    """The header of a cloud file as bytes.  With `fixed`, a second comment line of COUNT_DIGITS - len(str(count)) dashes stands behind
    the first: the header's length is then the same for every count, so the count can be filled in after the records are written."""
    count = int(count)
    if count < 0 or len(str(count)) > COUNT_DIGITS:
        raise ValueError("a PLY count is between 0 and 10**{} - 1".format(COUNT_DIGITS))
    lines = ["ply", "format binary_little_endian 1.0", "comment " + CONVENTION]
    if fixed:
        lines.append("comment " + "-" * (COUNT_DIGITS - len(str(count))))
    lines += ["element vertex {}".format(count)] + list(PROPERTIES) + ["end_header"]
    return ("\n".join(lines) + "\n").encode("ascii")


def _record_bytes(records):
    if isinstance(records, (bytes, bytearray, memoryview)):
        data = memoryview(records).cast("B")
    else:
        r = np.ascontiguousarray(records)
        if r.dtype != np.uint8 or (r.ndim == 2 and r.shape[1] != RECORD) or r.ndim > 2:
            raise ValueError("records are (n, 16) uint8")
        data = memoryview(r.reshape(-1))
    if len(data) % RECORD:
        raise ValueError("records are 16 bytes each")
    return data


def write_ply(path, records, fixed=False):
    """Header + the records' bytes as they are ((n,16) uint8, or a bytes-like slice of them): nothing is interleaved here."""
    data = _record_bytes(records)
    with open(path, "wb") as fh:
        fh.write(ply_header(len(data) // RECORD, fixed))
        fh.write(data)
    return path


class ScenePly:
    """A cloud file written once, front to back: the fixed-length header with a count of 0, the records as they come, and on close the
    header again with the count."""

    def __init__(self, path):
        self.path, self.count = path, 0
        self._fh = open(path, "wb")
        self._fh.write(ply_header(0, fixed=True))

    def append(self, records):
        data = _record_bytes(records)
        self._fh.write(data)
        self.count += len(data) // RECORD

    def close(self):
        if self._fh is not None:
            self._fh.seek(0)
            self._fh.write(ply_header(self.count, fixed=True))
            self._fh.close()
            self._fh = None
        return self.path

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def unpack_records(records):
    """(n,16) uint8 -> (xyz (n,3) float32, rgba (n,4) uint8)."""
    r = np.ascontiguousarray(records, dtype=np.uint8).reshape(-1, RECORD)
    return r[:, :12].copy().view("<f4").astype(np.float32).reshape(-1, 3), r[:, 12:].copy()


def read_ply(path):
    """A file `write_ply` or `ScenePly` wrote -> (xyz (n,3) float32, rgba (n,4) uint8, records (n,16) uint8).  Any other vertex layout
    is refused: this is no general PLY reader."""
    with open(path, "rb") as fh:
        raw = fh.read()
    end = raw.find(b"end_header\n")
    if not raw.startswith(b"ply\n") or end < 0:
        raise ValueError("{}: not a PLY file".format(path))
    lines = raw[:end].decode("ascii").split("\n")[:-1]
    body = raw[end + len(b"end_header\n"):]
    rest = [ln for ln in lines[1:] if not ln.startswith("comment")]
    if len(rest) != 2 + len(PROPERTIES) or rest[0] != "format binary_little_endian 1.0" or not rest[1].startswith("element vertex ") or \
            tuple(rest[2:]) != PROPERTIES:
        raise ValueError("{}: not the vertex layout of hipops.cloud".format(path))
    count = int(rest[1].split()[2])
    if len(body) != count * RECORD:
        raise ValueError("{}: {} bytes behind the header, {} vertices declared".format(path, len(body), count))
    records = np.frombuffer(body, dtype=np.uint8).reshape(count, RECORD).copy()
    return unpack_records(records) + (records,)


# ---- device --------------------------------------------------------------------------------------------------------------------------
def candidates(B, H, W, stride):
    """The number of candidates of a call: what the records buffer has room for."""
    return int(B) * (-(-int(H) // int(stride))) * (-(-int(W) // int(stride)))


def export_cloud(disp, color, H, W, intrinsics, *, disp_flipped=None, motion_mask=None, pose=None, min_depth, max_depth, max_range=None,
                 edge=0.05, motion_thresh=0.5, stride=1):
    """disp (B,1,h,w) or (B,h,w), color (B,3,h,w), optional disp_flipped, motion_mask (as disp) and pose (B,3,4) or (B,4,4), fp32 on
    the GPU -> (records (candidates,16) uint8, offsets (B+1,) int64) on the GPU: the first offsets[B] records are the cloud, the rest of
    the buffer is left as allocated.  Three launches on the current stream, no host sync: the caller fetches `offsets` when it
    wants the counts."""
    import torch
    d = _device_planes(disp, "export_cloud: disp")
    H, W = _size(H, W, "export_cloud")
    B, h, w = d.shape
    stride = int(stride)
    if stride < 1:
        raise L.DynamoHipError("export_cloud: stride >= 1, not {}".format(stride))
    if not (torch.is_tensor(color) and color.is_cuda and color.dtype == torch.float32 and tuple(color.shape) == (B, 3, h, w) and color.device == d.device):
        raise L.DynamoHipError("export_cloud: color must be an fp32 (B, 3, h, w) tensor on disp's device")
    r = lmask = m = T = None
    if disp_flipped is not None:
        r = _device_planes(disp_flipped, "export_cloud: disp_flipped")
        if r.shape != d.shape or r.device != d.device:
            raise L.DynamoHipError("export_cloud: disp_flipped must have disp's shape and device")
        lmask = _table("l_mask", w, d.device)
    if motion_mask is not None:
        m = _device_planes(motion_mask, "export_cloud: motion_mask")
        if m.shape != d.shape or m.device != d.device:
            raise L.DynamoHipError("export_cloud: motion_mask must have disp's shape and device")
    if pose is not None:
        if not (torch.is_tensor(pose) and pose.is_cuda and pose.dtype == torch.float32 and pose.device == d.device and pose.dim() == 3
                and tuple(pose.shape) in ((B, 3, 4), (B, 4, 4))):
            raise L.DynamoHipError("export_cloud: pose must be an fp32 (B, 3, 4) or (B, 4, 4) tensor on disp's device")
        T = pose[:, :3].contiguous()
    fx, fy, cx, cy = (float(v) for v in intrinsics)
    if not (np.isfinite(fx) and np.isfinite(fy) and _f32(fx) != 0 and _f32(fy) != 0):
        raise L.DynamoHipError("export_cloud: fx and fy are finite and not zero")
    if not (float(min_depth) > 0 and float(max_depth) > 0):
        raise L.DynamoHipError("export_cloud: min_depth and max_depth are positive")
    max_range = float(max_depth if max_range is None else max_range)
    lib = L.load()
    need = lib.dd_export_cloud_workspace_bytes(B, H, W, stride)
    if need == 0:
        raise L.DynamoHipError("export_cloud: {} x {} x {} at stride {} is more than one call takes".format(B, H, W, stride))
    with torch.cuda.device(d.device):
        records = torch.empty((candidates(B, H, W, stride), RECORD), dtype=torch.uint8, device=d.device)
        offsets = torch.empty((B + 1,), dtype=torch.int64, device=d.device)
        ws = torch.empty((need // 8,), dtype=torch.int64, device=d.device)
        color = color.contiguous()
        L.check(lib.dd_export_cloud(abi.ptr(d), abi.ptr(r), abi.ptr(lmask), abi.ptr(color), abi.ptr(m), abi.ptr(T), B, h, w, H, W, fx, fy, cx, cy,
                                    float(min_depth), float(max_depth), max_range, float(edge), float(motion_thresh), stride, abi.ptr(records),
                                    abi.ptr(offsets), abi.ptr(ws), need, L.current_stream()), "dd_export_cloud")
    return records, offsets
