"""Motion masks from per-object contour lists (csrc/dd_contour_fill.hip): the definition on the host in numpy, the
fixed-size records the loader workers ship instead of the (H, W) mask, and the launch.

Replaces `cv2.drawContours(mask, contours, -1, label, -1)` of the reference's Waymo reader (datasets/waymo_dataset.py:109-118).
The contours come from cv2.findContours(..., CHAIN_APPROX_SIMPLE) on a binary mask: closed, integer vertices, every segment
between consecutive vertices (and from the last back to the first) horizontal, vertical or a 45 degree diagonal.  For such input the
fill is exact in integers:

  edge pixels of an object   every integer pixel on a segment of one of its contours (a one-vertex contour: that pixel)
  interior                   even-odd over ALL contours of the object: a non-horizontal segment with end rows y0, y1 crosses the rows
                             min(y0, y1) <= y < max(y0, y1) at its integer x on that row; (x, y) is inside when the number of crossings
                             of row y at x' <= x is odd
  covered                    interior or edge
  mask                       the label of the LAST object in file order that covers the pixel, 0 where none does

An `objects` list is [(label, [contour, ...]), ...] in file order, label in 1..255, a contour an (n, 2) integer array of (x, y)."""
import numpy as np

V_CAP = 16384                       # vertices per sample (the tiny_waymo frame: 4 307) -- 64 KB of int16 pairs
C_CAP = 256                         # contours per sample (the tiny_waymo frame: 43)
REC_WORDS = 6                       # first vertex, vertex count, object index, label, first row, last row
MAX_SIZE = 32768                    # int16 vertices address 0 .. 32767


class OverCap(Exception):
    """The sample has more vertices or contours than the fixed records hold: it travels as a host-filled mask."""


def _segments(contour, height, width, name):
    """(x0, y0, dx, dy) int64 of the closed contour's segments, validated."""
    pts = np.asarray(contour).reshape(-1, 2).astype(np.int64)
    if pts.shape[0] < 1:
        raise ValueError("{}: a contour without vertices".format(name))
    if pts[:, 0].min() < 0 or pts[:, 0].max() >= width or pts[:, 1].min() < 0 or pts[:, 1].max() >= height:
        raise ValueError("{}: contour vertex outside the {}x{} image".format(name, width, height))
    d = np.roll(pts, -1, axis=0) - pts
    if bool(((d[:, 0] != 0) & (d[:, 1] != 0) & (np.abs(d[:, 0]) != np.abs(d[:, 1]))).any()):
        raise ValueError("{}: contour segment that is neither axis-aligned nor a 45 degree diagonal".format(name))
    return pts[:, 0], pts[:, 1], d[:, 0], d[:, 1]


def _cover(contours, height, width, name):
    """(y_first, x_first, covered bool (h, w)) of one object over its bounding box, None for an object without contours."""
    segs = [_segments(c, height, width, name) for c in contours]
    if not segs:
        return None
    x0, y0, dx, dy = (np.concatenate([s[k] for s in segs]) for k in range(4))
    steps = np.maximum(np.abs(dx), np.abs(dy))
    seg = np.repeat(np.arange(steps.size), steps + 1)                       # every pixel of every segment, end points included
    t = np.arange(seg.size) - np.repeat(np.cumsum(steps + 1) - (steps + 1), steps + 1)
    xs, ys = x0[seg] + np.sign(dx[seg]) * t, y0[seg] + np.sign(dy[seg]) * t
    xa, ya = int(xs.min()), int(ys.min())
    h, w = int(ys.max()) - ya + 1, int(xs.max()) - xa + 1
    edge = np.zeros((h, w), dtype=bool)
    edge[ys - ya, xs - xa] = True
    # half open in y: a downward segment counts on its rows but the last, an upward one on its rows but the first
    cross = ((dy[seg] > 0) & (t < steps[seg])) | ((dy[seg] < 0) & (t > 0))
    toggles = np.bincount((ys[cross] - ya) * w + (xs[cross] - xa), minlength=h * w).reshape(h, w)
    inside = (np.cumsum(toggles, axis=1) & 1).astype(bool)
    return ya, xa, inside | edge


def fill_host(objects, height, width, name="contours"):
    """The (height, width) uint8 mask of the definition above."""
    mask = np.zeros((height, width), dtype=np.uint8)
    for label, contours in objects:
        if not 1 <= int(label) <= 255:
            raise ValueError("{}: object label {} outside 1..255".format(name, label))
        got = _cover(contours, height, width, name)
        if got is not None:
            ya, xa, covered = got
            view = mask[ya:ya + covered.shape[0], xa:xa + covered.shape[1]]
            view[covered] = label
    return mask


def pack(objects, height, width, name="contours", v_cap=V_CAP, c_cap=C_CAP):
    """(vertices (v_cap, 2) int16 [x, y], contours (c_cap, 6) int32) of one sample.  A record is [first vertex, vertex count, object
    index, label, first row, last row]; the used records come first, in file order (so the contours of one object are adjacent and
    the objects ascend), a count of 0 ends the list.  ValueError for a vertex outside the image or an off-direction segment,
    OverCap when the sample does not fit."""
    if not (1 <= height <= MAX_SIZE and 1 <= width <= MAX_SIZE):
        raise ValueError("{}: int16 vertices cannot address a {}x{} image".format(name, width, height))
    vertices = np.zeros((v_cap, 2), dtype=np.int16)
    records = np.zeros((c_cap, REC_WORDS), dtype=np.int32)
    nv = nc = 0
    for index, (label, contours) in enumerate(objects):
        if not 1 <= int(label) <= 255:
            raise ValueError("{}: object label {} outside 1..255".format(name, label))
        for contour in contours:
            x, y, _, _ = _segments(contour, height, width, name)
            if nc == c_cap or nv + x.size > v_cap:
                raise OverCap(name)
            vertices[nv:nv + x.size, 0], vertices[nv:nv + x.size, 1] = x, y
            records[nc] = (nv, x.size, index, label, y.min(), y.max())
            nv, nc = nv + x.size, nc + 1
    return vertices, records


def unpack(vertices, records):
    """The objects that hold a contour, from one sample's records: [(label, [contour (n, 2) int32, ...]), ...]."""
    objects, last = [], None
    for first, count, index, label, _, _ in np.asarray(records).tolist():
        if count == 0:
            break
        if index != last:
            objects.append((label, []))
            last = index
        objects[-1][1].append(np.asarray(vertices)[first:first + count].astype(np.int32))
    return objects


def fill_contours(vertices, contours, H, W, out=None):
    """vertices (B, v_cap, 2) int16 and contours (B, c_cap, 6) int32 on the GPU (`pack`, collated) -> (B, H, W) uint8 masks: one
    launch on the current stream, no host sync; every byte of `out` is written."""
    import torch

    from . import abi
    from . import lib as L
    if not (vertices.is_cuda and contours.is_cuda and vertices.dtype == torch.int16 and contours.dtype == torch.int32 and vertices.dim() == 3
            and contours.dim() == 3 and vertices.shape[2] == 2 and contours.shape[2] == REC_WORDS and vertices.shape[0] == contours.shape[0]):
        raise L.DynamoHipError("fill_contours takes (B, v_cap, 2) int16 vertices and (B, c_cap, {}) int32 contour records on the GPU".format(REC_WORDS))
    vertices, contours = vertices.contiguous(), contours.contiguous()
    B = int(vertices.shape[0])
    if out is None:
        out = torch.empty((B, H, W), dtype=torch.uint8, device=vertices.device)
    elif not (out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and tuple(out.shape) == (B, H, W)):
        raise L.DynamoHipError("fill_contours: out must be a contiguous (B, H, W) uint8 tensor on the GPU")
    L.check(L.load().dd_fill_contours(abi.ptr(vertices), int(vertices.shape[1]), abi.ptr(contours), int(contours.shape[1]), B, H, W, abi.ptr(out),
                                      L.current_stream()), "dd_fill_contours")
    return out


_CODE_DX = (1, 1, 0, -1, -1, -1, 0, 1)
_CODE_DY = (0, -1, -1, -1, 0, 1, 1, 1)
_NBD, _RIGHT = 2, -126              # the marks of a followed border pixel; _RIGHT where the border leaves it to the right


def _follow(buf, start, step, x, y, is_hole):
    """One border of Suzuki and Abe's algorithm from buf[start] = pixel (x, y), 8-connected, marked as it goes: its vertices, those
    where the direction changes, in the order it is walked."""
    deltas = tuple(dx + dy * step for dx, dy in zip(_CODE_DX, _CODE_DY)) * 2
    out = []
    s_end = s = 0 if is_hole else 4
    while True:                                                 # the first neighbour, clockwise from the side the scan came from
        s = (s - 1) & 7
        i1 = start + deltas[s]
        if buf[i1] != 0 or s == s_end:
            break
    if s == s_end:                                              # an isolated pixel
        buf[start] = _RIGHT
        out.append((x, y))
        return out
    i3, prev_s = start, s ^ 4
    while True:
        s_end = s
        while True:                                             # counter-clockwise to the next border pixel
            s += 1
            i4 = i3 + deltas[s]
            if buf[i4] != 0:
                break
        s &= 7
        if s - 1 < s_end and s >= 1:                            # unsigned(s - 1) < unsigned(s_end): the pixel to the right was passed over
            buf[i3] = _RIGHT
        elif buf[i3] == 1:
            buf[i3] = _NBD
        if s != prev_s:
            out.append((x, y))
            prev_s = s
        x, y = x + _CODE_DX[s], y + _CODE_DY[s]
        if i4 == start and i3 == i1:
            return out
        i3 = i4
        s = (s + 4) & 7


def trace(mask):
    """`cv2.findContours(mask, cv2.RETR_TREE, cv2.CHAIN_APPROX_SIMPLE)[0]` without cv2: the outer and the hole borders of the
    8-connected non-zero pixels of a (H, W) or (H, W, 1) mask by Suzuki and Abe's border following, as a list of (n, 1, 2) int32
    arrays of [x, y] vertices, kept only where the direction changes.  An outer border starts at its first pixel in raster order
    and runs counter-clockwise on the screen (y down), a hole border at the foreground pixel left of the hole's first pixel, and
    runs clockwise.  The contours come in the order the raster scan meets them (cv2 lists the same contours in another order;
    `fill_host` and dd_fill_contours are even-odd over all of them).  Only the bounding box of the non-zero pixels, with one pixel
    of margin, is visited."""
    m = np.asarray(mask)
    if m.ndim == 3 and m.shape[2] == 1:
        m = m[:, :, 0]
    if m.ndim != 2:
        raise ValueError("trace takes a (H, W) or (H, W, 1) mask")
    fg = m != 0
    rows, cols = np.flatnonzero(fg.any(axis=1)), np.flatnonzero(fg.any(axis=0))
    if rows.size == 0:
        return []
    ya, xa = int(rows[0]), int(cols[0])
    box = fg[ya:int(rows[-1]) + 1, xa:int(cols[-1]) + 1]
    h, w = box.shape
    step = w + 2
    img = np.zeros((h + 2, step), dtype=np.int8)
    img[1:-1, 1:-1] = box
    buf = img.reshape(-1).tolist()
    found = []
    for y in range(1, h + 1):
        base, prev = y * step, 0
        for x in range(1, step):
            p = buf[base + x]
            if p == prev:
                continue
            if prev == 0 and p == 1:
                found.append(_follow(buf, base + x, step, x, y, False))
                p = buf[base + x]                               # the scan goes on from the mark it has just been given
            elif p == 0 and prev >= 1:
                found.append(_follow(buf, base + x - 1, step, x - 1, y, True))
            prev = p
    off = np.array([xa - 1, ya - 1], dtype=np.int32)
    return [(np.array(c, dtype=np.int32) + off).reshape(-1, 1, 2) for c in found]
