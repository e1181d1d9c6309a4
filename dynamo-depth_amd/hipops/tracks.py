"""Objects linked into tracks across frames (csrc/dd_tracks.hip): the definition of the link on the host in numpy, the
wrapper of the three-launch entry point, the host logic that turns links into tracks, the track image and what goes to JSON.

hipops/objects.py numbers the moving objects of every frame on their own.  The network already predicts where every pixel of frame i
lies in the frame in front of it: complete_flow carries the pixel's 3-D point into the camera of frame i-1 (the reference's
`sample_complete` is the projection of that point).  The link is a vote of these correspondences between two label maps, no matcher
of its own.  Everything is at the NETWORK's resolution h x w, in fp32, every operation rounded on its own; the camera convention is the
clouds' (hipops/cloud.py): x right, y down, z forward, integer pixel coordinates, intrinsics (fx, fy, cx, cy) in pixels of h x w.

  inputs      labels_src, labels_dst (B,h,w) int32: the object numbers of frame i and of its predecessor;  disp, disp_flipped as
              objects.py;  complete_flow (B,3,h,w) and ts (B,) of the gap to the predecessor;  lo, span from export.depth_params;
              M = max_objects, 1 <= M <= MAX_OBJECTS = 1024.  No pose: p + c is already in the predecessor's camera.
  per pixel   (b, y, x) with a = labels_src[b,y,x] in 1..M:  d = disp[y, x], or with `disp_flipped` export.py's fuse_host;
              s = lo + span * d;  z = 1 / s (IEEE);  xc = ((float)x - cx) * ifx, yc = ((float)y - cy) * ify with cloud.inverse_focal;
              p = (xc * z, yc * z, z);  c_k = complete_flow[b,k,y,x] * ts[b];  m_k = p_k + c_k;  un = m0 / m2, vn = m1 / m2 (IEEE);
              u = fx * un + cx, v = fy * vn + cy: the product rounded, then the sum;  uf = floorf(u + 0.5f), vf = floorf(v + 0.5f);
              inside = m2 > 0 and 0 <= uf <= w-1 and 0 <= vf <= h-1, compared in fp32, every comparison false for NaN.
              col = M+1 when not inside; otherwise t = labels_dst[b, (int)vf, (int)uf] and col = t if t is in 1..M, else 0.  The
              conversion to int happens only behind the range test (and is checked once more as an integer: for w - 1 above 2^24
              (float)(w-1) may lie above w - 1).
              A source label outside 1..M votes nowhere; a destination label outside 0..M counts as background.
  votes       (B, M, M+2) int32: votes[b, a-1, col] = the number of such pixels.  Column 0 is background, columns 1..M are the
              predecessor's objects, column M+1 is outside the image or behind the camera.
  links       (B, M, LINK = 6) int32 per row: dst, votes, dst2, votes2, background, outside.  dst is the smallest column in 1..M that
              holds the row's largest count over those columns if that count is positive, otherwise 0 with votes 0; dst2 the same
              over the columns other than dst; background and outside are the row's columns 0 and M+1.  Rows of numbers no pixel
              carries are zero.

  tracks      `TrackBuilder`, on the host in float64, fed frame by frame.  The first frame opens one track per object, ids 1, 2, ... in
              object order.  For a later frame its objects are visited by decreasing primary votes, ties by smaller object number.
              Object a is eligible for the predecessor's object d when d >= 1 and iou = votes / (pixels_a + pixels_d - votes) >= min_iou
              (the denominator is at least pixels_d >= 1, for votes <= pixels_a).  If a is eligible for dst and no object of this frame
              has claimed dst, a continues dst's track and claims it; otherwise the same test is made with (dst2, votes2).  The objects
              left over open new tracks afterwards, in increasing object number.  A track that no object continues ends: there is no
              re-identification after a gap.
  position    G_i . centroid in float64, with G from cloud.chain_poses (frame i -> the first interior frame); path_length is the sum
              of the distances between consecutive positions (a position that is not finite adds nothing).
  track image `track_image`: the 16-bit label image of objects.labels_u16 through a look-up table object number -> track id,
              0 for background, ids above 65535 saturate."""
import numpy as np

from . import abi
from . import lib as L
from .cloud import inverse_focal
from .export import _device_planes, _planes, _table, depth_params, fuse_host

_f32 = np.float32
LINK = abi.DD_TRACKS_LINK
MAX_OBJECTS = abi.DD_TRACKS_MAX_OBJECTS
DEFAULT_MIN_IOU = 0.25
GAP_NOTE = "a track that no object of the next frame continues ends there: an object that comes back after a gap opens a new track"
POSITION_NOTE = "position is the object's centroid in the camera coordinates of the first interior frame (the chained poses of poses.txt)"


def _cap(max_objects, error=ValueError):
    if not 1 <= int(max_objects) <= MAX_OBJECTS:
        raise error("tracks: max_objects is between 1 and {}, not {}".format(MAX_OBJECTS, max_objects))
    return int(max_objects)


def columns_host(labels_dst, disp, complete_flow, ts, intrinsics, *, disp_flipped=None, min_depth, max_depth, max_objects=256):
    """The per-pixel part of the definition at EVERY pixel: (B,h,w) int64, the column the pixel votes for if its source label is in 1..M."""
    M = _cap(max_objects)
    dst = np.asarray(labels_dst)
    d = _planes(disp, "disp")
    B, h, w = d.shape
    flow, ts = np.asarray(complete_flow, dtype=np.float32), np.asarray(ts, dtype=np.float32).reshape(-1)
    if dst.shape != d.shape or flow.shape != (B, 3, h, w) or ts.shape != (B,):
        raise ValueError("tracks: labels as disp, complete_flow (B, 3, h, w), ts (B,)")
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
        c = (flow * ts[:, None, None, None]).astype(np.float32)
        m0 = ((xc * z).astype(np.float32) + c[:, 0]).astype(np.float32)
        m1 = ((yc * z).astype(np.float32) + c[:, 1]).astype(np.float32)
        m2 = (z + c[:, 2]).astype(np.float32)
        un, vn = (m0 / m2).astype(np.float32), (m1 / m2).astype(np.float32)
        u = ((fx * un).astype(np.float32) + cx).astype(np.float32)
        v = ((fy * vn).astype(np.float32) + cy).astype(np.float32)
        uf, vf = np.floor((u + _f32(0.5)).astype(np.float32)), np.floor((v + _f32(0.5)).astype(np.float32))
        inside = (m2 > 0) & (uf >= 0) & (uf <= _f32(w - 1)) & (vf >= 0) & (vf <= _f32(h - 1))
        ui, vi = np.where(inside, uf, 0).astype(np.int64), np.where(inside, vf, 0).astype(np.int64)
    inside &= (ui < w) & (vi < h)
    ui, vi = np.where(inside, ui, 0), np.where(inside, vi, 0)
    t = dst[np.arange(B)[:, None, None], vi, ui].astype(np.int64)
    return np.where(inside, np.where((t >= 1) & (t <= M), t, 0), M + 1)


def links_from_votes(votes):
    """votes (B, M, M+2) -> links (B, M, LINK) int32: the definition's selection."""
    votes = np.asarray(votes)
    B, M, cols = votes.shape
    if cols != M + 2:
        raise ValueError("votes is (B, M, M + 2)")
    links = np.zeros((B, M, LINK), dtype=np.int32)
    v = votes[:, :, 1:M + 1].astype(np.int64)
    rows = np.arange(M)[None, :]
    batch = np.arange(B)[:, None]
    first = v.argmax(axis=2)                # the first of equal counts: the smallest column
    best = v[batch, rows, first]
    links[:, :, 0] = np.where(best > 0, first + 1, 0)
    links[:, :, 1] = np.where(best > 0, best, 0)
    rest = v.copy()
    rest[batch, rows, first] = np.where(best > 0, -1, rest[batch, rows, first])         # the columns other than dst
    second = rest.argmax(axis=2)
    count = rest[batch, rows, second]
    links[:, :, 2] = np.where(count > 0, second + 1, 0)
    links[:, :, 3] = np.where(count > 0, count, 0)
    links[:, :, 4] = votes[:, :, 0]
    links[:, :, 5] = votes[:, :, M + 1]
    return links


def link_host(labels_src, labels_dst, disp, complete_flow, ts, intrinsics, *, disp_flipped=None, min_depth, max_depth, max_objects=256):
    """The definition above in numpy: (votes (B,M,M+2) int32, links (B,M,LINK) int32)."""
    M = _cap(max_objects)
    src = np.asarray(labels_src).astype(np.int64)
    col = columns_host(labels_dst, disp, complete_flow, ts, intrinsics, disp_flipped=disp_flipped, min_depth=min_depth, max_depth=max_depth, max_objects=M)
    if src.shape != col.shape:
        raise ValueError("tracks: labels_src must have disp's shape")
    B = src.shape[0]
    votes = np.zeros((B, M, M + 2), dtype=np.int32)
    for b in range(B):
        act = (src[b] >= 1) & (src[b] <= M)
        votes[b] = np.bincount((src[b][act] - 1) * (M + 2) + col[b][act], minlength=M * (M + 2)).reshape(M, M + 2)
    return votes, links_from_votes(votes)


# ---- device --------------------------------------------------------------------------------------------------------------------------
def link_objects(labels_src, labels_dst, disp, complete_flow, ts, intrinsics, *, disp_flipped=None, min_depth, max_depth, max_objects=256):
    """labels_src, labels_dst (B,h,w) int32, disp (B,1,h,w) or (B,h,w), complete_flow (B,3,h,w), ts (B,) or (B,1), optional disp_flipped,
    fp32, all on one GPU -> (votes (B,M,M+2) int32, links (B,M,LINK) int32) on the GPU.  A memset and two launches on the current
    stream, no host sync."""
    import torch
    M = _cap(max_objects, L.DynamoHipError)
    d = _device_planes(disp, "link_objects: disp")
    B, h, w = d.shape

    def typed(t, dtype, shapes, what):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == dtype and t.device == d.device and tuple(t.shape) in shapes):
            raise L.DynamoHipError("link_objects: {} must be a {} tensor of shape {} on disp's device".format(what, dtype, " or ".join(str(s) for s in shapes)))
        return t

    src = typed(labels_src, torch.int32, ((B, h, w),), "labels_src").contiguous()
    dst = typed(labels_dst, torch.int32, ((B, h, w),), "labels_dst").contiguous()
    r = lmask = None
    if disp_flipped is not None:
        r = _device_planes(disp_flipped, "link_objects: disp_flipped")
        if r.shape != d.shape or r.device != d.device:
            raise L.DynamoHipError("link_objects: disp_flipped must have disp's shape and device")
        lmask = _table("l_mask", w, d.device)
    flow = typed(complete_flow, torch.float32, ((B, 3, h, w),), "complete_flow").contiguous()
    ts = typed(ts, torch.float32, ((B,), (B, 1)), "ts").reshape(B).contiguous()
    fx, fy, cx, cy = (float(v) for v in intrinsics)
    if not (np.isfinite(fx) and np.isfinite(fy) and _f32(fx) != 0 and _f32(fy) != 0):
        raise L.DynamoHipError("link_objects: fx and fy are finite and not zero")
    if not (float(min_depth) > 0 and float(max_depth) > 0):
        raise L.DynamoHipError("link_objects: min_depth and max_depth are positive")
    if B * h * w > 2 ** 31 - 1 or B * M * (M + 2) > 2 ** 31 - 1:
        raise L.DynamoHipError("link_objects: {} x {} x {} with {} objects is more than one call takes".format(B, h, w, M))
    lo, span = depth_params(min_depth, max_depth)
    lib = L.load()
    with torch.cuda.device(d.device):
        votes = torch.empty((B, M, M + 2), dtype=torch.int32, device=d.device)
        links = torch.empty((B, M, LINK), dtype=torch.int32, device=d.device)
        L.check(lib.dd_tracks_link(abi.ptr(src), abi.ptr(dst), abi.ptr(d), abi.ptr(r), abi.ptr(lmask), abi.ptr(flow), abi.ptr(ts), B, h, w, fx, fy, cx, cy,
                                   float(lo), float(span), M, abi.ptr(votes), abi.ptr(links), L.current_stream()), "dd_tracks_link")
    return votes, links


# ---- tracks --------------------------------------------------------------------------------------------------------------------------
def _position(G, centroid):
    if any(v is None for v in centroid):
        return [None, None, None]
    p = np.asarray(G, dtype=np.float64).reshape(4, 4) @ np.array([centroid[0], centroid[1], centroid[2], 1.0], dtype=np.float64)
    return [float(v) if np.isfinite(v) else None for v in p[:3]]


class TrackBuilder:
    """The host logic of the module's docstring.  `add` takes the frames in order; `tracks` is the result so far."""

    def __init__(self, min_iou=DEFAULT_MIN_IOU):
        self.min_iou = float(min_iou)
        self.tracks = []                # {"id", "frames": [...]} in id order
        self.accepted = self.refused = 0
        self._prev = []                 # per object of the frame before: (track id, pixels)

    def _open(self, entry):
        self.tracks.append({"id": len(self.tracks) + 1, "frames": [entry]})
        return len(self.tracks)

    def add(self, stem, objects, links, G):
        """stem; `objects`: the frame's list of objects.unpack_table; `links`: the frame's (M, LINK) rows, None for a frame without a
        predecessor (the drive's first interior frame); G (4,4): the frame -> the first interior frame.  Returns the track id of every
        object, in object order."""
        n = len(objects)
        entries = [{"stem": stem, "object": o["id"], "pixels": o["pixels"], "box": o["box"], "centroid": o["centroid"], "position": _position(G, o["centroid"]),
                    "motion": o["motion"], "speed": o["speed"], "confidence": o["confidence"], "iou": None} for o in objects]
        ids = [0] * n
        if links is not None and self._prev:
            rows = np.asarray(links).reshape(-1, LINK)
            if rows.shape[0] < n:
                raise ValueError("tracks: {} objects but {} rows of links".format(n, rows.shape[0]))
            claimed = set()
            for a in sorted(range(n), key=lambda k: (-int(rows[k, 1]), k)):
                pixels = int(objects[a]["pixels"])
                for d, votes in ((int(rows[a, 0]), int(rows[a, 1])), (int(rows[a, 2]), int(rows[a, 3]))):
                    if d < 1 or d > len(self._prev) or d in claimed:
                        continue
                    iou = votes / float(pixels + self._prev[d - 1][1] - votes)
                    if iou >= self.min_iou:
                        claimed.add(d)
                        ids[a] = self._prev[d - 1][0]
                        entries[a]["iou"] = iou
                        self.tracks[ids[a] - 1]["frames"].append(entries[a])
                        break
                if ids[a]:
                    self.accepted += 1
                elif int(rows[a, 0]) >= 1:
                    self.refused += 1
        for a in range(n):
            if not ids[a]:
                ids[a] = self._open(entries[a])
        self._prev = [(ids[a], int(objects[a]["pixels"])) for a in range(n)]
        return ids

    def summary(self):
        """One record per track: id, first, last, length, path_length, frames."""
        out = []
        for t in self.tracks:
            frames = t["frames"]
            path = 0.0
            for p, q in zip(frames[:-1], frames[1:]):
                if None not in p["position"] and None not in q["position"]:
                    path += float(np.sqrt(sum((float(u) - float(v)) ** 2 for u, v in zip(p["position"], q["position"]))))
            out.append({"id": t["id"], "first": frames[0]["stem"], "last": frames[-1]["stem"], "length": len(frames), "path_length": path, "frames": frames})
        return out


def track_image(labels16, ids):
    """labels16: a uint16 label image of objects.labels_u16 (any shape); ids: the track id of object 1, 2, ...  -> the image with every
    object number replaced by its track id (saturated at 65535), 0 for background and for numbers past the list."""
    labels16 = np.asarray(labels16)
    if labels16.dtype != np.uint16:
        raise ValueError("track_image takes a uint16 label image")
    lut = np.zeros(65536, dtype=np.uint16)
    ids = np.asarray(list(ids), dtype=np.int64)[:65535]
    lut[1:len(ids) + 1] = np.clip(ids, 0, 65535).astype(np.uint16)
    return lut[labels16]


def tracks_json(builder, params, notes=()):
    """What goes to tracks.json: the parameters, the conventions, the notes and the tracks."""
    tracks = builder.summary()
    return {"parameters": dict(params), "convention": "x right, y down, z forward; pixel centres at integer coordinates; boxes in source pixels, inclusive",
            "notes": list(notes) + [POSITION_NOTE, GAP_NOTE], "count": len(tracks), "longest": max([t["length"] for t in tracks], default=0),
            "links_accepted": builder.accepted, "links_refused": builder.refused, "tracks": tracks}
