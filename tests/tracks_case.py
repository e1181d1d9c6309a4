"""What the track tests share (hipops/tracks.py, csrc/dd_tracks.hip): the cases -- label maps from the object tests' masks, flow fields
built from the definition (none knows the kernel's tiling), the caps -- and the cached host reference of every case.  Everything the
link computes is an integer: the device is held to `link_host` exactly."""
import functools

import numpy as np

import objects_case as OC

_f32 = np.float32
SHAPES = [(1, 1), (1, 70), (5, 7), (37, 53), (130, 67)]
assert all(s in OC.SHAPES for s in SHAPES)
B = OC.B
TS = np.array([0.1, 1.7], dtype=np.float32)
CAPS = (4, 256, 1024)
FLOWS = ("zero", "shift", "smooth", "outside", "behind", "nonfinite", "ties")
# (source mask, destination mask, connectivity): different masks and the same mask; the 4-connected checkerboard has thousands of
# one-pixel objects, so labels above every cap are present in a map
PAIRS = (("blobs", "blobs", 8), ("blobs", "rings", 8), ("checker", "blobs", 4), ("full", "checker", 4), ("empty", "full", 8), ("rings", "rings", 4),
         ("checker", "checker", 4))
TIE_PAIR = ("full", "checker", 4)       # ties: every pixel of image 0 votes, and neighbouring destination pixels carry different labels


@functools.lru_cache(maxsize=None)
def labels(shape, name, connectivity):
    """(B,h,w) int32: every component of the mask an object (min_pixels 1), under a cap none of them reaches."""
    from hipops.objects import label_components_host
    out, found, _ = label_components_host(OC.inputs(shape, name)["mask"], thresh=OC.THRESH, connectivity=connectivity, min_pixels=1, max_objects=OC.CAP)
    assert (found <= OC.CAP).all()
    out.setflags(write=False)
    return out


def depth(shape, disp):
    """z of the unfused disparity, float64: what the flow fields are built from."""
    from hipops.export import depth_params
    lo, span = depth_params(OC.MIN_DEPTH, OC.MAX_DEPTH)
    with np.errstate(all="ignore"):
        return 1.0 / (float(lo) + float(span) * disp[:, 0].astype(np.float64))


def _u(f, x, z, ts, fx, cx, ifx):
    """The definition's u at one pixel for the flow value f in channel 0 (channel 2 zero, so m2 = z), in fp32 scalars."""
    with np.errstate(all="ignore"):
        m0 = _f32(_f32(_f32(_f32(x) - cx) * ifx) * z) + _f32(_f32(f) * ts)
        return _f32(_f32(fx * _f32(_f32(m0) / z)) + cx)


def tie_flow(x, z, ts, fx, cx, ifx, k):
    """The smallest fp32 f with u(f) >= k - 0.5, found by np.nextafter steps from the real-valued solution (u does not decrease with f);
    (f, exact): exact where u(f) == k - 0.5, so that u + 0.5 is the integer k there and uf == k - 1 one step below."""
    target = _f32(k - 0.5)
    xc = (float(x) - float(cx)) * float(ifx)
    f = _f32(((float(target) - float(cx)) / float(fx) * float(z) - xc * float(z)) / float(ts))
    for _ in range(4096):
        if not _u(f, x, z, ts, fx, cx, ifx) >= target:
            break
        f = np.nextafter(f, _f32(-np.inf))
    for _ in range(8192):
        if _u(f, x, z, ts, fx, cx, ifx) >= target:
            return f, bool(_u(f, x, z, ts, fx, cx, ifx) == target)
        f = np.nextafter(f, _f32(np.inf))
    return f, False


def _smooth(h, w, salt):
    rng = np.random.default_rng(salt)
    yy, xx = np.mgrid[0:h, 0:w]
    a, b, c, d = rng.uniform(0.5, 2.5, 4)
    return np.sin(a * yy / max(h, 1) * 3 + b) * np.cos(c * xx / max(w, 1) * 3 + d)


def flow_field(shape, kind, disp):
    """(flow (B,3,h,w) fp32, info): c = flow * TS.  `info` of the ties case: the number of pixels where u + 0.5 is exactly an integer."""
    h, w = shape
    fx, fy, cx, cy = (_f32(v) for v in OC.intrinsics(h, w))
    z = depth(shape, disp)
    z = np.where(np.isfinite(z), z, 1.0)
    c = np.zeros((B, 3, h, w))
    info = 0
    if kind == "shift":                 # an integer pixel shift: c = shift * z / f
        for b, (sx, sy) in enumerate(((3, -2), (-1, 1))):
            c[b, 0], c[b, 1] = sx * z[b] / float(fx), sy * z[b] / float(fy)
    elif kind in ("smooth", "nonfinite"):
        for b in range(B):
            c[b, 0] = 4.0 * _smooth(h, w, 11 + b) * z[b] / float(fx)
            c[b, 1] = 3.0 * _smooth(h, w, 23 + b) * z[b] / float(fy)
            c[b, 2] = 0.2 * _smooth(h, w, 37 + b) * z[b]
    elif kind == "outside":
        c[0, 0] = (w + 10) * z[0] / float(fx)
        c[1, 1] = -(h + 10) * z[1] / float(fy)
    elif kind == "behind":              # m2 <= 0: well behind the camera, and at (or within a rounding of) zero
        c[0, 2] = -2.0 * z[0]
        c[1, 2] = -z[1]
        c[1, 0] = 0.5 * z[1] / float(fx)
    flow = (c / TS[:, None, None, None].astype(np.float64)).astype(np.float32)
    if kind == "nonfinite":
        flat = flow.reshape(B, 3, h * w)
        for b in range(B):
            for k in range(3):
                for j, value in enumerate((np.nan, np.inf, -np.inf)):
                    flat[b, k, (5 * k + 3 * j + 7 * b) % (h * w)] = value
    if kind == "ties":
        from hipops.cloud import inverse_focal
        from hipops.export import depth_params
        lo, span = depth_params(OC.MIN_DEPTH, OC.MAX_DEPTH)
        ifx = inverse_focal(fx)
        targets = (-1, 0, w - 1, w, w // 2)
        n = 0
        for y in range(h):
            for x in range(0, w, 3 if w > 8 else 1):
                with np.errstate(all="ignore"):
                    zz = _f32(1) / _f32(lo + _f32(span * disp[0, 0, y, x]))
                if not (np.isfinite(zz) and zz > 0):
                    continue
                k = targets[n % len(targets)]
                f, exact = tie_flow(x, zz, TS[0], fx, cx, ifx, k)
                variant = (n // len(targets)) % 3          # exactly at the tie, its fp32 neighbour below, its neighbour above
                info += int(exact and variant == 0)
                flow[0, 0, y, x] = (f, np.nextafter(f, _f32(-np.inf)), np.nextafter(f, _f32(np.inf)))[variant]
                n += 1
                if n >= 150:
                    break
            if n >= 150:
                break
    return flow, info


def _case_list():
    out = []
    for si, shape in enumerate(SHAPES):
        for fi, kind in enumerate(FLOWS):
            pair = TIE_PAIR if kind == "ties" else PAIRS[(si + fi) % len(PAIRS)]
            out.append((shape, kind) + pair + (CAPS[(si + 2 * fi) % 3],))
    # every cap on the map with the most labels, and the same mask on both sides under a shift
    out += [((130, 67), "smooth", "checker", "checker", 4, M) for M in CAPS]
    out += [((37, 53), "shift", "blobs", "blobs", 8, 256), ((37, 53), "zero", "checker", "checker", 4, 4)]
    return list(dict.fromkeys(out))


CASES = _case_list()
CASE_IDS = ["{}x{}-{}-{}-{}-c{}-M{}".format(s[0], s[1], kind, a, b, conn, M) for s, kind, a, b, conn, M in CASES]


@functools.lru_cache(maxsize=None)
def inputs(case):
    """{"src", "dst" (B,h,w) int32, "disp", "flipped" (B,1,h,w), "flow" (B,3,h,w), "ts" (B,), "exact": ties only}: seeded, read-only.
    The disparities are the object tests': a NaN at the last foreground pixel of image 0, a negative z at that of image 1; the
    `nonfinite` case adds infinities and one more NaN to the disparity, beside those in its flow."""
    shape, kind, a, b, conn, M = case
    x = OC.inputs(shape, a)
    disp, flipped = x["disp"], x["flipped"]
    if kind == "nonfinite":
        disp, flipped = disp.copy(), flipped.copy()
        flat = disp.reshape(B, -1)
        for bi in range(B):
            for j, value in enumerate((np.inf, -np.inf, np.nan)):
                flat[bi, (11 * j + 2 + bi) % flat.shape[1]] = value
    flow, exact = flow_field(shape, kind, disp)
    out = {"src": labels(shape, a, conn), "dst": labels(shape, b, conn), "disp": disp, "flipped": flipped, "flow": flow, "ts": TS, "exact": exact}
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def host_args(x, shape, flip, M):
    return (x["src"], x["dst"], x["disp"], x["flow"], x["ts"], OC.intrinsics(*shape)), dict(
        disp_flipped=x["flipped"] if flip else None, min_depth=OC.MIN_DEPTH, max_depth=OC.MAX_DEPTH, max_objects=M)


@functools.lru_cache(maxsize=None)
def reference(case, flip):
    """link_host on the case: (votes, links), computed once, shared, read-only."""
    from hipops.tracks import link_host
    args, kw = host_args(inputs(case), case[0], flip, case[5])
    out = link_host(*args, **kw)
    for v in out:
        v.setflags(write=False)
    return out


def link_loops(src, dst, disp, flow, ts, intrinsics, lo, span, M):
    """The definition as a plain Python triple loop in fp32 scalars (no flip fuse): votes (B, M, M+2)."""
    from hipops.cloud import inverse_focal
    Bn, h, w = src.shape
    fx, fy, cx, cy = (_f32(v) for v in intrinsics)
    ifx, ify = inverse_focal(fx), inverse_focal(fy)
    votes = np.zeros((Bn, M, M + 2), dtype=np.int32)
    with np.errstate(all="ignore"):
        for b in range(Bn):
            for y in range(h):
                for x in range(w):
                    a = int(src[b, y, x])
                    if not 1 <= a <= M:
                        continue
                    z = _f32(1) / _f32(lo + _f32(span * disp[b, 0, y, x]))
                    p0, p1 = _f32(_f32(_f32(_f32(x) - cx) * ifx) * z), _f32(_f32(_f32(_f32(y) - cy) * ify) * z)
                    m0 = _f32(p0 + _f32(flow[b, 0, y, x] * ts[b]))
                    m1 = _f32(p1 + _f32(flow[b, 1, y, x] * ts[b]))
                    m2 = _f32(z + _f32(flow[b, 2, y, x] * ts[b]))
                    u = _f32(_f32(fx * _f32(m0 / m2)) + cx)
                    v = _f32(_f32(fy * _f32(m1 / m2)) + cy)
                    uf, vf = np.floor(_f32(u + _f32(0.5))), np.floor(_f32(v + _f32(0.5)))
                    col = M + 1
                    if m2 > 0 and uf >= 0 and uf <= _f32(w - 1) and vf >= 0 and vf <= _f32(h - 1):
                        t = int(dst[b, int(vf), int(uf)])
                        col = t if 1 <= t <= M else 0
                    votes[b, a - 1, col] += 1
    return votes
