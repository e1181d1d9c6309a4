"""What the point-cloud tests share: the shapes, seeded inputs with the value cases embedded, the searches that construct the exact
decisions of the keep rule (depth == max_range, (smax - smin) == edge * smin), the float64 evaluation of the definition
(hipops/cloud.py's docstring) with the rounding bound that holds the fp32 host definition to it, and the cached host reference."""
import functools
import itertools

import numpy as np

import export_case as EC

MIN_DEPTH, MAX_DEPTH, EPS = EC.MIN_DEPTH, EC.MAX_DEPTH, EC.EPS
EDGE, THRESH = 0.05, 0.5
_f32 = np.float32
# (B, h, w, H, W, stride): one source pixel; W % 4 != 0; same size (carries the exact decisions); down-scaling; a stride that divides
# neither side; more than one workgroup per candidate row (a workgroup is 256 candidates); 600 workgroups: the scan's one workgroup
# takes 16 counts per lane, and frame 1 begins at count 300, inside a lane's run
SHAPES = [(1, 1, 1, 3, 5, 1), (2, 2, 3, 7, 11, 1), (3, 5, 8, 5, 8, 1), (1, 9, 16, 4, 5, 1), (2, 6, 20, 37, 123, 3), (1, 6, 20, 3, 1100, 1),
          (2, 8, 8, 300, 5, 1)]
SAME_SIZE = SHAPES[2]
IDS = ["x".join(str(v) for v in s) for s in SHAPES]
VARIANTS = list(itertools.product([False, True], repeat=2))            # (motion mask, pose)


def intrinsics(H, W):
    """(fx, fy, cx, cy) in pixels of the H x W frame: KITTI's normalised focal lengths, a principal point off the centre."""
    return (0.58 * W, 1.92 * H, 0.5 * W - 0.25, 0.5 * H + 0.125)


def _s(d):
    from hipops.export import depth_params
    lo, span = depth_params(MIN_DEPTH, MAX_DEPTH)
    return _f32(lo + _f32(span * _f32(d)))


def _depth(d):
    return _f32(_f32(1) / _s(d))


def _walk(x, steps, direction):
    out = [_f32(x)]
    for _ in range(steps):
        out.append(np.nextafter(out[-1], _f32(direction)))
    return out


@functools.lru_cache(maxsize=None)
def range_case():
    """(max_range, d_at, d_above): fp32 disparities whose same-size depth 1 / (lo + span * d) equals max_range exactly, and the next
    fp32 number above max_range, found by search among the fp32 neighbours below the first disparity."""
    for start in (0.004, 0.0041, 0.0043, 0.0047, 0.0052):
        d_at = _f32(start)
        top = _depth(d_at)
        target = np.nextafter(top, _f32(np.inf))
        for d in _walk(d_at, 64, -np.inf)[1:]:
            if _depth(d) == target:
                return float(top), float(d_at), float(d)
    raise AssertionError("no disparity pair at the range bound")


@functools.lru_cache(maxsize=None)
def edge_case():
    """(d_low, d_at, d_above): fp32 disparities with s(d_at) - s(d_low) == EDGE * s(d_low) exactly in fp32, and s(d_above) the next fp32
    number above s(d_at), one ulp of s more.  Found by search as export_case.ties: walk d_low, look for the neighbours of the
    disparity that the bound asks for."""
    from hipops.export import depth_params
    lo, span = (np.float64(v) for v in depth_params(MIN_DEPTH, MAX_DEPTH))
    edge = _f32(EDGE)
    for d_low in _walk(0.1, 4000, np.inf):
        smin = _s(d_low)
        bound = _f32(edge * smin)
        want = _f32(smin + bound)
        if _f32(want - smin) != bound:
            continue
        above = np.nextafter(want, _f32(np.inf))
        hits = {}
        guess = _f32((np.float64(want) - lo) / span)
        for d in _walk(guess, 6, -np.inf) + _walk(guess, 6, np.inf):
            for name, s in (("at", want), ("above", above)):
                if _s(d) == s:
                    hits.setdefault(name, float(d))
        if len(hits) == 2 and _f32(above - smin) > bound:
            return float(d_low), hits["at"], hits["above"]
    raise AssertionError("no disparity triple at the edge bound")


def params():
    """The filters every case uses: max_range sits at the depth of the constructed range case."""
    return dict(min_depth=MIN_DEPTH, max_depth=MAX_DEPTH, max_range=range_case()[0], edge=EDGE, motion_thresh=THRESH)


# where the same-size case holds its decisions, frame 0, (Y, X) of the candidate: (kept?, what decides)
DECISIONS = {
    (0, 0): (True, "edge: smax - smin == edge * smin"), (0, 1): (True, "edge"), (1, 0): (True, "edge"), (1, 1): (True, "edge"),
    (0, 4): (False, "edge: one ulp of s more"), (0, 5): (False, "edge"), (1, 4): (False, "edge"), (1, 5): (False, "edge"),
    (3, 0): (True, "range: depth == max_range"), (3, 3): (False, "range: the next fp32 above max_range"),
    (2, 6): (False, "mask == motion_thresh"), (2, 7): (True, "mask: the next fp32 below motion_thresh"),
}


@functools.lru_cache(maxsize=None)
def inputs(B, h, w, seed=0):
    """{"disp", "flipped", "color", "mask", "pose"}: seeded, read-only.  disp / flipped: a smooth ramp with half a percent of noise, a
    step (a depth edge) and a few far pixels, so that every rule keeps some candidates and drops others; colour in [-0.1, 1.1] (both clamps of the byte); mask in [0, 0.8); pose a rotation by a seeded axis-angle and a translation.
    Value cases, as far as the maps have room: a NaN disparity, a disparity with s < 0 (depth <= 0), a NaN mask value.  The same-size
    shape's frame 0 is laid out by hand for DECISIONS: a constant disparity d_low (every tap equal: the edge rule holds with 0), the
    edge pair at (1,1) and (1,5), 2x2 blocks at the range bound and one ulp above it (the upper-left candidate of a block reads four
    equal taps), the two mask values on a constant mask."""
    rng = np.random.default_rng(7000 * seed + 100 * B + 10 * h + w)
    ramp = np.linspace(0.2, 0.3, w, dtype=np.float32)[None, None, :]
    disp = (ramp + 0.005 * rng.random((B, h, w), dtype=np.float32)).astype(np.float32)
    flipped = (ramp[:, :, ::-1] + 0.005 * rng.random((B, h, w), dtype=np.float32)).astype(np.float32)
    disp[:, h // 2:, w // 2:] += _f32(0.25)                 # a depth edge: the pixels that blend across it fail the edge rule
    flipped[:, h // 2:, :w - w // 2] += _f32(0.25)
    far = rng.random((B, h, w)) < 0.05                      # a few pixels beyond max_range
    disp[far], flipped[far[:, :, ::-1]] = 0.001, 0.001
    color = (1.2 * rng.random((B, 3, h, w), dtype=np.float32) - 0.1).astype(np.float32)
    mask = (0.8 * rng.random((B, h, w), dtype=np.float32)).astype(np.float32)
    axis = rng.standard_normal((B, 3))
    angle = np.linalg.norm(axis, axis=1, keepdims=True) * 0.3
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    Kx = np.zeros((B, 3, 3))
    Kx[:, 0, 1], Kx[:, 0, 2], Kx[:, 1, 0], Kx[:, 1, 2], Kx[:, 2, 0], Kx[:, 2, 1] = -axis[:, 2], axis[:, 1], axis[:, 2], -axis[:, 0], -axis[:, 1], axis[:, 0]
    R = np.eye(3)[None] + np.sin(angle)[:, :, None] * Kx + (1 - np.cos(angle))[:, :, None] * (Kx @ Kx)
    pose = np.concatenate([R, rng.standard_normal((B, 3, 1)) * 2.0], axis=2).astype(np.float32)
    if (B, h, w) == SAME_SIZE[:3]:
        max_range, d_at, d_above = range_case()
        d_low, e_at, e_above = edge_case()
        disp[0] = d_low
        disp[0, 1, 1], disp[0, 1, 5] = e_at, e_above
        disp[0, 3:5, 0:2], disp[0, 3:5, 3:5] = d_at, d_above
        mask[0] = 0.25
        mask[0, 2, 6], mask[0, 2, 7] = THRESH, np.nextafter(_f32(THRESH), _f32(0))
        disp[1, 2, 2], disp[1, 0, 6], mask[1, 4, 5] = np.nan, -0.02, np.nan
    elif h * w > 4:
        disp.reshape(-1)[1], disp.reshape(-1)[h * w - 2], mask.reshape(-1)[3] = np.nan, -0.02, np.nan
    out = {"disp": disp, "flipped": flipped, "color": color, "mask": mask, "pose": pose}
    for v in out.values():
        v.setflags(write=False)
    return out


def host_kwargs(B, h, w, flip, with_mask, with_pose, stride=1):
    x = inputs(B, h, w)
    return dict(params(), disp_flipped=x["flipped"] if flip else None, motion_mask=x["mask"] if with_mask else None,
                pose=x["pose"] if with_pose else None, stride=stride)


@functools.lru_cache(maxsize=None)
def host_reference(shape, flip, with_mask, with_pose):
    """export_cloud_host on the seeded case: (records, offsets), computed once, shared, read-only."""
    from hipops.cloud import export_cloud_host
    B, h, w, H, W, stride = shape
    x = inputs(B, h, w)
    out = export_cloud_host(x["disp"], x["color"], H, W, intrinsics(H, W), **host_kwargs(B, h, w, flip, with_mask, with_pose, stride))
    for v in out:
        v.setflags(write=False)
    return out


# ---- float64 ---------------------------------------------------------------------------------------------------------------------
def gamma(n):
    """n roundings in a row: the relative error of their product is at most n EPS / (1 - n EPS)."""
    return n * EPS / (1 - n * EPS)


def cloud64(disp, H, W, camera, flipped=None, pose=None, stride=1):
    """(xyz (B,Hc,Wc,3), bound (B,Hc,Wc,3)) in float64 from the fp32 inputs and the fp32 constants lo, span, cx, cy, 1/fx, 1/fy, R, t.
    depth and its bound D are export_case.depth64 / depth_bound.  Back-projection: x32 = fl(fl(fl(X - cx) * ifx) * depth32), three
    roundings on the product and depth32 = depth + e, |e| <= D:  |x32 - x| <= gamma(3) |x| + (1 + gamma(3)) |xc| D;  the same for y;
    z is the depth itself: D.  With a pose, p'_k = fl(fl(fl(fl(R0 x) + fl(R1 y)) + fl(R2 z)) + t): every term passes through at most
    four roundings (its product and the sums behind it), so with b the bounds of x, y, z:
    |p'32 - p'| <= gamma(4) (|R0 x| + |R1 y| + |R2 z| + |t|) + (1 + gamma(4)) (|R0| bx + |R1| by + |R2| bz)."""
    from hipops.cloud import inverse_focal
    fx, fy, cx, cy = (_f32(v) for v in camera)
    depth, u, u_bound = EC.depth64(disp, H, W, flipped)
    D = EC.depth_bound(depth, u, u_bound)
    depth, D = depth[:, ::stride, ::stride], D[:, ::stride, ::stride]
    xc = ((np.arange(W)[::stride] - np.float64(cx)) * np.float64(inverse_focal(fx)))[None, None, :]
    yc = ((np.arange(H)[::stride] - np.float64(cy)) * np.float64(inverse_focal(fy)))[None, :, None]
    p = [xc * depth, yc * depth, depth]
    b = [gamma(3) * np.abs(p[0]) + (1 + gamma(3)) * np.abs(xc) * D, gamma(3) * np.abs(p[1]) + (1 + gamma(3)) * np.abs(yc) * D, D]
    if pose is not None:
        T = pose.astype(np.float64)[:, :, :, None, None]
        q, c = [], []
        for k in range(3):
            terms = [T[:, k, j] * p[j] for j in range(3)]
            q.append(((terms[0] + terms[1]) + terms[2]) + T[:, k, 3])
            c.append(gamma(4) * (sum(np.abs(t) for t in terms) + np.abs(T[:, k, 3])) + (1 + gamma(4)) * sum(np.abs(T[:, k, j]) * b[j] for j in range(3)))
        p, b = q, c
    return np.stack(np.broadcast_arrays(*p), axis=-1), np.stack(np.broadcast_arrays(*b), axis=-1)
