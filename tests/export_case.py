"""What the depth-export tests share: the shapes, seeded disparities with the value cases embedded, the float64 evaluation of the
definition (hipops/export.py's docstring) with the rounding bound that holds the fp32 host definition to it, and the search that
constructs exact rounding ties of the 16-bit image."""
import functools

import numpy as np

MIN_DEPTH, MAX_DEPTH = 0.1, 100.0
EPS = 2.0 ** -24                                   # unit roundoff of fp32
# (B, h, w, H, W): one pixel; W % 4 != 0 and unaligned rgb rows; same size; down-scaling; odd everything; more than one workgroup row
SHAPES = [(1, 1, 1, 3, 5), (2, 2, 3, 7, 11), (3, 5, 8, 5, 8), (1, 9, 16, 4, 5), (2, 6, 20, 37, 123), (1, 24, 80, 160, 240)]
SUBSETS = [("depth",), ("depth16",), ("rgb",), ("depth", "depth16"), ("depth", "rgb"), ("depth16", "rgb"), ("depth", "depth16", "rgb")]


@functools.lru_cache(maxsize=None)
def ties(count=6, depth_scale=256.0):
    """[(disp, k)]: fp32 disparities whose same-size export gives depth * depth_scale == k + 0.5 exactly, `count` with even k and
    `count` with odd k, found by search: depth = (2k+1) / (2 depth_scale) is an fp32 number; try the fp32 neighbours of 1 / depth for s
    and of (s - lo) / span for the disparity, and keep what the fp32 definition maps back onto depth exactly."""
    from hipops.export import depth_params
    lo, span = depth_params(MIN_DEPTH, MAX_DEPTH)
    one = np.float32(1)
    found = {0: [], 1: []}
    for k in range(30, 20000):
        if len(found[k % 2]) >= count:
            if len(found[1 - k % 2]) >= count:
                break
            continue
        t = np.float32((2 * k + 1) / (2 * depth_scale))
        assert float(t) * depth_scale == k + 0.5
        s0 = one / t
        hit = None
        for s in _neighbours(s0):
            if one / s != t:
                continue
            for d in _neighbours(np.float32((np.float64(s) - np.float64(lo)) / np.float64(span))):
                if np.float32(lo + np.float32(span * d)) == s and 0 <= d <= 1:
                    hit = d
                    break
            if hit is not None:
                break
        if hit is not None:
            found[k % 2].append((float(hit), k))
    assert len(found[0]) >= count and len(found[1]) >= count, found
    return found[0][:count] + found[1][:count]


def _neighbours(x, n=3):
    out = [np.float32(x)]
    up = down = np.float32(x)
    for _ in range(n):
        up, down = np.nextafter(up, np.float32(np.inf)), np.nextafter(down, np.float32(-np.inf))
        out += [up, down]
    return out


@functools.lru_cache(maxsize=None)
def disparities(B, h, w, seed=0, values=True):
    """(disp, disp_flipped), each (B, h, w) fp32 in [0, 1): seeded noise on a smooth ramp; with `values` the value cases are written over
    the first elements of `disp` as far as the map has room: a NaN (it poisons every output pixel that reads it as a tap, even with
    weight 0: 0 * NaN), 0, 1, and two rounding ties."""
    rng = np.random.default_rng(1000 * seed + 100 * B + 10 * h + w)
    ramp = np.linspace(0.05, 0.6, w, dtype=np.float32)[None, None, :]
    disp = (ramp + 0.3 * rng.random((B, h, w), dtype=np.float32)).astype(np.float32)
    flipped = (ramp[:, :, ::-1] + 0.3 * rng.random((B, h, w), dtype=np.float32)).astype(np.float32)
    if values:
        t = ties()
        cases = [np.nan, 0.0, 1.0, t[0][0], t[len(t) // 2][0]]
        flat = disp.reshape(-1)
        for i, v in enumerate(cases[:max(flat.size - 1, 0)]):
            flat[i] = v
    disp.setflags(write=False)
    flipped.setflags(write=False)
    return disp, flipped


@functools.lru_cache(maxsize=None)
def host_reference(B, h, w, H, W, flip, depth_scale=256.0):
    """export_depth_host (every output) and export_plane_u8_host on the seeded case: computed once, shared, read-only."""
    from hipops.export import export_depth_host, export_plane_u8_host
    disp, flipped = disparities(B, h, w)
    out = export_depth_host(disp, H, W, disp_flipped=flipped if flip else None, min_depth=MIN_DEPTH, max_depth=MAX_DEPTH, depth_scale=depth_scale)
    out["plane_u8"] = export_plane_u8_host(disp * 1.5 - 0.2, H, W)         # values below 0 and above 1 included
    for v in out.values():
        v.setflags(write=False)
    return out


# ---- float64 -------------------------------------------------------------------------------------------------------------------
def _taps64(out_size, in_size):
    src = np.maximum((in_size / out_size) * (np.arange(out_size, dtype=np.float64) + 0.5) - 0.5, 0.0)
    i0 = np.minimum(src.astype(np.int64), in_size - 1)
    return i0, i0 + (i0 < in_size - 1), src - i0


def blend64(v, H, W):
    y0, y1, wy = _taps64(H, v.shape[1])
    x0, x1, wx = _taps64(W, v.shape[2])
    wy, wx = wy[None, :, None], wx[None, None, :]
    top = (1 - wx) * v[:, y0][:, :, x0] + wx * v[:, y0][:, :, x1]
    bot = (1 - wx) * v[:, y1][:, :, x0] + wx * v[:, y1][:, :, x1]
    return (1 - wy) * top + wy * bot


def fuse64(disp, flipped):
    """The fuse step in float64 on the fp32 inputs and the fp32 l_mask table, in the pinned order."""
    from hipops.export import l_mask_table
    l, r = disp.astype(np.float64), flipped.astype(np.float64)[:, :, ::-1]
    lm = l_mask_table(disp.shape[2]).astype(np.float64)[None, None, :]
    rm = lm[:, :, ::-1]
    m = 0.5 * (l + r)
    return (rm * l + lm * r) + ((1 - lm) - rm) * m


def fuse_bound(disp, flipped):
    """|fp32 fuse - float64 fuse| per element: eight rounded operations (rm*l, lm*r, their sum, 1-lm, -rm, l+r, the product with m, the
    last sum; 0.5* is exact), each within EPS of a quantity that is at most 2 D in magnitude, D = max(|l|, |r|) (lm, rm in [0,1],
    |(1-lm)-rm| <= 1): 16 EPS D, first order; 17 covers the second-order terms."""
    D = np.maximum(np.abs(disp.astype(np.float64)), np.abs(flipped.astype(np.float64)[:, :, ::-1]))
    return 17 * EPS * D


def _spread(a, axes=(1, 2), radius=2):
    """Largest value within `radius` elements along `axes`; a NaN counts as absent."""
    for ax in axes:
        pad = [(0, 0)] * a.ndim
        pad[ax] = (radius, radius)
        p = np.pad(a, pad, constant_values=np.nan)
        n = a.shape[ax]
        a = functools.reduce(np.fmax, [np.take(p, np.arange(k, k + n), axis=ax) for k in range(2 * radius + 1)])
    return a


def _at_taps(a, H, W):
    """A per-source-pixel quantity at the upper-left float64 tap of every output pixel."""
    y0, x0 = _taps64(H, a.shape[1])[0], _taps64(W, a.shape[2])[0]
    return a[:, y0][:, :, x0]


def depth64(disp, H, W, flipped=None):
    """(depth, u, bound on |fp32 u - float64 u|) in float64 from the fp32 inputs and the fp32 constants lo, span.
    The bound, per output pixel, first order in EPS.  S, dx, dy are local: the largest |s| and the largest difference of horizontally /
    vertically adjacent s values within two source pixels of the output pixel's upper-left tap -- that covers the four taps and the
    neighbouring cell the fp32 evaluation lands in when its source coordinate falls on the other side of an integer (the blend is
    continuous there: weight 1 on one side is weight 0 on the other).
      source coordinate  src = scale * (X + 0.5) - 0.5 in fp32: the ratio, the product and the difference are rounded, each within EPS
                         of at most `in_size`; X + 0.5 and src - i0 are exact.  |d wx| <= 3 EPS w and |d wy| <= 3 EPS h.
                         On u: 3 EPS (w dx + h dy).
      taps               s = lo + span * d: two roundings, 2 EPS S; with the fuse in front of it span * fuse_bound more.
      blend              each of the three interpolations rounds 1 - weight, two products and a sum, 3 EPS S with the weights summing to
                         one; the first two feed the third: 6 EPS S.
    depth = 1 / u then carries that relative error plus EPS of the division; `depth_bound` puts it together."""
    from hipops.export import depth_params
    lo, span = (np.float64(v) for v in depth_params(MIN_DEPTH, MAX_DEPTH))
    if flipped is None:
        d = disp.astype(np.float64)
        tap_err = np.zeros_like(d)
    else:
        d = fuse64(disp, flipped)
        tap_err = span * fuse_bound(disp, flipped)
    s = lo + span * d
    zeros = np.zeros_like(s)
    dx, dy = zeros.copy(), zeros.copy()
    dx[:, :, :-1] = np.abs(np.diff(s, axis=2))
    dy[:, :-1, :] = np.abs(np.diff(s, axis=1))
    S, dx, dy, tap_err = (_at_taps(_spread(a), H, W) for a in (np.abs(s), dx, dy, tap_err))
    u = blend64(s, H, W)
    bound = 3 * EPS * (s.shape[2] * dx + s.shape[1] * dy) + 8 * EPS * S + tap_err
    return 1.0 / u, u, bound


def depth_bound(depth, u, u_bound):
    """|fp32 depth - float64 depth| <= depth * (u_bound / (u - u_bound) + EPS), with one more EPS for second-order terms."""
    return np.abs(depth) * (u_bound / (np.abs(u) - u_bound) + 2 * EPS)
