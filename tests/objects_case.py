"""What the object tests share (hipops/objects.py, csrc/dd_objects.hip): the shapes, masks built analytically (none knows the kernel's
tile), seeded numeric inputs with the value cases embedded, the cached host reference of every case, the caps, and the bound that
holds two float64 sums of the same fp32 terms to each other."""
import functools

import numpy as np

MIN_DEPTH, MAX_DEPTH, THRESH = 0.1, 100.0, 0.5
_f32 = np.float32
# smaller than any tile (one pixel, one row, a few rows); odd and multi-tile; the network size of the predict tests; more tiles down than across
SHAPES = [(1, 1), (1, 70), (5, 7), (37, 53), (64, 96), (130, 67)]
B = 2
# the table comparisons count every component (min_pixels = 1) under a cap none of them reaches: the most components any case has is
# the 4-connected checkerboard's ceil(130 * 67 / 2) = 4355
CAP = 8192
DEFAULT_CAP = 256
# the truncation case: shape, mask, connectivity, components
TRUNCATED = ((37, 53), "checker", 4, 981)


def _serpentine(h, w):
    """Every second row, joined at alternating ends: one component, a one-pixel path through the whole image."""
    m = np.zeros((h, w), dtype=bool)
    m[0::2] = True
    for k, y in enumerate(range(1, h - 1, 2)):
        m[y, w - 1 if k % 2 == 0 else 0] = True
    return m


def _spiral(h, w):
    """A square spiral from the upper-left corner inwards, one pixel wide with one pixel between its turns."""
    m = np.zeros((h, w), dtype=bool)
    inside = lambda y, x: 0 <= y < h and 0 <= x < w          # noqa: E731
    y, x, dy, dx = 0, 0, 0, 1
    m[0, 0] = True
    while True:
        for _ in range(2):
            ny, nx, fy, fx = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            if inside(ny, nx) and not m[ny, nx] and not (inside(fy, fx) and m[fy, fx]):
                y, x = ny, nx
                m[y, x] = True
                break
            dy, dx = dx, -dy
        else:
            return m


def _rings(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.minimum(np.minimum(yy, xx), np.minimum(h - 1 - yy, w - 1 - xx)) % 2 == 0


def _comb(h, w):
    """U-shapes open to the top: columns 0 and 2 of every four, joined in the bottom row; column 3 keeps the Us apart."""
    m = np.zeros((h, w), dtype=bool)
    m[:, 0::4] = True
    m[:, 2::4] = True
    m[h - 1, 1::4] = True
    return m


def _diagonals(h, w):
    m = np.zeros((h, w), dtype=bool)
    i = np.arange(min(h, w))
    m[i, i] = True
    m[i, w - 1 - i] = True
    return m


def _corners(h, w):
    m = np.zeros((h, w), dtype=bool)
    m[0, 0] = m[0, w - 1] = m[h - 1, 0] = m[h - 1, w - 1] = True
    return m


def _rng(h, w, salt):
    return np.random.default_rng(1000003 * salt + 1009 * h + w)


def blob_field(h, w, seed=0, passes=3, keep=0.3):
    """A smooth field: seeded noise under `passes` 5 x 5 box filters (wrapping), the upper `keep` of its values foreground."""
    v = _rng(h, w, 77 + seed).random((h, w))
    for _ in range(passes):
        v = sum(np.roll(v, s, axis=0) for s in range(-2, 3)) / 5
        v = sum(np.roll(v, s, axis=1) for s in range(-2, 3)) / 5
    return v >= np.quantile(v, 1 - keep)


MASKS = {
    "empty": lambda h, w: np.zeros((h, w), dtype=bool),
    "full": lambda h, w: np.ones((h, w), dtype=bool),
    "checker": lambda h, w: np.add.outer(np.arange(h), np.arange(w)) % 2 == 0,
    "serpentine": _serpentine,
    "spiral": _spiral,
    "rings": _rings,
    "comb": _comb,
    "diagonals": _diagonals,
    "corners": _corners,
    "bernoulli30": lambda h, w: _rng(h, w, 30).random((h, w)) < 0.3,
    "bernoulli50": lambda h, w: _rng(h, w, 50).random((h, w)) < 0.5,
    "bernoulli60": lambda h, w: _rng(h, w, 60).random((h, w)) < 0.6,
    "blobs": blob_field,
    "nan_thresh": lambda h, w: _rng(h, w, 90).random((h, w)) < 0.5,
}
NAMES = list(MASKS)


def mask_values(fg, salt, special=False):
    """fp32 mask values of a boolean pattern: foreground in [THRESH, 1), background in [0, THRESH); with `special` a third of the
    foreground sits exactly AT the threshold, a third of the background one fp32 step below it and another third is NaN."""
    rng = np.random.default_rng(salt)
    u = rng.random(fg.shape)
    below = np.nextafter(_f32(THRESH), _f32(0))
    m = np.where(fg, THRESH + u * (1 - THRESH) * 0.999, u * float(below)).astype(np.float32)
    if special:
        pick = rng.integers(0, 3, fg.shape)
        m[fg & (pick == 0)] = THRESH
        m[~fg & (pick == 0)] = below
        m[~fg & (pick == 1)] = np.nan
    with np.errstate(invalid="ignore"):
        assert np.array_equal(m >= _f32(THRESH), fg)
    return m


@functools.lru_cache(maxsize=None)
def pattern(shape, name):
    """(B,h,w) bool: image 0 the named mask, image 1 its mirror image -- except `full` (image 1 empty) and `empty` (image 1 full):
    a label that leaks from one image into the next shows there."""
    h, w = shape
    first = MASKS[name](h, w)
    second = {"full": np.zeros_like(first), "empty": np.ones_like(first)}.get(name, first[:, ::-1])
    out = np.stack([first, second])
    out.setflags(write=False)
    return out


def intrinsics(h, w):
    return (0.58 * w, 1.92 * h, 0.5 * w - 0.25, 0.5 * h + 0.125)


@functools.lru_cache(maxsize=None)
def inputs(shape, name):
    """{"mask" (B,1,h,w), "disp", "flipped" (B,1,h,w) in (0,1), "flow" (B,3,h,w), "ts" (B,), "pose" (B,3,4)}: seeded, read-only.
    Value cases: the LAST foreground pixel of image 0 has a NaN disparity (its object's sums are NaN, its z is left out of the depth
    range), the last foreground pixel of image 1 a disparity whose z is negative (finite sums, left out of the depth range)."""
    h, w = shape
    fg = pattern(shape, name)
    salt = 7919 * NAMES.index(name) + 131 * h + w
    rng = np.random.default_rng(salt)
    mask = np.stack([mask_values(fg[b], salt + b, special=name == "nan_thresh") for b in range(B)])[:, None]
    disp = (0.02 + 0.96 * rng.random((B, 1, h, w))).astype(np.float32)
    flipped = (0.02 + 0.96 * rng.random((B, 1, h, w))).astype(np.float32)
    flow = (0.3 * rng.standard_normal((B, 3, h, w))).astype(np.float32)
    ts = np.array([0.1, 1.7], dtype=np.float32)
    axis = rng.standard_normal((B, 3))
    angle = np.linalg.norm(axis, axis=1, keepdims=True) * 0.05
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    Kx = np.zeros((B, 3, 3))
    Kx[:, 0, 1], Kx[:, 0, 2], Kx[:, 1, 0], Kx[:, 1, 2], Kx[:, 2, 0], Kx[:, 2, 1] = -axis[:, 2], axis[:, 1], axis[:, 2], -axis[:, 0], -axis[:, 1], axis[:, 0]
    R = np.eye(3)[None] + np.sin(angle)[:, :, None] * Kx + (1 - np.cos(angle))[:, :, None] * (Kx @ Kx)
    pose = np.concatenate([R, rng.standard_normal((B, 3, 1)) * 0.5], axis=2).astype(np.float32)
    for b, value in ((0, np.nan), (1, -0.02)):
        at = np.flatnonzero(fg[b].reshape(-1))
        if len(at):
            disp[b, 0].reshape(-1)[at[-1]] = value
            flipped[b, 0].reshape(-1)[w * (at[-1] // w) + (w - 1 - at[-1] % w)] = value          # the pixel the fuse pairs it with
    out = {"mask": mask, "disp": disp, "flipped": flipped, "flow": flow, "ts": ts, "pose": pose}
    for v in out.values():
        v.setflags(write=False)
    return out


def uses_flip(shape, name):
    """Half the cases run with the flip fuse."""
    return (SHAPES.index(shape) + NAMES.index(name)) % 2 == 1


def host_kwargs(shape, name):
    x = inputs(shape, name)
    return dict(disp_flipped=x["flipped"] if uses_flip(shape, name) else None, min_depth=MIN_DEPTH, max_depth=MAX_DEPTH)


@functools.lru_cache(maxsize=None)
def quantities(shape, name):
    from hipops.objects import pixel_quantities_host
    x = inputs(shape, name)
    return pixel_quantities_host(x["mask"], x["disp"], x["flow"], x["ts"], x["pose"], intrinsics(*shape), **host_kwargs(shape, name))


@functools.lru_cache(maxsize=None)
def reference(shape, name, connectivity, min_pixels=1, max_objects=CAP):
    """objects_host on the seeded case: (labels, table, counts), computed once, shared, read-only."""
    from hipops.objects import label_components_host, object_table_host
    x = inputs(shape, name)
    labels, found, truncated = label_components_host(x["mask"], thresh=THRESH, connectivity=connectivity, min_pixels=min_pixels, max_objects=max_objects)
    counts = np.stack([np.minimum(found, max_objects), found, truncated.astype(np.int32)], axis=1).astype(np.int32)
    out = (labels, object_table_host(labels, quantities(shape, name), max_objects), counts)
    for v in out:
        v.setflags(write=False)
    return out


def check_caps():
    """On the host alone: the truncation case truncates under the default cap, and no case reaches the cap its comparison runs under."""
    shape, name, connectivity, components = TRUNCATED
    counts = reference(shape, name, connectivity, 1, DEFAULT_CAP)[2]
    assert counts[0].tolist() == [DEFAULT_CAP, components, 1], counts
    for shape in SHAPES:
        for name in NAMES:
            for connectivity in (4, 8):
                counts = reference(shape, name, connectivity)[2]
                assert (counts[:, 2] == 0).all() and (counts[:, 1] <= CAP).all(), (shape, name, connectivity, counts)


def sum_bound(labels, q, max_objects):
    """(B, max_objects, 7): 2 * pixels * 2**-53 * sum |x_i| per object and sum.  Two float64 sums of the same n fp32 terms, in any two
    orders, are each within (n - 1) u / (1 - (n - 1) u) * sum |x_i| of the exact sum, u = 2**-53: their distance is below this."""
    Bn, h, w = labels.shape
    values = np.abs(np.concatenate([q["p"], q["r"], q["mask"][:, None]], axis=1).reshape(Bn, 7, h * w).astype(np.float64))
    out = np.zeros((Bn, max_objects, 7))
    with np.errstate(all="ignore"):
        for b in range(Bn):
            lab = labels[b].reshape(-1)
            n = int(lab.max())
            pixels = np.bincount(lab, minlength=n + 1)[1:]
            for k in range(7):
                out[b, :n, k] = 2.0 * pixels * 2.0 ** -53 * np.bincount(lab, weights=values[b, k], minlength=n + 1)[1:]
    return out


def compare(got_labels, got_table, got_counts, want, bound, what):
    """Device (or second-run) outputs against a reference triple: labels, counts and the integer and depth-range columns exactly, the
    sums within `bound`; a sum that is not finite in the reference is the same non-finite value (or NaN) on the other side."""
    from hipops.objects import rows
    labels, table, counts = want
    assert np.array_equal(got_counts, counts), (what, got_counts, counts)
    assert np.array_equal(got_labels, labels), (what, "labels")
    g, r = rows(got_table), rows(table)
    for column in ("pixels", "box", "anchor"):
        assert np.array_equal(g[column], r[column]), (what, column)
    assert np.array_equal(g["z"].view(np.int32), r["z"].view(np.int32)), (what, "z_min / z_max")
    finite = np.isfinite(r["sums"])
    assert np.array_equal(np.isfinite(g["sums"]), finite), (what, "which sums are finite")
    assert np.array_equal(g["sums"][~finite], r["sums"][~finite], equal_nan=True), (what, "the non-finite sums")
    err = np.abs(g["sums"][finite] - r["sums"][finite])              # where the reference is NaN, so is the bound: those were compared above
    assert (err <= bound[finite]).all(), (what, "sums", float(err.max()), int(np.argmax(err - bound[finite])))
