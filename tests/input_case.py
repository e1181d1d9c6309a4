"""Case tables, content generators and references shared by tests/test_input_inputs.py (CPU: the cases are what they claim) and
tests/test_input_parity_gpu.py (GPU: dd_jpeg_decode, dd_prepare_frames and dd_pyramid_down2 on them).  Plain module, no fixtures.

References: PIL's decode for the JPEG files (oracle/ref_jpeg.py is pinned against it on the same files); the oracle's torch
ColorJitter restatement (oracle/ref_input.py) run on double input for the jitter; a float64 numpy restatement of the antialiased
bicubic tap set for the pyramid.  Every generator has a fixed seed; every list is built once and left unchanged."""
import collections
import functools
import io
import itertools
import random

import numpy as np
import torch
from PIL import Image

import oracle.ref_input as ori
import oracle.ref_jpeg as rj

# ---- content: (h, w) -> (h, w, 3) uint8 ---------------------------------------------------------------------------------------


def noise(h, w, seed=0):
    return np.random.default_rng(100 + seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def edges(h, w, seed=0):
    """0 / 255 per channel: every pixel a corner of the colour cube"""
    return (np.random.default_rng(200 + seed).integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)


def sat(h, w, seed=0):
    """left half black, right half white, a band across both with only red at 255"""
    out = np.zeros((h, w, 3), np.uint8)
    out[:, w // 2:] = 255
    top = h // 3
    out[top:max(top + 1, 2 * h // 3)] = (255, 0, 0)
    return out


def primaries(h, w, seed=0):
    """pure R, G, B columns in turn"""
    out = np.zeros((h, w, 3), np.uint8)
    for x in range(w):
        out[:, x, (x + seed) % 3] = 255
    return out


def neargrey(h, w, seed=0):
    """grey +-1 in one channel: max - min = 1/255, the hue's divisor at its smallest"""
    rng = np.random.default_rng(300 + seed)
    out = np.repeat(rng.integers(1, 255, (h, w, 1)), 3, axis=2)
    ch, sign = rng.integers(0, 3, (h, w)), rng.integers(0, 2, (h, w)) * 2 - 1
    yy, xx = np.mgrid[:h, :w]
    out[yy, xx, ch] += sign
    return out.astype(np.uint8)


def ties(h, w, seed=0):
    """two channels share the maximum: r == g, g == b and r == b in turn"""
    rng = np.random.default_rng(400 + seed)
    lo = rng.integers(0, 128, (h, w))
    hi = lo + rng.integers(1, 128, (h, w))
    yy, xx = np.mgrid[:h, :w]
    low_ch = (2 - (yy + xx + seed) % 3)                      # the channel that is NOT at the maximum: b, r, g
    out = np.repeat(hi[..., None], 3, axis=2)
    out[yy, xx, low_ch] = lo
    return out.astype(np.uint8)


def black(h, w, seed=0):
    return np.zeros((h, w, 3), np.uint8)


def white(h, w, seed=0):
    return np.full((h, w, 3), 255, np.uint8)


CONTENT = collections.OrderedDict((f.__name__, f) for f in (noise, edges, sat, primaries, neargrey, ties, black, white))

# ---- JPEG files ---------------------------------------------------------------------------------------------------------------
JpegFile = collections.namedtuple("JpegFile", "label data")

JPEG_CONTENT = ("noise", "edges", "sat", "primaries")
JPEG_SIZES = [(1, 1), (7, 5), (8, 8), (9, 17), (16, 16), (17, 33), (101, 67)]             # (w, h)
JPEG_SAMPLINGS = (0, 1, 2)                                                                  # PIL: 4:4:4, 4:2:2, 4:2:0
JPEG_QUALITIES = (1, 5, 25, 100)
RESTART_CONTENT = ("noise", "edges")
RESTART_SIZES = [(17, 33), (96, 64), (101, 67)]
RESTART_QUALITIES = (5, 100)
RESTART_BLOCKS = (0, 1, 3)
ROWS_SIZES = [(17, 33), (101, 67)]
QTABLES = ([[1] * 64, [255] * 64], [[255] * 64, [1] * 64])
GREY_SIZES = [(1, 1), (7, 5), (9, 17), (72, 40)]
GREY_QUALITIES = (1, 25, 100)
META_SIZE = (47, 33)
META_ICC_BYTES = 70000


# the geometries (w, h, components, h[3], v[3]) the lists above produce, stated without encoding anything (test ids); PIL's default
# sub-sampling, which the metadata files take, is 4:2:0
_LUMA = {0: ((1, 1, 1), (1, 1, 1)), 1: ((2, 1, 1), (1, 1, 1)), 2: ((2, 1, 1), (2, 1, 1))}
JPEG_GEOMETRIES = ([(w, h, 3) + _LUMA[ss] for (w, h) in JPEG_SIZES + [(96, 64)] for ss in JPEG_SAMPLINGS] +
                   [(w, h, 1, (1, 0, 0), (1, 0, 0)) for (w, h) in GREY_SIZES] + [META_SIZE + (3,) + _LUMA[2]])


def encode(arr, grey=False, **kw):
    im = Image.fromarray(arr)
    if grey:
        im = im.convert("L")
    buf = io.BytesIO()
    im.save(buf, "JPEG", **kw)
    return buf.getvalue()


def pil_decode(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


@functools.lru_cache(maxsize=None)
def jpeg_lists():
    """{list name: [JpegFile]} -- the main matrix, the restart matrix and the four further lists, encoded in memory.  Within a list
    the quality varies fastest, so that neighbouring files carry different quantisation (and, optimised, Huffman) tables."""
    out = collections.OrderedDict()
    out["main"] = [JpegFile("main %s %dx%d ss%d opt%d q%d" % (c, w, h, ss, opt, q), encode(CONTENT[c](h, w), subsampling=ss, optimize=bool(opt), quality=q))
                   for (w, h) in JPEG_SIZES for ss in JPEG_SAMPLINGS for c in JPEG_CONTENT for opt in (0, 1) for q in JPEG_QUALITIES]
    out["restart"] = [JpegFile("restart %s %dx%d ss%d rst%d q%d" % (c, w, h, ss, rb, q),
                               encode(CONTENT[c](h, w, seed=1), subsampling=ss, quality=q, **({"restart_marker_blocks": rb} if rb else {})))
                      for (w, h) in RESTART_SIZES for ss in JPEG_SAMPLINGS for c in RESTART_CONTENT for rb in RESTART_BLOCKS for q in RESTART_QUALITIES]
    out["restart_rows"] = [JpegFile("rows %s %dx%d ss%d q%d" % (c, w, h, ss, q), encode(CONTENT[c](h, w, seed=2), subsampling=ss, quality=q, restart_marker_rows=1))
                           for (w, h) in ROWS_SIZES for ss in JPEG_SAMPLINGS for c in RESTART_CONTENT for q in RESTART_QUALITIES]
    out["qtables"] = [JpegFile("qtables %s %dx%d ss%d luma %d" % (c, w, h, ss, qt[0][0]), encode(CONTENT[c](h, w, seed=3), subsampling=ss, qtables=qt))
                      for (w, h) in ROWS_SIZES for ss in JPEG_SAMPLINGS for c in RESTART_CONTENT for qt in QTABLES]
    out["grey"] = [JpegFile("grey %s %dx%d opt%d q%d" % (c, w, h, opt, q), encode(CONTENT[c](h, w, seed=4), grey=True, optimize=bool(opt), quality=q))
                   for (w, h) in GREY_SIZES for c in RESTART_CONTENT for opt in (0, 1) for q in GREY_QUALITIES]
    w, h = META_SIZE
    icc = bytes(np.random.default_rng(5).integers(0, 256, META_ICC_BYTES, dtype=np.uint8))
    exif = Image.Exif()
    exif[0x010E] = "input-side parity case"                     # ImageDescription
    exif[0x0112] = 1                                            # Orientation: upright, so that nothing may turn the decode
    out["meta"] = [JpegFile("meta comment+exif+icc %dx%d q90" % (w, h), encode(noise(h, w, seed=5), quality=90, comment=b"c" * 300, exif=exif, icc_profile=icc)),
                   JpegFile("meta plain %dx%d q30" % (w, h), encode(noise(h, w, seed=6), quality=30))]
    return out


def jpeg_files():
    return [f for files in jpeg_lists().values() for f in files]


def geometry(data):
    """(w, h, components, h[3], v[3]) from the oracle's parse, in the form hipops.jpeg.parse_header returns it"""
    hd = rj.JpegHeader(data)
    hs = tuple(c[1] for c in hd.components) + (0,) * (3 - len(hd.components))
    vs = tuple(c[2] for c in hd.components) + (0,) * (3 - len(hd.components))
    return (hd.width, hd.height, len(hd.components), hs, vs)


@functools.lru_cache(maxsize=None)
def jpeg_batches():
    """{geometry: [JpegFile]} in list order: one decode_batch call per geometry carries every content, quality, optimize setting,
    restart interval and table set of that geometry together"""
    out = collections.OrderedDict()
    for f in jpeg_files():
        out.setdefault(geometry(f.data), []).append(f)
    return out


def batch_id(geom):
    w, h, nc, hs, vs = geom
    return "%dx%d-c%d-h%dv%d" % (w, h, nc, hs[0], vs[0])


@functools.lru_cache(maxsize=None)
def pil_batch(geom):
    """PIL's decode of every file of a batch, (n, h, w, 3) uint8"""
    return np.stack([pil_decode(f.data) for f in jpeg_batches()[geom]])


# ---- jitter cases -------------------------------------------------------------------------------------------------------------
JITTER_CASES = [(1, 1, 1, 1), (4, 6, 5, 7), (8, 3, 37, 53), (1, 4, 64, 130), (2, 3, 64, 96)]            # (B, F, H, W)
ORDERS = list(itertools.permutations(range(4)))
IDENTITY = (1.0, 1.0, 1.0, 0.0)
JitterCase = collections.namedtuple("JitterCase", "frames params flip")


def jitter_ranges():
    """(brightness, contrast, saturation, hue) ranges the loader draws from"""
    from datasets.base_dataset import ColorJitter
    return ColorJitter().ranges


@functools.lru_cache(maxsize=None)
def jitter_pool():
    """24 distinct value rows: the 16 corners of the loader's ranges, the identity, 7 random draws"""
    ranges = jitter_ranges()
    rng = random.Random(7)
    return list(itertools.product(*ranges)) + [IDENTITY] + [tuple(rng.uniform(*r) for r in ranges) for _ in range(7)]


def frame_content(k, h, w):
    """frame k of a case: frames too low for bands, and every second frame otherwise, hold ONE generator (an all-black or all-white
    frame has a grey mean of 0 or 1); the others stack a band of every generator"""
    names = list(CONTENT)
    if h < len(names):
        return CONTENT[names[k % len(names)]](h, w, seed=k)
    if k % 2 == 0:
        return CONTENT[names[(k // 2) % len(names)]](h, w, seed=k)
    cuts = [h * i // len(names) for i in range(len(names) + 1)]
    return np.concatenate([CONTENT[names[(i + k) % len(names)]](cuts[i + 1] - cuts[i], w, seed=k) for i in range(len(names))], 0)


@functools.lru_cache(maxsize=None)
def jitter_case(shape):
    """frames (B,F,H,W,3) uint8, params (B,F,9) fp32 rows [apply, order[4], b, c, s, h], flip (B,) int32.  Row k = (b, f) takes
    order 7k + c and pool entry k + 5c (c the case's index): 24 rows see all 24 orders and the whole pool, every row is distinct;
    rows 3, 8, 13 ... are not applied; b = 0, 2, ... are flipped."""
    B, F, H, W = shape
    c = JITTER_CASES.index(shape)
    pool = jitter_pool()
    params = torch.zeros(B, F, 9)
    frames = np.zeros((B, F, H, W, 3), np.uint8)
    for k in range(B * F):
        b, f = divmod(k, F)
        params[b, f] = torch.tensor([0.0 if k % 5 == 3 else 1.0] + [float(o) for o in ORDERS[(7 * k + c) % 24]] + list(pool[(k + 5 * c) % 24]))
        frames[b, f] = frame_content(k, H, W)
    flip = torch.tensor([(b + 1) % 2 for b in range(B)], dtype=torch.int32)
    return JitterCase(torch.from_numpy(frames), params, flip)


def float64_jitter(color, params):
    """color (F,B,3,H,W) fp32 (ToTensor + flip), params (B,F,9) fp32 -> color_aug (F,B,3,H,W) float64: the oracle's torch code on
    double input, with the float32-rounded parameters"""
    out = color.double().clone()
    F, B = color.shape[:2]
    for f in range(F):
        for b in range(B):
            p = params[b, f]
            if float(p[0]) > 0.5:
                out[f, b] = ori.color_jitter(color[f, b].double(), [int(x) for x in p[1:5]], float(p[5]), float(p[6]), float(p[7]), float(p[8]))
    return out


JitterRef = collections.namedtuple("JitterRef", "color aug32 aug64 applied")


@functools.lru_cache(maxsize=None)
def jitter_ref(shape):
    """color, the float32 oracle's color_aug (oracle/ref_input.prepare_inputs as it is), the float64 color_aug -- all (F,B,3,H,W) --
    and applied (F,B) bool"""
    case = jitter_case(shape)
    F = case.frames.shape[1]
    got = ori.prepare_inputs({f: case.frames[:, f] for f in range(F)}, {f: case.params[:, f] for f in range(F)}, case.flip, [0])
    color = torch.stack([got[("color", f, 0)] for f in range(F)])
    aug32 = torch.stack([got[("color_aug", f, 0)] for f in range(F)])
    return JitterRef(color, aug32, float64_jitter(color, case.params), (case.params[:, :, 0] > 0.5).t().contiguous())


def jitter_trace(shape):
    """per applied row of a case, in float64: (what the brightness blend sees, its factor, the hue the shift computes, the shift) --
    the op loop of oracle/ref_input.color_jitter walked one op at a time"""
    case, ref = jitter_case(shape), jitter_ref(shape)
    F, B = ref.color.shape[:2]
    for f in range(F):
        for b in range(B):
            p = case.params[b, f]
            if float(p[0]) <= 0.5:
                continue
            img, seen = ref.color[f, b].double(), {}
            for op in [int(x) for x in p[1:5]]:
                if op == 0:
                    seen["brightness_in"] = img
                elif op == 3:
                    seen["hue_in"] = img
                img = ori.color_jitter(img, [op], float(p[5]), float(p[6]), float(p[7]), float(p[8]))
            assert torch.equal(img, ref.aug64[f, b])
            yield seen["brightness_in"], float(p[5]), ori._rgb2hsv(seen["hue_in"])[0], float(p[8]), seen["hue_in"]


# ---- pyramid cases ------------------------------------------------------------------------------------------------------------
PYRAMID_SHAPES = [(2, 2), (2, 4), (4, 2), (4, 6), (6, 10), (2, 34), (34, 2), (8, 12), (18, 514)]          # (H, W)
PYRAMID_PLANES = (1, 6)
PYRAMID_KINDS = ("uniform", "edges", "zero")
PYRAMID_CASES = [(H, W, planes, kind) for (H, W) in PYRAMID_SHAPES for planes in PYRAMID_PLANES for kind in PYRAMID_KINDS]


@functools.lru_cache(maxsize=None)
def pyramid_input(H, W, planes, kind):
    """(1, planes, H, W) fp32"""
    gen = torch.Generator().manual_seed(1000 * H + W + planes)
    if kind == "uniform":
        return torch.rand(1, planes, H, W, generator=gen)
    if kind == "edges":
        return torch.randint(0, 2, (1, planes, H, W), generator=gen).float()
    return torch.zeros(1, planes, H, W)


def cubic(x):
    """Keys cubic, a = -0.5"""
    x = abs(x)
    return (1.5 * x - 2.5) * x * x + 1 if x < 1 else (((-0.5 * x + 2.5) * x - 4) * x + 2 if x < 2 else 0.0)


def down2_last_axis(v):
    """one axis of the 2x antialiased bicubic down-scale in float64: taps 2i-3 .. 2i+4 clipped to the image, weights
    cubic((t - 3.5) / 2) renormalised over the taps that remain"""
    n = v.shape[-1]
    out = np.zeros(v.shape[:-1] + (n // 2,))
    for i in range(n // 2):
        taps = [(2 * i - 3 + t, cubic((t - 3.5) * 0.5)) for t in range(8) if 0 <= 2 * i - 3 + t < n]
        tot = sum(w for _, w in taps)
        out[..., i] = sum(v[..., j] * w for j, w in taps) / tot
    return out


def pyramid_down2_f64(x):
    """(..., H, W) array -> (..., H/2, W/2) float64, horizontal pass then vertical, NOT clamped"""
    x = np.asarray(x, np.float64)
    return down2_last_axis(down2_last_axis(x).swapaxes(-1, -2)).swapaxes(-1, -2)


@functools.lru_cache(maxsize=None)
def pyramid_ref(H, W, planes, kind):
    return pyramid_down2_f64(pyramid_input(H, W, planes, kind).numpy())
