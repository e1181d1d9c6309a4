"""Shared plumbing of tests/test_metrics_parity_gpu.py and tests/test_metrics_inputs.py: depth_metrics_kernel (csrc/dd_metrics.hip,
dd_depth_metrics / dd_depth_metrics_masked) stage by stage: cases, the float64 oracle, the bounds and the judge.  Helpers only, no test.

Oracle (oracle_sample): tools.DepthMetrics and compute_errors as the reference states them (tools.py:6-73, 269-288), in numpy float64 on
the CPU on the exact fp32 values the kernel receives.  It imports neither tools.DepthMetrics nor a golden file.
  * keep rule, exact: crop bounds int(double * int); row / column / depth compared as fp32 values (torch turns the integer bounds and the
    Python depth bounds into the tensor's fp32); valid kept if non-zero (-0.0 is zero); coordinates truncated toward zero.
  * sampling: ATen's align_corners=False formula in float64 (scale = in / out, src = max(scale (d + 1/2) - 1/2, 0), i1 = min(i0 + 1, in - 1),
    value = (1-ly)((1-lx) a + lx b) + ly ((1-lx) c + lx d)), the reciprocal in float64.  (float64's own roundings, 2^-53, are left out.)
  * medians: element (n-1)//2 of the sorted kept values (torch.median: the lower one).
  * errors: scale by med_gt / med_pd, clamp to [min_depth, max_depth] as fp32 values, compute_errors; the same over each label's points.

Criterion, nothing in it from the kernel's output; U = 2^-24, every counted number of roundings floored at MIN_ROUNDINGS = 16:
  1. per point, read from the workspace (layout: include/dynamo_hip.h): ground truth bit-equal to z or -1, label and kept count equal;
       |v32 - v64| <= U (R max(taps) + 3 (src_y + 1) |bottom - top| + 3 (src_x + 1) max(|b - a|, |d - c|))
     R = BLEND_ROUNDINGS; the second and third term: the fp32 source coordinate carries three roundings of relative size U and moves the
     sampling position by up to 3 U (src + 1).  The predicted depth 1 / v adds the division's rounding.  The kernel does not store v, so
     what is compared is p = 1 / v against [1 / (v64 + bv), 1 / (v64 - bv)] widened by U.
  2. medians: med_gt has no error at all; the k-th order statistic is 1-Lipschitz in the sup norm, so |med_pd32 - med_pd64| <= E_med =
     max_i |p32_i - p64_i|'s bound.  The kernel keeps its medians to itself; what dm_select returns is judged through the metrics, here
     with these bounds and far more sharply by item 7.  The relative error of the scaled
     prediction p_i * (med_gt / med_pd) is eps_i = (1 + dp_i) (1 + U)^2 / (1 - dm) - 1 (dp_i, dm: the relative bounds of p_i and med_pd;
     two roundings: the quotient and the product); the clamp is monotone, so the clamped value lies in [clamp(s (1 - eps)), clamp(s (1 + eps))].
  3. the four error metrics, overall and per label: every term is evaluated at both ends of that interval and, where the interval
     contains g (the term's minimum, 0), there as well; the largest distance from the term at the centre counts.  Added: the roundings
     of the fp32 per-point arithmetic (TERM_ROUNDINGS) * U * the largest of those term values; for the log term the error of logf,
     LOGF_ULP ulp of each logarithm: 2 |dl| e + e^2 with e = LOGF_ULP * 2U (|log g| + |log p|).  LOGF_ULP = 3 is the OpenCL C
     specification's bound for log ("Relative error as ULPs", full profile), the requirement the ROCm device library behind HIP's logf is
     written to; HIP's math API reference lists a smaller measured figure, so 3 is the conservative documented one.  The sums are float64
     and add nothing; the final casts and square roots add one fp32 rounding each.
  4. a1..a3: a point is undecided for threshold T if |th64 - T| <= T (eps_i + 4U); the kernel's count lies within the oracle's count +-
     the undecided points.  tests/test_metrics_inputs.py asserts that no drawn case has more than one undecided point per threshold
     and sample.  `exact` cases (identity geometry, power-of-two disparities, power-of-two median ratio): the interpolation, the
     reciprocal, the ratio and the scaling are exact in fp32 and t1 = g / p, t2 = p / g are correctly rounded divisions, so the oracle
     evaluates th in numpy float32, nothing is undecided and the counts must be equal (a tie th == T is not counted).
  5. mean: recomputed in fp32, in batch order, from the kernel's own per_sample rows: bit-equal.
  6. tests/test_metrics_inputs.py runs tools.DepthMetrics._forward_torch on the CPU through the same judge (sample by sample), and
     asserts ATen's fp32 F.interpolate <= the bound of item 1 for every case: the criterion is no stricter than the reference's fp32.

  7. the fp32 chain (`chain` cases: identity geometry, every point on a pixel of its own whose four taps are equal): the sampled disparity is
     the tap itself, and every later step up to abs_rel, sq_rel and rms is ONE correctly rounded fp32 operation on known operands --
     p = 1 / v, the two medians (order statistics: no arithmetic), ratio = med_gt / med_pd, p * ratio, the clamp, d = g - p, |d| / g, d * d,
     (d * d) / g -- summed in float64, scaled, cast, square-rooted.  chain32 restates that in numpy float32 with float64 sums.  The kernel
     adds its float64 terms in another order, which moves the sum by n 2^-53 at most, so the two doubles cast to the same float or to
     neighbours: |kernel - chain32| <= one fp32 ulp of chain32's value (np.spacing), for the three metrics (stage `fp32`; log_rms goes
     through logf and keeps item 3).  Here a median that is one ulp off, or the neighbouring element, is seen: tests/test_metrics_inputs.py
     asserts from chain32 alone that such a median puts a metric outside that ulp in the cases built for it (median-bytes: z differs in
     one byte, all predictions 16; median-bytes-pd: the disparity differs in one byte, all z 12; both with the two middle values distinct).

`dyadic` cases (integer up-scale, disparities k/64): every product and sum of the blend is exact in fp32 whatever the order or
contraction, so the workspace must hold 1 / (ATen's fp32 value), bit for bit.

Outside the kernel's stated domain ("all values are positive") and not tested: zero, negative and infinite disparities.  A NaN disparity
under a kept point is tested (NaN in the sample's four error metrics).  A mask smaller than the ground truth: label 0 outside it.

SEED: no draw has broken the one-undecided-point condition or put ATen over the bound so far; if one does, change it and say so here.
"""
import functools
import types

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
MIN_ROUNDINGS = 16
SEED = 41
THRESHOLDS = (1.25, 1.5625, 1.953125)
ERR_NAMES = ("abs_rel", "sq_rel", "rms", "log_rms")
# the kernel's longest path, one per multiply / add / subtract, contraction to fma ignored (csrc/dd_bilinear.h, csrc/dd_metrics.hip)
BLEND_ROUNDINGS = 9            # w = src - i0, 1 - wx, (1-wx) a, wx b, +, 1 - wy, (1-wy) top, wy bot, +
TERM_ROUNDINGS = {"abs_rel": 2,     # d = g - p, |d| / g
                  "sq_rel": 4,      # d (twice through the square), d * d, / g
                  "sq": 3,          # d (twice), d * d
                  "sq_log": 3}      # dl = logf - logf (twice through the square), dl * dl; logf itself: LOGF_ULP
LOGF_ULP = 3
FULL = (0.0, 1.0, 0.0, 1.0)
KEEP_BOUND = (0.29, 0.57, 0.29, 0.58)


def rnd(k):
    return max(k, MIN_ROUNDINGS) * U


def _gen(*key):
    return torch.Generator().manual_seed(SEED + sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)))


def f32(x):
    return np.float32(x)


def next32(x, up):
    return np.nextafter(np.float32(x), np.float32(np.inf if up else -np.inf))


# ---- cases -------------------------------------------------------------------------------------------------------------------------
def _case(name, disp, gt_dim, samples, catches, bound=FULL, min_depth=1e-3, max_depth=80.0, mask=None, exact=False, dyadic=False, M=None, chain=False):
    """samples: per sample a list / array of rows (r, c, z, valid).  Padded to M (default: the longest) with (0, 0, 0, valid 0)."""
    B = len(samples)
    M = M or max(len(s) for s in samples)
    lidar, valid = torch.zeros((B, M, 3)), torch.zeros((B, M))
    for b, s in enumerate(samples):
        a = torch.as_tensor(np.asarray(s, dtype=np.float32).reshape(-1, 4))
        lidar[b, :a.shape[0]], valid[b, :a.shape[0]] = a[:, :3], a[:, 3]
    c = types.SimpleNamespace(name=name, disp=disp.float().contiguous(), lidar=lidar, valid=valid,
                              gt_dim=torch.as_tensor(gt_dim, dtype=torch.int32).reshape(B, 2), bound=tuple(float(v) for v in bound),
                              min_depth=float(min_depth), max_depth=float(max_depth), mask=mask, exact=exact, dyadic=dyadic or exact,
                              catches=catches, chain=chain or exact)
    c.B, c.M, c.H, c.W = B, M, disp.shape[2], disp.shape[3]
    assert disp.shape[0] == B and disp.shape[1] == 1 and bool((disp > 0).all())
    return c


def slice_case(c, b):
    """sample b alone"""
    s = types.SimpleNamespace(**vars(c))
    s.name, s.B = "%s[%d]" % (c.name, b), 1
    s.disp, s.lidar, s.valid, s.gt_dim = c.disp[b:b + 1], c.lidar[b:b + 1], c.valid[b:b + 1], c.gt_dim[b:b + 1]
    s.mask = None if c.mask is None else c.mask[b:b + 1]
    return s


def smooth_disp(B, H, W, g):
    """0.03 .. 0.12, a ramp and one slow wave: neighbouring taps differ by a few percent, so the blend term of the bound leads"""
    yy, xx = torch.arange(H).view(1, 1, H, 1) / max(H, 1), torch.arange(W).view(1, 1, 1, W) / max(W, 1)
    ph = torch.rand((B, 1, 1, 1), generator=g)
    return 0.05 + 0.02 * yy + 0.03 * xx + 0.01 * torch.sin(6.0 * (yy + xx + ph)) + 1e-4 * torch.rand((B, 1, H, W), generator=g)


def _depth_at(disp_b, gh, gw, r, c):
    full = F.interpolate(disp_b.double()[None], (gh, gw), mode="bilinear", align_corners=False)[0, 0]
    return 1.0 / full[torch.as_tensor(r).long(), torch.as_tensor(c).long()]


def _points(disp_b, gh, gw, r, c, g, frac=False, spread=0.25, min_depth=1e-3, max_depth=80.0):
    """(r, c, z, 1) rows: z = the true depth at the pixel times a log-normal factor; frac: r + 0.5, c + 0.75 (truncated by .long())"""
    r, c = torch.as_tensor(r), torch.as_tensor(c)
    z = (_depth_at(disp_b, gh, gw, r, c) * torch.exp(spread * torch.randn(r.shape[0], generator=g).double())).clamp(2 * min_depth, 0.98 * max_depth)
    rr, cc = (r.double() + 0.5, c.double() + 0.75) if frac else (r.double(), c.double())
    return torch.stack((rr, cc, z, torch.ones_like(z)), 1).float().numpy()


def _grid(gh, gw):
    r, c = torch.meshgrid(torch.arange(gh), torch.arange(gw), indexing="ij")
    return r.reshape(-1), c.reshape(-1)


def _border_and_random(gh, gw, count, g):
    """every pixel of the first and last row and column, then random pixels up to `count` points"""
    r, c = _grid(gh, gw)
    edge = (r == 0) | (r == gh - 1) | (c == 0) | (c == gw - 1)
    er, ec = r[edge], c[edge]
    k = count - er.shape[0]
    assert k > 0
    return torch.cat((er, torch.randint(0, gh, (k,), generator=g))), torch.cat((ec, torch.randint(0, gw, (k,), generator=g)))


def _geometry(name, H, W, gts, count, catches, key, disp=None, dyadic=False, frac=False):
    g = _gen(key)
    B = len(gts)
    disp = smooth_disp(B, H, W, g) if disp is None else disp
    samples = []
    for b, (gh, gw) in enumerate(gts):
        r, c = _grid(gh, gw) if count is None else _border_and_random(gh, gw, count, g)
        samples.append(_points(disp[b], gh, gw, r, c, g, frac=frac))
    return _case(name, disp, gts, samples, catches, dyadic=dyadic)


def _identity(name, samples, h, w, catches, key=0, **kw):
    """identity geometry (gt_dim = the disparity's size, 2h x 2w); samples: per sample rows (z, p, valid).  Point i sits on pixel
    (2 (s // w), 2 (s % w)), s = i % (h w), whose disparity is fp32(1 / p of the first point on it); the three pixels to its right and
    below repeat that value, so all four taps of a point are equal and the bound of its value is 16 U times the value itself"""
    B = len(samples)
    low = torch.ones((B, 1, h, w))
    rows = []
    for b, s in enumerate(samples):
        s = np.asarray(s, dtype=np.float64).reshape(-1, 3)
        n = min(s.shape[0], h * w)
        low[b, 0].view(-1)[:n] = torch.as_tensor((1.0 / s[:n, 1]).astype(np.float32))
        slot = np.arange(s.shape[0]) % (h * w)
        rows.append(np.stack((2 * (slot // w), 2 * (slot % w), s[:, 0], s[:, 2]), 1))
    disp = low.repeat_interleave(2, 2).repeat_interleave(2, 3)
    return _case(name, disp, [(2 * h, 2 * w)] * B, rows, catches, chain=True, **kw)


def _scatter(rows, M, g):
    """the rows at random places of an M-row sample whose other points are dropped (valid 0, plausible values otherwise)"""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 3)
    out = np.stack((5.0 + 20.0 * torch.rand(M, generator=g).double().numpy(), 5.0 + 20.0 * torch.rand(M, generator=g).double().numpy(), np.zeros(M)), 1)
    at = torch.randperm(M, generator=g)[:rows.shape[0]].numpy()
    out[at] = rows
    return out


def _keep_rule_case():
    g = _gen(11)
    gh = gw = 100
    disp = smooth_disp(1, 10, 10, g)
    z_ok = 14.0
    lo, hi = f32(1e-3), f32(80.0)
    rows = []
    for r in (27, 28, 29, 55, 56, 57, 28 - 0.25, 28 + 0.75, 56 - 0.5):
        rows.append((r, 40, z_ok, 1))
    for c in (27, 28, 29, 56, 57, 58, 28 - 0.25, 28 + 0.75, 57 - 0.5):
        rows.append((40, c, z_ok, 1))
    for z in (lo, next32(lo, False), next32(lo, True), hi, next32(hi, False), next32(hi, True)):
        rows.append((40, 41, z, 1))
    for v in (0.0, -0.0, 0.5, 2.0, -1.0):
        rows.append((41, 42, z_ok, v))
    r = 28 + torch.randint(0, 28, (40,), generator=g)
    c = 28 + torch.randint(0, 29, (40,), generator=g)
    rows += [tuple(p) for p in _points(disp[0], gh, gw, r, c, g, frac=True)]
    # what the reference keeps of the hand-placed rows above, in their order
    want = [0, 1, 1, 1, 0, 0, 0, 1, 1] + [0, 1, 1, 1, 0, 0, 0, 1, 1] + [0, 0, 1, 0, 1, 0] + [0, 0, 1, 1, 1]
    c = _case("keep-rule", disp, [(gh, gw)], [rows], "bounds in float (29, 57, 29, 58 instead of 28, 56, 28, 57); <= at a crop or depth bound; "
              "rounding instead of truncation; valid != 0", bound=KEEP_BOUND)
    c.want_keep = want
    return c


def _tie_rows(p):
    """(z, p, valid) rows with z = T p exactly, the float above and the float below, for the three thresholds"""
    rows = []
    for T in THRESHOLDS:
        gT = f32(T) * f32(p)
        rows += [(gT, p, 1), (next32(gT, True), p, 1), (next32(gT, False), p, 1)]
    return rows


def _cases():
    cs = []
    # ---- geometry: the per-point stage
    cs.append(_geometry("identity-7x9", 7, 9, [(7, 9)], None, "M = 63; src = d exactly: any half-pixel offset; the last row / column: i1 = i0", 1))
    for f, (h, w) in ((2, (6, 5)), (4, (3, 4))):
        g = _gen(2, f)
        disp = torch.randint(8, 41, (2, 1, h, w), generator=g).float() / 64
        cs.append(_geometry("dyadic-x%d" % f, h, w, [(f * h, f * w)] * 2, None, "one border tap off, a swapped weight: bit equality with ATen", 20 + f,
                            disp=disp, dyadic=True))
    cs.append(_geometry("kitti-like", 12, 40, [(37, 123)] * 2, 1025, "M = 1025: the point behind the 1024-thread stride; a non-integer up-scale, both clamps", 3))
    cs.append(_geometry("down-scale", 50, 70, [(17, 23)], None, "scale > 1: taps 2.9 pixels apart, no clamp at the far border", 4))
    cs.append(_geometry("disp-1x1", 1, 1, [(5, 7)], None, "in_size 1 on both axes: i0 = i1 = 0 everywhere", 5))
    cs.append(_geometry("disp-1x13", 1, 13, [(4, 30)], None, "one row: y1 = y0", 6))
    cs.append(_geometry("disp-13x1", 13, 1, [(30, 4)], None, "one column: h and w swapped", 7))
    cs.append(_geometry("two-gt-dims", 12, 40, [(37, 123), (24, 80)], 500, "gt_dim read per sample; fractional coordinates", 8, frac=True))
    g = _gen(9)
    cs.append(_geometry("white-noise", 12, 40, [(37, 123)], 1024, "M = 1024; taps that differ by two orders of magnitude: the coordinate term leads", 9,
                        disp=0.01 + 0.99 * torch.rand((1, 1, 12, 40), generator=g)))
    # ---- keep rule
    cs.append(_keep_rule_case())
    # ---- medians (identity geometry: z and p of every point chosen)
    cs.append(_identity("median-M1", [[(10.0, 7.0, 1)]], 1, 1, "M = 1, n = 1"))
    g = _gen(12)
    dup = [(1, 3, 1), (2, 4, 1), (3, 5, 1), (4, 5.5, 1), (5, 6, 1), (5, 6, 1), (5, 6, 1), (8, 7, 1), (9, 9, 1), (10, 11, 1)]
    even = [(float(z), float(p), 1) for z, p in zip(2 + 40 * torch.rand(8, generator=g), 2 + 40 * torch.rand(8, generator=g))]
    cs.append(_identity("median-small-n", [_scatter([(10, 5, 1), (30, 40, 1)], 63, g), _scatter([(3, 9, 1), (12, 2, 1), (40, 30, 1)], 63, g),
                                           _scatter(even, 63, g), [(7.5, 3.0, 1)] * 63, _scatter(dup, 63, g)], 7, 9,
                        "n = 2, 3, 8: the upper median; all values equal; duplicates on both sides of the middle; kept among dropped", 12))
    g = _gen(13)
    def two_sided(lo, mid, hi, half):
        """`half` byte values below `mid` and `half` above it, shuffled: duplicates everywhere, the two middle values distinct, the
        mean off the median (a shifted median then moves rms in first order)"""
        v = torch.cat((torch.randint(lo, mid, (half,), generator=g), torch.randint(mid + 1, hi, (half,), generator=g)))
        return v[torch.randperm(2 * half, generator=g)].numpy().astype(np.uint32)

    def with_byte(base, byte, v):
        return ((np.uint32(base) & ~np.uint32(0xFF << (8 * byte))) | (v << np.uint32(8 * byte))).astype(np.uint32).view(np.float32).astype(np.float64)

    # byte 2 holds the lowest exponent bit: kept set, so that z stays within one binade; byte 3: 0x3B.. (0.002) to 0x42.. (33)
    spans = ((0, 100, 256), (0, 100, 256), (0x80, 0xB0, 0x100), (0x3B, 0x3D, 0x43))
    samples = []
    for byte in range(4):
        z = with_byte(0x4103C5E7 if byte == 3 else 0x41A3C5E7, byte, two_sided(*spans[byte], 512))
        samples.append(np.stack((z, np.full(1024, 16.0), np.ones(1024)), 1))
    cs.append(_identity("median-bytes", samples, 25, 35, "a radix pass of the ground-truth select that mishandles one byte, or equal values: z differs in "
                        "byte 0 / 1 / 2 / 3 only (sample = byte), every prediction is 16", 13))
    # the same for the prediction's select: the DISPARITY differs in one byte (1.27 * 2^-4 -> p about 12.6; distinct d give distinct p there)
    spans = ((0, 100, 256), (0, 100, 256), (0x80, 0xB0, 0x100), (0x3A, 0x3D, 0x42))
    samples = []
    for byte in range(4):
        d = with_byte(0x3D03C5E7 if byte == 3 else 0x3DA3C5E7, byte, two_sided(*spans[byte], 400))
        samples.append(np.stack((np.full(800, 12.0), 1.0 / d, np.ones(800)), 1))
    c = _identity("median-bytes-pd", samples, 25, 35, "a radix pass of the prediction's select that mishandles one byte: the disparity differs in "
                  "byte 0 / 1 / 2 / 3 only, every z is 12", 18)
    for byte in range(4):          # the disparity itself, not fp32(1 / (1 / d))
        low = torch.as_tensor(samples[byte][:, 1] ** -1).float()
        c.disp[byte, 0, 0::2, 0::2].reshape(-1)[:800] = low
        c.disp[byte, 0] = c.disp[byte, 0, 0::2, 0::2].repeat_interleave(2, 0).repeat_interleave(2, 1)
    cs.append(c)
    g = _gen(14)
    samples = []
    for b in range(2):
        z = 2.0 ** (-9.0 + 15.0 * torch.rand(1025, generator=g).double().numpy())
        p = 2.0 ** (-9.0 + 15.0 * torch.rand(1025, generator=g).double().numpy())
        v = (torch.rand(1025, generator=g) < 0.5).double().numpy() if b == 0 else np.ones(1025)
        samples.append(np.stack((z, p, v), 1))
    cs.append(_identity("median-exponents", samples, 25, 35, "values across fifteen exponents; half of sample 0 dropped at random; M = 1025", 14))
    g = _gen(15)
    samples = []
    for b in range(2):
        z = 2.0 + 60.0 * torch.rand(2500, generator=g).double().numpy()
        p = z * np.exp(0.2 * torch.randn(2500, generator=g).double().numpy())
        v = (np.arange(2500) > 2048).astype(np.float64) if b == 0 else np.ones(2500)
        samples.append(np.stack((z, p, v), 1))
    cs.append(_identity("median-M2500", samples, 25, 25, "M = 2500: three trips of the stride; sample 0 keeps only points beyond index 2048", 15))
    # ---- clamp (exact: powers of two, min_depth = 2^-4, max_depth = 64)
    ps = [2.0 ** -8, 2.0 ** -6, 2.0 ** -4, 16.0, 64.0, 256.0] + [1.0] * 9
    z1 = [0.08, 0.1, 0.2, 20.0, 30.0, 50.0, 0.5, 0.7, 0.9, 1.0, 1.0, 2.0, 3.0, 4.0, 5.0]              # lower median 1: ratio 1
    z4 = [0.3, 0.4, 0.8, 30.0, 40.0, 60.0, 2.0, 2.8, 3.6, 4.0, 4.0, 8.0, 12.0, 16.0, 20.0]            # lower median 4: ratio 4
    cs.append(_identity("clamp", [[(z, p, 1) for z, p in zip(z1, ps)], [(z, p, 1) for z, p in zip(z4, ps)]], 3, 5,
                        "a clamp on the wrong side or missing: scaled predictions below min_depth, on it, on max_depth, above it (ratio 1 and 4)",
                        min_depth=2.0 ** -4, max_depth=64.0, exact=True))
    # ---- threshold ties (exact)
    s0 = _tie_rows(8.0) + [(8.0, 8.0, 1)] + [(4.0, 8.0, 1)] * 9
    s1 = []
    for p in (2.0, 4.0, 8.0, 16.0):
        s1 += _tie_rows(p)
    s1 += [(1.5, 2.0, 1)] * 30 + [(2.0, 2.0, 1)] * 7
    cs.append(_identity("threshold-ties", [s0, s1], 8, 10, "th <= T: g = T p exactly, and the float above and below, T = 1.25, 1.25^2, 1.25^3", exact=True))
    # ---- masked path
    g = _gen(16)
    gh, gw = 37, 123
    disp = smooth_disp(3, 12, 40, g)
    idx = torch.arange(gh * gw)
    mask = torch.zeros((3, gh, gw), dtype=torch.uint8)
    mask[0] = (idx % 256).to(torch.uint8).view(gh, gw)                       # all 256 labels; horizontal neighbours differ
    m1 = torch.where(torch.arange(gw) < 60, 0, 255).to(torch.uint8).repeat(gh, 1)
    m1[5, 5], m1[6, 100], m1[30, 30] = 7, 8, 9                                  # 7 and 8: one point each; 9: under a dropped point only
    mask[1] = m1
    mask[2] = 3
    r, c = _border_and_random(gh, gw, 1019, g)
    hit = ((r == 5) & (c == 5)) | ((r == 6) & (c == 100)) | ((r == 30) & (c == 30))     # the pixels of labels 7, 8, 9 get their points below
    r[hit], c[hit] = 1, 1
    extra = torch.tensor([[5, 5], [6, 100], [5, 6], [6, 99], [30, 30], [30, 31]])
    samples = []
    for b in range(3):
        if b == 0:             # the first 1025 pixels: every label at least four times
            rows = _points(disp[b], gh, gw, idx[:1025] // gw, idx[:1025] % gw, g, frac=True)
        else:
            rows = _points(disp[b], gh, gw, torch.cat((r, extra[:, 0])), torch.cat((c, extra[:, 1])), g, frac=True)
        if b == 1:
            on9 = (rows[:, 0].astype(np.int64) == 30) & (rows[:, 1].astype(np.int64) == 30)
            rows[on9, 3] = 0.0
        if b == 2:
            rows[:, 3] = 0.0
        samples.append(rows)
    cs.append(_case("masked-labels", disp, [(gh, gw)] * 3, samples, "a label loop that ends at 255; the label of a neighbouring pixel under fractional "
                    "coordinates; single-point labels; a label under dropped points only; a sample with n = 0 inside a masked batch", mask=mask))
    g = _gen(17)
    disp = smooth_disp(1, 12, 40, g)
    r, c = _border_and_random(gh, gw, 400, g)
    cs.append(_case("masked-small-mask", disp, [(gh, gw)], [_points(disp[0], gh, gw, r, c, g)], "a mask of 20x60 under 37x123 ground truth: label 0 "
                    "outside it, the row stride of the mask is mask_w", mask=torch.randint(1, 5, (1, 20, 60), generator=g, dtype=torch.uint8)))
    return cs


CASES = _cases()
CASE_IDS = [c.name for c in CASES]


def by_name(name):
    return CASES[CASE_IDS.index(name)]


# ---- the float64 oracle ------------------------------------------------------------------------------------------------------------
def _axis(d, in_size, out_size):
    scale = float(in_size) / float(out_size)
    raw = scale * (d.astype(np.float64) + 0.5) - 0.5
    src = np.maximum(raw, 0.0)
    i0 = np.minimum(np.floor(src).astype(np.int64), in_size - 1)
    i1 = np.minimum(i0 + 1, in_size - 1)
    return raw, src, i0, i1, src - i0


def _terms(g, p):
    d, dl = g - p, np.log(g) - np.log(p)
    return {"abs_rel": np.abs(d) / g, "sq_rel": d * d / g, "sq": d * d, "sq_log": dl * dl}


def _stats(o, sel, c):
    """metrics and bounds over the kept points picked by `sel`"""
    s = types.SimpleNamespace(n=int(sel.sum()))
    g, pc, lo, hi, eps = o.z64[sel], o.pc64[sel], o.lo[sel], o.hi[sel], o.eps[sel]
    t_c, t_lo, t_hi = _terms(g, pc), _terms(g, lo), _terms(g, hi)
    inside = (lo <= g) & (g <= hi)
    mean, delta = {}, {}
    for k in t_c:
        dev = np.maximum(np.abs(t_lo[k] - t_c[k]), np.abs(t_hi[k] - t_c[k]))
        dev = np.maximum(dev, np.where(inside, t_c[k], 0.0))
        top = np.maximum(np.maximum(t_lo[k], t_hi[k]), t_c[k])
        dev = dev + rnd(TERM_ROUNDINGS[k]) * top
        if k == "sq_log":
            e = LOGF_ULP * 2 * U * (np.abs(np.log(g)) + np.maximum(np.abs(np.log(lo)), np.abs(np.log(hi))))
            dev = dev + 2 * np.sqrt(top) * e + e * e
        mean[k], delta[k] = float(t_c[k].mean()), float(dev.mean())
    s.m64, s.bound = np.zeros(4), np.zeros(4)
    for j, k in enumerate(("abs_rel", "sq_rel")):
        s.m64[j], s.bound[j] = mean[k], delta[k] + U * (mean[k] + delta[k])
    for j, k in ((2, "sq"), (3, "sq_log")):
        r = np.sqrt(mean[k])
        up = np.sqrt((mean[k] + delta[k]) * (1 + U)) * (1 + U)
        dn = np.sqrt(max(mean[k] - delta[k], 0.0) * (1 - U)) * (1 - U)
        s.m64[j], s.bound[j] = r, max(up - r, r - dn)
    if c.exact:
        th = o.th32[sel]
        s.cnt = [int((th < f32(T)).sum()) for T in THRESHOLDS]
        s.und = [0, 0, 0]
    else:
        th = np.maximum(g / pc, pc / g)
        s.cnt = [int((th < T).sum()) for T in THRESHOLDS]
        s.und = [int((np.abs(th - T) <= T * (eps + 4 * U)).sum()) for T in THRESHOLDS]
    return s


def shift32(x, ulps):
    return (np.asarray(x, dtype=np.float32).view(np.uint32) + np.uint32(ulps)).view(np.float32) if ulps >= 0 else \
        (np.asarray(x, dtype=np.float32).view(np.uint32) - np.uint32(-ulps)).view(np.float32)


def chain32(o, c, gt_ulps=0, pd_ulps=0, upper=False):
    """abs_rel, sq_rel, rms of sample `o` of a chain case as the fp32 operations give them (criterion 7).  gt_ulps, pd_ulps, upper: a
    median that many ulps off / the upper median -- what tests/test_metrics_inputs.py uses to show that such a fault is seen"""
    lo32, hi32 = f32(c.min_depth), f32(c.max_depth)
    p = (f32(1.0) / o.v64.astype(np.float32)).astype(np.float32)
    k = o.n // 2 if upper else (o.n - 1) // 2
    ratio = f32(shift32(np.sort(o.z)[k], gt_ulps) / shift32(np.sort(p)[k], pd_ulps))
    s = (p * ratio).astype(np.float32)
    s = np.where(s < lo32, lo32, np.where(s > hi32, hi32, s)).astype(np.float32)
    d = (o.z - s).astype(np.float32)
    dd = (d * d).astype(np.float32)
    inv = 1.0 / float(o.n)
    tot = [float((np.abs(d) / o.z).astype(np.float32).astype(np.float64).sum()), float((dd / o.z).astype(np.float32).astype(np.float64).sum()),
           float(dd.astype(np.float64).sum())]
    return np.asarray([f32(tot[0] * inv), f32(tot[1] * inv), np.sqrt(f32(tot[2] * inv))], dtype=np.float32)


def oracle_sample(c, b):
    o = types.SimpleNamespace()
    disp = c.disp[b, 0].numpy()
    pts, valid = c.lidar[b].numpy(), c.valid[b].numpy()
    r, col, z = pts[:, 0], pts[:, 1], pts[:, 2]
    gh, gw = int(c.gt_dim[b, 0]), int(c.gt_dim[b, 1])
    H, W = disp.shape
    up, down = int(c.bound[0] * gh), int(c.bound[1] * gh)
    left, right = int(c.bound[2] * gw), int(c.bound[3] * gw)
    lo32, hi32 = f32(c.min_depth), f32(c.max_depth)
    o.bounds_int = (up, down, left, right)
    o.keep = (valid != 0) & (r >= f32(up)) & (r < f32(down)) & (col >= f32(left)) & (col < f32(right)) & (z > lo32) & (z < hi32)
    o.n = int(o.keep.sum())
    o.idx = np.nonzero(o.keep)[0]
    o.rows, o.cols = np.trunc(r[o.keep]).astype(np.int64), np.trunc(col[o.keep]).astype(np.int64)
    o.z = z[o.keep]
    o.z64 = o.z.astype(np.float64)
    o.labels = None
    if c.mask is not None:
        m = c.mask[b].numpy()
        ins = (o.rows < m.shape[0]) & (o.cols < m.shape[1])
        o.labels = np.where(ins, m[np.minimum(o.rows, m.shape[0] - 1), np.minimum(o.cols, m.shape[1] - 1)], 0).astype(np.int64)
    o.by_label = {}
    if o.n == 0:
        return o
    # sampling
    o.raw_y, sy, y0, y1, ly = _axis(o.rows, H, gh)
    o.raw_x, sx, x0, x1, lx = _axis(o.cols, W, gw)
    o.y0, o.x0 = y0, x0
    d64 = disp.astype(np.float64)
    ta, tb, tc, td = d64[y0, x0], d64[y0, x1], d64[y1, x0], d64[y1, x1]
    top, bot = (1 - lx) * ta + lx * tb, (1 - lx) * tc + lx * td
    o.v64 = (1 - ly) * top + ly * bot
    tmax = np.maximum(np.maximum(ta, tb), np.maximum(tc, td))
    o.blend_part = rnd(BLEND_ROUNDINGS) * tmax
    o.coord_part = U * (3 * (sy + 1) * np.abs(bot - top) + 3 * (sx + 1) * np.maximum(np.abs(tb - ta), np.abs(td - tc)))
    o.bv = o.blend_part + o.coord_part
    assert bool((o.bv < o.v64).all())
    o.p64 = 1.0 / o.v64
    ep = 1.0 / (o.v64 - o.bv) - o.p64
    o.ep = ep + U * (o.p64 + ep)
    full32 = F.interpolate(c.disp[b][None], (gh, gw), mode="bilinear", align_corners=False)[0, 0]
    o.aten32 = full32[torch.as_tensor(o.rows), torch.as_tensor(o.cols)].numpy()
    o.p_aten32 = (f32(1.0) / o.aten32).astype(np.float32)
    # medians
    k = (o.n - 1) // 2
    o.med_gt = np.sort(o.z)[k]
    o.med_pd64 = np.sort(o.p64)[k]
    o.e_med = float(o.ep.max())
    dm = o.e_med / o.med_pd64
    assert dm < 0.5
    ratio = float(o.med_gt) / o.med_pd64
    s64 = o.p64 * ratio
    o.eps = (1 + o.ep / o.p64) * (1 + U) ** 2 / (1 - dm) - 1
    lo64, hi64 = float(lo32), float(hi32)
    o.s64 = s64
    o.pc64 = np.clip(s64, lo64, hi64)
    o.lo, o.hi = np.clip(s64 * (1 - o.eps), lo64, hi64), np.clip(s64 * (1 + o.eps), lo64, hi64)
    if c.exact:              # everything up to th is exact or one correctly rounded fp32 operation: evaluate it in fp32
        p32 = f32(1.0) / o.v64.astype(np.float32)
        r32 = np.float32(o.med_gt) / np.sort(p32)[k]
        s32 = (p32 * r32).astype(np.float32)
        o.exact_ok = bool((o.v64.astype(np.float32).astype(np.float64) == o.v64).all() and (p32.astype(np.float64) == o.p64).all()
                          and float(r32) == ratio and (s32.astype(np.float64) == s64).all())
        s32 = np.where(s32 < lo32, lo32, np.where(s32 > hi32, hi32, s32)).astype(np.float32)
        o.th32 = np.maximum(o.z / s32, s32 / o.z)
    o.all = _stats(o, np.ones(o.n, dtype=bool), c)
    o.all.m32 = None
    if c.chain:
        o.chain_ok = bool((o.v64.astype(np.float32).astype(np.float64) == o.v64).all() and (o.aten32.astype(np.float64) == o.v64).all())
        o.all.m32 = chain32(o, c)
    if o.labels is not None:
        for l in np.unique(o.labels):
            o.by_label[int(l)] = _stats(o, o.labels == l, c)
    return o


@functools.lru_cache(maxsize=None)
def oracle(ci):
    c = CASES[ci]
    return [oracle_sample(c, b) for b in range(c.B)]


# ---- the judge ---------------------------------------------------------------------------------------------------------------------
STAGES = ("point",) + ERR_NAMES + ("fp32", "counts", "labels")


class Judge:
    """Collects the comparisons of one case; finish() prints the case's `worst:` line (profiles/metrics_parity.txt keeps them): per stage
    the largest error-to-bound ratio (exact stages: 0 or inf), and returns the failures."""

    def __init__(self, c, what="dd_depth_metrics", fp32_chain=True):
        """fp32_chain=False leaves criterion 7 out: it rests on the kernel's float64 sums, and the CPU restatement (the reference's
        own arithmetic) takes its means in fp32"""
        self.c, self.what, self.fails, self.fp32_chain = c, what, [], fp32_chain
        self.worst = {s: 0.0 for s in STAGES}
        self.exact_checks = 0

    def _ratio(self, stage, err, bound, msg):
        err = np.atleast_1d(np.asarray(err, dtype=np.float64))
        bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), err.shape)
        if err.size == 0:
            return
        bad = ~np.isfinite(err)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(err == 0, 0.0, err / bound)
        ratio = np.where(bad, np.inf, ratio)
        i = int(np.argmax(ratio))
        self.worst[stage] = max(self.worst[stage], float(ratio[i]))
        if not ratio[i] <= 1.0:
            self.fails.append("%s %s: %d of %d over the bound, worst %.3gx at %d: err %.3e, bound %.3e" % (
                self.c.name, msg, int((ratio > 1.0).sum()), err.size, float(ratio[i]), i, float(err[i]), float(bound[i])))

    def same(self, stage, ok, msg):
        self.exact_checks += 1
        if not ok:
            self.worst[stage] = float("inf")
            self.fails.append("%s %s" % (self.c.name, msg))

    def points(self, b, o, ws_gt, ws_pd, ws_label=None):
        """the workspace of sample b: ws_gt, ws_pd (M,) float32, ws_label (M,) int32 or None"""
        want_gt = np.where(o.keep, self.c.lidar[b, :, 2].numpy(), f32(-1.0)).astype(np.float32)
        self.same("point", np.array_equal(want_gt.view(np.uint32), ws_gt.view(np.uint32)),
                   "sample %d: ground-truth slots differ at %s" % (b, np.nonzero(want_gt.view(np.uint32) != ws_gt.view(np.uint32))[0][:8]))
        self.same("point", bool((ws_pd[~o.keep] == f32(-1.0)).all()), "sample %d: a dropped point's prediction slot is not -1" % b)
        if o.n == 0:
            return
        got = ws_pd[o.keep]
        if self.c.dyadic:
            self.same("point", np.array_equal(got.view(np.uint32), o.p_aten32.view(np.uint32)),
                       "sample %d: 1 / interpolated disparity is not ATen's, bit for bit (%d of %d differ)" % (b, int((got != o.p_aten32).sum()), o.n))
        self._ratio("point", np.abs(got.astype(np.float64) - o.p64), o.ep, "sample %d predicted depth" % b)
        if ws_label is not None:
            self.same("point", np.array_equal(ws_label[o.keep].astype(np.int64), o.labels), "sample %d: labels differ" % b)

    def _row(self, stage_of, s, row, msg, count=True):
        row = np.asarray(row, dtype=np.float32)
        if count:
            self.same(stage_of("count"), float(row[7]) == s.n, "%s: count %r, oracle %d" % (msg, float(row[7]), s.n))
        for j, name in enumerate(ERR_NAMES):
            self._ratio(stage_of(name), abs(float(row[j]) - s.m64[j]), s.bound[j], "%s %s (oracle %.9g)" % (msg, name, s.m64[j]))
        if self.fp32_chain and getattr(s, "m32", None) is not None:          # criterion 7: within one ulp of the fp32 chain
            for j, name in enumerate(ERR_NAMES[:3]):
                self._ratio("fp32", abs(float(row[j]) - float(s.m32[j])), float(np.spacing(s.m32[j])), "%s %s (fp32 chain %.9g)" % (msg, name, s.m32[j]))
        for j, T in enumerate(THRESHOLDS):
            a = float(row[4 + j])
            k = int(round(a * s.n)) if np.isfinite(a) else -1
            ok = k >= 0 and abs(a - k / s.n) <= 2 * U and abs(k - s.cnt[j]) <= s.und[j]
            self.same(stage_of("a"), ok, "%s a%d: %r = %d of %d, oracle %d +- %d" % (msg, j + 1, a, k, s.n, s.cnt[j], s.und[j]))

    def sample(self, b, o, row, count=True):
        """per_sample[b] (8,)"""
        row = np.asarray(row, dtype=np.float32)
        if o.n == 0:
            self.same("counts", bool(np.isnan(row[:7]).all()) and (not count or row[7] == 0), "sample %d: no kept point, row %s" % (b, row))
            return
        self._row(lambda name: name if name in ERR_NAMES else "counts", o.all, row, "sample %d" % b, count)

    def labels(self, b, o, rows, count=True):
        """per_label[b] (256, 8); count=False: rows[:, 7] is not looked at for labels that occur (the CPU restatement has none)"""
        rows = np.asarray(rows, dtype=np.float32)
        total = 0
        for l in range(256):
            if l in o.by_label:
                self._row(lambda name: "labels", o.by_label[l], rows[l], "sample %d label %d" % (b, l), count)
                total += o.by_label[l].n
            else:
                self.same("labels", bool((rows[l].view(np.uint32) == 0).all()), "sample %d label %d: not a zero row: %s" % (b, l, rows[l]))
        self.same("labels", total == o.n, "sample %d: the label counts do not sum to n" % b)

    def mean(self, per_sample, mean):
        """bit-equal to the fp32 sum of the kernel's own rows in batch order, divided by B"""
        per_sample, mean = np.asarray(per_sample, dtype=np.float32), np.asarray(mean, dtype=np.float32)
        acc = np.zeros(7, dtype=np.float32)
        with np.errstate(invalid="ignore"):
            for b in range(per_sample.shape[0]):
                acc = (acc + per_sample[b, :7]).astype(np.float32)
            want = (acc / f32(per_sample.shape[0])).astype(np.float32)
        same = bool(((want.view(np.uint32) == mean.view(np.uint32)) | (np.isnan(want) & np.isnan(mean))).all())
        self.same("counts", same, "mean %s, from the rows %s" % (mean, want))

    def finish(self):
        print("worst: %s | %s | %s | %d exact checks" % (self.what, self.c.name, " | ".join("%s %.3f" % (s, self.worst[s]) for s in STAGES), self.exact_checks))
        return self.fails
