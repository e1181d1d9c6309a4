"""Shared plumbing of tests/test_fewch_parity_gpu.py and tests/test_fewch_inputs.py: the few-channel convolutions between the encoders
and the loss -- csrc/dd_conv_small.hip (the motion decoders' 3x3 and 1x1 convolutions on 1-16 channels), csrc/dd_conv_head.hip (the
disparity heads, 3x3 to one channel), conv3x3_cout1_bwd_data_kernel of csrc/dd_dwconv.hip (the heads' data gradient) and
csrc/dd_redu.hip (conv1x1(cat(a, b)) to 1 or 3 channels): cases, float64 references, bounds, the launch-geometry arithmetic restated
from the kernels' constants, and thin C-ABI launchers that put every output and every workspace between NaN guard bands.  Helpers
only, no test.

Reference: F.conv2d and its autograd adjoints (conv2d_input, conv2d_weight) in float64 on the CPU on the exact fp32 values the kernel
gets; the same in fp32 gives rho_32.  Nothing in a bound comes from the kernel's output.

  * element-wise outputs (y, g_x, out, g_a, g_b):   |kernel_i - ref64_i| <= scale_i * max(4 * rho_32, F)
      scale_i = the operator's sum of absolute terms (the same torch call on |x|, |w|, |b| resp. |g|), F = 2^-24 * max(R, 16) with R the
      roundings on the kernel's longest leaf-to-output path (ROUNDINGS), rho_32 = max_j |ref32_j - ref64_j| / scale_j;
      tests/test_fewch_inputs.py asserts rho_32 <= F for every case: the fp32 reference is inside F * scale_i by itself, and the bound
      in force is F * scale_i wherever 4 rho_32 <= F, never more than 4 F * scale_i.  Measured rho_32 in units of 2^-24 (F in
      brackets): conv_small 3x3 y 6-10 (81-144), g_x 6-9 (81-144), 1x1 3-4 (16); head out 6 / 8 (17 / 18), g_x 4 (16); redu y 15 (16)
      at C = 64-256 and 8 (19) at C = 512, g_a / g_b 3 (16).
  * sums over pixels (g_weight, g_bias):            |kernel - ref64| <= 2^-24 * (D + 1) * sum |terms|
      sum |terms| = conv2d_weight(|x|, |g|) resp. sum |g| in float64; D the additions on the kernel's longest chain for that launch
      (cs_depth, ch_depth, rd_depth: tiles per workgroup, matrix steps per tile times 4, the 4-wave add, both fold levels), + 1 for
      the product.  No fp32 yardstick: the fp32 CPU conv2d_weight has its own summation order.
  * kind "int": |x| <= 4, |w| <= 2, |g| <= 4, |b| <= 8 on the integers with sum |terms| < 2^24 for every output: every partial sum in
      any order is exact in fp32, the comparison is torch.equal -- the test that sees a dropped or doubled pixel, tap, channel or
      partial (one pixel of 2 * 10^5 is inside D * 2^-24).

Inputs ("off"): x = |N(0,1)| + 1 (post-ELU / image stacks: a mean), w = 0.2 N + 0.1, g = 0.5 N + 1, b = N(0,1); "zero": the
zero-centred draws of the older tests, one control per family.  The generator is seeded from the case key."""
import collections
import functools

import torch
import torch.nn.functional as F

import norm_case as NC
import ops_case as OC
from norm_case import Judge, U, FACTOR, MIN_ROUNDINGS, rho32, elem_bound, guarded, guards_intact          # noqa: F401 (re-exported)

F32 = torch.float32
SEED = 53          # no draw has put an fp32 reference over F so far; if one does, change the case and say so here (never the bound)
KINDS = ("off", "zero", "int")
INT_X, INT_W, INT_G, INT_B = 4, 2, 4, 8
EXACT_LIMIT = 2 ** 24


def _ceil(a, b):
    return -(-a // b)


def _log2(n):
    assert n & (n - 1) == 0
    return n.bit_length() - 1


# the longest leaf-to-output path in the kernel: one per multiply, add and fma (an fma rounds once)
ROUNDINGS = {
    # csrc/dd_conv_small.hip, conv_small_kernel: acc = bias, then one fmaf per (tap, ci); the data gradient is the same kernel, roles swapped
    "cs y": lambda ks, cin, cout: ks * ks * cin,
    "cs g_x": lambda ks, cin, cout: ks * ks * cout,
    # csrc/dd_conv_head.hip, conv_head_fwd_kernel: dot4 = a product and three fmaf (4); acc += dot4 for nine taps (9); the shuffle tree
    # over the pixel's LPP lanes (log2 LPP); + bias (1)
    "ch out": lambda lpp: 4 + 9 + _log2(lpp) + 1,
    # csrc/dd_dwconv.hip, conv3x3_cout1_bwd_data_kernel: one fmaf per tap in the image
    "c1 g_x": lambda: 9,
    # csrc/dd_redu.hip, redu_fwd_kernel: per quad rd_dot4(a) (4), rd_dot4(b) in parallel, their sum (1), acc += (1): 6; the shuffle tree; + bias
    "rd y": lambda lpp, quads: quads * 6 + _log2(lpp) + 1,
    # redu_bwd_data_kernel: one fmaf per output channel
    "rd g_ab": lambda cout: cout,
}


def floor(kind, *args):
    return max(ROUNDINGS[kind](*args), MIN_ROUNDINGS) * U


def _gen(*key):
    return torch.Generator().manual_seed(SEED + sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)))


def _draw(gen, kind, what, shape):
    if kind == "int":
        m = {"x": INT_X, "w": INT_W, "g": INT_G, "b": INT_B}[what]
        return torch.randint(-m, m + 1, shape, generator=gen).float()
    n = torch.randn(shape, generator=gen)
    if kind == "zero":
        return {"x": n, "w": 0.2 * n, "g": n, "b": n}[what]
    return {"x": n.abs() + 1.0, "w": 0.2 * n + 0.1, "g": 0.5 * n + 1.0, "b": n}[what]


# ---- the one reference: a convolution, its data gradient and its weight / bias gradient --------------------------------------------
def _conv_pass(x, w, g, pad, D, absolute, want_gw):
    cv = (lambda t: t.to(D).abs()) if absolute else (lambda t: t.to(D).clone())          # never the stored tensor itself: .to() returns it at D = fp32
    xl, wl = cv(x).requires_grad_(), cv(w).requires_grad_()
    y = F.conv2d(xl, wl, None, 1, pad)
    grads = torch.autograd.grad(y, [xl, wl] if want_gw else [xl], cv(g))
    return y.detach(), grads[0], (grads[1] if want_gw else None)


def conv_ref(x, w, b, g, pad, exact):
    """x (B,cin,H,W), w (cout,cin,k,k), b (cout,), g (B,cout,Ho,Wo): fp32 CPU tensors.  -> Ref with, in float64: y0 (no bias), y, g_x,
    g_w, g_b; the fp32 evaluations y0_32, y_32, g_x32; the scales s_y0, s_y, s_gx and the sums of absolute terms t_gw, t_gb.
    exact: small-integer operands -- the float64 results only, and the assertion that every sum of absolute terms is below 2^24."""
    r = OC.Ref()
    r.x, r.w, r.b, r.g, r.pad, r.exact = x, w, b, g, pad, exact
    r.y0, r.g_x, r.g_w = _conv_pass(x, w, g, pad, torch.float64, False, True)
    r.y = r.y0 + b.double().view(1, -1, 1, 1)
    r.g_b = g.double().sum((0, 2, 3))
    r.t_gb = g.double().abs().sum((0, 2, 3))
    if exact:
        cin, k = w.shape[1], w.shape[2]
        pixels = g.shape[0] * g.shape[2] * g.shape[3]
        # sufficient for every output: terms per output times the largest term
        r.exact_sums = (k * k * cin * INT_X * INT_W + INT_B, k * k * w.shape[0] * INT_G * INT_W, pixels * INT_X * INT_G, pixels * INT_G)
        assert float(x.abs().max()) <= INT_X and float(w.abs().max()) <= INT_W and float(g.abs().max()) <= INT_G and float(b.abs().max()) <= INT_B
        return r
    r.s_y0, r.s_gx, r.t_gw = _conv_pass(x, w, g, pad, torch.float64, True, True)
    r.s_y = r.s_y0 + b.double().abs().view(1, -1, 1, 1)
    y0_32, g_x32, _ = _conv_pass(x, w, g, pad, torch.float32, False, False)
    r.y0_32, r.g_x32 = y0_32.double(), g_x32.double()
    r.y_32 = (y0_32 + b.view(1, -1, 1, 1)).double()
    return r


def depth_bound(D, terms):
    return U * (D + 1) * terms


def _fold_chain(nparts, fold, unroll):
    """additions on the longest chain of a first fold level: slice 0 adds ceil(nparts / fold) partials into `unroll` accumulators
    (at most floor(n / unroll) in the unrolled body and unroll - 1 in the tail, never more than n) and adds the accumulators in a tree"""
    n = _ceil(nparts, fold)
    return min(n, n // unroll + unroll - 1) + _log2(unroll)


def _fold2_chain(fold):
    """the second level: `fold` slices into four accumulators, then a two-level tree"""
    return fold // 4 + 2


# ---- dd_conv_small -----------------------------------------------------------------------------------------------------------------
CS_NT, CS_TH, CS_TW, CS_MAXC = 256, 8, 32, 16          # dd_conv_small.hip:24-25
CS_WG_BLOCKS = 1024                                    # dd_conv_small.hip:26
CS_FOLD = 32                                           # dd_conv_small.hip:195
CS_MTS = (1, 6, 7, 8, 10)                              # dd_conv_small.hip:270, the instantiations of DD_CS_WG (:318)
# DD_CS_PAIRS, dd_conv_small.hip:244-246
CS_PAIRS = ((3, 12, 9), (3, 10, 9), (3, 9, 9), (3, 9, 12), (3, 9, 10), (3, 16, 12), (3, 13, 12), (3, 12, 12), (3, 12, 16), (3, 12, 13),
            (1, 9, 3), (1, 9, 1), (1, 3, 9), (1, 1, 9), (1, 12, 3), (1, 12, 1), (1, 3, 12), (1, 1, 12))


def cs_mt(ks, cin):
    """conv_small_mt: M-tiles of the patch matrix, KS*KS*cin rows and the one bias row"""
    return _ceil(ks * ks * cin + 1, 16)


def cs_supported(ks, cin, cout):
    """dd_conv_small_supported restated: both roles of the pair are instantiated and the weight gradient has its M-tile count"""
    if ks not in (1, 3) or not (1 <= cin <= CS_MAXC and 1 <= cout <= CS_MAXC) or cs_mt(ks, cin) not in CS_MTS:
        return False
    return (ks, cin, cout) in CS_PAIRS and (ks, cout, cin) in CS_PAIRS


CS_TRIPLES = tuple(t for t in CS_PAIRS if cs_supported(*t))


def cs_plan(B, H, W):
    """(tiles, workgroups of the weight gradient, tiles the busiest workgroup walks, tiles the idlest walks)"""
    ntiles = B * _ceil(H, CS_TH) * _ceil(W, CS_TW)
    blocks = min(ntiles, CS_WG_BLOCKS)
    return ntiles, blocks, _ceil(ntiles, blocks), ntiles // blocks


def cs_depth(B, H, W):
    """D of g_weight / g_bias: a wave adds its 64 pixels of a tile in 16 matrix steps of four products (64 per tile, tile after tile
    in the same accumulator); the four waves' accumulators in a tree (2); fold level one, 4x unrolled; fold level two"""
    _, blocks, trips, _ = cs_plan(B, H, W)
    return trips * 16 * 4 + 2 + _fold_chain(blocks, CS_FOLD, 4) + _fold2_chain(CS_FOLD)


def cs_workspace_bytes(ks, cin, cout):
    wp = ks * ks * cin * cout * 4
    return ((wp + 255) & ~255) + (CS_WG_BLOCKS + CS_FOLD) * cs_mt(ks, cin) * 256 * 4


CsCase = collections.namedtuple("CsCase", "ks cin cout B H W kinds catches")
CS_EDGE_SHAPES = ((1, 1, 1), (1, 3, 5), (1, 8, 32), (2, 9, 33), (1, 7, 31))
# one triple per weight-gradient instantiation (MT = 1, 6, 7, 8, 10); (3,10,9): the bias row inside the last M-tile, (3,16,12): the
# bias row is the first row of an M-tile of its own; (1,3,12) has run only as another layer's data gradient so far
CS_MT_TRIPLES = ((1, 3, 12), (3, 10, 9), (3, 12, 9), (3, 13, 12), (3, 16, 12))
# ragged images with a given tile count: around the fold's first slice round (32), its unrolled body (more than 96) and the cap
CS_TILE_SHAPES = {31: (1, 5, 965), 32: (2, 9, 225), 33: (3, 8, 323), 96: (2, 17, 483), 97: (1, 5, 3073), 98: (2, 49, 193),
                  1024: (2, 2, 16353), 1025: (5, 3, 6529)}
CS_WALK_SHAPES = ((5, 41, 1089), (3, 2, 22369))          # 1050 tiles: 26 workgroups walk two; 2100: 52 walk three, the others two
CS_CONTROL = (3, 12, 9, 2, 9, 33)


def _cs_cases():
    cs = []
    for t in CS_TRIPLES:
        for s in CS_EDGE_SHAPES:
            kinds = ("off", "zero", "int") if t + s == CS_CONTROL else ("off", "int")
            cs.append(CsCase(*t, *s, kinds, "edge shape"))
    for t in CS_MT_TRIPLES:
        for n, s in CS_TILE_SHAPES.items():
            cs.append(CsCase(*t, *s, ("off", "int"), "%d tiles, MT = %d" % (n, cs_mt(t[0], t[1]))))
    for s in CS_WALK_SHAPES:
        cs.append(CsCase(3, 12, 9, *s, ("off", "int"), "%d tiles: workgroups walk different numbers of tiles" % cs_plan(*s)[0]))
    return cs


CS_CASES = _cs_cases()
CS_CASE_IDS = ["k%d-%dto%d-%dx%dx%d" % c[:6] for c in CS_CASES]


@functools.lru_cache(maxsize=2)
def cs_ref(ci, kind):
    c = CS_CASES[ci]
    gen = _gen(1, ci, KINDS.index(kind))
    x = _draw(gen, kind, "x", (c.B, c.cin, c.H, c.W))
    w = _draw(gen, kind, "w", (c.cout, c.cin, c.ks, c.ks))
    b = _draw(gen, kind, "b", (c.cout,))
    g = _draw(gen, kind, "g", (c.B, c.cout, c.H, c.W))
    r = conv_ref(x, w, b, g, c.ks // 2, kind == "int")
    r.case, r.kind = c, kind
    r.fl_y, r.fl_gx = floor("cs y", c.ks, c.cin, c.cout), floor("cs g_x", c.ks, c.cin, c.cout)
    r.D = cs_depth(c.B, c.H, c.W)
    return r


# ---- dd_conv_head and the heads' data gradient --------------------------------------------------------------------------------------
CH_NT, CH_ROWS, CH_FOLD = 256, 8, 32                   # dd_conv_head.hip:19-21
CH_CHANNELS = (32, 64)                                 # head_lpp, dd_conv_head.hip:153


def ch_lpp(C):
    return {32: 8, 64: 16}[C]


def ch_px(C):
    return CH_NT // ch_lpp(C)


def ch_blocks(B, Ho, Wo, C):
    return B * _ceil(Ho, CH_ROWS) * _ceil(Wo, ch_px(C))


def ch_depth(B, Ho, Wo, C):
    """D of the head's g_weight / g_bias: a lane adds the rows of its strip, one fmaf each (at most CH_ROWS); an element adds the
    workgroup's PX pixels one by one; fold level one, 2x unrolled; fold level two"""
    return min(CH_ROWS, Ho) + ch_px(C) + _fold_chain(ch_blocks(B, Ho, Wo, C), CH_FOLD, 2) + _fold2_chain(CH_FOLD)


def ch_workspace_bytes(B, Hp, Wp, C):
    return (ch_blocks(B, Hp - 2, Wp - 2, C) + CH_FOLD) * (9 * C + 1) * 4


ChCase = collections.namedtuple("ChCase", "B C Ho Wo kinds catches")
CH_BLOCK_SHAPES = {32: {32: (2, 9, 225), 33: (3, 1, 321), 64: (2, 25, 225), 65: (5, 8, 385)},
                   64: {32: (1, 9, 241), 33: (1, 17, 161), 64: (4, 8, 241), 65: (1, 33, 193)}}
CH_CONTROL = (2, 32, 9, 33)


def _ch_cases():
    cs = []
    for C in CH_CHANNELS:
        px = ch_px(C)
        for i, Wo in enumerate((1, px - 1, px, px + 1)):
            for k, Ho in enumerate((1, 7, 8, 9)):
                B = 1 + (i + k + 1) % 2
                kinds = ("off", "zero", "int") if (B, C, Ho, Wo) == CH_CONTROL else ("off", "int")
                cs.append(ChCase(B, C, Ho, Wo, kinds, "strip and row-block edges"))
        for n, s in CH_BLOCK_SHAPES[C].items():
            cs.append(ChCase(s[0], C, s[1], s[2], ("off", "int"), "%d workgroups" % n))
    return cs


CH_CASES = _ch_cases()
CH_CASE_IDS = ["B%d-C%d-%dx%d" % c[:4] for c in CH_CASES]


@functools.lru_cache(maxsize=2)
def ch_ref(ci, kind):
    """the head on its padded input (B, C, Ho + 2, Wo + 2): no padding of its own"""
    c = CH_CASES[ci]
    gen = _gen(2, ci, KINDS.index(kind))
    x = _draw(gen, kind, "x", (c.B, c.C, c.Ho + 2, c.Wo + 2))
    w = _draw(gen, kind, "w", (1, c.C, 3, 3))
    b = _draw(gen, kind, "b", (1,))
    g = _draw(gen, kind, "g", (c.B, 1, c.Ho, c.Wo))
    r = conv_ref(x, w, b, g, 0, kind == "int")
    r.case, r.kind = c, kind
    r.fl_y, r.fl_gx = floor("ch out", ch_lpp(c.C)), floor("c1 g_x")
    r.D = ch_depth(c.B, c.Ho, c.Wo, c.C)
    return r


# conv3x3_cout1_bwd_data_kernel by itself: the channel counts the heads do not have and padding 1 (ConvBiasFn)
DW_NT = 256                                            # dd_dwconv.hip (DW_NT): one thread per pixel and channel quad
C1Case = collections.namedtuple("C1Case", "B C Hi Wi pad kinds catches")


def c1_blocks_x(Wi, C):
    return _ceil(Wi * (C // 4), DW_NT)


def _c1_cases():
    cs = []
    for pad in (0, 1):
        for B, C, Hi, Wi, what in ((1, 4, 3, 255, "Wi * C / 4 = 255: one thread short of a workgroup"),
                                   (2, 4, 4, 256, "exactly one workgroup"),
                                   (1, 4, 5, 257, "one thread in the second workgroup"),
                                   (2, 32, 3, 3, "Hi = Wi = 3: at padding 0 one output pixel"),
                                   (1, 32, 9, 7, "the shape the older test has, at C = 32"),
                                   (1, 64, 5, 33, "three workgroups per row, the last partial"),
                                   (1, 512, 3, 3, "C = 512: the widest weight stage; Hi = Wi = 3"),
                                   (2, 512, 4, 5, "C = 512, three workgroups per row")):
            kinds = ("off", "zero", "int") if (C, Hi, pad) == (32, 9, 1) else ("off", "int")
            cs.append(C1Case(B, C, Hi, Wi, pad, kinds, what))
    return cs


C1_CASES = _c1_cases()
C1_CASE_IDS = ["B%d-C%d-%dx%d-pad%d" % c[:5] for c in C1_CASES]
C1_FUNCTION_CASE = C1_CASE_IDS.index("B1-C32-9x7-pad1")          # also run through ConvBiasFn


@functools.lru_cache(maxsize=2)
def c1_ref(ci, kind):
    c = C1_CASES[ci]
    gen = _gen(3, ci, KINDS.index(kind))
    x = _draw(gen, kind, "x", (c.B, c.C, c.Hi, c.Wi))
    w = _draw(gen, kind, "w", (1, c.C, 3, 3))
    b = _draw(gen, kind, "b", (1,))
    g = _draw(gen, kind, "g", (c.B, 1, c.Hi + 2 * c.pad - 2, c.Wi + 2 * c.pad - 2))
    r = conv_ref(x, w, b, g, c.pad, kind == "int")
    r.case, r.kind = c, kind
    r.fl_gx = floor("c1 g_x")
    return r


# ---- dd_redu -----------------------------------------------------------------------------------------------------------------------
RD_NT, RD_MAX_BLOCKS, RD_FOLD = 256, 1024, 32          # dd_redu.hip:19-21
RD_GROUPS_PER_BLOCK = 8                                # redu_blocks, dd_redu.hip:198: "at least eight pixel groups per workgroup"
RD_SHAPES = {64: (16, 1), 128: (32, 1), 256: (64, 1), 512: (64, 2)}          # redu_shape, dd_redu.hip:190-193: (LPP, QUADS)
RD_COUTS = (1, 3)


def rd_px(C):
    return RD_NT // RD_SHAPES[C][0]


def rd_plan(P, C):
    """(pixel groups, workgroups, groups the busiest workgroup walks, groups the idlest walks)"""
    groups = _ceil(P, rd_px(C))
    blocks = min(max(_ceil(groups, RD_GROUPS_PER_BLOCK), 1), RD_MAX_BLOCKS)
    return groups, blocks, _ceil(groups, blocks), groups // blocks


def rd_depth(P, C):
    """D of the reduction's g_weight / g_bias: a lane adds one pixel per group its workgroup walks, one fmaf each -- at most eight below
    the cap (min(groups, 8): the count itself is not monotone, nine groups are two workgroups of five and four), ceil(groups / 1024)
    above it; an element adds the workgroup's PX pixel lanes one by one; fold level one, 2x unrolled; fold level two"""
    groups, blocks, trips, _ = rd_plan(P, C)
    walk = min(groups, RD_GROUPS_PER_BLOCK) if groups <= RD_GROUPS_PER_BLOCK * RD_MAX_BLOCKS else trips
    assert walk >= trips
    return walk + rd_px(C) + _fold_chain(blocks, RD_FOLD, 2) + _fold2_chain(RD_FOLD)


def rd_workspace_bytes(P, C, cout):
    return (rd_plan(P, C)[1] + RD_FOLD) * (cout * 2 * C + cout) * 4


RdCase = collections.namedtuple("RdCase", "C cout P kinds catches")
RD_BLOCK_CASES = {32: ((64, 3), (512, 1)), 33: ((128, 1), (256, 3)), 64: ((64, 1), (256, 1)), 65: ((128, 3), (512, 3))}
RD_CAP_P = RD_GROUPS_PER_BLOCK * RD_MAX_BLOCKS * 4 + 3          # C = 256: four pixels per group; 8193 groups on 1024 workgroups, the last of three pixels
RD_CONTROL = (128, 3, 65)


def _rd_cases():
    cs = []
    for C in RD_SHAPES:
        px = rd_px(C)
        for cout in RD_COUTS:
            for P in (1, px - 1, px, px + 1, 8 * px, 8 * px + 1):
                kinds = ("off", "zero", "int") if (C, cout, P) == RD_CONTROL else ("off", "int")
                cs.append(RdCase(C, cout, P, kinds, "pixel-group and workgroup edges"))
    for n, combos in RD_BLOCK_CASES.items():
        for C, cout in combos:
            cs.append(RdCase(C, cout, RD_GROUPS_PER_BLOCK * rd_px(C) * (n - 1) + 1, ("off", "int"), "%d workgroups" % n))
    cs.append(RdCase(256, 3, RD_CAP_P, ("off", "int"), "above RD_MAX_BLOCKS: workgroup 0 walks nine groups, the others eight"))
    return cs


RD_CASES = _rd_cases()
RD_CASE_IDS = ["C%d-to%d-P%d" % c[:3] for c in RD_CASES]


@functools.lru_cache(maxsize=2)
def rd_ref(ci, kind):
    """conv1x1(cat(a, b)) on P pixels as a (1, 2C, P, 1) image; r.a, r.b (P, C), r.wm (cout, 2C): the matrices the C ABI takes"""
    c = RD_CASES[ci]
    gen = _gen(4, ci, KINDS.index(kind))
    x = _draw(gen, kind, "x", (1, 2 * c.C, c.P, 1))
    w = _draw(gen, kind, "w", (c.cout, 2 * c.C, 1, 1))
    b = _draw(gen, kind, "b", (c.cout,))
    g = _draw(gen, kind, "g", (1, c.cout, c.P, 1))
    r = conv_ref(x, w, b, g, 0, kind == "int")
    r.case, r.kind = c, kind
    lpp, quads = RD_SHAPES[c.C]
    r.fl_y, r.fl_gx = floor("rd y", lpp, quads), floor("rd g_ab", c.cout)
    r.D = rd_depth(c.P, c.C)
    return r


def rd_matrix(t):
    """(1, K, P, 1) -> (P, K)"""
    return t[0, :, :, 0].t()


# ---- C-ABI launchers: every output and every workspace between NaN guard bands ------------------------------------------------------
def nhwc_dev(t):
    """an NCHW-shaped CPU tensor -> its dense NHWC memory on the device, (B, H, W, C) contiguous"""
    return t.permute(0, 2, 3, 1).contiguous().cuda()


class Guarded:
    """the guarded buffers of one launch sequence; check() -> what was violated"""

    def __init__(self):
        self.bufs = []

    def out(self, name, n):
        buf, view = guarded(n)
        self.bufs.append((name, buf, n, True))
        return view

    def workspace(self, name, nbytes):
        """exactly nbytes long, NaN-filled: a fold that reads a partial nobody wrote turns its output NaN"""
        assert nbytes % 4 == 0
        buf, view = guarded(nbytes // 4)
        self.bufs.append((name, buf, nbytes // 4, False))
        return view

    def check(self):
        torch.cuda.synchronize()
        fails = []
        for name, buf, n, is_out in self.bufs:
            g = buf.shape[0] - n
            if not (bool(torch.isnan(buf[:g // 2]).all()) and bool(torch.isnan(buf[g // 2 + n:]).all())):
                fails.append("%s: a store outside its %d floats" % (name, n))
            if is_out and not bool(torch.isfinite(buf[g // 2:g // 2 + n]).all()):
                fails.append("%s: an element never written, or not finite" % name)
        return fails


def _lib():
    from hipops import lib as L
    return L, L.load()


def _p(t):
    return None if t is None else t.data_ptr()


def weight_layout(w, layout):
    """(cout, cin, k, k) on the device with channels-last ("cl": memory (cout, k, k, cin)) or NCHW-contiguous ("nchw") strides,
    whatever the sizes (torch.channels_last is ambiguous at cin = 1 or k = 1)"""
    w = w.cuda()
    return w.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2) if layout == "cl" else w.contiguous()


def cs_launch(r, layout="cl", bias=True, g_bias=True):
    """dd_conv_small_fwd, _bwd_data, _bwd_weight -> ({y, g_x, g_weight, g_bias} as NCHW-shaped views, guard failures)"""
    L, lib = _lib()
    c, G = r.case, Guarded()
    B, H, W, ks, cin, cout = c.B, c.H, c.W, c.ks, c.cin, c.cout
    x, g = nhwc_dev(r.x), nhwc_dev(r.g)
    w = weight_layout(r.w, layout)
    b = r.b.cuda() if bias else None
    sw = w.stride()
    nbytes = int(lib.dd_conv_small_workspace_bytes(ks, cin, cout))
    assert nbytes == cs_workspace_bytes(ks, cin, cout)
    st = L.current_stream()
    y = G.out("y", B * H * W * cout)
    L.check(lib.dd_conv_small_fwd(_p(x), _p(w), sw[0], sw[1], sw[2], sw[3], _p(b), B, H, W, cin, cout, ks, _p(y), _p(G.workspace("fwd workspace", nbytes)),
                                  nbytes, st), "dd_conv_small_fwd")
    gx = G.out("g_x", B * H * W * cin)
    L.check(lib.dd_conv_small_bwd_data(_p(g), _p(w), sw[0], sw[1], sw[2], sw[3], B, H, W, cin, cout, ks, _p(gx), _p(G.workspace("bwd_data workspace", nbytes)),
                                       nbytes, st), "dd_conv_small_bwd_data")
    gw = G.out("g_weight", cout * ks * ks * cin)
    gb = G.out("g_bias", cout) if g_bias else None
    L.check(lib.dd_conv_small_bwd_weight(_p(x), _p(g), B, H, W, cin, cout, ks, _p(gw), _p(gb), _p(G.workspace("bwd_weight workspace", nbytes)), nbytes, st),
            "dd_conv_small_bwd_weight")
    fails = G.check()
    return {"y": y.view(B, H, W, cout).permute(0, 3, 1, 2), "g_x": gx.view(B, H, W, cin).permute(0, 3, 1, 2),
            "g_weight": gw.view(cout, ks, ks, cin).permute(0, 3, 1, 2), "g_bias": gb}, fails


def c1_launch(g, w, B, C, Hi, Wi, pad):
    """dd_conv3x3_cout1_bwd_data: g (B, 1, Ho, Wo) and w (1, C, 3, 3) CPU tensors -> (g_x as a (B, C, Hi, Wi) view, guard failures)"""
    L, lib = _lib()
    G = Guarded()
    gd, wd = g.contiguous().cuda(), w.contiguous().cuda()
    gx = G.out("g_x", B * Hi * Wi * C)
    L.check(lib.dd_conv3x3_cout1_bwd_data(_p(gd), _p(wd), B, Hi, Wi, C, pad, _p(gx), L.current_stream()), "dd_conv3x3_cout1_bwd_data")
    fails = G.check()
    return gx.view(B, Hi, Wi, C).permute(0, 3, 1, 2), fails


def ch_launch(r, layout="cl", bias=True, g_bias=True):
    """dd_conv_head_fwd, dd_conv_head_bwd_weight -> ({out, g_weight, g_bias}, guard failures)"""
    L, lib = _lib()
    c, G = r.case, Guarded()
    B, C, Hp, Wp = c.B, c.C, c.Ho + 2, c.Wo + 2
    x, g = nhwc_dev(r.x), r.g.contiguous().cuda()
    w = weight_layout(r.w, layout)
    b = r.b.cuda() if bias else None
    sw = w.stride()
    st = L.current_stream()
    out = G.out("out", B * c.Ho * c.Wo)
    L.check(lib.dd_conv_head_fwd(_p(x), _p(w), sw[1], sw[2], sw[3], _p(b), B, Hp, Wp, C, _p(out), st), "dd_conv_head_fwd")
    nbytes = int(lib.dd_conv_head_workspace_bytes(B, Hp, Wp, C))
    assert nbytes == ch_workspace_bytes(B, Hp, Wp, C)
    gw = G.out("g_weight", 9 * C)
    gb = G.out("g_bias", 1) if g_bias else None
    L.check(lib.dd_conv_head_bwd_weight(_p(x), _p(g), B, Hp, Wp, C, _p(gw), _p(gb), _p(G.workspace("bwd_weight workspace", nbytes)), nbytes, st),
            "dd_conv_head_bwd_weight")
    fails = G.check()
    return {"out": out.view(B, 1, c.Ho, c.Wo), "g_weight": gw.view(1, 3, 3, C).permute(0, 3, 1, 2), "g_bias": gb}, fails


def rd_launch(r, bias=True, g_bias=True, want=("g_a", "g_b")):
    """dd_redu_fwd, _bwd_data, _bwd_weight -> ({y, g_a, g_b, g_weight, g_bias} shaped as the (1, K, P, 1) references, guard failures)"""
    L, lib = _lib()
    c, G = r.case, Guarded()
    C, cout, P = c.C, c.cout, c.P
    xm = rd_matrix(r.x)
    a, bm = xm[:, :C].contiguous().cuda(), xm[:, C:].contiguous().cuda()
    g = rd_matrix(r.g).contiguous().cuda()
    wm = r.w.view(cout, 2 * C).contiguous().cuda()
    b = r.b.cuda() if bias else None
    st = L.current_stream()
    y = G.out("y", P * cout)
    L.check(lib.dd_redu_fwd(_p(a), _p(bm), _p(wm), _p(b), P, C, cout, _p(y), st), "dd_redu_fwd")
    ga = G.out("g_a", P * C) if "g_a" in want else None
    gb_ = G.out("g_b", P * C) if "g_b" in want else None
    L.check(lib.dd_redu_bwd_data(_p(g), _p(wm), P, C, cout, _p(ga), _p(gb_), st), "dd_redu_bwd_data")
    nbytes = int(lib.dd_redu_workspace_bytes(P, C, cout))
    assert nbytes == rd_workspace_bytes(P, C, cout)
    gw = G.out("g_weight", cout * 2 * C)
    gbias = G.out("g_bias", cout) if g_bias else None
    L.check(lib.dd_redu_bwd_weight(_p(a), _p(bm), _p(g), P, C, cout, _p(gw), _p(gbias), _p(G.workspace("bwd_weight workspace", nbytes)), nbytes, st),
            "dd_redu_bwd_weight")
    fails = G.check()

    def image(t):
        return None if t is None else t.view(P, -1).t().reshape(1, -1, P, 1)
    return {"y": image(y), "g_a": image(ga), "g_b": image(gb_), "g_weight": gw.view(cout, 2 * C, 1, 1), "g_bias": gbias}, fails
