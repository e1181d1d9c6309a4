"""Shared plumbing of tests/test_glue_parity_gpu.py and tests/test_glue_inputs.py: the glue of the disparity decoders
(dd_up_cat_pad_t / _bwd_t, csrc/dd_decoder.hip), the channels-last reflection pad (dd_reflect_pad1_nhwc_t / _bwd_t) and the bias
gradient (dd_channel_sum_nhwc_t, both csrc/dd_ops.hip): cases, references, bounds and the judge.  Helpers only, no test.

Reference: the reference's own operator sequence F.elu -> F.interpolate(scale_factor=2) -> torch.cat -> F.pad(mode="reflect") in
float64 on the CPU on the exact values the kernel gets (half-type inputs are drawn in the half type and then widened), its gradients
by torch.autograd.  The same sequence in fp32 on the CPU gives e_32.

ONE criterion, element by element, for tensor type T, nothing in it from the kernel's output (Judge.check_elem):

    |kernel_i - ref64_i| <= u_T |ref64_i| + q_T + scale_i * max(4 * rho_32, F)

  * u_T: the one rounding on store (0 / 2^-11 / 2^-8 for fp32 / fp16 / bf16); q_T = 2^-25 for fp16 results below 2^-14 (half a
    subnormal step), 0 otherwise.
  * scale_i: the same linear operator applied to absolute values -- forward pad(cat(up(|elu(x)|), |skip|)), backward the float64
    adjoint applied to |g| times |elu'(x)|: the sum of the absolute terms of element i, so cancellation among the taps is accounted
    for and nothing else is.  |elu'(x)| = exp(x) enters no smaller than 2^-126: below its normal range fp32 rounds to 2^-150 =
    2^-24 * 2^-126 absolute, not to 2^-24 relative (exp(-104) is 0 in fp32; ELU_EDGES holds -104).
  * F = 2^-24 * R, R the roundings on the kernel's longest path (ROUNDINGS), at least 16.
  * rho_32 = max_j |fp32 reference_j - ref64_j| / scale_j: there only so that the criterion is no stricter than ATen's own fp32.
    tests/test_glue_inputs.py asserts rho_32 <= F for every case: the bound in force is F * scale_i everywhere.
  * pure copies (the skip half, nearest / same-size with ELU off, the whole reflect-pad forward): torch.equal.

Channel sums: |kernel_c - sum64_c| <= 2^-24 * D * sum_r |x_rc|, D the longest chain of additions of the kernel's own order
(channel_sum_depth).  Half inputs widen exactly, so the bound is the same for the three types.
"""
import collections
import functools

import torch
import torch.nn.functional as F

import ops_case as OC

U = 2.0 ** -24
FACTOR = 4.0
MIN_ROUNDINGS = 16
FP32_MIN_NORMAL = 2.0 ** -126
DTYPES = (torch.float32, torch.float16, torch.bfloat16)
U_STORE = {torch.float32: 0.0, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
MODES = {0: "nearest", 1: "bilinear", 2: None}
SEED = 23          # no draw has put a reference over a bound so far; if one does, change this and say so here (never the bound)

# longest leaf-to-output path in the kernel, one per multiply / add / exp (csrc/dd_decoder.hip, csrc/dd_ops.hip); weights 0.25, 0.75
# and their products are exact but counted, contraction to fma ignored
ROUNDINGS = {
    "out nearest": 6,       # elu1: four Horner steps, v * (.) and the fit's own error above -1/4; v * log2 e, exp2, - 1 below
    "out same": 6,          # elu1
    "out bilinear": 12,     # elu1 (6), hx*a, lx*b, +, hy*(.), ly*(.), +
    "g_x nearest": 12,      # pad_fold (4 adds), wy*wx, wgt*t, 2x2 positions added (4), expf, *
    "g_x bilinear": 24,     # pad_fold (4), wy*wx, wgt*t, 4x4 positions added (16), expf, *
    "g_x same": 6,          # pad_fold (4), expf, *
    "g_skip": 4,            # pad_fold (4)
    "pad g_x": 4,           # up to four mirrored positions added
}


def floor_factor(kind):
    return max(ROUNDINGS[kind], MIN_ROUNDINGS) * U


def dtype_name(dtype):
    return {torch.float32: "fp32", torch.float16: "fp16", torch.bfloat16: "bf16"}[dtype]


def _gen(*key):
    return torch.Generator().manual_seed(SEED + sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)))


# ---- the judge ---------------------------------------------------------------------------------------------------------------------
class Judge(OC.Judge):
    """ops_case.Judge with the element-wise criterion; a row is the element closest to (or furthest over) its bound."""

    def check_elem(self, qty, got, want64, want32, scale, kind, dtype):
        got = got.detach().double().cpu().reshape(want64.shape)
        if not bool(torch.isfinite(got).all()):
            self.rows.append((qty, float("inf"), 0.0, 0.0))
            self.fails.append("%s: non-finite elements" % qty)
            return
        bound = elem_bound(want64, want32, scale, kind, dtype)
        e_k, e_32 = (got - want64).abs(), (want32 - want64).abs()
        ratio = torch.where(e_k == 0, torch.zeros_like(e_k), e_k / bound)             # bound 0 and e_k > 0: inf
        i = int(ratio.argmax())
        over = int((e_k > bound).sum())
        self.rows.append((qty, float(e_k.flatten()[i]), float(e_32.flatten()[i]), float(bound.flatten()[i])))
        if over:
            self.fails.append("%s: %d of %d elements over their bound, worst %.2fx at %s: e_k %.3e > bound %.3e (ref64 %.6e, scale %.3e)" % (
                qty, over, e_k.numel(), float(ratio.flatten()[i]), tuple(int(v) for v in torch.unravel_index(torch.tensor(i), e_k.shape)),
                float(e_k.flatten()[i]), float(bound.flatten()[i]), float(want64.flatten()[i]), float(scale.flatten()[i])))

    def check_sum(self, qty, got, want64, want32, bound):
        """per-channel sums: bound is a tensor computed by the caller (channel_sum_bound)"""
        got = got.detach().double().cpu().reshape(want64.shape)
        if not bool(torch.isfinite(got).all()):
            self.rows.append((qty, float("inf"), 0.0, 0.0))
            self.fails.append("%s: non-finite elements" % qty)
            return
        e_k, e_32 = (got - want64).abs(), (want32.double() - want64).abs()
        ratio = torch.where(e_k == 0, torch.zeros_like(e_k), e_k / bound)
        i = int(ratio.argmax())
        self.rows.append((qty, float(e_k[i]), float(e_32[i]), float(bound[i])))
        if bool((e_k > bound).any()):
            self.fails.append("%s: channel %d: e_k %.3e > bound %.3e (sum64 %.6e)" % (qty, i, float(e_k[i]), float(bound[i]), float(want64[i])))


def rho32(want64, want32, scale):
    """the fp32 reference's worst element-wise error in units of scale_i (0 / 0 counts as 0)"""
    e = (want32.double() - want64).abs()
    r = torch.where(e == 0, torch.zeros_like(e), e / scale)
    return float(r.max()) if r.numel() else 0.0


def elem_bound(want64, want32, scale, kind, dtype, factor=FACTOR):
    q = torch.zeros_like(want64)
    if dtype == torch.float16:
        q = torch.where(want64.abs() < 2.0 ** -14, torch.full_like(want64, 2.0 ** -25), q)
    return U_STORE[dtype] * want64.abs() + q + scale * max(factor * rho32(want64, want32, scale), floor_factor(kind))


# ---- dd_up_cat_pad -----------------------------------------------------------------------------------------------------------------
# xkind: "normal" 1.5 N(0,1) | "edges" (ELU_EDGES placed by make_x) | "small_neg" U(-0.05, 0) alone | "ramp" (below)
Case = collections.namedtuple("Case", "name B C1 C2 h w mode elu xkind catches")

ELU_TINY = (0.0, -0.0, FP32_MIN_NORMAL, -FP32_MIN_NORMAL)
ELU_EDGES = ELU_TINY + (-20.0, -104.0, 50.0)           # and U(-0.05, 0) on row 0
EDGE_HW = (5, 5)


def _cases():
    cs = []
    for mode in (0, 1, 2):
        for elu in (True, False):
            hw = (4, 4) if mode == 2 else (2, 2)
            cs.append(Case("mode%d-elu%d" % (mode, elu), 2, 8, 4, hw[0], hw[1], mode, elu, "normal",
                           "the border rules of bilinear_src / up_taps (i == 0, i == n-1) and pad_fold (Y == 1, Y == H-2) on adjacent indices"))
    for mode in (0, 1):
        for hw in ((3, 5), (5, 3)):
            cs.append(Case("mode%d-%dx%d" % (mode, hw[0], hw[1]), 2, 4, 4, hw[0], hw[1], mode, True, "normal", "h and w swapped somewhere"))
    for c1, c2 in ((4, 0), (4, 8), (12, 8), (8, 20)):
        cs.append(Case("channels-%d+%d" % (c1, c2), 2, c1, c2, 3, 2, 1, True, "normal", "j / Cq with Cq = %d, the skip offset cq - C1q" % ((c1 + c2) // 4)))
    cs.append(Case("channels-8+20-nearest", 2, 8, 20, 2, 3, 0, False, "normal", "the skip offset with C2 > C1 beside a pure copy"))
    cs.append(Case("channels-12+8-same", 2, 12, 8, 4, 5, 2, True, "normal", "Cq = 5 without up-sampling"))
    cs.append(Case("row-258", 2, 8, 4, 2, 42, 1, True, "normal", "a padded row of 258 channel groups: ends inside the second workgroup, pixel 85 split 255|256"))
    cs.append(Case("row-260", 2, 12, 8, 2, 25, 0, True, "normal", "a padded row of 260 channel groups of 5: pixel 51 split across the workgroup boundary"))
    for mode in (0, 1, 2):
        cs.append(Case("elu-edges-mode%d" % mode, 2, 8, 4, EDGE_HW[0], EDGE_HW[1], mode, True, "edges", "ELU at 0, -0, +-2^-126, U(-0.05, 0), -20, -104, +50"))
    for mode in (1, 2):
        cs.append(Case("elu-small-negatives-mode%d" % mode, 2, 8, 0, 4, 4, mode, True, "small_neg",
                       "expf(v) - 1 instead of expm1f(v): the scale is small everywhere, so the lost 2^-24 shows"))
    cs.append(Case("ramp", 2, 4, 4, 6, 7, 1, True, "ramp", "a wrong 0.25 / 0.75: the taps nearly cancel in the backward, a global tolerance hides it"))
    cs.append(Case("batch-3", 3, 8, 4, 2, 3, 1, True, "normal", "the batch strides of x, skip and out, all different"))
    return cs


CASES = _cases()
CASE_IDS = [c.name for c in CASES]
NEEDS = ((True, True), (True, False), (False, True))      # gradient requests: both, x only, skip only


def dims(c):
    return (c.h, c.w) if c.mode == 2 else (2 * c.h, 2 * c.w)


def make_x(c, g):
    shape = (c.B, c.C1, c.h, c.w)
    if c.xkind == "normal":
        return 1.5 * torch.randn(shape, generator=g)
    if c.xkind == "small_neg":
        return -0.05 * torch.rand(shape, generator=g)
    if c.xkind == "ramp":
        # smooth and far from 0: ELU is the identity, a 0.25 that should be 0.75 moves the output by a slope, 1e-3 of the values
        yy, xx = torch.arange(c.h).view(1, 1, c.h, 1), torch.arange(c.w).view(1, 1, 1, c.w)
        return 8.0 + 0.01 * yy + 0.02 * xx + 0.1 * torch.arange(c.C1).view(1, c.C1, 1, 1) + 1e-3 * torch.randn(shape, generator=g)
    if c.xkind == "edges":
        # h = w = 5.  The tiny values (0, -0, +-2^-126) sit at (odd, odd) only: every output then has a tap of ordinary size (1.5 N(0,1),
        # -20, 50 ...) with weight >= 1/16, so no output is the sum of subnormal products alone (bf16 has no u_T relative rounding there)
        assert (c.h, c.w) == EDGE_HW
        x = 1.5 * torch.randn(shape, generator=g)
        x[:, :, 0, :] = -0.05 * torch.rand((c.B, c.C1, c.w), generator=g)          # U(-0.05, 0) on the row bilinear_src clamps
        x[:, :, 2, 0], x[:, :, 2, 2], x[:, :, 2, 4] = -20.0, -104.0, 50.0
        x[:, :, 4, 0], x[:, :, 4, 4] = -20.0, -104.0                                 # the corner: weight 1 in up_taps
        for b in range(c.B):
            for ch in range(c.C1):
                for k, (y, xx) in enumerate(((1, 1), (1, 3), (3, 1), (3, 3))):
                    x[b, ch, y, xx] = ELU_TINY[(b + ch + k) % 4]
        return x
    raise ValueError(c.xkind)


def sequence(x, skip, mode, elu):
    """the reference's operators (networks/layers.py ConvBlock / upsample, networks/depth_decoder.py), NCHW"""
    y = F.elu(x) if elu else x
    if mode != 2:
        y = F.interpolate(y, scale_factor=2, mode=MODES[mode])
    if skip is not None:
        y = torch.cat((y, skip), 1)
    return F.pad(y, (1, 1, 1, 1), mode="reflect")


def _run_sequence(x, skip, g, mode, elu, dtype):
    x = x.detach().to(dtype).clone().requires_grad_()
    skip = None if skip is None else skip.detach().to(dtype).clone().requires_grad_()
    out = sequence(x, skip, mode, elu)
    grads = torch.autograd.grad((out * g.to(dtype)).sum(), [x] if skip is None else [x, skip])
    return out.detach().double(), grads[0].double(), (None if skip is None else grads[1].double())


@functools.lru_cache(maxsize=None)
def glue_ref(case_index, dtype):
    """Inputs in `dtype` (x, skip, g; NCHW-shaped CPU tensors), the float64 and fp32 references of out / g_x / g_skip, their scales."""
    c = CASES[case_index]
    H, W = dims(c)
    gen = _gen(case_index)
    r = OC.Ref()
    r.case, r.dtype = c, dtype
    r.x = make_x(c, gen).to(dtype)
    r.skip = torch.randn((c.B, c.C2, H, W), generator=gen).to(dtype) if c.C2 else None
    g = torch.randn((c.B, c.C1 + c.C2, H + 2, W + 2), generator=gen)
    if c.xkind == "ramp":      # alternating sign, nearly constant size: what every low-resolution element gathers nearly cancels
        sign = 1.0 - 2.0 * ((torch.arange(H + 2).view(-1, 1) + torch.arange(W + 2).view(1, -1)) % 2)
        g = sign * (1.0 + 0.01 * g)
    r.g = g.to(dtype)
    x64, s64, g64 = r.x.double(), (None if r.skip is None else r.skip.double()), r.g.double()
    r.out64, r.gx64, r.gs64 = _run_sequence(x64, s64, g64, c.mode, c.elu, torch.float64)
    r.out32, r.gx32, r.gs32 = _run_sequence(x64, s64, g64, c.mode, c.elu, torch.float32)
    # scales: the linear part on absolute values
    ya = (F.elu(x64) if c.elu else x64).abs().detach().requires_grad_()
    sa = None if s64 is None else s64.abs().detach().requires_grad_()
    lin = sequence(ya, sa, c.mode, False)
    ga = torch.autograd.grad((lin * g64.abs()).sum(), [ya] if sa is None else [ya, sa])
    d = torch.where(x64 <= 0, torch.exp(x64), torch.ones_like(x64)).clamp_min(FP32_MIN_NORMAL) if c.elu else torch.ones_like(x64)
    r.s_out, r.s_gx, r.s_gs = lin.detach(), ga[0] * d, (None if sa is None else ga[1])
    return r


def out_kind(c):
    return "out " + ("same" if c.mode == 2 else MODES[c.mode])


def gx_kind(c):
    return "g_x " + ("same" if c.mode == 2 else MODES[c.mode])


def x_half_is_a_copy(c):
    return c.mode != 1 and not c.elu


# ---- dd_reflect_pad1_nhwc_t --------------------------------------------------------------------------------------------------------
PAD_B = 2
PAD_CASES = [(H, W, C) for (H, W) in ((4, 4), (4, 7), (9, 4)) for C in (1, 2, 3, 17)] + [(4, 255, 1)]      # the last: (W + 2) * C = 257


@functools.lru_cache(maxsize=None)
def pad_ref(H, W, C, dtype):
    gen = _gen(H, W, C, 5)
    r = OC.Ref()
    r.x = torch.randn((PAD_B, C, H, W), generator=gen).to(dtype)
    r.g = torch.randn((PAD_B, C, H + 2, W + 2), generator=gen).to(dtype)
    x64, g64 = r.x.double().requires_grad_(), r.g.double()
    out = F.pad(x64, (1, 1, 1, 1), mode="reflect")
    r.out = out.detach().to(dtype)                                   # a copy: exact in every type
    r.gx64 = torch.autograd.grad((out * g64).sum(), x64)[0]
    x32 = r.x.float().requires_grad_()
    r.gx32 = torch.autograd.grad((F.pad(x32, (1, 1, 1, 1), mode="reflect") * r.g.float()).sum(), x32)[0]
    xa = torch.ones_like(x64).requires_grad_()
    r.s_gx = torch.autograd.grad((F.pad(xa, (1, 1, 1, 1), mode="reflect") * g64.abs()).sum(), xa)[0]
    return r


# ---- dd_channel_sum_nhwc_t ---------------------------------------------------------------------------------------------------------
CS_NT, CS_MAX_BLOCKS = 256, 2048            # stated here, not imported: the launch of dd_channel_sum_nhwc_t
CS_NARROW_C, CS_NARROW_ROWS = (1, 2, 3, 7, 9, 255, 256), (1, 2, 31, 257, 4099)
CS_WIDE_C, CS_WIDE_ROWS = (257, 300, 1344), (1, 3, 33, 65, 4097)
CS_CAPPED_NARROW = (9, 480_000)             # 4.32 M elements: 2110 workgroups wanted, 2048 launched
CS_CAPPED_WIDE = (257, 66_001)              # 2063 chunks wanted, 2048 of 33 rows launched: chunks 2001 .. 2047 start past the end
CS_MEANS = (0.0, 100.0)                     # N(100, 1): a dropped or doubled element cannot hide in cancellation


def _ceil(a, b):
    return -(-a // b)


def channel_sum_launch(rows, C):
    """(workgroups or chunks, stride or rows per chunk) as channel_sum_launch of dd_ops.hip computes them"""
    if C > CS_NT:
        chunks = min(_ceil(rows, 32), CS_MAX_BLOCKS)
        return chunks, _ceil(rows, chunks)
    total = rows * C
    blocks = max(1, min(_ceil(total, CS_NT * 8), CS_MAX_BLOCKS))
    return blocks, max((blocks * CS_NT // C) * C, C)


def channel_sum_depth(rows, C):
    """D: the additions on the longest chain from an element to out[c], in the kernel's own order.
    narrow (C <= 256): a thread adds every stride-th element to its sum: ceil(total / stride); thread c then adds the workgroup's
      entries of channel c, one every C threads: ceil(256 / C).
    wide: a thread owns one column of one chunk; a0 takes one addition per four rows and one per row of the tail: per // 4 + per % 4;
      then (a0 + a1) + (a2 + a3): 2.
    fold kernel, both: a thread adds every 256th partial: ceil(n / 256); the wave's butterfly over 64 lanes: 6; red[0] + .. + red[3]: 3."""
    n, step = channel_sum_launch(rows, C)
    if C > CS_NT:
        chain = step // 4 + step % 4 + 2
    else:
        chain = _ceil(rows * C, step) + _ceil(CS_NT, C)
    return chain + _ceil(n, CS_NT) + 6 + 3


def channel_sum_input(rows, C, mean, dtype):
    return (mean + torch.randn((rows, C), generator=_gen(rows, C, int(mean), 9))).to(dtype)


def channel_sum_bound(x, rows, C):
    """x: the (rows, C) input in its own type -> (sum64, fp32 reference, bound), each (C,)"""
    x64 = x.double()
    return x64.sum(0), x.float().sum(0), U * channel_sum_depth(rows, C) * x64.abs().sum(0)
