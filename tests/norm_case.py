"""Shared plumbing of tests/test_norm_parity_gpu.py and tests/test_norm_inputs.py: BatchNorm with its fused activation and residual
(csrc/dd_bn.hip, hipops.functions.BatchNormActFn), the channels-last LayerNorm and the layer-scale residual (csrc/dd_ln.hip, LayerNormFn,
LayerScaleResidualFn) and the depth-wise dilated 3x3 convolution (csrc/dd_dwconv.hip, DepthwiseConv3x3NHWCFn): cases, references,
bounds and the judge.  Helpers only, no test.

Reference: the reference operators (F.batch_norm, F.layer_norm, F.conv2d(groups=C), res + y * scale, relu / gelu) in float64 on the CPU
on the exact values the kernel gets (half-type inputs are drawn in the half type and then widened; eps and momentum are the fp32 values
the C entry points receive), gradients by torch.autograd.  The same operators in fp32 on the CPU give e_32.

ONE criterion, element by element, for tensor type T, nothing in it from the kernel's output (Judge.check_elem):

    |kernel_i - ref64_i| <= u_T |ref64_i| + q_T + scale_i * max(4 * rho_32, F) [+ band_i]

  * u_T: the one rounding on store (0 / 2^-11 / 2^-8 for fp32 / fp16 / bf16); q_T = 2^-25 for fp16 results below 2^-14 (half a
    subnormal step, as in tests/glue_case.py: g * scale of the layer-scale residual is ~1e-6), 0 otherwise.
  * F = 2^-24 * R, R the roundings on the kernel's longest path (ROUNDINGS, counted from the kernel source; where a sum is on the
    path its depth D in the kernel's own order is added), at least 16.
  * rho_32 = max_j |fp32 reference_j - ref64_j| / scale_j; tests/test_norm_inputs.py asserts rho_32 <= F for every case, so the bound
    in force is F * scale_i.
  * scale_i: the operator's sum of absolute terms.
      normalisation outputs  z_abs = |gamma| invstd (|x_i| + |mean|) + |beta| (+ |res_i|), through the activation's Lipschitz constant
                             (ReLU 1, GELU 1.13);
      their input gradient   dx = k (g' - mean(g') - xhat c), c = mean(g' xhat), k = gamma invstd.  First order in the errors of its
                             parts: |k| (s' + mean(s') + xhat_abs |c| + |xhat| mean(s' xhat_abs)) with xhat_abs = invstd (|x| + |mean|)
                             -- the absolute terms of xhat, which is where the fp32 save_mean / invstd enter -- and s' the scale of
                             g' = g act'(z): |g| |act'(z)|, for GELU plus |g| 0.8 z_abs (|GELU''| <= 0.8 turns the error of z into one
                             of GELU'(z));
                             LayerNorm: the same forms with the row's statistics, which are fp32 results of the row itself:
                             mean |x| for |mean|, and xhat_abs + |xhat| kappa for xhat_abs, kappa = mean(|xhat| xhat_abs) what the
                             error of (x - mu) does to rstd through var = mean (x - mu)^2 (ln_ref);
      dwconv                 conv(|x|, |w|), the adjoint on |g| for the data gradient;
      layer scale            |res| + |y scale|, |g scale|.
  * band_i (ReLU only): an element whose float64 pre-activation is within F * z_abs of 0 may be masked either way by a correct fp32
    kernel.  Its |g_i| enters the bounds of the gradients as an absolute term, taken through the same linear map (band terms below);
    which elements those are is decided by the float64 reference alone.
  * column and row sums (d gamma, d beta, d w, d scale): 2^-24 * D * sum |terms| (check_abs), D the additions on the kernel's longest
    chain (bn_depth, ln_depth, ls_depth, dw_depth); where the terms hold xhat, R_xhat roundings on xhat_abs are added to D.
  * running_mean / running_var against float64 with the momentum update applied: 2^-24 |value| + momentum F (|mean| resp. var).
"""
import collections
import functools
import math

import torch
import torch.nn.functional as F

import glue_case as GC
import ops_case as OC

U = GC.U
FACTOR = GC.FACTOR
MIN_ROUNDINGS = GC.MIN_ROUNDINGS
DTYPES, U_STORE, dtype_name = GC.DTYPES, GC.U_STORE, GC.dtype_name
HALF = (torch.float16, torch.bfloat16)
SEED = 41          # no draw has put a reference over a bound so far; if one does, change the case and say so here (never the bound)
GELU_LIP, GELU_CURV = 1.13, 0.8           # sup |GELU'| = 1.1290, sup |GELU''| = 2 phi(0) = 0.798

# longest leaf-to-output path in the kernel, one per multiply / add / divide / sqrt / erf / exp and per rounding to fp32 (contraction to
# fma ignored); "+ D" marks the paths a sum is on, its depth is added by floor()
ROUNDINGS = {
    # csrc/dd_bn.hip
    "bn out": 12,        # (float)var, + eps, sqrt, 1/x, gamma * invstd, (float)mean, mean * k, beta - ., v * k, + sh, + res
    "bn out gelu": 17,   # the first ten of those, z * 0.7071, erff (2), 1 + ., 0.5 * z, * .
    "bn xhat": 7,        # R_xhat: save_mean (1), save_invstd (4), v - m, * i
    "bn g'": 13,         # GELU': z * 0.7071, erff (2), 1 + ., 0.5 * .; z * z, -0.5 * ., expf (2), z * 0.3989, * .; +; g * .
    "bn g_x": 19,        # gamma * invstd, g' (13), - a, - xhat * c (2), k * .;   through a or c: "bn g_x sum"
    "bn g_x sum": 6,     # + D: the sum (D), / rows, to fp32, xhat * c, -, k * ., gamma * invstd
    "bn running": 1,     # the update is formed in fp64 from the fp64 statistics and rounded once on store
    # csrc/dd_ln.hip
    "ln y": 28,          # mu: 2 + log2 LP additions (<= 8), 1 / C, * (10); v - mu; var: d * d, 8 additions, * 1/C (10); + eps, sqrt, 1/x; d * rs, * gamma, + beta
    "ln xhat": 25,       # R_xhat: mu (10), v - mu, rs (10 + 3), * rs
    "ln g_x": 20,        # g * gamma; b: * xhat, 8 additions, 1 / C, * (11); xhat * b, - a, - ., rs * .
    "ls out": 2,         # y * scale, + res
    "ls g_y": 1,         # g * scale
    # csrc/dd_dwconv.hip
    "dw out": 18,        # nine taps: multiply and add each (w * mask is exact)
    "dw g_x": 18,
}


def floor(kind, depth=0):
    return max(ROUNDINGS[kind] + depth, MIN_ROUNDINGS) * U


def _gen(*key):
    return torch.Generator().manual_seed(SEED + sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)))


def _ceil(a, b):
    return -(-a // b)


def leaf(t, D):
    """a fresh leaf of type D (never the stored tensor itself: .to() returns it when the type is already D)"""
    return t.detach().to(D).clone().requires_grad_()


def f32(v):
    """the fp32 value a C entry point receives for the Python float v, as a Python float"""
    return float(torch.tensor(v, dtype=torch.float32))


# ---- the judge ---------------------------------------------------------------------------------------------------------------------
def rho32(want64, want32, scale, band=None):
    """the fp32 reference's worst element-wise error in units of scale_i (0 / 0 counts as 0), after what the band allows"""
    e = (want32.double() - want64).abs()
    if band is not None:
        e = (e - band).clamp_min(0.0)
    r = torch.where(e == 0, torch.zeros_like(e), e / scale)
    return float(r.max()) if r.numel() else 0.0


def elem_bound(want64, want32, scale, fl, dtype, band=None, factor=FACTOR):
    b = U_STORE[dtype] * want64.abs() + scale * max(factor * rho32(want64, want32, scale, band), fl)
    if dtype == torch.float16:
        b = b + torch.where(want64.abs() < 2.0 ** -14, torch.full_like(want64, 2.0 ** -25), torch.zeros_like(want64))
    return b if band is None else b + band


class Judge(OC.Judge):
    """ops_case.Judge with the element-wise criterion; a row is the element closest to (or furthest over) its bound."""

    def _row(self, qty, got, want64, e_32, bound, what):
        got = got.detach().double().cpu().reshape(want64.shape)
        if not bool(torch.isfinite(got).all()):
            self.rows.append((qty, float("inf"), 0.0, 0.0))
            self.fails.append("%s: non-finite elements" % qty)
            return
        e_k = (got - want64).abs()
        ratio = torch.where(e_k == 0, torch.zeros_like(e_k), e_k / bound)             # bound 0 and e_k > 0: inf
        i = int(ratio.argmax())
        over = int((e_k > bound).sum())
        self.rows.append((qty, float(e_k.flatten()[i]), float(e_32.flatten()[i]), float(bound.flatten()[i])))
        if over:
            self.fails.append("%s: %d of %d %s over their bound, worst %.2fx at %s: e_k %.3e > bound %.3e (ref64 %.6e)" % (
                qty, over, e_k.numel(), what, float(ratio.flatten()[i]), tuple(int(v) for v in torch.unravel_index(torch.tensor(i), e_k.shape)),
                float(e_k.flatten()[i]), float(bound.flatten()[i]), float(want64.flatten()[i])))

    def check_elem(self, qty, got, want64, want32, scale, fl, dtype, band=None):
        self._row(qty, got, want64, (want32.double() - want64).abs(), elem_bound(want64, want32, scale, fl, dtype, band), "elements")

    def check_abs(self, qty, got, want64, want32, bound):
        """sums and running statistics: `bound` is a tensor computed by the caller from the float64 reference"""
        self._row(qty, got, want64, (want32.double() - want64).abs(), bound, "entries")

    def finish(self):
        """the `worst:` line of ops_case.Judge, and one `ratios:` line: the largest e_k / bound per kind of quantity (its first word)"""
        best = {}
        for qty, e_k, _, bound in self.rows:
            ratio = 0.0 if e_k == 0.0 else (float("inf") if bound == 0.0 else e_k / bound)
            best[qty.split()[0]] = max(best.get(qty.split()[0], 0.0), ratio)
        print("ratios: %s | %s | %s" % (self.op, self.case, " ".join("%s=%.3f" % kv for kv in sorted(best.items()))))
        return super().finish()


def guarded(n, dtype=torch.float32, guard=256):
    """a NaN-filled CUDA buffer of guard + n + guard elements and the view of its middle n (tests/test_mfma_store_tail_gpu.py)"""
    buf = torch.full((n + 2 * guard,), float("nan"), dtype=dtype, device="cuda")
    return buf, buf[guard:guard + n]


def guards_intact(buf, n, guard=256):
    return bool(torch.isnan(buf[:guard]).all()) and bool(torch.isnan(buf[guard + n:]).all()) and bool(torch.isfinite(buf[guard:guard + n]).all())


# ---- BatchNorm ---------------------------------------------------------------------------------------------------------------------
BN_NT, BN_ROWS_PER_THREAD, BN_MAX_CHUNKS, BN_MAX_BLOCKS = 1024, 8, 256, 1024          # stated here, not imported: bn_plan of dd_bn.hip
BN_MOMENTUM = 0.125        # exact in fp32, and so is 1 - momentum: the float64 reference applies the update the kernel is asked for
BN_EPS = f32(1e-5)
BN_ACT_CODE = {None: 0, "relu": 1, "gelu": 2}
BN_COMBOS = ((None, False), ("relu", False), ("relu", True), ("gelu", False), (None, True))
BN_GROUPS = (1, 2)
# per-channel centring, channel c takes KINDS[c % 9]: a number is mean / sigma; "small": mean 1, sigma 1e-3 (mean / sigma = 1000);
# "const": every element 3.  The first four hold a +100 and a -1000, so a C = 4 tensor is off-centre too.
BN_KINDS = (0.0, 100.0, -1000.0, 10.0, "small", -100.0, 1000.0, -10.0, "const")
BN_KINDS_HALF = (0.0, 100.0, -10.0, 10.0, "const", -100.0)          # mean / sigma <= 100: |x| < 300, inside both half types
BN_OUTLIER = 1000.0        # "outlier" variant: row 0 of every group sits 1000 sigma from the channel mean

BnCase = collections.namedtuple("BnCase", "name shape outlier combos groups catches")
BN_LARGE = (2, 512, 96, 96)


def _bn_cases():
    cs = []
    for shape, what in (((1, 8, 1, 2), "two rows, unbiased factor 2"),
                        ((1, 4, 3, 5), "C = 4: 1024 lanes"),
                        ((1, 12, 5, 7), "C / 4 = 3: 1023 threads"),
                        ((2, 8, 12, 20), "fewer rows than lanes, one chunk"),
                        ((2, 48, 9, 11), "a width that does not divide 1024 (85 lanes)"),
                        ((2, 80, 7, 9), "a width that does not divide 1024 (51 lanes)"),
                        ((3, 64, 24, 40), "six chunks, ragged last chunk"),
                        ((1, 508, 3, 5), "C / 4 = 127: 1016 threads")):
        cs.append(BnCase("x".join(map(str, shape)), shape, False, BN_COMBOS, BN_GROUPS, what))
    for shape in ((1, 12, 5, 7), (2, 8, 12, 20), (3, 64, 24, 40)):
        cs.append(BnCase("x".join(map(str, shape)) + "-outlier", shape, True, (("relu", True), (None, False)), (1,),
                         "a shift taken from the first row: it sits 1000 sigma off"))
    # 38 MB: one group (two would be 76 MB), the two combinations that cover both activations and the residual
    cs.append(BnCase("x".join(map(str, BN_LARGE)), BN_LARGE, False, (("relu", True), ("gelu", False)), (1,),
                     "18432 rows: 288 chunks wanted, 256 launched, nine rows per thread"))
    return cs


BN_CASES = _bn_cases()
BN_CASE_IDS = [c.name for c in BN_CASES]
BN_HALF_CASES = [BN_CASE_IDS.index(n) for n in ("1x12x5x7", "2x80x7x9", "3x64x24x40")]


def bn_plan(rows, C):
    """(lanes, chunks, rows per chunk, blocks, rows per block) as bn_plan of dd_bn.hip computes them"""
    lanes = max(BN_NT // (C // 4), 1)
    want = _ceil(rows, lanes * BN_ROWS_PER_THREAD)
    chunks = min(max(want, 1), BN_MAX_CHUNKS)
    per_chunk = _ceil(rows, chunks)
    chunks = _ceil(rows, per_chunk)
    nb = min(max(want, 1), BN_MAX_BLOCKS)
    per_block = _ceil(rows, nb)
    return lanes, chunks, per_chunk, _ceil(rows, per_block), per_block


def bn_depth(rows, C):
    """D of the backward's sums: a thread adds its rows of a chunk in fp32: ceil(rows per chunk / lanes); lanes, chunks and fold lanes
    are added in fp64 and each of the three totals is rounded to fp32: 3"""
    lanes, _, per_chunk, _, _ = bn_plan(rows, C)
    return _ceil(per_chunk, lanes) + 3


def bn_kinds(dtype):
    return BN_KINDS if dtype == torch.float32 else BN_KINDS_HALF


def bn_channel_kinds(C, dtype):
    k = bn_kinds(dtype)
    return [k[c % len(k)] for c in range(C)]


def bn_ratio(kind):
    """|mean| / sigma of a channel kind (const: 0, there is no sigma)"""
    return 1000.0 if kind == "small" else (0.0 if kind == "const" else abs(kind))


def _bn_input(c, groups, dtype, gen):
    B, C, H, W = c.shape
    kinds = bn_channel_kinds(C, dtype)
    sigma = 0.5 + 1.5 * torch.rand(C, generator=gen)
    mean = torch.zeros(C)
    for ch, k in enumerate(kinds):
        if k == "small":
            mean[ch], sigma[ch] = 1.0, 1e-3
        elif k == "const":
            mean[ch], sigma[ch] = 3.0, 0.0
        else:
            mean[ch] = k * sigma[ch]
    x = mean.view(1, C, 1, 1) + sigma.view(1, C, 1, 1) * torch.randn((groups * B, C, H, W), generator=gen)
    if c.outlier:
        for k in range(groups):
            x[k * B, :, 0, 0] = mean + BN_OUTLIER * sigma
    return x


def _act(y, act):
    return F.relu(y) if act == "relu" else (F.gelu(y) if act == "gelu" else y)


def _bn_run(r, D):
    """the reference operators in type D: out, running_mean, running_var, (g_x, g_w, g_b, g_res or None), float64 copies"""
    c, per = r.case, r.case.shape[0]
    x = leaf(r.x, D)
    res = None if r.res is None else leaf(r.res, D)
    w, b = leaf(r.w, D), leaf(r.b, D)
    rm, rv = r.rm0.to(D).clone(), r.rv0.to(D).clone()
    outs = []
    for k in range(r.groups):
        y = F.batch_norm(x[k * per:(k + 1) * per], rm, rv, w, b, True, BN_MOMENTUM, BN_EPS)
        if res is not None:
            y = y + res[k * per:(k + 1) * per]
        outs.append(_act(y, r.act))
    out = torch.cat(outs)
    grads = torch.autograd.grad((out * r.g.to(D)).sum(), [x, w, b] + ([res] if res is not None else []))
    grads = [t.double() for t in grads] + ([None] if res is None else [])
    return out.detach().double(), rm.double(), rv.double(), grads


def _chan(t):
    return t.view(1, -1, 1, 1)


@functools.lru_cache(maxsize=2)
def bn_ref(ci, dtype, act, with_res, groups):
    """Inputs in `dtype` (NCHW-shaped CPU tensors; x, res and g hold the groups back to back along the batch axis), the float64 and
    fp32 references of the output, the running statistics and the four gradients, their scales, bands and bounds."""
    c = BN_CASES[ci]
    B, C, H, W = c.shape
    gen = _gen(ci, {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}[dtype], BN_ACT_CODE[act], with_res, groups)
    r = OC.Ref()
    r.case, r.dtype, r.act, r.groups, r.rows = c, dtype, act, groups, B * H * W
    r.x = _bn_input(c, groups, dtype, gen).to(dtype)
    r.res = torch.randn(r.x.shape, generator=gen).to(dtype) if with_res else None
    r.g = torch.randn(r.x.shape, generator=gen).to(dtype)
    r.w = (0.5 + torch.rand(C, generator=gen)) * (1.0 - 2.0 * (torch.arange(C) % 3 == 2))          # every third gamma negative
    r.b = 0.2 * torch.randn(C, generator=gen)
    x64 = r.x.double()
    m_all = x64.mean((0, 2, 3))
    # running statistics of a net that has seen such batches: the mean's own sign (the update adds, it does not cancel)
    r.rm0 = (0.5 * m_all + torch.where(m_all < 0, -1.0, 1.0) * 0.3 * torch.rand(C, generator=gen).double()).float()
    r.rv0 = (0.5 + torch.rand(C, generator=gen))
    r.out64, r.rm64, r.rv64, r.g64 = _bn_run(r, torch.float64)
    r.out32, r.rm32, r.rv32, r.g32 = _bn_run(r, torch.float32)

    # ---- scales, bands and bounds: float64, from the inputs alone -------------------------------------------------------------------
    D = bn_depth(r.rows, C)
    fl_out = floor("bn out gelu" if act == "gelu" else "bn out")
    w64, b64, g64 = r.w.double(), r.b.double(), r.g.double()
    s_out, s_gp, band_gp, s_gx, band_gx = [], [], [], [], []
    b_gw, b_gb = torch.zeros(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
    rm, rv = r.rm0.double(), r.rv0.double()
    b_rm, b_rv = torch.zeros_like(rm), torch.zeros_like(rv)
    r.mean, r.var, r.unbiased = [], [], []
    for k in range(groups):
        sl = slice(k * B, (k + 1) * B)
        xk, gk = x64[sl], g64[sl]
        mean = xk.mean((0, 2, 3))
        var = ((xk - _chan(mean)) ** 2).mean((0, 2, 3))
        unb = var * r.rows / max(r.rows - 1, 1)
        invstd = 1.0 / torch.sqrt(var + BN_EPS)
        r.mean.append(mean), r.var.append(var), r.unbiased.append(unb)
        # running statistics after this group's update, and what the update may add to their error
        rm, rv = (1 - BN_MOMENTUM) * rm + BN_MOMENTUM * mean, (1 - BN_MOMENTUM) * rv + BN_MOMENTUM * unb
        b_rm = (1 - BN_MOMENTUM) * b_rm + U * rm.abs() + BN_MOMENTUM * floor("bn running") * mean.abs()
        b_rv = (1 - BN_MOMENTUM) * b_rv + U * rv.abs() + BN_MOMENTUM * floor("bn running") * unb
        kk = w64 * invstd
        xhat = (xk - _chan(mean)) * _chan(invstd)
        xhat_abs = (xk.abs() + _chan(mean.abs())) * _chan(invstd)
        z = xhat * _chan(w64) + _chan(b64) + (0.0 if r.res is None else r.res.double()[sl])
        z_abs = xhat_abs * _chan(w64.abs()) + _chan(b64.abs()) + (0.0 if r.res is None else r.res.double()[sl].abs())
        s_out.append(z_abs * (GELU_LIP if act == "gelu" else 1.0))
        if act == "relu":
            d_act, band = (z > 0).double(), (z.abs() <= fl_out * z_abs).double() * gk.abs()
        elif act == "gelu":
            d_act = 0.5 * (1 + torch.erf(z / math.sqrt(2.0))) + z * torch.exp(-0.5 * z * z) / math.sqrt(2 * math.pi)
            band = torch.zeros_like(z)
        else:
            d_act, band = torch.ones_like(z), torch.zeros_like(z)
        gp = gk * d_act
        sp = gk.abs() * (d_act.abs() + (GELU_CURV * z_abs if act == "gelu" else 0.0))
        cc = (gp * xhat).mean((0, 2, 3))
        s_gp.append(sp), band_gp.append(band)
        s_gx.append(_chan(kk.abs()) * (sp + _chan(sp.mean((0, 2, 3))) + xhat_abs * _chan(cc.abs()) + xhat.abs() * _chan((sp * xhat_abs).mean((0, 2, 3)))))
        band_gx.append(_chan(kk.abs()) * (band + _chan(band.mean((0, 2, 3))) + xhat.abs() * _chan((band * xhat.abs()).mean((0, 2, 3)))))
        b_gb += max((D + ROUNDINGS["bn g'"] * (act == "gelu")) * U, floor("bn g'")) * sp.sum((0, 2, 3)) + band.sum((0, 2, 3))
        b_gw += max((D + ROUNDINGS["bn xhat"] + ROUNDINGS["bn g'"] * (act == "gelu")) * U, floor("bn g'")) * (sp * xhat_abs).sum((0, 2, 3)) \
            + (band * xhat.abs()).sum((0, 2, 3))
    if groups > 1:          # the groups' gradients are added in fp32
        b_gw, b_gb = b_gw + U * r.g64[1].abs(), b_gb + U * r.g64[2].abs()
    r.s_out, r.s_gp, r.band_gp, r.s_gx, r.band_gx = (torch.cat(t) for t in (s_out, s_gp, band_gp, s_gx, band_gx))
    r.fl_out, r.fl_gp = fl_out, floor("bn g'")
    r.fl_gx = max(floor("bn g_x"), floor("bn g_x sum", D))
    r.b_gw, r.b_gb, r.b_rm, r.b_rv = b_gw, b_gb, b_rm, b_rv
    return r


def bn_raw_sums_model(x, rows, C):
    """The statistics this suite was written against, in plain torch: fp32 sum x and sum x * x per thread of bn_plan's geometry, every
    chunk total and every fold lane rounded to fp32, var = s2 / n - mean^2 in float64.  x: (rows, C) fp32.  -> mean, var (float64)."""
    lanes, chunks, per_chunk, _, _ = bn_plan(rows, C)
    tot = torch.zeros(lanes, 2, C, dtype=torch.float64)
    for k in range(chunks):
        xc = x[k * per_chunk:(k + 1) * per_chunk]
        xc = torch.cat((xc, torch.zeros(_ceil(xc.shape[0], lanes) * lanes - xc.shape[0], C))).view(-1, lanes, C)
        s1, s2 = torch.zeros(lanes, C), torch.zeros(lanes, C)
        for v in xc:                                                     # a thread's rows, in order
            s1, s2 = s1 + v, (s2.double() + v.double() * v.double()).float()          # fmaf: one rounding
        tot[k % lanes, 0] += s1.double().sum(0).float().double()         # lanes in fp64, the chunk total stored as a float
        tot[k % lanes, 1] += s2.double().sum(0).float().double()
    s = tot.float().double().sum(0)                                      # each fold lane rounded to fp32, then added in fp64
    mean = s[0] / rows
    return mean, (s[1] / rows - mean * mean).clamp_min(0.0)


def bn_first_row_shift_model(x, rows, C):
    """the same raw fp32 sums of x - x[0]: a shift taken naively from the first element.  The variance does not depend on the shift in
    exact arithmetic; with row 0 an outlier every d is ~1000 sigma and the cancellation is back.  -> mean, var (float64)"""
    mean, var = bn_raw_sums_model(x - x[0:1], rows, C)
    return mean + x[0].double(), var


def bn_model_outputs(r, mean, var):
    """out (act None, no residual) and running_var of one group from a model's (mean, var), with the kernel's fp32 arithmetic"""
    assert r.groups == 1 and r.act is None and r.res is None
    invstd = 1.0 / torch.sqrt(var.float() + torch.tensor(BN_EPS, dtype=torch.float32))
    k = r.w * invstd
    sh = r.b - mean.float() * k
    out = r.x.float() * _chan(k) + _chan(sh)
    unb = var * r.rows / max(r.rows - 1, 1)
    return out.double(), ((1 - BN_MOMENTUM) * r.rv0.double() + BN_MOMENTUM * unb).float().double()


@functools.lru_cache(maxsize=None)
def bn_grid_case():
    """ReLU-mask consistency: x on the integers, every channel's mean an integer itself (each of -2 .. 2 equally often, plus an integer
    offset), beta = 0: a fifth of the pre-activations are fmaf(mean, k, -mean * k), within one rounding of 0.  (B, C, H, W) fp32."""
    B, C, H, W = 2, 12, 5, 7
    gen = _gen(99)
    rows = B * H * W
    assert rows % 5 == 0
    base = torch.arange(rows) % 5 - 2.0
    offs = torch.tensor([0.0, 3.0, -7.0, 100.0, 1.0, -1.0, 12.0, -33.0, 5.0, 2.0, -2.0, 64.0])
    x = torch.stack([base[torch.randperm(rows, generator=gen)] + offs[ch] for ch in range(C)], 1)          # (rows, C)
    x = x.view(B, H, W, C).permute(0, 3, 1, 2).contiguous()
    w = 0.5 + torch.rand(C, generator=gen)
    g = torch.randn(B, C, H, W, generator=gen)
    return x, w, torch.zeros(C), g, offs


# ---- LayerNorm ---------------------------------------------------------------------------------------------------------------------
LN_NT, LN_MAX_BLOCKS, LN_ROWS_PER_THREAD = 256, 512, 8          # stated here, not imported
LN_EPS = f32(1e-6)
LN_WIDTHS = (4, 60, 64, 68, 124, 128, 132, 252, 256)
LN_HALF_WIDTHS = (68, 132, 252)
LN_KINDS = ("centred", "off", "mixed", "const")          # row mean 0 | 1000 sigma | r % 4: 0, +1000 sigma, -1000 sigma, nearly constant | sigma = 1e-4 |mean|
LN_OFF = {torch.float32: 1000.0, torch.float16: 100.0, torch.bfloat16: 100.0}          # |row mean| / sigma of the off-centre rows: at 1000 a bf16
# row holds three or four distinct values, its sigma is the quantisation's and F.layer_norm's fp32 backward (which cancels at (mean / sigma)^2) is
# 200 x over F there: the half types get 100, as in the BatchNorm cases
LN_CAPPED = ((4, 65536 + 37), (132, 2 * 16384 + 5))      # more than 512 blocks wanted: 1 MB, 17 MB


def ln_lp(C):
    return 16 if C // 4 <= 16 else (32 if C // 4 <= 32 else 64)


def ln_rpb(C):
    return LN_NT // ln_lp(C)


def ln_row_counts(C):
    return (1, ln_rpb(C) - 1, ln_rpb(C) + 1, 1000)


def ln_blocks(rows, C):
    return min(max(_ceil(rows, ln_rpb(C) * LN_ROWS_PER_THREAD), 1), LN_MAX_BLOCKS)


def ln_depth(rows, C):
    """D of d gamma / d beta: a thread adds its rows: ceil(rows / (blocks * RPB)); thread (which, c) adds the block's RPB row groups;
    the fold: a lane adds every 64th block's record: ceil(blocks / 64), the wave's tree: 6"""
    blocks = ln_blocks(rows, C)
    return _ceil(rows, blocks * ln_rpb(C)) + ln_rpb(C) + _ceil(blocks, 64) + 6


def _ln_input(rows, C, kind, gen, ratio):
    sigma = 0.5 + 1.5 * torch.rand(rows, 1, generator=gen)
    z = torch.randn(rows, C, generator=gen)
    sign = 1.0 - 2.0 * (torch.arange(rows).view(-1, 1) % 2)
    off, const = ratio * sigma * sign + sigma * z, 5.0 * sign * (1.0 + 1e-4 * z)
    if kind == "centred":
        return sigma * z
    if kind == "off":
        return off
    if kind == "const":
        return const
    sel = (torch.arange(rows) % 4).view(-1, 1)
    return torch.where(sel == 0, sigma * z, torch.where(sel == 3, const, off * torch.where(sel == 1, sign, -sign)))


def _ln_run(r, D):
    x, w, b = leaf(r.x, D), leaf(r.w, D), leaf(r.b, D)
    y = F.layer_norm(x, (x.shape[-1],), w, b, LN_EPS)
    grads = torch.autograd.grad((y * r.g.to(D)).sum(), [x, w, b])
    return y.detach().double(), [t.double() for t in grads]


@functools.lru_cache(maxsize=4)
def ln_ref(rows, C, kind, dtype):
    gen = _gen(rows, C, LN_KINDS.index(kind), 3)
    r = OC.Ref()
    r.rows, r.C, r.kind, r.dtype = rows, C, kind, dtype
    r.x = _ln_input(rows, C, kind, gen, LN_OFF[dtype]).to(dtype)
    r.g = torch.randn(rows, C, generator=gen).to(dtype)
    r.w = (0.5 + torch.rand(C, generator=gen)) * (1.0 - 2.0 * (torch.arange(C) % 3 == 2))
    r.b = 0.3 * torch.randn(C, generator=gen)
    r.y64, r.g64 = _ln_run(r, torch.float64)
    r.y32, r.g32 = _ln_run(r, torch.float32)
    x64, g64, w64 = r.x.double(), r.g.double(), r.w.double()
    mean = x64.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x64 - mean) ** 2).mean(1, keepdim=True) + LN_EPS)
    # xhat = (x - mu) rstd with mu and rstd fp32 results of the row itself (BatchNorm's come from fp64 sums): the absolute terms of mu
    # are mean |x|, and var = mean (x - mu)^2 inherits 2 |x - mu| per unit of (x - mu)'s error: rstd carries kappa = mean(|xhat| xhat_abs)
    # relative units per unit of F, every factor rstd with it
    xhat = (x64 - mean) * rstd
    xhat_abs = (x64.abs() + x64.abs().mean(1, keepdim=True)) * rstd
    kappa = (xhat.abs() * xhat_abs).mean(1, keepdim=True)
    xhat_tot = xhat_abs + xhat.abs() * kappa
    r.s_y = xhat_tot * w64.abs() + r.b.double().abs()
    gg = (g64 * w64).abs()
    bb = (g64 * w64 * xhat).mean(1, keepdim=True)
    r.s_gx = rstd * (gg + gg.mean(1, keepdim=True) + xhat_tot * bb.abs() + xhat.abs() * (gg * xhat_tot).mean(1, keepdim=True)) + r.g64[0].abs() * kappa
    D = ln_depth(rows, C)
    r.b_gw = (D + ROUNDINGS["ln xhat"]) * U * (g64.abs() * xhat_tot).sum(0)
    r.b_gb = max(D, MIN_ROUNDINGS) * U * g64.abs().sum(0)
    return r


# ---- layer-scale residual ----------------------------------------------------------------------------------------------------------
LS_NT, LS_MAX_CHUNKS = 256, 64          # stated here, not imported
LS_CASES = [(B, hw, C) for C in (4, 252, 1024) for hw in (1, 7, 23 * 23) for B in (1, 3)]
LS_GAMMA = 1e-6


def ls_plan(rows, C):
    """(lanes, chunks, rows per chunk) as dd_layer_scale_bwd_t computes them"""
    lanes = max(LS_NT // (C // 4), 1)
    chunks = min(_ceil(rows, lanes * 8), LS_MAX_CHUNKS)
    per = _ceil(rows, chunks)
    return lanes, _ceil(rows, per), per


def ls_depth(rows, C):
    """D of d scale: a thread adds its rows of a chunk: ceil(per / lanes); thread c adds the lanes one by one: lanes; the fold adds
    the chunks one by one: chunks"""
    lanes, chunks, per = ls_plan(rows, C)
    return _ceil(per, lanes) + lanes + chunks


@functools.lru_cache(maxsize=None)
def ls_ref(B, hw, C, dtype):
    """res, y, g (B, hw, 1, C) in `dtype`; scale (B, 1, 1, C) fp32 = gamma * drop with gamma ~ 1e-6 and image B - 1 dropped (factor
    exactly 0; at B = 1 the one image is kept)"""
    gen = _gen(B, hw, C, 7)
    r = OC.Ref()
    r.res, r.y, r.g = (torch.randn(B, hw, 1, C, generator=gen).to(dtype) for _ in range(3))
    gamma = LS_GAMMA * (1.0 + 0.1 * torch.randn(C, generator=gen)) * (1.0 - 2.0 * (torch.arange(C) % 3 == 2))
    drop = torch.full((B, 1, 1, 1), 1.0 / 0.7)
    if B > 1:
        drop[B - 1] = 0.0
    r.scale = (gamma.view(1, 1, 1, C) * drop).float()
    r.dropped = B - 1 if B > 1 else None
    for D, tag in ((torch.float64, "64"), (torch.float32, "32")):
        res, y, sc = leaf(r.res, D), leaf(r.y, D), leaf(r.scale, D)
        out = res + y * sc
        grads = torch.autograd.grad((out * r.g.to(D)).sum(), [res, y, sc])
        setattr(r, "out" + tag, out.detach().double())
        setattr(r, "g" + tag, [t.double() for t in grads])
    y64, g64, s64 = r.y.double(), r.g.double(), r.scale.double()
    r.s_out = r.res.double().abs() + (y64 * s64).abs()
    r.s_gy = (g64 * s64).abs()
    r.b_gs = max(ls_depth(hw, C), MIN_ROUNDINGS) * U * (g64 * y64).abs().sum((1, 2), keepdim=True)
    return r


# ---- depth-wise dilated 3x3 convolution --------------------------------------------------------------------------------------------
DW_NT, DW_ROWS, DW_FOLD = 256, 4, 8          # stated here, not imported
DwCase = collections.namedtuple("DwCase", "B C H W dil catches")
DW_CASES = [
    DwCase(1, 4, 1, 255, 1, "H = 1: only the middle tap row; W * C / 4 = 255, one thread short of a workgroup"),
    DwCase(1, 4, 2, 256, 2, "dil >= H; W * C / 4 = 256, exactly one workgroup"),
    DwCase(3, 4, 3, 257, 3, "dil >= H; W * C / 4 = 257, one thread in the second workgroup; B * H = 9"),
    DwCase(1, 12, 5, 85, 5, "dil >= H; W * C / 4 = 255 with three channel groups; H = 5: three of four rows of the second row block unused"),
    DwCase(3, 12, 6, 86, 6, "dil >= H; W * C / 4 = 258: pixel 85 split across two workgroups; B * H = 18"),
    DwCase(1, 36, 7, 9, 1, "H = 7: one row of the second row block unused; nine channel groups; B * H = 7"),
    DwCase(3, 36, 3, 5, 5, "dil >= H and dil >= W: only the centre tap is in the image"),
    DwCase(1, 508, 2, 3, 2, "C / 4 = 127: two weight-gradient lanes, 254 threads"),
    DwCase(3, 512, 5, 4, 1, "C = 512: the widest weight stage; B * H = 15"),
    DwCase(1, 512, 7, 2, 3, "dil >= W: only the middle tap column"),
    DwCase(3, 4, 1, 7, 6, "H = 1 at three images: B * H = 3; lanes = W = 7"),
    DwCase(1, 12, 6, 3, 6, "dil >= H and dil >= W at H = 6"),
    DwCase(1, 36, 5, 40, 2, "dilation 2 with every tap in the image somewhere; 28 lanes over 40 columns"),
    DwCase(3, 12, 7, 11, 3, "B * H = 21; dilation 3"),
]
DW_CASE_IDS = ["B%d-C%d-%dx%d-dil%d" % c[:5] for c in DW_CASES]
DW_HALF_CASES = (2, 5, 8)
DW_GUARD_CASES = (3, 5, 8)          # H = 5, 7, 5: not multiples of the four rows a thread computes


def dw_depth(B, H, W, C):
    """D of d w: a thread adds its columns of a row: ceil(W / lanes); thread i adds the lanes one by one: lanes; the fold: a slice adds
    every eighth row record: ceil(B * H / 8), the eight slices one by one: 8"""
    lanes = max(min(DW_NT // (C // 4), W), 1)
    return _ceil(W, lanes) + lanes + _ceil(B * H, DW_FOLD) + DW_FOLD


def _dw_run(r, D):
    c = r.case
    x, w = leaf(r.x, D), leaf(r.w, D)
    y = F.conv2d(x, w, None, 1, c.dil, c.dil, c.C)
    grads = torch.autograd.grad((y * r.g.to(D)).sum(), [x, w])
    return y.detach().double(), [t.double() for t in grads]


@functools.lru_cache(maxsize=None)
def dw_ref(ci, dtype):
    c = DW_CASES[ci]
    gen = _gen(ci, 13)
    r = OC.Ref()
    r.case, r.dtype = c, dtype
    r.x = (0.4 + 1.7 * torch.randn(c.B, c.C, c.H, c.W, generator=gen)).to(dtype)
    r.g = torch.randn(c.B, c.C, c.H, c.W, generator=gen).to(dtype)
    r.w = 0.3 * torch.randn(c.C, 1, 3, 3, generator=gen)
    r.y64, r.g64 = _dw_run(r, torch.float64)
    r.y32, r.g32 = _dw_run(r, torch.float32)
    xa, wa = r.x.double().abs().requires_grad_(), r.w.double().abs().requires_grad_()
    ya = F.conv2d(xa, wa, None, 1, c.dil, c.dil, c.C)
    ga = torch.autograd.grad((ya * r.g.double().abs()).sum(), [xa, wa])
    r.s_y, r.s_gx = ya.detach(), ga[0]
    r.b_gw = max(dw_depth(c.B, c.H, c.W, c.C), MIN_ROUNDINGS) * U * ga[1]
    return r
