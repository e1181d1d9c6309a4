"""BatchNorm with its fused activation and residual (csrc/dd_bn.hip), the channels-last LayerNorm and the layer-scale residual
(csrc/dd_ln.hip) and the depth-wise dilated 3x3 convolution (csrc/dd_dwconv.hip) against the reference operators in float64 on the CPU,
element by element, in fp32, fp16 and bf16, at the shapes where a thread-to-row mapping, a chunk cap or a fold can go wrong and on the
values where a normalisation can: channels whose mean is 10, 100 and 1000 sigma from 0, a small-variance and a constant channel, a first
row 1000 sigma off, rows nearly constant, a layer scale of 1e-6 with a dropped image, dilations that leave only the centre tap in the
image.  Guard bands around every output of the LayerNorm and depth-wise entry points, bit-reproducibility of every fixed-order sum, and
the ReLU mask of the BatchNorm backward recomputed from x against the one read from the saved output.

tests/norm_case.py holds the cases, the references and the one criterion (nothing in a bound from the kernel's output);
tests/test_norm_inputs.py asserts on the CPU that the inputs are what is claimed here, that the bound in force is F * scale_i, and that
BatchNorm statistics from raw fp32 sums -- what dd_bn.hip computed before its sums went to fp64 -- break these bounds.

Every case prints one `worst:` line (run with -s).  Largest error / bound per family on one MI355X run:

    family        type   largest e_k / bound per kind of quantity
    batch_norm    fp32   out 0.21  running_mean 0.88  running_var 0.99  g_x 1.00  g_res 1.00  g_weight 0.42  g_bias 1.00
    batch_norm    fp16   out 1.00  running_mean 0.83  running_var 0.97  g_x 1.00  g_res 1.00  g_weight 0.03  g_bias 0.06
    batch_norm    bf16   out 0.99  running_mean 0.79  running_var 0.96  g_x 0.99  g_res 0.00  g_weight 0.06  g_bias 0.01
    layer_norm    fp32   y 0.06  g_x 0.08  g_weight 0.03  g_bias 0.13
    layer_norm    fp16   y 0.99  g_x 0.99  g_weight 0.03  g_bias 0.04
    layer_norm    bf16   y 0.99  g_x 0.99  g_weight 0.03  g_bias 0.02
    layer_scale   fp32   out 0.06  g_y 0.06  g_scale 0.15
    layer_scale   fp16   out 0.99  g_y 1.00  g_scale 0.15
    layer_scale   bf16   out 0.95  g_y 1.00  g_scale 0.07
    dwconv3x3     fp32   y 0.16  g_x 0.18  g_weight 0.11
    dwconv3x3     fp16   y 0.99  g_x 0.99  g_weight 0.09
    dwconv3x3     bf16   y 0.99  g_x 0.99  g_weight 0.10

The ratios at 0.95 .. 1.00 are roundings that the bound names one by one, not arithmetic near its limit: an element stored in a half type
is up to half a step of that type from float64 (u_T |ref64|, q_T), the running statistics are one fp32 rounding of the fp64 update
(2^-24 |value|), and a ReLU element inside the band was masked the other way (its |g_i| is the band term: g_x, g_res, g_bias of
batch_norm).  What the arithmetic itself uses of F * scale is the fp32 rows without a band: 0.06 .. 0.42.  profiles/norm_parity.txt
keeps the `worst:` lines of that run, and the line of the same test on the raw-fp32-sums kernel (running_var 12 800 x over its bound).
"""
import pytest
import torch

import norm_case as NC
from norm_case import Judge

pytestmark = pytest.mark.gpu
CL = torch.channels_last
F32 = torch.float32


def nhwc(t, requires_grad=False):
    """an NCHW-shaped CPU tensor -> the CUDA tensor of that shape whose memory is NHWC whatever the sizes (H = W = 1 included)"""
    return None if t is None else t.detach().cuda().permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2).requires_grad_(requires_grad)


# ---- BatchNorm ---------------------------------------------------------------------------------------------------------------------
BN_PARAMS = [(ci, F32) for ci in range(len(NC.BN_CASES))] + [(ci, h) for ci in NC.BN_HALF_CASES for h in NC.HALF]


def _bn_apply(r, x, w, b, res, rm, rv):
    from hipops.functions import BatchNormActFn
    return BatchNormActFn.apply(x, w, b, [(rm, rv)] * r.groups, res, NC.BN_MOMENTUM, NC.BN_EPS, NC.BN_ACT_CODE[r.act], r.groups)


@pytest.mark.parametrize("ci,dtype", BN_PARAMS, ids=["%s-%s" % (NC.BN_CASE_IDS[ci], NC.dtype_name(d)) for ci, d in BN_PARAMS])
def test_batch_norm(ci, dtype):
    """output, both running statistics and the gradients of x, residual, weight and bias, for every activation / residual combination
    of the case and for one and two groups (two independent batches back to back, the running statistics updated in turn)"""
    c = NC.BN_CASES[ci]
    fails = []
    for act, with_res in c.combos:
        for groups in c.groups:
            r = NC.bn_ref(ci, dtype, act, with_res, groups)
            x, res, g = nhwc(r.x, True), nhwc(r.res, True), nhwc(r.g)
            w, b = r.w.cuda().requires_grad_(), r.b.cuda().requires_grad_()
            rm, rv = r.rm0.cuda().clone(), r.rv0.cuda().clone()
            out = _bn_apply(r, x, w, b, res, rm, rv)
            assert out.shape == r.x.shape and out.dtype == dtype and out.is_contiguous(memory_format=CL) and out.grad_fn.name().startswith("BatchNormActFn")
            out.backward(g)
            torch.cuda.synchronize()
            j = Judge("batch_norm", "%s %s act=%s res=%d groups=%d" % (c.name, NC.dtype_name(dtype), act, with_res, groups))
            j.check_elem("out", out, r.out64, r.out32, r.s_out, r.fl_out, dtype)
            j.check_abs("running_mean", rm, r.rm64, r.rm32, r.b_rm)
            j.check_abs("running_var", rv, r.rv64, r.rv32, r.b_rv)
            assert x.grad.dtype == dtype and w.grad.dtype == F32 and b.grad.dtype == F32
            j.check_elem("g_x", x.grad, r.g64[0], r.g32[0], r.s_gx, r.fl_gx, dtype, r.band_gx)
            if with_res:
                assert res.grad.dtype == dtype
                j.check_elem("g_res", res.grad, r.g64[3], r.g32[3], r.s_gp, r.fl_gp, dtype, r.band_gp)
            j.check_abs("g_weight", w.grad, r.g64[1], r.g32[1], r.b_gw)
            j.check_abs("g_bias", b.grad, r.g64[2], r.g32[2], r.b_gb)
            fails += j.finish()
    assert not fails, fails


def test_batch_norm_module_counts_its_batches_and_equals_the_function():
    """networks.layers.BatchNorm2d on the HIP path: num_batches_tracked goes up by one per pass and by the number of groups in a
    grouped pass; output and running statistics are those of BatchNormActFn bit for bit"""
    from networks.layers import BatchNorm2d, batch_groups
    ci = NC.BN_CASE_IDS.index("2x48x9x11")
    r = NC.bn_ref(ci, F32, "relu", True, 2)
    C = r.case.shape[1]
    bn = BatchNorm2d(C, eps=NC.BN_EPS, momentum=NC.BN_MOMENTUM).cuda().train()
    with torch.no_grad():
        bn.weight.copy_(r.w), bn.bias.copy_(r.b), bn.running_mean.copy_(r.rm0), bn.running_var.copy_(r.rv0)
    x, res = nhwc(r.x), nhwc(r.res)
    with batch_groups(2):
        out = bn(x, act="relu", residual=res)
    assert out.grad_fn.name().startswith("BatchNormActFn")
    assert int(bn.state_dict()["num_batches_tracked"]) == 2
    rm, rv = r.rm0.cuda().clone(), r.rv0.cuda().clone()
    want = _bn_apply(r, x, r.w.cuda(), r.b.cuda(), res, rm, rv)
    torch.cuda.synchronize()
    assert torch.equal(out, want) and torch.equal(bn.running_mean, rm) and torch.equal(bn.running_var, rv)
    per = r.case.shape[0]
    bn(x[:per], act="relu", residual=res[:per])
    assert int(bn.state_dict()["num_batches_tracked"]) == 3


def test_batch_norm_relu_mask_from_x_equals_the_mask_from_the_output():
    """Without a residual the backward recomputes the ReLU mask from x, with one it reads the mask from the saved output.  x on the
    integers with integer channel means and beta = 0: a fifth of the pre-activations are within one rounding of 0, so one differing
    bit of k or sh between the forward and the backward flips masks.  residual=None against an all-zero residual: the same bits in the
    output, g_x and the weight and bias gradients -- and in a second run of either."""
    from hipops.functions import BatchNormActFn
    xc, wc, bc, gc, _ = NC.bn_grid_case()
    got = []
    for with_res in (False, True, False, True):
        x, g = nhwc(xc, True), nhwc(gc)
        w, b = wc.cuda().requires_grad_(), bc.cuda().requires_grad_()
        res = torch.zeros_like(x).requires_grad_() if with_res else None
        out = BatchNormActFn.apply(x, w, b, None, res, NC.BN_MOMENTUM, NC.BN_EPS, 1, 1)
        out.backward(g)
        torch.cuda.synchronize()
        got.append((out.detach(), x.grad, w.grad, b.grad))
    near = (nhwc(xc) == nhwc(xc).mean((0, 2, 3), keepdim=True))
    assert 0.15 < float(near.float().mean()) < 0.25
    assert bool(torch.isfinite(got[0][1]).all()) and float(got[0][0].max()) > 0
    for other in got[1:]:
        for name, a, o in zip(("out", "g_x", "g_weight", "g_bias"), got[0], other):
            assert torch.equal(a, o), name


# ---- LayerNorm ---------------------------------------------------------------------------------------------------------------------
LN_PARAMS = [(C, F32) for C in NC.LN_WIDTHS] + [(C, h) for C in NC.LN_HALF_WIDTHS for h in NC.HALF]


def _ln_case(rows, C, kind, dtype, j):
    from hipops.functions import LayerNormFn
    r = NC.ln_ref(rows, C, kind, dtype)
    runs = []
    for _ in range(2):
        x, w, b = r.x.cuda().requires_grad_(), r.w.cuda().requires_grad_(), r.b.cuda().requires_grad_()
        y = LayerNormFn.apply(x, w, b, NC.LN_EPS)
        assert y.dtype == dtype and y.shape == (rows, C)
        y.backward(r.g.cuda())
        runs.append((y.detach(), x.grad, w.grad, b.grad))
    torch.cuda.synchronize()
    tag = "rows=%d %s" % (rows, kind)
    y, gx, gw, gb = runs[0]
    assert gx.dtype == dtype and gw.dtype == F32 and gb.dtype == F32
    j.check_elem("y " + tag, y, r.y64, r.y32, r.s_y, NC.floor("ln y"), dtype)
    j.check_elem("g_x " + tag, gx, r.g64[0], r.g32[0], r.s_gx, NC.floor("ln g_x"), dtype)
    j.check_abs("g_weight " + tag, gw, r.g64[1], r.g32[1], r.b_gw)
    j.check_abs("g_bias " + tag, gb, r.g64[2], r.g32[2], r.b_gb)
    for name, a, o in zip(("y", "g_x", "g_weight", "g_bias"), runs[0], runs[1]):          # no atomics: the same bits
        j.equal("second run %s %s" % (name, tag), o, a)


@pytest.mark.parametrize("C,dtype", LN_PARAMS, ids=["C%d-%s" % (C, NC.dtype_name(d)) for C, d in LN_PARAMS])
def test_layer_norm(C, dtype):
    """y and the three gradients at 1, RPB - 1, RPB + 1 and 1000 rows, on centred rows, rows 1000 sigma off (100 in the half types),
    both mixed with nearly constant rows, and nearly constant rows alone; a second run gives the same bits"""
    j = Judge("layer_norm", "C = %d %s (groups of %d lanes)" % (C, NC.dtype_name(dtype), NC.ln_lp(C)))
    for rows in NC.ln_row_counts(C):
        for kind in NC.LN_KINDS:
            _ln_case(rows, C, kind, dtype, j)
    fails = j.finish()
    assert not fails, fails


@pytest.mark.parametrize("C,rows", NC.LN_CAPPED, ids=["C4-65573-rows", "C132-32773-rows"])
def test_layer_norm_capped(C, rows):
    """more row groups than 512 blocks of eight passes hold: the grid-stride loop's ninth trip and beyond"""
    j = Judge("layer_norm", "C = %d rows = %d fp32 (capped, D = %d)" % (C, rows, NC.ln_depth(rows, C)))
    _ln_case(rows, C, "mixed", F32, j)
    fails = j.finish()
    assert not fails, fails


@pytest.mark.parametrize("C,rows", [(4, 16 * 8 + 3), (68, 8 * 8 * 2 + 5), (132, 37), (256, 4 * 8 + 1), (60, 1)])
@pytest.mark.parametrize("dtype", (F32, torch.bfloat16), ids=NC.dtype_name)
def test_layer_norm_writes_nothing_but_its_outputs(C, rows, dtype):
    """the C entry points with x, y, mean, rstd and g_x as views inside NaN-filled buffers, at ragged row counts: after the forward and
    the backward every element outside the outputs is untouched, every output element written, and the results are LayerNormFn's"""
    from hipops import lib as L
    from hipops.functions import DTYPE_CODE, LayerNormFn, _p, _ws, _ws_bytes
    lib, code, n = L.load(), DTYPE_CODE[dtype], rows * C
    r = NC.ln_ref(rows, C, "mixed", dtype)
    w, b = r.w.cuda(), r.b.cuda()
    xb, x = NC.guarded(n, dtype)
    gb_, g = NC.guarded(n, dtype)
    x.copy_(r.x.cuda().flatten()), g.copy_(r.g.cuda().flatten())
    yb, y = NC.guarded(n, dtype)
    mb, mean = NC.guarded(rows)
    rb, rstd = NC.guarded(rows)
    gxb, gx = NC.guarded(n, dtype)
    gwbb, gwb = NC.guarded(2 * C)
    L.check(lib.dd_layer_norm_fwd_t(_p(x), rows, C, _p(w), _p(b), NC.LN_EPS, _p(y), _p(mean), _p(rstd), code, L.current_stream()), "dd_layer_norm_fwd_t")
    nbytes = _ws_bytes("dd_layer_norm_workspace_bytes", C)
    ws = _ws(nbytes, "cuda")
    L.check(lib.dd_layer_norm_bwd_t(_p(x), _p(g), _p(w), _p(mean), _p(rstd), rows, C, _p(gx), _p(gwb), _p(ws), nbytes, code, L.current_stream()),
            "dd_layer_norm_bwd_t")
    torch.cuda.synchronize()
    for name, buf, k in (("y", yb, n), ("mean", mb, rows), ("rstd", rb, rows), ("g_x", gxb, n), ("g_gamma_beta", gwbb, 2 * C)):
        assert NC.guards_intact(buf, k), name
    assert bool(torch.isnan(xb[:256]).all()) and bool(torch.isnan(xb[256 + n:]).all()) and torch.equal(x, r.x.cuda().flatten())
    x2, w2, b2 = r.x.cuda().requires_grad_(), w.clone().requires_grad_(), b.clone().requires_grad_()
    y2 = LayerNormFn.apply(x2, w2, b2, NC.LN_EPS)
    y2.backward(r.g.cuda())
    assert torch.equal(y.view(rows, C), y2.detach()) and torch.equal(gx.view(rows, C), x2.grad)
    assert torch.equal(gwb[:C], w2.grad) and torch.equal(gwb[C:], b2.grad)


# ---- layer-scale residual ----------------------------------------------------------------------------------------------------------
LS_PARAMS = [c + (d,) for c in NC.LS_CASES for d in NC.DTYPES]


@pytest.mark.parametrize("B,hw,C,dtype", LS_PARAMS, ids=["B%d-hw%d-C%d-%s" % (p[0], p[1], p[2], NC.dtype_name(p[3])) for p in LS_PARAMS])
def test_layer_scale_residual(B, hw, C, dtype):
    """res + y * scale with scale ~ 1e-6 and the last image dropped (factor exactly 0): the output (the HIP forward in the half types),
    g_res = g, g_y (exactly 0 on the dropped image) and g_scale = sum g * y (on the dropped image too); the sums bit-reproducible"""
    from hipops.functions import LayerScaleResidualFn
    r = NC.ls_ref(B, hw, C, dtype)
    runs = []
    for _ in range(2):
        res, y, scale = r.res.cuda().requires_grad_(), r.y.cuda().requires_grad_(), r.scale.cuda().requires_grad_()
        out = LayerScaleResidualFn.apply(res, y, scale)
        assert out.dtype == dtype and out.grad_fn.name().startswith("LayerScaleResidualFn")
        out.backward(r.g.cuda())
        runs.append((out.detach(), res.grad, y.grad, scale.grad))
    torch.cuda.synchronize()
    out, gres, gy, gs = runs[0]
    assert gy.dtype == dtype and gs.dtype == F32 and gs.shape == (B, 1, 1, C)
    j = Judge("layer_scale", "B = %d hw = %d C = %d %s (D = %d)" % (B, hw, C, NC.dtype_name(dtype), NC.ls_depth(hw, C)))
    j.check_elem("out", out, r.out64, r.out32, r.s_out, NC.floor("ls out"), dtype)
    j.equal("g_res (copy)", gres, r.g)
    j.check_elem("g_y", gy, r.g64[1], r.g32[1], r.s_gy, NC.floor("ls g_y"), dtype)
    j.check_abs("g_scale", gs, r.g64[2], r.g32[2], r.b_gs)
    if r.dropped is not None:
        j.equal("g_y of the dropped image", gy[r.dropped], torch.zeros_like(gy[r.dropped]))
    for name, a, o in zip(("out", "g_res", "g_y", "g_scale"), runs[0], runs[1]):
        j.equal("second run " + name, o, a)
    fails = j.finish()
    assert not fails, fails


# ---- depth-wise convolution --------------------------------------------------------------------------------------------------------
DW_PARAMS = [(ci, F32) for ci in range(len(NC.DW_CASES))] + [(ci, h) for ci in NC.DW_HALF_CASES for h in NC.HALF]


@pytest.mark.parametrize("ci,dtype", DW_PARAMS, ids=["%s-%s" % (NC.DW_CASE_IDS[ci], NC.dtype_name(d)) for ci, d in DW_PARAMS])
def test_depthwise_conv(ci, dtype):
    """forward, data gradient and weight gradient; the weight gradient of a second run has the same bits"""
    from hipops.functions import DepthwiseConv3x3NHWCFn
    r = NC.dw_ref(ci, dtype)
    c = r.case
    runs = []
    for _ in range(2):
        x, w = nhwc(r.x, True), r.w.cuda().requires_grad_()
        y = DepthwiseConv3x3NHWCFn.apply(x, w, c.dil)
        assert y.dtype == dtype and y.shape == r.x.shape and y.is_contiguous(memory_format=CL)
        y.backward(nhwc(r.g))
        runs.append((y.detach(), x.grad, w.grad))
    torch.cuda.synchronize()
    y, gx, gw = runs[0]
    assert gx.dtype == dtype and gw.dtype == F32 and gw.shape == r.w.shape
    j = Judge("dwconv3x3", "%s %s (D = %d)" % (NC.DW_CASE_IDS[ci], NC.dtype_name(dtype), NC.dw_depth(c.B, c.H, c.W, c.C)))
    j.check_elem("y", y, r.y64, r.y32, r.s_y, NC.floor("dw out"), dtype)
    j.check_elem("g_x", gx, r.g64[0], r.g32[0], r.s_gx, NC.floor("dw g_x"), dtype)
    j.check_abs("g_weight", gw, r.g64[1], r.g32[1], r.b_gw)
    j.equal("second run g_weight", runs[1][2], gw)
    fails = j.finish()
    assert not fails, fails


@pytest.mark.parametrize("ci", NC.DW_GUARD_CASES, ids=[NC.DW_CASE_IDS[i] for i in NC.DW_GUARD_CASES])
@pytest.mark.parametrize("dtype", (F32, torch.float16), ids=NC.dtype_name)
def test_depthwise_conv_writes_nothing_but_its_output(ci, dtype):
    """H is no multiple of the four rows a thread computes: the rows past the end are computed and must not be stored.  The C entry
    point with the output as a view inside a NaN-filled buffer; the result is DepthwiseConv3x3NHWCFn's"""
    from hipops import lib as L
    from hipops.functions import DTYPE_CODE, DepthwiseConv3x3NHWCFn, _p
    r = NC.dw_ref(ci, dtype)
    c = r.case
    n = c.B * c.C * c.H * c.W
    x, w = nhwc(r.x), r.w.cuda()
    buf, out = NC.guarded(n, dtype)
    L.check(L.load().dd_dwconv3x3_nhwc_t(_p(x), _p(w), c.B, c.H, c.W, c.C, c.dil, _p(out), DTYPE_CODE[dtype], L.current_stream()), "dd_dwconv3x3_nhwc_t")
    torch.cuda.synchronize()
    assert NC.guards_intact(buf, n)
    want = DepthwiseConv3x3NHWCFn.apply(x, w, c.dil)
    assert torch.equal(out.view(c.B, c.H, c.W, c.C), want.permute(0, 2, 3, 1))
