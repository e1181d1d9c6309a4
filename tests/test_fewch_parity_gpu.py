"""The few-channel convolutions between the encoders and the loss -- csrc/dd_conv_small.hip, csrc/dd_conv_head.hip,
conv3x3_cout1_bwd_data_kernel of csrc/dd_dwconv.hip and csrc/dd_redu.hip -- against F.conv2d and its adjoints in float64 on the CPU,
element by element, on off-centre inputs (activations and image stacks have a mean), at the shapes where a tile, a strip, a persistent
loop, a workgroup cap or a fold can go wrong: images of one pixel, one short of / exactly / one over a tile or a pixel group, tile and
workgroup counts on both sides of every fold boundary (31..33, 96..98 partials at the 4x-unrolled fold, 32, 33, 64, 65 at the 2x ones)
and of the caps (1024, 1025, 1050, 2100 tiles; 8193 pixel groups), all 18 supported (ks, cin, cout) triples as a forward layer.

Every case also runs on small integers, where every sum in any order is exact in fp32: torch.equal against float64 -- what sees a
dropped or doubled pixel, tap, channel or partial.  Every entry point is launched through the C ABI with each output between NaN guard
bands and each workspace exactly dd_*_workspace_bytes long, between guards and pre-filled with NaN (a fold that reads a partial nobody
wrote, or a store past the advertised size, fails); every launch runs twice and must give the same bits; NULL bias, NULL g_bias, one of
g_a / g_b NULL, the weight in either layout.  The autograd wrappers run on a subset.

tests/fewch_case.py holds the cases, the references and the criterion (nothing in a bound from the kernel's output);
tests/test_fewch_inputs.py asserts on the CPU that the fp32 reference is inside F * scale_i by itself and that every shape reaches what it names.

Every case prints one `worst:` and one `ratios:` line (run with -s).  Largest e_k / bound per family and quantity on one MI355X run:

    family (C ABI)            largest e_k / bound per quantity, off-centre and zero-centred inputs
    conv_small                y 0.19  g_x 0.25  g_weight 0.06  g_bias 0.05
    conv_head                 out 0.10  g_x 0.25  g_weight 0.13  g_bias 0.05
    conv3x3_cout1_bwd_data    g_x 0.20
    redu                      y 0.10  g_a 0.17  g_b 0.17  g_weight 0.14  g_bias 0.08
    SmallConvFn               y 0.12  g_x 0.08  g_weight 0.03  g_bias 0.03
    HeadConvFn / ConvBiasFn   out 0.08  g_x 0.20 / 0.14  g_weight 0.07  g_bias 0.02
    ReduFn                    y 0.06  g_a 0.12  g_b 0.13  g_weight 0.11  g_bias 0.04

Every integer case is bit-equal to float64 and every second launch bit-equal to the first.  profiles/fewch_parity.txt keeps these
figures and what the file does to five arithmetic mutants of the kernels (a tap flip dropped, the persistent loop left after one tile,
an accumulator added twice in the first fold, a shuffle step short, a fold slice short): each fails its narrowest case here, by 4.9 x
to 2 * 10^5 x its bound and in torch.equal.
"""
import pytest
import torch

import fewch_case as FC
from fewch_case import Judge

pytestmark = pytest.mark.gpu
F32 = torch.float32

CS_PARAMS = list(range(len(FC.CS_CASES)))
CH_PARAMS = list(range(len(FC.CH_CASES)))
C1_PARAMS = list(range(len(FC.C1_CASES)))
RD_PARAMS = list(range(len(FC.RD_CASES)))
VARIANTS = [(layout, bias) for layout in ("cl", "nchw") for bias in (True, False)]          # the weight's layout; bias and g_bias given or NULL


def _elem(j, r, qty, got, w64, w32, scale, fl):
    if r.exact:
        j.equal(qty, got.detach().double().cpu().reshape(w64.shape), w64)
    else:
        j.check_elem(qty, got, w64, w32, scale, fl, F32)


def _sum(j, r, qty, got, w64, terms):
    if r.exact:
        j.equal(qty, got.detach().double().cpu().reshape(w64.shape), w64)
    else:
        j.check_abs(qty, got, w64, w64, FC.depth_bound(r.D, terms))


def _twice(j, launch):
    """the launch sequence twice, each into fresh guarded buffers: the guards of both, and the same bits"""
    first, fails = launch()
    second, fails2 = launch()
    j.fails += fails + fails2
    for k, v in first.items():
        if v is not None:
            j.equal(k + " again", second[k], v)
    return first


def test_supported_set_is_the_eighteen_triples():
    from hipops import lib as L
    lib = L.load()
    got = {(ks, ci, co) for ks in range(0, 6) for ci in range(0, 19) for co in range(0, 19) if lib.dd_conv_small_supported(ks, ci, co)}
    assert got == set(FC.CS_TRIPLES) and len(got) == 18
    assert all(bool(lib.dd_conv_head_supported(C)) == (C in FC.CH_CHANNELS) for C in range(0, 130))
    assert all(bool(lib.dd_redu_supported(C, co)) == (C in FC.RD_SHAPES and co in FC.RD_COUTS) for C in range(0, 1030, 2) for co in range(0, 5))


# ---- dd_conv_small -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", CS_PARAMS, ids=FC.CS_CASE_IDS)
def test_small_conv(ci):
    """forward, data gradient, weight + bias gradient: the weight channels-last and NCHW-contiguous (addressed through its strides),
    each with bias and g_bias and with both NULL"""
    c = FC.CS_CASES[ci]
    fails = []
    for kind in c.kinds:
        r = FC.cs_ref(ci, kind)
        for layout, bias in VARIANTS:
            j = Judge("conv_small", "%s %s %s bias=%d" % (FC.CS_CASE_IDS[ci], kind, layout, bias))
            o = _twice(j, lambda: FC.cs_launch(r, layout, bias, bias))
            if bias:
                _elem(j, r, "y", o["y"], r.y, None if r.exact else r.y_32, None if r.exact else r.s_y, r.fl_y)
                _sum(j, r, "g_bias", o["g_bias"], r.g_b, r.t_gb)
            else:
                _elem(j, r, "y", o["y"], r.y0, None if r.exact else r.y0_32, None if r.exact else r.s_y0, r.fl_y)
                assert o["g_bias"] is None
            _elem(j, r, "g_x", o["g_x"], r.g_x, None if r.exact else r.g_x32, None if r.exact else r.s_gx, r.fl_gx)
            _sum(j, r, "g_weight", o["g_weight"], r.g_w, None if r.exact else r.t_gw)
            fails += j.finish()
    assert not fails, fails


CS_FN = [("k3-12to9-2x9x33", "nchw", "nchw", False, (True, True)),          # NCHW input and gradient (converted on the way in), contiguous weight, no bias
         ("k1-3to12-1x7x31", "cl", "cl", True, (False, True)),              # the weight and bias gradient alone
         ("k3-9to12-1x7x31", "cl", "nchw", True, (True, False)),            # the data gradient alone
         ("k3-16to12-3x8x323", "cl", "cl", True, (True, True))]


@pytest.mark.parametrize("name,x_layout,w_layout,bias,needs", CS_FN, ids=[p[0] for p in CS_FN])
def test_small_conv_function(name, x_layout, w_layout, bias, needs):
    """SmallConvFn hands over the same arguments: layouts, needs_input_grad subsets, the permuted view returned for g_weight"""
    from hipops.functions import SmallConvFn
    ci = FC.CS_CASE_IDS.index(name)
    c = FC.CS_CASES[ci]
    fails = []
    for kind in ("off", "int"):
        r = FC.cs_ref(ci, kind)
        outs = []
        for _ in range(2):
            x = (r.x.cuda() if x_layout == "nchw" else FC.nhwc_dev(r.x).permute(0, 3, 1, 2)).requires_grad_(needs[0])
            w = FC.weight_layout(r.w, w_layout).requires_grad_(needs[1])
            b = r.b.cuda().requires_grad_(needs[1]) if bias else None
            g = r.g.cuda() if x_layout == "nchw" else FC.nhwc_dev(r.g).permute(0, 3, 1, 2)
            y = SmallConvFn.apply(x, w, b)
            y.backward(g)
            outs.append((y.detach(), x.grad, w.grad, None if b is None else b.grad))
        torch.cuda.synchronize()
        j = Judge("SmallConvFn", "%s %s" % (name, kind))
        y, gx, gw, gb = outs[0]
        for k, (p, q) in zip(("y", "g_x", "g_weight", "g_bias"), zip(*outs)):
            assert (p is None) == (q is None)
            if p is not None:
                j.equal(k + " again", q, p)
        assert y.shape == (c.B, c.cout, c.H, c.W) and (gx is None) == (not needs[0]) and (gw is None) == (not needs[1]) and (gb is None) == (not (bias and needs[1]))
        if bias:
            _elem(j, r, "y", y, r.y, None if r.exact else r.y_32, None if r.exact else r.s_y, r.fl_y)
        else:
            _elem(j, r, "y", y, r.y0, None if r.exact else r.y0_32, None if r.exact else r.s_y0, r.fl_y)
        if gx is not None:
            assert gx.shape == r.x.shape
            _elem(j, r, "g_x", gx, r.g_x, None if r.exact else r.g_x32, None if r.exact else r.s_gx, r.fl_gx)
        if gw is not None:
            assert gw.shape == r.w.shape
            _sum(j, r, "g_weight", gw, r.g_w, None if r.exact else r.t_gw)
        if gb is not None:
            _sum(j, r, "g_bias", gb, r.g_b, r.t_gb)
        fails += j.finish()
    assert not fails, fails


# ---- dd_conv_head and its data gradient ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", CH_PARAMS, ids=FC.CH_CASE_IDS)
def test_disparity_head(ci):
    """forward and weight + bias gradient with the weight in either layout, with and without bias, g_bias NULL; the data gradient
    (dd_conv3x3_cout1_bwd_data at padding 0 on the padded input's shape)"""
    c = FC.CH_CASES[ci]
    fails = []
    for kind in c.kinds:
        r = FC.ch_ref(ci, kind)
        for layout, bias in VARIANTS:
            j = Judge("conv_head", "%s %s %s bias=%d" % (FC.CH_CASE_IDS[ci], kind, layout, bias))
            o = _twice(j, lambda: FC.ch_launch(r, layout, bias, bias))
            if bias:
                _elem(j, r, "out", o["out"], r.y, None if r.exact else r.y_32, None if r.exact else r.s_y, r.fl_y)
                _sum(j, r, "g_bias", o["g_bias"], r.g_b, r.t_gb)
            else:
                _elem(j, r, "out", o["out"], r.y0, None if r.exact else r.y0_32, None if r.exact else r.s_y0, r.fl_y)
            _sum(j, r, "g_weight", o["g_weight"], r.g_w, None if r.exact else r.t_gw)
            fails += j.finish()
        j = Judge("conv_head", "%s %s data gradient" % (FC.CH_CASE_IDS[ci], kind))

        def data_gradient():
            gx, f = FC.c1_launch(r.g, r.w, c.B, c.C, c.Ho + 2, c.Wo + 2, 0)
            return {"g_x": gx}, f
        o = _twice(j, data_gradient)
        _elem(j, r, "g_x", o["g_x"], r.g_x, None if r.exact else r.g_x32, None if r.exact else r.s_gx, r.fl_gx)
        fails += j.finish()
    assert not fails, fails


CH_FN = [("B2-C32-9x33", "cl", True, (True, True)), ("B2-C32-9x33", "nchw", False, (True, True)), ("B2-C64-7x17", "nchw", True, (False, True)),
         ("B1-C64-33x193", "cl", True, (True, False))]


@pytest.mark.parametrize("name,w_layout,bias,needs", CH_FN, ids=["%s-%s-bias%d" % p[:3] for p in CH_FN])
def test_disparity_head_function(name, w_layout, bias, needs):
    """HeadConvFn: the weight through its strides in either layout, no bias, needs_input_grad subsets, the permuted g_weight view"""
    from hipops.functions import HeadConvFn
    ci = FC.CH_CASE_IDS.index(name)
    fails = []
    for kind in ("off", "int"):
        r = FC.ch_ref(ci, kind)
        x = FC.nhwc_dev(r.x).permute(0, 3, 1, 2).requires_grad_(needs[0])
        w = FC.weight_layout(r.w, w_layout).requires_grad_(needs[1])
        b = r.b.cuda().requires_grad_(needs[1]) if bias else None
        y = HeadConvFn.apply(x, w, b)
        y.backward(r.g.cuda())
        torch.cuda.synchronize()
        j = Judge("HeadConvFn", "%s %s %s" % (name, kind, w_layout))
        assert y.shape == r.g.shape and (x.grad is None) == (not needs[0]) and (w.grad is None) == (not needs[1])
        if bias:
            _elem(j, r, "out", y, r.y, None if r.exact else r.y_32, None if r.exact else r.s_y, r.fl_y)
        else:
            _elem(j, r, "out", y, r.y0, None if r.exact else r.y0_32, None if r.exact else r.s_y0, r.fl_y)
        if needs[0]:
            _elem(j, r, "g_x", x.grad, r.g_x, None if r.exact else r.g_x32, None if r.exact else r.s_gx, r.fl_gx)
        if needs[1]:
            assert w.grad.shape == r.w.shape
            _sum(j, r, "g_weight", w.grad, r.g_w, None if r.exact else r.t_gw)
            if bias:
                _sum(j, r, "g_bias", b.grad, r.g_b, r.t_gb)
        fails += j.finish()
    assert not fails, fails


@pytest.mark.parametrize("ci", C1_PARAMS, ids=FC.C1_CASE_IDS)
def test_one_channel_data_gradient(ci):
    """dd_conv3x3_cout1_bwd_data at padding 0 and 1, 4 to 512 channels"""
    c = FC.C1_CASES[ci]
    fails = []
    for kind in c.kinds:
        r = FC.c1_ref(ci, kind)
        j = Judge("conv3x3_cout1_bwd_data", "%s %s" % (FC.C1_CASE_IDS[ci], kind))

        def launch():
            gx, f = FC.c1_launch(r.g, r.w, c.B, c.C, c.Hi, c.Wi, c.pad)
            return {"g_x": gx}, f
        o = _twice(j, launch)
        _elem(j, r, "g_x", o["g_x"], r.g_x, None if r.exact else r.g_x32, None if r.exact else r.s_gx, r.fl_gx)
        fails += j.finish()
    assert not fails, fails


def test_one_channel_data_gradient_inside_the_biased_convolution():
    """ConvBiasFn at padding 1 with one output channel takes the same kernel for the data gradient"""
    from hipops.functions import ConvBiasFn
    ci = FC.C1_FUNCTION_CASE
    c = FC.C1_CASES[ci]
    assert c.pad == 1
    fails = []
    for kind in ("off", "int"):
        r = FC.c1_ref(ci, kind)
        x = FC.nhwc_dev(r.x).permute(0, 3, 1, 2).requires_grad_()
        assert x.is_contiguous(memory_format=torch.channels_last) and not x.is_contiguous()
        w, b = r.w.cuda().requires_grad_(), r.b.cuda().requires_grad_()
        y = ConvBiasFn.apply(x, w, b, (1, 1), (1, 1), (1, 1), 1)
        y.backward(r.g.cuda())
        torch.cuda.synchronize()
        j = Judge("ConvBiasFn", "%s %s" % (FC.C1_CASE_IDS[ci], kind))
        _elem(j, r, "g_x", x.grad, r.g_x, None if r.exact else r.g_x32, None if r.exact else r.s_gx, r.fl_gx)
        fails += j.finish()
    assert not fails, fails


# ---- dd_redu -----------------------------------------------------------------------------------------------------------------------
def _rd_judge(j, r, o, bias, want):
    C = r.case.C
    if bias:
        _elem(j, r, "y", o["y"], r.y, None if r.exact else r.y_32, None if r.exact else r.s_y, r.fl_y)
        _sum(j, r, "g_bias", o["g_bias"], r.g_b, r.t_gb)
    else:
        _elem(j, r, "y", o["y"], r.y0, None if r.exact else r.y0_32, None if r.exact else r.s_y0, r.fl_y)
    for k, sl in (("g_a", slice(0, C)), ("g_b", slice(C, 2 * C))):
        if k in want:
            _elem(j, r, k, o[k], r.g_x[:, sl], None if r.exact else r.g_x32[:, sl], None if r.exact else r.s_gx[:, sl], r.fl_gx)
        else:
            assert o[k] is None
    _sum(j, r, "g_weight", o["g_weight"], r.g_w, None if r.exact else r.t_gw)


@pytest.mark.parametrize("ci", RD_PARAMS, ids=FC.RD_CASE_IDS)
def test_reduction(ci):
    """forward, both data gradients, weight + bias gradient; then no bias, g_bias NULL and g_a alone; then g_b alone"""
    c = FC.RD_CASES[ci]
    fails = []
    for kind in c.kinds:
        r = FC.rd_ref(ci, kind)
        for bias, want in ((True, ("g_a", "g_b")), (False, ("g_a",)), (True, ("g_b",))):
            j = Judge("redu", "%s %s bias=%d %s" % (FC.RD_CASE_IDS[ci], kind, bias, "+".join(want)))
            o = _twice(j, lambda: FC.rd_launch(r, bias, bias, want))
            _rd_judge(j, r, o, bias, want)
            fails += j.finish()
    assert not fails, fails


RD_FN = [("C128-to3-P65", True, (True, True, True)), ("C64-to1-P15", False, (True, False, True)), ("C512-to3-P33", True, (False, True, False)),
         ("C256-to1-P4", True, (False, False, True))]


@pytest.mark.parametrize("name,bias,needs", RD_FN, ids=[p[0] for p in RD_FN])
def test_reduction_function(name, bias, needs):
    """ReduFn: a (cout, 2C, 1, 1) weight, needs_input_grad subsets (a alone, b alone, the weight alone), no bias"""
    from hipops.functions import ReduFn
    ci = FC.RD_CASE_IDS.index(name)
    c = FC.RD_CASES[ci]
    fails = []
    for kind in ("off", "int"):
        r = FC.rd_ref(ci, kind)
        xm = FC.rd_matrix(r.x)
        a = xm[:, :c.C].contiguous().cuda().view(1, c.P, 1, c.C).permute(0, 3, 1, 2).requires_grad_(needs[0])
        b = xm[:, c.C:].contiguous().cuda().view(1, c.P, 1, c.C).permute(0, 3, 1, 2).requires_grad_(needs[1])
        w = r.w.cuda().requires_grad_(needs[2])
        bv = r.b.cuda().requires_grad_(needs[2]) if bias else None
        y = ReduFn.apply(a, b, w, bv)
        y.backward(r.g.cuda())
        torch.cuda.synchronize()
        assert y.shape == r.g.shape and (a.grad is None) == (not needs[0]) and (b.grad is None) == (not needs[1]) and (w.grad is None) == (not needs[2])
        j = Judge("ReduFn", "%s %s" % (name, kind))
        o = {"y": y, "g_a": a.grad, "g_b": b.grad, "g_weight": w.grad, "g_bias": None if bv is None else bv.grad}
        if bias and needs[2]:
            _sum(j, r, "g_bias", o["g_bias"], r.g_b, r.t_gb)
        if bias:
            _elem(j, r, "y", y, r.y, None if r.exact else r.y_32, None if r.exact else r.s_y, r.fl_y)
        else:
            _elem(j, r, "y", y, r.y0, None if r.exact else r.y0_32, None if r.exact else r.s_y0, r.fl_y)
        for k, sl, need in (("g_a", slice(0, c.C), needs[0]), ("g_b", slice(c.C, 2 * c.C), needs[1])):
            if need:
                assert o[k].shape == (1, c.C, c.P, 1)
                _elem(j, r, k, o[k], r.g_x[:, sl], None if r.exact else r.g_x32[:, sl], None if r.exact else r.s_gx[:, sl], r.fl_gx)
        if needs[2]:
            assert w.grad.shape == r.w.shape
            _sum(j, r, "g_weight", w.grad, r.g_w, None if r.exact else r.t_gw)
        fails += j.finish()
    assert not fails, fails
