"""The decoder glue (dd_up_cat_pad_t / _bwd_t), the channels-last reflection pad (dd_reflect_pad1_nhwc_t / _bwd_t) and the bias
gradient (dd_channel_sum_nhwc_t) against the reference's operator sequence in float64 on the CPU, element by element, in fp32, fp16
and bf16, at the shapes where a thread-to-pixel mapping, a border rule or a fold can go wrong: the two border rules on adjacent
indices, odd unequal sizes, channel groups of 1 / 3 / 5 / 7, a padded row that ends inside a workgroup and a pixel split across two,
one gradient requested without the other, ELU at 0, -0, +-2^-126, small negatives, -20, -104 and +50, taps that nearly cancel,
three batches; column sums on both paths of the kernel up to the cap of 2048 workgroups and the wide path's empty chunks.

tests/glue_case.py holds the cases, the references and the one criterion (nothing in a bound from the kernel's output);
tests/test_glue_inputs.py asserts on the CPU that the inputs are what is claimed here.

Every case prints one `worst:` line (run with -s); profiles/glue_parity.txt keeps those of one MI355X run as a record.
"""
import pytest
import torch

import glue_case as GC
from glue_case import Judge

gpu = pytest.mark.gpu
HIP_ERROR_INVALID_VALUE = 1
CL = torch.channels_last


def nhwc(t, requires_grad=False):
    return None if t is None else t.detach().cuda().contiguous(memory_format=CL).requires_grad_(requires_grad)


# ---- dd_up_cat_pad -----------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dtype", GC.DTYPES, ids=GC.dtype_name)
@pytest.mark.parametrize("ci", range(len(GC.CASES)), ids=GC.CASE_IDS)
def test_up_cat_pad(ci, dtype):
    from hipops.functions import UpCatPadFn, up_cat_pad_ok
    r = GC.glue_ref(ci, dtype)
    c = r.case
    H, W = GC.dims(c)
    fails = []
    for needs in (GC.NEEDS if c.C2 else GC.NEEDS[:1]):
        x, skip, g = nhwc(r.x, needs[0]), nhwc(r.skip, needs[1] and c.C2 > 0), nhwc(r.g)
        assert up_cat_pad_ok(x, skip, c.mode)
        out = UpCatPadFn.apply(x, skip, c.mode, c.elu)
        assert out.shape == (c.B, c.C1 + c.C2, H + 2, W + 2) and out.dtype == dtype and out.is_contiguous(memory_format=CL)
        out.backward(g)
        torch.cuda.synchronize()
        j = Judge("up_cat_pad", "%s %s gradient of %s" % (c.name, GC.dtype_name(dtype), "+".join(n for n, need in zip(("x", "skip"), needs) if need)))
        if GC.x_half_is_a_copy(c):
            j.equal("out[:, :C1] (copy)", out[:, :c.C1], r.out64[:, :c.C1].to(dtype))
        else:
            j.check_elem("out[:, :C1]", out[:, :c.C1], r.out64[:, :c.C1], r.out32[:, :c.C1], r.s_out[:, :c.C1], GC.out_kind(c), dtype)
        if c.C2:
            j.equal("out[:, C1:] (copy)", out[:, c.C1:], r.out64[:, c.C1:].to(dtype))
        if needs[0]:
            assert x.grad.dtype == dtype
            j.check_elem("g_x", x.grad, r.gx64, r.gx32, r.s_gx, GC.gx_kind(c), dtype)
        else:
            assert x.grad is None
        if c.C2 and needs[1]:
            assert skip.grad.dtype == dtype
            j.check_elem("g_skip", skip.grad, r.gs64, r.gs32, r.s_gs, "g_skip", dtype)
        elif c.C2:
            assert skip.grad is None
        fails += j.finish()
    assert not fails, fails


@gpu
def test_up_cat_pad_backward_returns_none_for_what_is_not_asked():
    """UpCatPadFn.backward itself: the gradient that is not needed is None (g_x / g_skip NULL in the C ABI), the other is what the
    both-gradients call gives, bit for bit"""
    import types
    from hipops.functions import UpCatPadFn
    ci = GC.CASE_IDS.index("mode1-elu1")
    r = GC.glue_ref(ci, torch.float32)
    c = r.case
    got = {}
    for needs in GC.NEEDS:
        ctx = types.SimpleNamespace(saved_tensors=(nhwc(r.x),), cfg=(c.C2, c.mode, int(c.elu)), needs_input_grad=needs + (False, False))
        grads = UpCatPadFn.backward(ctx, nhwc(r.g))
        assert len(grads) == 4 and (grads[0] is None) == (not needs[0]) and (grads[1] is None) == (not needs[1]), needs
        assert grads[2] is None and grads[3] is None
        got[needs] = grads
    torch.cuda.synchronize()
    assert torch.equal(got[(True, False)][0], got[(True, True)][0]) and torch.equal(got[(False, True)][1], got[(True, True)][1])


@gpu
@pytest.mark.parametrize("w", [3, 2])
def test_up_cat_pad_refuses_same_size_below_four_columns(w):
    """mode 2 with w < 4: hipErrorInvalidValue from both entry points and an untouched output (at W = 3 column 1 is mirrored by both
    padded borders; F.pad's column multiplicities are 1, 3, 1 and pad_fold has one mirror slot).  Nothing is launched."""
    from hipops import lib as L
    from hipops.functions import DTYPE_CODE, _p
    lib = L.load()
    B, h, C1, C2 = 2, 4, 8, 4
    for dtype in GC.DTYPES:
        code = DTYPE_CODE[dtype]
        x = torch.randn(B, h, w, C1, device="cuda").to(dtype)
        skip = torch.randn(B, h, w, C2, device="cuda").to(dtype)
        g = torch.randn(B, h + 2, w + 2, C1 + C2, device="cuda").to(dtype)
        out, gx, gs = torch.full_like(g, 7.0), torch.full_like(x, 7.0), torch.full_like(skip, 7.0)
        err = lib.dd_up_cat_pad_t(_p(x), _p(skip), B, h, w, C1, C2, 2, 1, _p(out), code, L.current_stream())
        torch.cuda.synchronize()
        assert err == HIP_ERROR_INVALID_VALUE, err
        assert bool((out == 7.0).all())
        err = lib.dd_up_cat_pad_bwd_t(_p(g), _p(x), B, h, w, C1, C2, 2, 1, _p(gx), _p(gs), code, L.current_stream())
        torch.cuda.synchronize()
        assert err == HIP_ERROR_INVALID_VALUE, err
        assert bool((gx == 7.0).all()) and bool((gs == 7.0).all())


# ---- dd_reflect_pad1_nhwc_t --------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dtype", GC.DTYPES, ids=GC.dtype_name)
@pytest.mark.parametrize("shape", GC.PAD_CASES, ids=str)
def test_reflect_pad(shape, dtype):
    """C > 1 through ReflectPad1NHWCFn; C = 1 (which Python routes to ATen) through the C ABI, which takes it"""
    from hipops import lib as L
    from hipops.functions import DTYPE_CODE, ReflectPad1NHWCFn, _p
    H, W, C = shape
    B, r = GC.PAD_B, GC.pad_ref(H, W, C, dtype)
    if C > 1:
        x = nhwc(r.x, True)
        out = ReflectPad1NHWCFn.apply(x)
        assert out.is_contiguous(memory_format=CL) and out.dtype == dtype
        out.backward(nhwc(r.g))
        gx = x.grad
    else:
        lib = L.load()
        x, g = r.x.permute(0, 2, 3, 1).contiguous().cuda(), r.g.permute(0, 2, 3, 1).contiguous().cuda()
        out_l = torch.full((B, H + 2, W + 2, C), float("nan"), device="cuda", dtype=dtype)
        gx_l = torch.full((B, H, W, C), float("nan"), device="cuda", dtype=dtype)
        L.check(lib.dd_reflect_pad1_nhwc_t(_p(x), B, H, W, C, _p(out_l), DTYPE_CODE[dtype], L.current_stream()), "dd_reflect_pad1_nhwc_t")
        L.check(lib.dd_reflect_pad1_nhwc_bwd_t(_p(g), B, H, W, C, _p(gx_l), DTYPE_CODE[dtype], L.current_stream()), "dd_reflect_pad1_nhwc_bwd_t")
        out, gx = out_l.permute(0, 3, 1, 2), gx_l.permute(0, 3, 1, 2)
    torch.cuda.synchronize()
    j = Judge("reflect_pad1", "%s %s %s" % (shape, GC.dtype_name(dtype), "autograd" if C > 1 else "C ABI"))
    j.equal("out (copy)", out, r.out)
    j.check_elem("g_x", gx, r.gx64, r.gx32, r.s_gx, "pad g_x", dtype)
    fails = j.finish()
    assert not fails, fails


# ---- dd_channel_sum_nhwc_t ---------------------------------------------------------------------------------------------------------
def channel_sum_case(C, rows, dtype, j):
    from hipops import lib as L
    from hipops.functions import DTYPE_CODE, _channel_sum
    for mean in GC.CS_MEANS:
        x = GC.channel_sum_input(rows, C, mean, dtype)
        want, ref32, bound = GC.channel_sum_bound(x, rows, C)
        xg = x.cuda()
        got = _channel_sum(xg, rows, C, DTYPE_CODE[dtype], L.current_stream())
        again = _channel_sum(xg, rows, C, DTYPE_CODE[dtype], L.current_stream())
        torch.cuda.synchronize()
        assert got.dtype == torch.float32 and got.shape == (C,)
        j.check_sum("sum C=%d rows=%d N(%g,1)" % (C, rows, mean), got, want, ref32, bound)
        j.equal("second run C=%d rows=%d N(%g,1)" % (C, rows, mean), again, got)         # no atomics: the same bits


@gpu
@pytest.mark.parametrize("dtype", GC.DTYPES, ids=GC.dtype_name)
@pytest.mark.parametrize("C", GC.CS_NARROW_C + GC.CS_WIDE_C)
def test_channel_sum(C, dtype):
    j = Judge("channel_sum", "C = %d %s (%s path)" % (C, GC.dtype_name(dtype), "wide" if C > GC.CS_NT else "narrow"))
    for rows in (GC.CS_WIDE_ROWS if C > GC.CS_NT else GC.CS_NARROW_ROWS):
        channel_sum_case(C, rows, dtype, j)
    fails = j.finish()
    assert not fails, fails


@gpu
@pytest.mark.parametrize("dtype", GC.DTYPES, ids=GC.dtype_name)
@pytest.mark.parametrize("C,rows", [GC.CS_CAPPED_NARROW, GC.CS_CAPPED_WIDE], ids=["narrow-2048-workgroups", "wide-empty-chunks"])
def test_channel_sum_capped(C, rows, dtype):
    """the cap of 2048 workgroups (narrow) and of 2048 chunks, 47 of which start past the last row (wide): the sum is still right"""
    j = Judge("channel_sum", "C = %d rows = %d %s (capped, D = %d)" % (C, rows, GC.dtype_name(dtype), GC.channel_sum_depth(rows, C)))
    channel_sum_case(C, rows, dtype, j)
    fails = j.finish()
    assert not fails, fails
