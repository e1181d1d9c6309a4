"""The output store of the 32x32 accumulator tiles (csrc/dd_store_tile.h) in the five kernels that share it: conv_mfma_kernel and
conv_mfma_flat_kernel (csrc/dd_conv_mfma.hip), pw_gemm_kernel and mlp_fwd_kernel (csrc/dd_pw_gemm.hip), conv_half_kernel
(csrc/dd_conv_half.hip).  A full tile stores straight-line, an edge tile tests every store: the shapes here are the smallest at which
either path can go wrong -- partial tiles on both pixel axes, one / a partial second / a partial third block of output channels, two
channel tiles with a partial last one, row counts of 1, 33 and 257 -- none is a workload shape.

Exactness: small-integer operands against the float64 convolution.  Every product and every partial sum is an integer below 2^24,
exact in fp32 in any summation order, so the reference does not depend on the code under test and the comparison is torch.equal
after the cast to the output type (for the half types that cast is the one rounding the kernel itself does on the way out).

Guards: the C entry points write a dense (pixels, channels) matrix -- there is no pitch argument, hence no memory BETWEEN two pixel
rows that belongs to nobody: the output sits between two NaN-filled guard bands (the split-contraction workspace of the flat kernel
too), every guard element must still be NaN afterwards and every output element finite AND equal to the exact reference -- a stray
store of a lane beyond the last channel would land on the neighbouring pixel's channels and show there."""
import functools
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
os.environ.setdefault("DD_MLP", "1")          # as tests/test_pw_gemm_gpu.py: the point-wise path is opt-in

GUARD = 256                                    # floats in front of and behind the output (1 KB: keeps the 16-byte alignment)
HO, WO = 9, 33                                 # output pixels of the ragged image: a partial 8 x 32 tile on both axes


def _ints(gen, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=gen).float()


@functools.lru_cache(maxsize=None)
def _conv_case(cin, cout, pad, bias, B=1, Ho=HO, Wo=WO, xmax=4, wmax=2):
    """x (B,Hi,Wi,cin) channels-last, w (cout,cin,3,3), integer bias, an integer output gradient; the float64 forward and data
    gradient.  Computed once per case and shared (nothing below writes to them)."""
    gen = torch.Generator().manual_seed(1000 * cin + 10 * cout + pad)
    Hi, Wi = Ho + 2 - 2 * pad, Wo + 2 - 2 * pad
    x = _ints(gen, -xmax, xmax, B, Hi, Wi, cin).cuda().permute(0, 3, 1, 2)
    w = _ints(gen, -wmax, wmax, cout, cin, 3, 3).cuda()
    b = _ints(gen, -8, 8, cout).cuda() if bias else None
    g = _ints(gen, -4, 4, B, Ho, Wo, cout).cuda().permute(0, 3, 1, 2)
    ref = F.conv2d(x.double(), w.double(), None if b is None else b.double(), padding=pad)
    gref = torch.nn.grad.conv2d_input(x.shape, w.double(), g.double(), padding=pad)
    assert float(ref.abs().max()) < 2 ** 24 and float(gref.abs().max()) < 2 ** 24
    return x, w, b, g, ref, gref


def _guarded(n, dtype=torch.float32):
    """a NaN-filled buffer of GUARD + n + GUARD elements and the address of element GUARD"""
    buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=dtype, device="cuda")
    return buf, buf.data_ptr() + GUARD * buf.element_size()


def _check_guards(buf, n):
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[:GUARD]).all()), "a store in front of the output"
    assert bool(torch.isnan(buf[GUARD + n:]).all()), "a store behind the output"
    out = buf[GUARD:GUARD + n]
    assert bool(torch.isfinite(out).all()), "an output element was never written"
    return out


# ---- conv_mfma_kernel --------------------------------------------------------------------------------------------------------------
# cout: NB = 1; a partial second block; a partial third block; two channel tiles of 64 with a partial last one
TILE = [(pad, cout, bias) for pad in (0, 1) for cout in (16, 40, 72, 100) for bias in (True, False)]
TILE_IDS = ["pad%d-cout%d-%s" % (p, c, "bias" if b else "nobias") for p, c, b in TILE]


@pytest.mark.parametrize("pad,cout,bias", TILE, ids=TILE_IDS)
def test_tile_kernel_is_exact_on_ragged_tiles(pad, cout, bias):
    """|y| <= 9 * 16 * 8 + |b|; forward and data gradient (the same kernel, n_out = 16, pad' = 2 - pad: an 11 x 35 image at pad 0)"""
    from hipops import functions as Fn
    x, w, b, g, ref, gref = _conv_case(16, cout, pad, bias)
    assert not Fn._flat_shape(1, x.shape[2], x.shape[3], pad, 16, cout) and not Fn._flat_shape(1, x.shape[2], x.shape[3], pad, cout, 16)
    xr = x.clone().requires_grad_(True)
    y = Fn.mfma_conv(xr, w, b, pad)
    assert y.shape == ref.shape and torch.equal(y.detach(), ref.float()), float((y.detach().double() - ref).abs().max())
    (gx,) = torch.autograd.grad(y, xr, g)
    assert gx.shape == x.shape and torch.equal(gx, gref.float()), float((gx.double() - gref).abs().max())


def _tile_launch(inp, pack, bias, k_in, n_out, pad, ref):
    """dd_conv3x3_mfma through the C ABI into a guarded buffer; inp: (B,k_in,Hi,Wi) on channels-last memory"""
    from hipops import lib as L
    from hipops.functions import _p
    lib = L.load()
    B, _, Hi, Wi = inp.shape
    Ho, Wo = Hi + 2 * pad - 2, Wi + 2 * pad - 2
    n = B * Ho * Wo * n_out
    buf, yp = _guarded(n)
    L.check(lib.dd_conv3x3_mfma(_p(inp), _p(pack), _p(bias), B, Hi, Wi, k_in, n_out, pad, yp, L.current_stream()), "dd_conv3x3_mfma")
    out = _check_guards(buf, n).view(B, Ho, Wo, n_out).permute(0, 3, 1, 2)
    assert torch.equal(out, ref.float())


def _packs(w, name="dd_conv3x3_mfma"):
    from hipops import lib as L
    from hipops.functions import _p
    lib = L.load()
    cout, cin = w.shape[:2]
    pf = torch.empty(int(getattr(lib, name + "_pack_bytes")(cout, cin)) // 4, device="cuda")
    pb = torch.empty(int(getattr(lib, name + "_pack_bytes")(cin, cout)) // 4, device="cuda")
    sw = w.stride()
    L.check(lib.dd_conv3x3_mfma_pack(_p(w), sw[0], sw[1], sw[2], sw[3], cout, cin, _p(pf), _p(pb), L.current_stream()), "dd_conv3x3_mfma_pack")
    return pf, pb


@pytest.mark.parametrize("pad,cout,bias", TILE, ids=TILE_IDS)
def test_tile_kernel_writes_nothing_outside_its_output(pad, cout, bias):
    x, w, b, g, ref, gref = _conv_case(16, cout, pad, bias)
    pf, pb = _packs(w)
    _tile_launch(x, pf, b, 16, cout, pad, ref)
    _tile_launch(g, pb, None, cout, 16, 2 - pad, gref)


# ---- conv_mfma_flat_kernel ---------------------------------------------------------------------------------------------------------
# the smallest ragged cases of tests/test_conv_mfma_gpu.py's FLAT_CASES (B, cin, cout, H, W): a tile that ends inside an image with two
# channel tiles; fewer pixels than one 32-pixel block
FLAT = [(3, 64, 128, 7, 13), (5, 320, 64, 3, 3)]


@pytest.mark.parametrize("splits", ["1", "2"])
@pytest.mark.parametrize("case", FLAT, ids=lambda c: "x".join(map(str, c)))
def test_flat_kernel_is_exact_on_ragged_tiles(case, splits, monkeypatch):
    """|y| <= 9 * 320 * 8 + |b| < 2^24; gated as tests/test_conv_mfma_gpu.py gates its flat cases"""
    from hipops import functions as Fn
    from hipops import lib as L
    B, cin, cout, H, W = case
    monkeypatch.setenv("DD_FLAT_SPLITS", splits)
    Fn._WS_BYTES.clear()
    lib = L.load()
    assert lib.dd_conv3x3_mfma_flat_supported(B, H, W, cin, cout) and lib.dd_conv3x3_mfma_flat_supported(B, H, W, cout, cin)
    assert Fn._flat_shape(B, H, W, 1, cin, cout)
    x, w, b, g, ref, gref = _conv_case(cin, cout, 1, True, B=B, Ho=H, Wo=W)
    xr = x.clone().requires_grad_(True)
    before = Fn._FLAT_CONV_CALLS[0]
    y = Fn.mfma_conv(xr, w, b, 1)
    assert Fn._FLAT_CONV_CALLS[0] == before + 1
    assert y.shape == ref.shape and torch.equal(y.detach(), ref.float()), float((y.detach().double() - ref).abs().max())
    (gx,) = torch.autograd.grad(y, xr, g)
    assert gx.shape == x.shape and torch.equal(gx, gref.float()), float((gx.double() - gref).abs().max())
    Fn._WS_BYTES.clear()


def _flat_launch(inp, pack, bias, k_in, n_out, ref, want_splits):
    from hipops import lib as L
    from hipops.functions import _p
    lib = L.load()
    B, _, H, W = inp.shape
    n = B * H * W * n_out
    wsb = int(lib.dd_conv3x3_mfma_flat_workspace_bytes(B, H, W, k_in, n_out))
    assert wsb == (want_splits * n * 4 if want_splits > 1 else 16)
    buf, yp = _guarded(n)
    wbuf, wp = _guarded(wsb // 4)
    L.check(lib.dd_conv3x3_mfma_flat(_p(inp), _p(pack), _p(bias), B, H, W, k_in, n_out, yp, wp, wsb, L.current_stream()), "dd_conv3x3_mfma_flat")
    out = _check_guards(buf, n).view(B, H, W, n_out).permute(0, 3, 1, 2)
    assert torch.equal(out, ref.float())
    torch.cuda.synchronize()
    assert bool(torch.isnan(wbuf[:GUARD]).all()) and bool(torch.isnan(wbuf[GUARD + wsb // 4:]).all()), "a store outside the workspace"
    if want_splits > 1:
        assert bool(torch.isfinite(wbuf[GUARD:GUARD + wsb // 4]).all())


@pytest.mark.parametrize("splits", [1, 2])
@pytest.mark.parametrize("case", FLAT, ids=lambda c: "x".join(map(str, c)))
def test_flat_kernel_writes_nothing_outside_its_output_or_workspace(case, splits, monkeypatch):
    B, cin, cout, H, W = case
    monkeypatch.setenv("DD_FLAT_SPLITS", str(splits))
    x, w, b, g, ref, gref = _conv_case(cin, cout, 1, True, B=B, Ho=H, Wo=W)
    pf, pb = _packs(w)
    _flat_launch(x, pf, b, cin, cout, ref, splits)
    _flat_launch(g, pb, None, cout, cin, gref, splits)


# ---- conv_half_kernel --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("cout", [32, 40])
@pytest.mark.parametrize("pad", [0, 1])
@pytest.mark.parametrize("kind", ["fp16", "bf16"])
def test_half_kernel_is_exact_on_ragged_tiles(kind, pad, cout, bias):
    """x in [-2,2], w in [-1,1], cin = 32: |y| <= 9 * 32 * 2 = 576 (+ |b|), an integer that fp32 accumulates exactly; the kernel rounds it
    once, to nearest even, to the half type -- what the cast of the float64 reference does (fp16 holds every such integer; bf16 every
    one up to 256 and the nearest even-spaced one beyond)."""
    from hipops.functions import half_conv
    dtype = {"fp16": torch.float16, "bf16": torch.bfloat16}[kind]
    x, w, b, g, ref, gref = _conv_case(32, cout, pad, bias, xmax=2, wmax=1)
    xr = x.to(dtype).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    y = half_conv(xr, w, b, pad)
    assert y.dtype == dtype and y.shape == ref.shape
    assert torch.equal(y.detach(), ref.to(dtype)), float((y.detach().double() - ref).abs().max())
    (gx,) = torch.autograd.grad(y, xr, g.to(dtype).contiguous(memory_format=torch.channels_last))
    assert gx.shape == x.shape and torch.equal(gx, gref.to(dtype)), float((gx.double() - gref).abs().max())


# ---- pw_gemm_kernel / mlp_fwd_kernel -----------------------------------------------------------------------------------------------
def _err(a, ref):
    return float((a.double() - ref).abs().max() / ref.abs().max())


@functools.lru_cache(maxsize=None)
def _mlp_case(C):
    """a block's parameters and 257 rows; the float64 and the torch fp32 pre-activation and output.  Row counts 1 and 33 are the leading
    rows of the same tensors (every output row depends on its own input row only)."""
    gen = torch.Generator().manual_seed(C)
    y = (torch.randn(257, C, generator=gen) * 1.5).cuda()
    w1 = (torch.randn(6 * C, C, generator=gen) / C ** 0.5).cuda()
    b1 = torch.randn(6 * C, generator=gen).cuda()
    w2 = (torch.randn(C, 6 * C, generator=gen) / (6 * C) ** 0.5).cuda()
    b2 = torch.randn(C, generator=gen).cuda()
    pre64 = F.linear(y.double(), w1.double(), b1.double())
    out64 = F.linear(F.gelu(pre64), w2.double(), b2.double())
    pre32 = F.linear(y, w1, b1)
    out32 = F.linear(F.gelu(pre32), w2, b2)
    return y, w1, b1, w2, b2, pre64, out64, pre32, out32


def _gemm_guarded(x, w, b, gelu):
    """y = act(x) . w^T + b through dd_mlp_pack + dd_pw_gemm (as tests/test_pw_gemm_gpu.py's _gemm), into a guarded buffer"""
    from hipops import lib as L
    lib = L.load()
    M, K = x.shape
    N = w.shape[0]
    pack = torch.empty(int(lib.dd_pw_gemm_pack_bytes(N, K)) // 4, dtype=torch.float32, device="cuda")
    st = L.current_stream()
    dummy = torch.zeros(K, N, device="cuda")
    L.check(lib.dd_mlp_pack(w.data_ptr(), w.stride(0), w.stride(1), dummy.data_ptr(), dummy.stride(0), dummy.stride(1), K, N, pack.data_ptr(), None, None,
                            None, None, st), "dd_mlp_pack")
    buf, yp = _guarded(M * N)
    L.check(lib.dd_pw_gemm(x.data_ptr(), pack.data_ptr(), None if b is None else b.data_ptr(), M, K, N, int(gelu), yp, st), "dd_pw_gemm")
    return _check_guards(buf, M * N).view(M, N)


@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("M", [1, 33, 257])
def test_pw_gemm_on_ragged_row_counts(M, C):
    """both Linears of a block (narrow -> wide, and wide -> narrow behind the GELU prologue), tests/test_pw_gemm_gpu.py's rule: own error
    against float64 <= 2 x torch's fp32 error on the same inputs (floor 2e-6, as there)"""
    y, w1, b1, w2, b2, pre64, out64, pre32, out32 = _mlp_case(C)
    pre = _gemm_guarded(y[:M].contiguous(), w1, b1, False)
    e_own, e_lib = _err(pre, pre64[:M]), _err(pre32[:M], pre64[:M])
    print("pw_gemm  first  M %-4d C %-4d own %.2e  torch fp32 %.2e" % (M, C, e_own, e_lib))
    assert e_own <= max(2.0 * e_lib, 2e-6), (e_own, e_lib)
    ref2 = F.linear(F.gelu(pre32[:M].double()), w2.double(), b2.double())          # the second Linear on the SAME fp32 pre-activation
    lib2 = F.linear(F.gelu(pre32[:M]), w2, b2)
    out = _gemm_guarded(pre32[:M].contiguous(), w2, b2, True)
    e_own, e_lib = _err(out, ref2), _err(lib2, ref2)
    print("pw_gemm  second M %-4d C %-4d own %.2e  torch fp32 %.2e" % (M, C, e_own, e_lib))
    assert e_own <= max(2.0 * e_lib, 2e-6), (e_own, e_lib)


@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("M", [1, 33, 257])
def test_mlp_fwd_on_ragged_row_counts(M, C):
    """dd_mlp_fwd through the C ABI into a guarded buffer (one partial 128-row workgroup; two full ones and one row), same rule"""
    from hipops import lib as L
    lib = L.load()
    y, w1, b1, w2, b2, pre64, out64, pre32, out32 = _mlp_case(C)
    hid = 6 * C
    nb1, nb2 = int(lib.dd_pw_gemm_pack_bytes(hid, C)), int(lib.dd_pw_gemm_pack_bytes(C, hid))
    packs = torch.empty((nb1 + nb2) // 4, dtype=torch.float32, device="cuda")
    p0, st = packs.data_ptr(), L.current_stream()
    L.check(lib.dd_mlp_pack(w1.data_ptr(), w1.stride(0), w1.stride(1), w2.data_ptr(), w2.stride(0), w2.stride(1), C, hid, p0, None, None, None, p0 + nb1, st),
            "dd_mlp_pack")
    x = y[:M].contiguous()
    buf, yp = _guarded(M * C)
    L.check(lib.dd_mlp_fwd(x.data_ptr(), p0, p0 + nb1, b1.data_ptr(), b2.data_ptr(), M, C, yp, st), "dd_mlp_fwd")
    out = _check_guards(buf, M * C).view(M, C)
    e_own, e_lib = _err(out, out64[:M]), _err(out32[:M], out64[:M])
    print("mlp_fwd M %-4d C %-4d own %.2e  torch fp32 %.2e" % (M, C, e_own, e_lib))
    assert e_own <= max(2.0 * e_lib, 2e-6), (e_own, e_lib)
