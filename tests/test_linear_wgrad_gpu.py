"""dd_linear_wgrad (csrc/dd_linear_wgrad.hip) against float64: the weight and bias gradient of LiteMono's point-wise Linears (reference
networks/depth_encoder.py:200-203, :58-60) from one pass over g (M, cout) and x (M, cin) on the bf16 matrix pipe, three bf16 pieces per fp32
operand, per-workgroup partials folded in a fixed order.  The yardstick is torch's own fp32 result on the same inputs, the rule that of
tests/test_pw_gemm_gpu.py: e_own <= max(2 e_lib, 2e-6), both against float64 and relative to max|result|."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

# (M, cout, cin): one row; fewer rows than a 16-row group; one row more than two groups; ragged rows with 224 = 7 x 32 on either side
# (a block with an empty half); channel counts that are no multiple of 32; many co blocks against a quarter-filled ci block
CASES = [(1, 32, 32), (31, 64, 32), (33, 32, 96), (4097, 96, 224), (5760, 224, 96), (1000, 40, 36), (257, 300, 8)]
_IDS = ["x".join(map(str, c)) for c in CASES]


def _err(a, ref):
    return float((a.double() - ref).abs().max() / ref.abs().max())


def _inputs(case):
    M, cout, cin = case
    gen = torch.Generator().manual_seed(sum(case))
    return (torch.randn(M, cout, generator=gen) * 1.5).cuda(), torch.randn(M, cin, generator=gen).cuda()


_REF = {}


def _ref64(case):
    """float64 g^T x and column sums of the case's inputs, computed once and shared (never written to)"""
    if case not in _REF:
        g, x = _inputs(case)
        _REF[case] = (g.double().t() @ x.double(), g.double().sum(0))
    return _REF[case]


def _wgrad(g, x, products=6, bias=True, out=None):
    """raw C ABI -> (gw, gb); `out` = (gw, gb, ws) to write into"""
    from hipops import lib as L
    lib = L.load()
    M, cout = g.shape
    cin = x.shape[1]
    assert lib.dd_linear_wgrad_supported(M, cout, cin)
    nbytes = int(lib.dd_linear_wgrad_workspace_bytes(M, cout, cin))
    if out is None:
        out = (torch.empty(cout, cin, device="cuda"), torch.empty(cout, device="cuda") if bias else None, torch.empty(max(nbytes // 4, 1), device="cuda"))
    gw, gb, ws = out
    assert ws.numel() * 4 >= nbytes
    L.check(lib.dd_linear_wgrad_n(g.data_ptr(), x.data_ptr(), M, cout, cin, products, gw.data_ptr(), None if gb is None else gb.data_ptr(), ws.data_ptr(), nbytes,
                                  L.current_stream()), "dd_linear_wgrad_n")
    return gw, gb


def _check(case, gw, gb, g, x, what=""):
    ref_w, ref_b = _ref64(case)
    for name, own, lib32, ref in (("g_weight", gw, g.t() @ x, ref_w), ("g_bias", gb, g.sum(0), ref_b)):
        e_own, e_lib = _err(own, ref), _err(lib32, ref)
        print("%s %-16s %-9s own %.2e  torch fp32 %.2e" % (what, case, name, e_own, e_lib))
        assert e_own <= max(2.0 * e_lib, 2e-6), (name, e_own, e_lib)


@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_matches_float64_beside_the_library(case):
    g, x = _inputs(case)
    gw, gb = _wgrad(g, x)
    _check(case, gw, gb, g, x)
    gw2, none = _wgrad(g, x, bias=False)          # g_bias may be NULL: the same weights
    assert none is None and torch.equal(gw, gw2)


@pytest.mark.parametrize("splits", ["1", "1000"])
def test_split_count_forced(splits, monkeypatch):
    """One workgroup per block over all rows; more row ranges than 16-row groups (most of them empty: their partials are zeros)."""
    case = (4097, 96, 224)                         # 257 groups
    monkeypatch.setenv("DD_LINEAR_WGRAD_SPLITS", splits)
    g, x = _inputs(case)
    gw, gb = _wgrad(g, x)
    _check(case, gw, gb, g, x, "splits " + splits)


def _tf32(t):
    """Operands as TF32 holds them (10 explicit significand bits, round to nearest even)"""
    bits = t.contiguous().view(torch.int32)
    bits = (bits + 0x0FFF + ((bits >> 13) & 1)) & ~0x1FFF
    return bits.view(torch.float32)


@pytest.mark.parametrize("products", [3, 1])
@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_fewer_partial_products_are_what_their_names_say(case, products):
    """3 (bf16x3): within 3e-5 of max|result| of float64 and at least eight times closer to it than the same product of TF32-rounded
    operands; 1: the float64 product of the bf16-ROUNDED operands to fp32 accumulation error.  The bias sums the raw fp32 values with
    either: held to the fp32 rule."""
    g, x = _inputs(case)
    gw, gb = _wgrad(g, x, products)
    ref_w, ref_b = _ref64(case)
    if products == 3:
        e_own, e_tf = _err(gw, ref_w), _err(_tf32(g).double().t() @ _tf32(x).double(), ref_w)
        print("%-16s bf16x3 %.2e  TF32 operands %.2e" % (case, e_own, e_tf))
        assert e_own < 3e-5 and e_own * 8 < e_tf, (e_own, e_tf)
    else:
        e = _err(gw, g.bfloat16().double().t() @ x.bfloat16().double())
        print("%-16s bf16 operands: against their float64 product %.2e" % (case, e))
        assert e < 2e-6, e
    e_own, e_lib = _err(gb, ref_b), _err(g.sum(0), ref_b)
    assert e_own <= max(2.0 * e_lib, 2e-6), (e_own, e_lib)


@pytest.mark.parametrize("case", [(2048, 96, 224), (777, 40, 36), (1, 32, 32)], ids=lambda c: "x".join(map(str, c)))
def test_exact_on_small_integers(case):
    """Integers in [-8, 8]: every product and every partial sum (|sum| <= 2048 * 64 = 2^17) is exact in fp32, whatever the order."""
    M, cout, cin = case
    gen = torch.Generator().manual_seed(M)
    g = torch.randint(-8, 9, (M, cout), generator=gen).float().cuda()
    x = torch.randint(-8, 9, (M, cin), generator=gen).float().cuda()
    gw, gb = _wgrad(g, x)
    assert torch.equal(gw.double(), g.double().t() @ x.double())
    assert torch.equal(gb.double(), g.double().sum(0))


def test_every_piece_counts():
    """Operands whose bf16 head is 1 and whose signal sits beyond it, against a power of two: v = 1 + 2^-9 splits (dd_split.h) into
    1, 2^-9, 0 -- the second piece carries the signal --, v = 1 + 2^-9 + 2^-18 into 1, 2^-9, 2^-18: the residual after the head needs more
    than bf16's eight significand bits, so the THIRD piece carries 2^-18.  With M = 64 rows of v against 1 / 64 every product and every
    partial sum is exact in fp32 (19 significant bits at most, sums of equal terms), so the result is v bit for bit only if that piece took
    part: on the g side (a3 b1) and on the x side (a1 b3).  64 channels on both sides: all four accumulators of a wave."""
    M = 64
    for v in (1.0 + 2.0 ** -9, 1.0 + 2.0 ** -9 + 2.0 ** -18):
        # what the test relies on: the split of v as stated (bfloat16 casts round to nearest even, as split2 does)
        t = torch.tensor(v)
        p1 = t.bfloat16().float()
        p2 = (t - p1).bfloat16().float()
        p3 = t - p1 - p2
        assert float(p1) == 1.0 and float(p2) == 2.0 ** -9 and float(p3) == (2.0 ** -18 if v > 1.0 + 2.0 ** -9 else 0.0)
        for on_g in (True, False):
            g = torch.full((M, 64), v if on_g else 1.0).cuda()
            x = torch.full((M, 64), (1.0 if on_g else v) / M).cuda()
            gw, _ = _wgrad(g, x)
            assert float((gw.double() - v).abs().max()) == 0.0, (v, on_g)


def test_bit_reproducible():
    case = (5760, 224, 96)
    g, x = _inputs(case)
    gw, gb = _wgrad(g, x)
    gw2, gb2 = _wgrad(g, x)
    assert torch.equal(gw, gw2) and torch.equal(gb, gb2)


@pytest.mark.parametrize("case", [(1000, 40, 36), (4097, 96, 224), (31, 64, 32)], ids=lambda c: "x".join(map(str, c)))
def test_no_zero_fill_needed_and_nothing_outside_touched(case):
    """Outputs and workspace start as NaN between NaN guard bands: the fold writes every element of both results from partials the
    kernel wrote, and not one float beside the three arrays changes."""
    from hipops import lib as L
    M, cout, cin = case
    g, x = _inputs(case)
    band = 64
    n_ws = int(L.load().dd_linear_wgrad_workspace_bytes(M, cout, cin)) // 4
    sizes = (cout * cin, cout, n_ws)
    buf = torch.full((sum(sizes) + 4 * band,), float("nan"), device="cuda")
    parts, guards, pos = [], [], 0
    for n in sizes:
        guards.append((pos, pos + band))
        parts.append(buf[pos + band:pos + band + n])
        pos += band + n
    guards.append((pos, pos + band))
    gw, gb = _wgrad(g, x, out=(parts[0].view(cout, cin), parts[1], parts[2]))
    torch.cuda.synchronize()
    assert not torch.isnan(gw).any() and not torch.isnan(gb).any()
    for a, b in guards:
        assert torch.isnan(buf[a:b]).all(), (a, b)
    _check(case, gw, gb, g, x, "nan-filled")


@pytest.mark.parametrize("shape,cout", [((2, 3, 5, 32), 96), ((1, 12, 40, 224), 672)])
def test_autograd_both_paths(shape, cout, monkeypatch):
    """pointwise_linear's weight and bias gradient with dd_linear_wgrad and with DD_STOCK_LINEAR_WGRAD=1 (the library's 1x1 weight
    gradient + the column sum), each held to the fp32 rule; the counter tells which one ran."""
    import torch.nn as nn
    from hipops.functions import linear_wgrad_calls, pointwise_linear
    gen = torch.Generator().manual_seed(cout)
    layer = nn.Linear(shape[-1], cout).cuda()
    x = torch.randn(*shape, generator=gen).cuda()
    g = torch.randn(*shape[:-1], cout, generator=gen).cuda()
    g2, x2 = g.reshape(-1, cout), x.reshape(-1, shape[-1])
    ref_w, ref_b = g2.double().t() @ x2.double(), g2.double().sum(0)
    e_lib_w, e_lib_b = _err(g2.t() @ x2, ref_w), _err(g2.sum(0), ref_b)
    for stock in (False, True):
        if stock:
            monkeypatch.setenv("DD_STOCK_LINEAR_WGRAD", "1")
        n0 = linear_wgrad_calls()
        y = pointwise_linear(x.clone().requires_grad_(), layer)
        assert y.grad_fn.name().startswith("PointwiseLinearFn")
        gw, gb = torch.autograd.grad(y, (layer.weight, layer.bias), g)
        assert linear_wgrad_calls() == n0 + (0 if stock else 1)
        e_w, e_b = _err(gw, ref_w), _err(gb, ref_b)
        print("stock" if stock else "own  ", shape, cout, "g_weight %.2e (torch fp32 %.2e)  g_bias %.2e (%.2e)" % (e_w, e_lib_w, e_b, e_lib_b))
        assert e_w <= max(2.0 * e_lib_w, 2e-6) and e_b <= max(2.0 * e_lib_b, 2e-6), (stock, e_w, e_lib_w, e_b, e_lib_b)


def test_autocast_keeps_the_library_path():
    import torch.nn as nn
    from hipops.functions import linear_wgrad_calls, pointwise_linear
    layer = nn.Linear(64, 96).cuda()
    x = torch.randn(2, 6, 10, 64, device="cuda", requires_grad=True)
    n0 = linear_wgrad_calls()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = pointwise_linear(x, layer)
    assert y.dtype == torch.bfloat16
    y.float().sum().backward()
    assert layer.weight.grad is not None and layer.weight.grad.dtype == torch.float32
    assert linear_wgrad_calls() == n0


def test_litemono_training_step_uses_it():
    """One LiteMono training step at the size of test_trainer_gpu's hooks-against-stock tests (192 x 640, batch 2)."""
    import numpy as np
    from torch.utils.data import DataLoader
    from Trainer import Trainer
    from hipops.functions import linear_wgrad_calls
    from test_networks import make_opt
    torch.manual_seed(5)
    opt = make_opt("litemono", ["--synthetic", "--channels_last"])
    opt.batch_size = 2
    tr = Trainer(opt)
    tr.num_steps_per_epoch = 100
    tr.setup_phase("fine_tune")
    tr.bool_automask = False
    tr.step = 50
    tr.set_train()
    batch = next(iter(DataLoader(tr.get_dataset(["s 0", "s 1"]), batch_size=2)))
    rs = np.random.RandomState(1)
    tr.rand_idx_override = {s: rs.randint(0, int(0.4 * (opt.height >> s)) * (opt.width >> s), (2, 500)).astype(np.int64) for s in opt.scales}
    n0 = linear_wgrad_calls()
    _, losses = tr.process_batch(batch)
    losses["loss"].backward()
    torch.cuda.synchronize()
    assert linear_wgrad_calls() > n0
    assert all(torch.isfinite(p.grad).all() for n in tr.base_model.module_names for p in getattr(tr.base_model, n).parameters() if p.grad is not None)
