"""dd_mlp_fwd_n at C = 224 (csrc/dd_pw_gemm.hip: mlp_fwd224_kernel + mlp_fold224_kernel): LiteMono's stage-3 block (reference
networks/depth_encoder.py:200-203,216-224,262-272; hidden width 1344 = 42 blocks of 32) in one kernel, the hidden range split over S
workgroups per 128-row group and the partials folded in split order.  Judged as tests/test_pw_gemm_gpu.py judges: the own error against
float64 beside torch's fp32 error on the same inputs.  Shapes: the smallest at which the kernel can go wrong -- one row, one short of and
one past a wave's 32 rows, one past a workgroup's 128, several workgroups with a ragged last one; S = 1 (no fold), 2, 5 (uneven ranges:
8 or 9 hidden blocks) and 42 (one hidden block per workgroup: the loop's prologue and tail alone)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

C, HID, GUARD = 224, 1344, 64          # guard bands of 64 floats keep the 16-byte alignment the entry point asks for
ROWS = [1, 31, 33, 129, 1000]
SPLITS = [1, 2, 5, 42]
_CACHE = {}


def _err(a, ref):
    return float((a.double() - ref).abs().max() / ref.abs().max())


def _inputs(M):
    """x, the block's parameters (b1 scaled by 3: a hidden unit that meets the wrong W2 column shows), the float64 result
    and torch's fp32 result -- computed once per row count and left unchanged"""
    if M not in _CACHE:
        g = torch.Generator().manual_seed(1000 + M)
        x = (torch.randn(M, C, generator=g) * 1.5).cuda()
        w1 = (torch.randn(HID, C, generator=g) / C ** 0.5).cuda()
        b1 = (torch.randn(HID, generator=g) * 3.0 / C ** 0.5).cuda()
        w2 = (torch.randn(C, HID, generator=g) / HID ** 0.5).cuda()
        b2 = torch.randn(C, generator=g).cuda()
        ref = F.gelu(x.double() @ w1.double().t() + b1.double()) @ w2.double().t() + b2.double()
        lib = F.gelu(x @ w1.t() + b1) @ w2.t() + b2
        _CACHE[M] = (x, w1, b1, w2, b2, ref, lib)
    return _CACHE[M]


def _guarded(n):
    """n floats between two NaN-filled guard bands, NaN-filled themselves: (whole buffer, view of the n floats)"""
    buf = torch.full((n + 2 * GUARD,), float("nan"), device="cuda")
    return buf, buf[GUARD:GUARD + n]


def _intact(buf, n):
    return bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + n:]).all())


def _run(M, S, products=6):
    """dd_mlp_pack + dd_mlp_fwd_n through the C ABI into guarded buffers; checks the guards and that every element inside was written"""
    from hipops import lib as L
    lib = L.load()
    x, w1, b1, w2, b2 = _inputs(M)[:5]
    nb1, nb2 = int(lib.dd_pw_gemm_pack_bytes(HID, C)), int(lib.dd_pw_gemm_pack_bytes(C, HID))
    packs = torch.empty((nb1 + nb2) // 4, device="cuda")
    p0, st = packs.data_ptr(), L.current_stream()
    L.check(lib.dd_mlp_pack(w1.data_ptr(), w1.stride(0), w1.stride(1), w2.data_ptr(), w2.stride(0), w2.stride(1), C, HID, p0, None, None, None, p0 + nb1, st),
            "dd_mlp_pack")
    nbytes = int(lib.dd_mlp_fwd_workspace_bytes(M, C, S))
    assert nbytes == (S * M * C * 4 if S > 1 else 0)
    ybuf, y = _guarded(M * C)
    wbuf, ws = _guarded(nbytes // 4)
    L.check(lib.dd_mlp_fwd_n(x.data_ptr(), p0, p0 + nb1, b1.data_ptr(), b2.data_ptr(), M, C, products, S, y.data_ptr(), ws.data_ptr(), nbytes, st), "dd_mlp_fwd_n")
    torch.cuda.synchronize()
    assert _intact(ybuf, M * C) and _intact(wbuf, nbytes // 4), "a guard band was written"
    assert not bool(torch.isnan(y).any()), "an output element was not written"
    assert not bool(torch.isnan(ws).any()), "a workspace element was not written"
    return y.view(M, C).clone()


@pytest.mark.parametrize("S", SPLITS)
@pytest.mark.parametrize("M", ROWS)
def test_forward_matches_float64_inside_its_bounds(M, S):
    ref, lib32 = _inputs(M)[5:]
    own = _run(M, S)
    e_own, e_lib = _err(own, ref), _err(lib32, ref)
    print("mlp_fwd224 M %-5d S %-2d own %.2e  torch fp32 %.2e" % (M, S, e_own, e_lib))
    assert e_own <= max(2.0 * e_lib, 2e-6), (e_own, e_lib)


@pytest.mark.parametrize("S", [1, 5])
def test_two_runs_are_bit_identical(S):
    assert torch.equal(_run(129, S), _run(129, S))


def test_split_count_chosen_from_the_rows_is_one_round_of_the_chip():
    from hipops import lib as L
    lib = L.load()
    for M in (1, 128, 129, 1920, 5760, 11520, 40000):
        S = int(lib.dd_mlp_fwd_splits(M, C))
        groups = (M + 127) // 128
        assert 1 <= S <= 42 and (groups * S <= 256 or S == 1), (M, S)
    assert int(lib.dd_mlp_fwd_splits(11520, C)) == 2 and int(lib.dd_mlp_fwd_splits(5760, C)) == 5
    assert int(lib.dd_mlp_fwd_splits(11520, 64)) == 1
    # the entry point refuses what it cannot run: more splits than hidden blocks, a workspace that is too small, an unknown product count
    x, w1, b1, w2, b2 = _inputs(33)[:5]
    y = torch.empty(33, C, device="cuda")
    ws = torch.empty(33 * C * 2, device="cuda")
    args = (x.data_ptr(), ws.data_ptr(), ws.data_ptr(), b1.data_ptr(), b2.data_ptr(), 33, C)
    assert lib.dd_mlp_fwd_n(*args, 6, 43, y.data_ptr(), ws.data_ptr(), ws.numel() * 4, None) != 0
    assert lib.dd_mlp_fwd_n(*args, 6, 3, y.data_ptr(), ws.data_ptr(), ws.numel() * 4, None) != 0
    assert lib.dd_mlp_fwd_n(*args, 2, 2, y.data_ptr(), ws.data_ptr(), ws.numel() * 4, None) != 0


def _tf32(t):
    """round to TF32's ten explicit significand bits (half away from zero, as the matrix units' conversion)"""
    return ((t.contiguous().view(torch.int32) + 0x1000) & ~0x1FFF).view(torch.float32)


@pytest.mark.parametrize("products", [3, 1])
def test_fewer_partial_products_are_what_their_names_say(products):
    """3 (bf16x3): within 3e-5 of max|result| of float64 and at least eight times closer to it than the same block on TF32-rounded operands
    (tests/test_linear_wgrad_gpu.py's rule).  1: the float64 block of the bf16-ROUNDED operands to fp32 accumulation error (2e-6 of
    max|result|) -- plus, because the second GEMM's operand is rounded to bf16 AFTER an fp32 computation, one bf16 ulp of one hidden value
    per output: a pre-activation that differs from float64's in its last fp32 place can round the other way (2^-8 max|h| max|w2|)."""
    M, S = 200, 2
    x, w1, b1, w2, b2, ref, _ = _inputs(M)
    own = _run(M, S, products)
    if products == 3:
        h = F.gelu(_tf32(x).double() @ _tf32(w1).double().t() + b1.double())
        tf = _tf32(h.float()).double() @ _tf32(w2).double().t() + b2.double()
        e_own, e_tf = _err(own, ref), _err(tf, ref)
        print("mlp_fwd224 bf16x3 %.2e  TF32 operands %.2e" % (e_own, e_tf))
        assert e_own < 3e-5 and e_own * 8 < e_tf, (e_own, e_tf)
    else:
        h = F.gelu(x.bfloat16().double() @ w1.bfloat16().double().t() + b1.double())
        r1 = h.float().bfloat16().double() @ w2.bfloat16().double().t() + b2.double()
        e = float((own.double() - r1).abs().max())
        bound = 2e-6 * float(r1.abs().max()) + 2.0 ** -8 * float(h.abs().max()) * float(w2.abs().max())
        print("mlp_fwd224 bf16 operands: against their float64 block %.2e (bound %.2e)" % (e, bound))
        assert e <= bound, (e, bound)


class _Block(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.pwconv1 = torch.nn.Linear(C, HID)
        self.act = torch.nn.GELU()
        self.pwconv2 = torch.nn.Linear(HID, C)

    def forward(self, y):
        return self.pwconv2(self.act(self.pwconv1(y)))


def test_the_module_path_takes_it_and_counts_it(monkeypatch):
    """mlp_fused_ok / mlp_fused (what networks/depth_encoder.py:_mlp_residual calls without a tape) at (1, 5, 7, 224): the row gate is
    per width, DD_MLP_FUSED_MIN_ROWS overrides it, the stock switch and the tape turn the path off"""
    from hipops.functions import mlp_fused, mlp_fused_calls, mlp_fused_ok
    torch.manual_seed(7)
    blk = _Block().cuda()
    with torch.no_grad():
        blk.pwconv1.bias.mul_(3.0)
        y = torch.randn(1, 5, 7, C, device="cuda") * 1.5
        big = torch.empty(24, 12, 40, C, device="cuda")
        assert mlp_fused_ok(big, blk) and not mlp_fused_ok(y, blk)          # the side batch's rows pass the default gate, 35 rows do not
        monkeypatch.setenv("DD_MLP_FUSED_MIN_ROWS", "1")
        assert mlp_fused_ok(y, blk)
        before = mlp_fused_calls()
        own, lib = mlp_fused(y, blk), blk(y)
        assert mlp_fused_calls() == before + 1
        ref = blk.double()(y.double())
        blk.float()
        monkeypatch.setenv("DD_STOCK_MLP_FUSED", "1")
        assert not mlp_fused_ok(y, blk)
        monkeypatch.delenv("DD_STOCK_MLP_FUSED")
    e_own, e_lib = _err(own, ref), _err(lib, ref)
    assert own.shape == ref.shape and e_own <= max(2.0 * e_lib, 2e-6), (e_own, e_lib)
    assert not mlp_fused_ok(y, blk)            # with the tape on it is not this path


def test_litemono_step_runs_stage3_of_the_side_batch_fused(monkeypatch):
    """One LiteMono step at batch 2 (192x640) with the row gate lowered: the statistics-only side batch runs all of its 4 + 4 + 10 blocks
    through dd_mlp_fwd (8 before stage 3 was covered), and losses and gradient norms meet the stock-switch run inside the tolerances of
    test_trainer_gpu.hooks_against_stock (2e-3 and 2e-2), which does the comparison"""
    from hipops import functions as HF
    from test_trainer_gpu import hooks_against_stock
    monkeypatch.setenv("DD_MLP_FUSED_MIN_ROWS", "256")
    before = HF.mlp_fused_calls()
    hooks_against_stock([], 2)
    assert HF.mlp_fused_calls() - before == 18
