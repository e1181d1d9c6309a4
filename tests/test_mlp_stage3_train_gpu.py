"""The training pass of LiteMono's stage-3 block at C = 224 (csrc/dd_pw_gemm.hip: mlp_fwd224_kernel as MLP_TRAIN and MLP_DGRAD; reference
networks/depth_encoder.py:200-203,216-224,262-272): dd_mlp_train_fwd stores h = GELU(pre) and d = GELU'(pre) beside the output, and
dd_mlp_train_bwd computes dx = ((g . w2) * d) . w1 in one kernel and stores gpre = (g . w2) * d.  Shapes, inputs and judging are those of
tests/test_mlp_stage3_gpu.py: one row, one short of and one past a wave's 32 rows, one past a workgroup's 128, several workgroups with a
ragged last one; S = 1, 2, 5 (uneven ranges), 42 (prologue and tail alone); every quantity against float64 beside torch's fp32 result."""
import math

import pytest
import torch
import torch.nn.functional as F

from test_mlp_stage3_gpu import C, HID, ROWS, SPLITS, _Block, _err, _guarded, _inputs, _intact, _run, _tf32

pytestmark = pytest.mark.gpu

_REFS, _RUNS = {}, {}


def _d_gelu(pre):
    """GELU'(pre) = cdf + pre * pdf in pre's own precision"""
    return 0.5 * (1.0 + torch.erf(pre * math.sqrt(0.5))) + pre * torch.exp(-0.5 * pre * pre) * (1.0 / math.sqrt(2.0 * math.pi))


def _refs(M):
    """g ~ N(0,1) and, for test_mlp_stage3_gpu._inputs(M), the float64 and torch-fp32 values of y, h, d, gpre, dx -- computed once"""
    if M not in _REFS:
        x, w1, b1, w2, b2, y64, y32 = _inputs(M)
        g = torch.randn(M, C, generator=torch.Generator().manual_seed(5000 + M)).cuda()
        pre64 = x.double() @ w1.double().t() + b1.double()
        d64 = _d_gelu(pre64)
        gpre64 = (g.double() @ w2.double()) * d64
        ref = {"y": y64, "h": F.gelu(pre64), "d": d64, "gpre": gpre64, "dx": gpre64 @ w1.double()}
        pre32 = x @ w1.t() + b1
        gpre32 = torch.ops.aten.gelu_backward(g @ w2, pre32)
        lib = {"y": y32, "h": F.gelu(pre32), "d": torch.ops.aten.gelu_backward(torch.ones_like(pre32), pre32), "gpre": gpre32, "dx": gpre32 @ w1}
        _REFS[M] = (g, ref, lib)
    return _REFS[M]


def _packs(lib, st, w1, w2):
    nb = int(lib.dd_pw_gemm_pack_bytes(HID, C))
    assert nb == int(lib.dd_pw_gemm_pack_bytes(C, HID))
    packs = torch.empty(nb, device="cuda")             # four operands of nb bytes each
    p0 = packs.data_ptr()
    from hipops import lib as L
    L.check(lib.dd_mlp_train_pack(w1.data_ptr(), w1.stride(0), w1.stride(1), w2.data_ptr(), w2.stride(0), w2.stride(1), C, HID, p0, p0 + nb, p0 + 2 * nb,
                                  p0 + 3 * nb, st), "dd_mlp_train_pack")
    return packs, [p0 + i * nb for i in range(4)]


def _train(M, S, products=6, d_in=None, fresh=False):
    """dd_mlp_train_pack + dd_mlp_train_fwd + dd_mlp_train_bwd through the C ABI, every output and both workspaces NaN-filled between NaN
    guard bands: the guards stay intact, every inner element is written.  The backward reads the forward's d, or d_in.  Cached per case."""
    key = (M, S, products, d_in is not None)
    if key in _RUNS and not fresh:
        return _RUNS[key]
    from hipops import lib as L
    lib = L.load()
    x, w1, b1, w2, b2 = _inputs(M)[:5]
    g = _refs(M)[0]
    st = L.current_stream()
    packs, (pf1, pf2, pb2, pb1) = _packs(lib, st, w1, w2)
    nf, nbw = int(lib.dd_mlp_fwd_workspace_bytes(M, C, S)), int(lib.dd_mlp_train_bwd_workspace_bytes(M, C, S))
    assert nf == nbw == (S * M * C * 4 if S > 1 else 0)
    bufs = {k: _guarded(n) for k, n in (("y", M * C), ("h", M * HID), ("d", M * HID), ("gpre", M * HID), ("dx", M * C), ("wf", nf // 4), ("wb", nbw // 4))}
    v = {k: b[1] for k, b in bufs.items()}
    L.check(lib.dd_mlp_train_fwd(x.data_ptr(), pf1, pf2, b1.data_ptr(), b2.data_ptr(), M, C, products, S, v["y"].data_ptr(), v["h"].data_ptr(),
                                 v["d"].data_ptr(), v["wf"].data_ptr(), nf, st), "dd_mlp_train_fwd")
    d = v["d"] if d_in is None else d_in.contiguous()
    L.check(lib.dd_mlp_train_bwd(g.data_ptr(), d.data_ptr(), pb2, pb1, M, C, products, S, v["dx"].data_ptr(), v["gpre"].data_ptr(), v["wb"].data_ptr(),
                                 nbw, st), "dd_mlp_train_bwd")
    torch.cuda.synchronize()
    for k, (buf, view) in bufs.items():
        assert _intact(buf, view.numel()), "a guard band of %s was written" % k
        assert not bool(torch.isnan(view).any()), "an element of %s was not written" % k
    out = {k: v[k].view(M, C if k in ("y", "dx") else HID).clone() for k in ("y", "h", "d", "gpre", "dx")}
    _RUNS[key] = out
    return out


@pytest.mark.parametrize("S", SPLITS)
@pytest.mark.parametrize("M", ROWS)
def test_every_quantity_matches_float64_inside_its_bounds(M, S):
    _, ref, lib32 = _refs(M)
    own = _train(M, S)
    bad = []
    for k in ("y", "h", "d", "gpre", "dx"):
        e_own, e_lib = _err(own[k], ref[k]), _err(lib32[k], ref[k])
        print("mlp train M %-5d S %-2d %-4s own %.2e  torch fp32 %.2e" % (M, S, k, e_own, e_lib))
        if not e_own <= max(2.0 * e_lib, 2e-6):
            bad.append((k, e_own, e_lib))
    assert not bad, bad


@pytest.mark.parametrize("S", SPLITS)
@pytest.mark.parametrize("M", [33, 129])
def test_saving_does_not_change_the_output(M, S):
    """the training forward's y is dd_mlp_fwd_n's at the same split count, bit for bit"""
    assert torch.equal(_train(M, S)["y"], _run(M, S))


@pytest.mark.parametrize("S", [1, 5])
def test_two_runs_are_bit_identical(S):
    a, b = _train(129, S, fresh=True), _train(129, S, fresh=True)
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("products", [3, 1])
def test_fewer_partial_products_are_what_their_names_say(products):
    """test_mlp_stage3_gpu's two rules applied to dx at M = 200, S = 2, the backward reading the float64 d rounded to fp32 (so that the
    forward's own product count plays no part).  3: within 3e-5 of max|dx| of float64 and at least eight times closer to it than the same
    data gradient on TF32-rounded operands.  1: the float64 data gradient of the bf16-ROUNDED operands to fp32 accumulation error (2e-6 of
    max|dx|) plus one bf16 ulp of one gpre value per output (2^-8 max|gpre| max|w1|): gpre is rounded to bf16 AFTER an fp32 computation."""
    M, S = 200, 2
    x, w1, b1, w2, b2 = _inputs(M)[:5]
    g, ref64, _ = _refs(M)
    d32 = ref64["d"].float()
    own = _train(M, S, products, d_in=d32)
    assert torch.equal(own["y"], _run(M, S, products))
    ref = ((g.double() @ w2.double()) * d32.double()) @ w1.double()
    if products == 3:
        gp = (_tf32(g).double() @ _tf32(w2).double()) * d32.double()
        tf = _tf32(gp.float()).double() @ _tf32(w1).double()
        e_own, e_tf = _err(own["dx"], ref), _err(tf, ref)
        print("mlp dgrad bf16x3 %.2e  TF32 operands %.2e" % (e_own, e_tf))
        assert e_own < 3e-5 and e_own * 8 < e_tf, (e_own, e_tf)
    else:
        gp = (g.bfloat16().double() @ w2.bfloat16().double()) * d32.double()
        r1 = gp.float().bfloat16().double() @ w1.bfloat16().double()
        e = float((own["dx"].double() - r1).abs().max())
        bound = 2e-6 * float(r1.abs().max()) + 2.0 ** -8 * float(gp.abs().max()) * float(w1.abs().max())
        print("mlp dgrad bf16 operands: against their float64 data gradient %.2e (bound %.2e)" % (e, bound))
        assert e <= bound, (e, bound)


def test_the_entry_points_refuse_what_they_cannot_run():
    from hipops import lib as L
    lib = L.load()
    M = 33
    x, w1, b1, w2, b2 = _inputs(M)[:5]
    g = _refs(M)[0]
    st = L.current_stream()
    packs, (pf1, pf2, pb2, pb1) = _packs(lib, st, w1, w2)
    y, dx = torch.empty(M, C, device="cuda"), torch.empty(M, C, device="cuda")
    h, d, gpre = (torch.zeros(M, HID, device="cuda") for _ in range(3))
    ws = torch.empty(2 * M * C, device="cuda")
    full = ws.numel() * 4

    def fwd(Cc, products, S, nbytes):
        return lib.dd_mlp_train_fwd(x.data_ptr(), pf1, pf2, b1.data_ptr(), b2.data_ptr(), M, Cc, products, S, y.data_ptr(), h.data_ptr(), d.data_ptr(),
                                    ws.data_ptr(), nbytes, st)

    def bwd(Cc, products, S, nbytes):
        return lib.dd_mlp_train_bwd(g.data_ptr(), d.data_ptr(), pb2, pb1, M, Cc, products, S, dx.data_ptr(), gpre.data_ptr(), ws.data_ptr(), nbytes, st)

    for f in (fwd, bwd):
        assert f(C, 6, 2, full) == 0
        assert f(C, 6, 43, full) != 0            # more splits than hidden blocks
        assert f(C, 6, 2, full - 4) != 0         # a short workspace
        assert f(C, 2, 2, full) != 0             # an unknown product count
        assert f(128, 6, 2, full) != 0           # another width
    assert int(lib.dd_mlp_train_bwd_workspace_bytes(M, 128, 2)) == 0
    assert lib.dd_mlp_train_pack(w1.data_ptr(), w1.stride(0), w1.stride(1), w2.data_ptr(), w2.stride(0), w2.stride(1), 128, 768, pf1, pf2, pb2, pb1, st) != 0
    torch.cuda.synchronize()


def test_the_module_path_takes_it_and_counts_it(monkeypatch):
    """mlp_train_ok / mlp_train (what networks/depth_encoder.py:_mlp_residual calls with a tape) at (1, 5, 7, 224): output and all five
    gradients against float64 beside the stock module, the output gradient arriving NON-contiguous; the path counts itself and leaves the
    three counters bench.py reads alone; it is off without a tape, under autocast, under DD_STOCK_MLP=1 and below the default gate"""
    from hipops import functions as HF
    torch.manual_seed(7)
    blk = _Block().cuda()
    with torch.no_grad():
        blk.pwconv1.bias.mul_(3.0)
    y = (torch.randn(1, 5, 7, C, device="cuda") * 1.5).requires_grad_(True)
    gout = torch.randn(1, C, 5, 7, device="cuda")                  # the gradient reaches the block through a permute: not contiguous
    big = torch.empty(12, 12, 40, C, device="cuda")
    assert HF.mlp_train_ok(big, blk) and not HF.mlp_train_ok(y, blk)          # the workload's 5 760 rows pass the default gate, 35 do not
    monkeypatch.setenv("DD_MLP_TRAIN_MIN_ROWS", "1")
    assert HF.mlp_train_ok(y, blk)
    with torch.no_grad():
        assert not HF.mlp_train_ok(y, blk)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        assert not HF.mlp_train_ok(y, blk)
    monkeypatch.setenv("DD_STOCK_MLP", "1")
    assert not HF.mlp_train_ok(y, blk)
    monkeypatch.delenv("DD_STOCK_MLP")

    def grads(module, inp, run, g):
        module.zero_grad()
        inp.grad = None
        out = run(inp)
        (out.permute(0, 3, 1, 2) * g).sum().backward()
        return [out.detach()] + [t.grad.detach().clone() for t in (inp, module.pwconv1.weight, module.pwconv1.bias, module.pwconv2.weight, module.pwconv2.bias)]

    counters = (HF.mlp_calls(), HF.mlp_recompute_calls(), HF.mlp_fused_calls())
    before = HF.mlp_train_calls()
    own = grads(blk, y, lambda t: HF.mlp_train(t, blk), gout)
    assert HF.mlp_train_calls() == before + 1
    assert (HF.mlp_calls(), HF.mlp_recompute_calls(), HF.mlp_fused_calls()) == counters
    lib = grads(blk, y, blk, gout)
    blk.double()
    y64 = y.detach().double().requires_grad_(True)
    ref = grads(blk, y64, blk, gout.double())
    blk.float()
    bad = []
    for name, o, l, r in zip(("out", "dy", "dW1", "db1", "dW2", "db2"), own, lib, ref):
        e_own, e_lib = _err(o, r), _err(l, r)
        print("mlp train module %-3s own %.2e  torch fp32 %.2e" % (name, e_own, e_lib))
        if not (o.shape == r.shape and e_own <= max(2.0 * e_lib, 2e-6)):
            bad.append((name, e_own, e_lib))
    assert not bad, bad


def test_litemono_step_runs_the_stage3_training_blocks_through_it(monkeypatch):
    """One LiteMono step at batch 2 (192x640) with the row gate lowered: the ten stage-3 blocks of the training pass run through
    dd_mlp_train_fwd / dd_mlp_train_bwd in the hooked leg (the stock leg sets DD_STOCK_MLP=1), and losses and gradient norms meet the
    stock-switch run inside the tolerances of test_trainer_gpu.hooks_against_stock (2e-3 and 2e-2), which does the comparison"""
    from hipops import functions as HF
    from test_trainer_gpu import hooks_against_stock
    monkeypatch.setenv("DD_MLP_TRAIN_MIN_ROWS", "256")
    before = HF.mlp_train_calls()
    hooks_against_stock([], 2)
    assert HF.mlp_train_calls() - before == 10
