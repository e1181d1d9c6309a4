"""The training pass of LiteMono's stage-1 and stage-2 blocks at C = 64 / 128 (csrc/dd_pw_gemm.hip: mlp_fwd_kernel as MLP_TRAIN and MLP_DGRAD;
reference networks/depth_encoder.py:200-203,216-224,262-272): dd_mlp_train_fwd stores h = GELU(pre) and d = GELU'(pre) beside the output, and
dd_mlp_train_bwd computes dx = ((g . w2) * d) . w1 in one kernel and stores gpre = (g . w2) * d.  Judging is that of
tests/test_mlp_stage3_train_gpu.py: every quantity against float64 beside torch's fp32 result.  Rows: one, one short of and one past a wave's
32, one past a workgroup's 128, several workgroups with a ragged last one.  The hidden range is never split at these widths."""

import pytest
import torch
import torch.nn.functional as F

from test_mlp_stage3_gpu import _err, _guarded, _intact, _tf32
from test_mlp_stage3_train_gpu import _d_gelu

pytestmark = pytest.mark.gpu

WIDTHS = [64, 128]
ROWS = [1, 31, 33, 129, 1000]
_IN, _REFS, _RUNS = {}, {}, {}


def _inputs(C, M):
    """test_mlp_stage3_gpu._inputs at width C: x, the block's parameters (b1 scaled by 3: the pre-activation reaches the GELU's tails), the
    float64 result and torch's fp32 result -- computed once per shape and left unchanged"""
    if (C, M) not in _IN:
        HID = 6 * C
        g = torch.Generator().manual_seed(1000 * C + M)
        x = (torch.randn(M, C, generator=g) * 1.5).cuda()
        w1 = (torch.randn(HID, C, generator=g) / C ** 0.5).cuda()
        b1 = (torch.randn(HID, generator=g) * 3.0 / C ** 0.5).cuda()
        w2 = (torch.randn(C, HID, generator=g) / HID ** 0.5).cuda()
        b2 = torch.randn(C, generator=g).cuda()
        ref = F.gelu(x.double() @ w1.double().t() + b1.double()) @ w2.double().t() + b2.double()
        lib = F.gelu(x @ w1.t() + b1) @ w2.t() + b2
        _IN[(C, M)] = (x, w1, b1, w2, b2, ref, lib)
    return _IN[(C, M)]


def _refs(C, M):
    """g ~ N(0,1) and the float64 and torch-fp32 values of y, h, d, gpre, dx -- computed once"""
    if (C, M) not in _REFS:
        x, w1, b1, w2, b2, y64, y32 = _inputs(C, M)
        g = torch.randn(M, C, generator=torch.Generator().manual_seed(5000 * C + M)).cuda()
        pre64 = x.double() @ w1.double().t() + b1.double()
        d64 = _d_gelu(pre64)
        gpre64 = (g.double() @ w2.double()) * d64
        ref = {"y": y64, "h": F.gelu(pre64), "d": d64, "gpre": gpre64, "dx": gpre64 @ w1.double()}
        pre32 = x @ w1.t() + b1
        gpre32 = torch.ops.aten.gelu_backward(g @ w2, pre32)
        lib = {"y": y32, "h": F.gelu(pre32), "d": torch.ops.aten.gelu_backward(torch.ones_like(pre32), pre32), "gpre": gpre32, "dx": gpre32 @ w1}
        _REFS[(C, M)] = (g, ref, lib)
    return _REFS[(C, M)]


def _packs(lib, st, C, w1, w2):
    from hipops import lib as L
    nb = int(lib.dd_pw_gemm_pack_bytes(6 * C, C))
    assert nb == int(lib.dd_pw_gemm_pack_bytes(C, 6 * C))
    packs = torch.empty(nb, device="cuda")             # four operands of nb bytes each
    p0 = packs.data_ptr()
    L.check(lib.dd_mlp_train_pack_narrow(w1.data_ptr(), w1.stride(0), w1.stride(1), w2.data_ptr(), w2.stride(0), w2.stride(1), C, 6 * C, p0, p0 + nb,
                                         p0 + 2 * nb, p0 + 3 * nb, st), "dd_mlp_train_pack_narrow")
    return packs, [p0 + i * nb for i in range(4)]


def _train(C, M, S=0, products=6, d_in=None, fresh=False):
    """dd_mlp_train_pack_narrow + dd_mlp_train_fwd + dd_mlp_train_bwd through the C ABI, every output NaN-filled between NaN guard bands: the
    guards stay intact, every inner element is written.  The backward reads the forward's d, or d_in.  Cached per case."""
    key = (C, M, S, products, d_in is not None)
    if key in _RUNS and not fresh:
        return _RUNS[key]
    from hipops import lib as L
    lib = L.load()
    HID = 6 * C
    x, w1, b1, w2, b2 = _inputs(C, M)[:5]
    g = _refs(C, M)[0]
    st = L.current_stream()
    packs, (pf1, pf2, pb2, pb1) = _packs(lib, st, C, w1, w2)
    assert int(lib.dd_mlp_fwd_workspace_bytes(M, C, S)) == 0 and int(lib.dd_mlp_train_bwd_workspace_bytes(M, C, S)) == 0
    bufs = {k: _guarded(n) for k, n in (("y", M * C), ("h", M * HID), ("d", M * HID), ("gpre", M * HID), ("dx", M * C))}
    v = {k: b[1] for k, b in bufs.items()}
    L.check(lib.dd_mlp_train_fwd(x.data_ptr(), pf1, pf2, b1.data_ptr(), b2.data_ptr(), M, C, products, S, v["y"].data_ptr(), v["h"].data_ptr(),
                                 v["d"].data_ptr(), None, 0, st), "dd_mlp_train_fwd")
    d = v["d"] if d_in is None else d_in.contiguous()
    L.check(lib.dd_mlp_train_bwd(g.data_ptr(), d.data_ptr(), pb2, pb1, M, C, products, S, v["dx"].data_ptr(), v["gpre"].data_ptr(), None, 0, st),
            "dd_mlp_train_bwd")
    torch.cuda.synchronize()
    for k, (buf, view) in bufs.items():
        assert _intact(buf, view.numel()), "a guard band of %s was written" % k
        assert not bool(torch.isnan(view).any()), "an element of %s was not written" % k
    out = {k: v[k].view(M, C if k in ("y", "dx") else HID).clone() for k in ("y", "h", "d", "gpre", "dx")}
    _RUNS[key] = out
    return out


def _fwd(C, M):
    """dd_mlp_pack + dd_mlp_fwd: the no-grad kernel's output on the same inputs"""
    from hipops import lib as L
    lib = L.load()
    x, w1, b1, w2, b2 = _inputs(C, M)[:5]
    nb1, nb2 = int(lib.dd_pw_gemm_pack_bytes(6 * C, C)), int(lib.dd_pw_gemm_pack_bytes(C, 6 * C))
    packs = torch.empty((nb1 + nb2) // 4, device="cuda")
    p0, st = packs.data_ptr(), L.current_stream()
    L.check(lib.dd_mlp_pack(w1.data_ptr(), w1.stride(0), w1.stride(1), w2.data_ptr(), w2.stride(0), w2.stride(1), C, 6 * C, p0, None, None, None, p0 + nb1, st),
            "dd_mlp_pack")
    y = torch.empty(M, C, device="cuda")
    L.check(lib.dd_mlp_fwd(x.data_ptr(), p0, p0 + nb1, b1.data_ptr(), b2.data_ptr(), M, C, y.data_ptr(), st), "dd_mlp_fwd")
    torch.cuda.synchronize()
    return y


@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("C", WIDTHS)
def test_every_quantity_matches_float64_inside_its_bounds(C, M):
    _, ref, lib32 = _refs(C, M)
    own = _train(C, M, S=M % 2)                       # splits 0 and 1 are the same launch
    bad = []
    for k in ("y", "h", "d", "gpre", "dx"):
        e_own, e_lib = _err(own[k], ref[k]), _err(lib32[k], ref[k])
        print("mlp narrow train C %-3d M %-5d %-4s own %.2e  torch fp32 %.2e" % (C, M, k, e_own, e_lib))
        if not e_own <= max(2.0 * e_lib, 2e-6):
            bad.append((k, e_own, e_lib))
    assert not bad, bad


@pytest.mark.parametrize("M", [33, 129])
@pytest.mark.parametrize("C", WIDTHS)
def test_saving_does_not_change_the_output(C, M):
    """the training forward's y is dd_mlp_fwd's at six products, bit for bit"""
    assert torch.equal(_train(C, M)["y"], _fwd(C, M))


@pytest.mark.parametrize("C", WIDTHS)
def test_two_runs_are_bit_identical(C):
    a, b = _train(C, 129, fresh=True), _train(C, 129, fresh=True)
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("products", [3, 1])
@pytest.mark.parametrize("C", WIDTHS)
def test_fewer_partial_products_are_what_their_names_say(C, products):
    """test_mlp_stage3_train_gpu's two rules applied to dx at M = 200, the backward reading the float64 d rounded to fp32 (so that the
    forward's own product count plays no part).  3: within 3e-5 of max|dx| of float64 and at least eight times closer to it than the same
    data gradient on TF32-rounded operands.  1: the float64 data gradient of the bf16-ROUNDED operands to fp32 accumulation error (2e-6 of
    max|dx|) plus one bf16 ulp of one gpre value per output (2^-8 max|gpre| max|w1|): gpre is rounded to bf16 AFTER an fp32 computation."""
    M = 200
    x, w1, b1, w2, b2 = _inputs(C, M)[:5]
    g, ref64, _ = _refs(C, M)
    d32 = ref64["d"].float()
    own = _train(C, M, 0, products, d_in=d32)
    ref = ((g.double() @ w2.double()) * d32.double()) @ w1.double()
    if products == 3:
        gp = (_tf32(g).double() @ _tf32(w2).double()) * d32.double()
        tf = _tf32(gp.float()).double() @ _tf32(w1).double()
        e_own, e_tf = _err(own["dx"], ref), _err(tf, ref)
        print("mlp narrow dgrad C %d bf16x3 %.2e  TF32 operands %.2e" % (C, e_own, e_tf))
        assert e_own < 3e-5 and e_own * 8 < e_tf, (e_own, e_tf)
    else:
        gp = (g.bfloat16().double() @ w2.bfloat16().double()) * d32.double()
        r1 = gp.float().bfloat16().double() @ w1.bfloat16().double()
        e = float((own["dx"].double() - r1).abs().max())
        bound = 2e-6 * float(r1.abs().max()) + 2.0 ** -8 * float(gp.abs().max()) * float(w1.abs().max())
        print("mlp narrow dgrad C %d bf16 operands: against their float64 data gradient %.2e (bound %.2e)" % (C, e, bound))
        assert e <= bound, (e, bound)


@pytest.mark.parametrize("C", WIDTHS)
def test_the_entry_points_refuse_what_they_cannot_run_before_any_launch(C):
    from hipops import lib as L
    lib = L.load()
    M, HID = 33, 6 * C
    x, w1, b1, w2, b2 = _inputs(C, M)[:5]
    g = _refs(C, M)[0]
    st = L.current_stream()
    packs, (pf1, pf2, pb2, pb1) = _packs(lib, st, C, w1, w2)
    bufs = {k: _guarded(n) for k, n in (("y", M * C), ("h", M * HID), ("d", M * HID), ("gpre", M * HID), ("dx", M * C), ("ws", 2 * M * C))}
    v = {k: b[1] for k, b in bufs.items()}
    d_in = torch.ones(M, HID, device="cuda")
    full = 2 * M * C * 4

    def fwd(products, S, x_ptr=x.data_ptr(), h_ptr=v["h"].data_ptr()):
        return lib.dd_mlp_train_fwd(x_ptr, pf1, pf2, b1.data_ptr(), b2.data_ptr(), M, C, products, S, v["y"].data_ptr(), h_ptr, v["d"].data_ptr(),
                                    v["ws"].data_ptr(), full, st)

    def bwd(products, S, g_ptr=g.data_ptr(), gpre_ptr=v["gpre"].data_ptr()):
        return lib.dd_mlp_train_bwd(g_ptr, d_in.data_ptr(), pb2, pb1, M, C, products, S, v["dx"].data_ptr(), gpre_ptr, v["ws"].data_ptr(), full, st)

    for f in (fwd, bwd):
        assert f(6, 2) != 0                      # the hidden range is not split at these widths
        assert f(6, 42) != 0
        assert f(2, 0) != 0                      # an unknown product count
        assert f(6, -1) != 0
    assert fwd(6, 0, x_ptr=x.data_ptr() + 4) != 0 and fwd(6, 0, h_ptr=v["h"].data_ptr() + 4) != 0            # a misaligned pointer
    assert bwd(6, 0, g_ptr=g.data_ptr() + 4) != 0 and bwd(6, 0, gpre_ptr=v["gpre"].data_ptr() + 4) != 0
    assert int(lib.dd_mlp_train_bwd_workspace_bytes(M, C, 2)) == 0 and int(lib.dd_mlp_train_bwd_workspace_bytes(M, C, 0)) == 0
    # the stage-3 pack entry keeps refusing these widths, the narrow one refuses stage 3's and a hidden width that is not 6C
    pbuf, pv = _guarded(packs.numel())
    p0, nb = pv.data_ptr(), packs.numel()
    args = (w1.data_ptr(), w1.stride(0), w1.stride(1), w2.data_ptr(), w2.stride(0), w2.stride(1))
    assert lib.dd_mlp_train_pack(*args, C, HID, p0, p0 + nb, p0 + 2 * nb, p0 + 3 * nb, st) != 0
    assert lib.dd_mlp_train_pack_narrow(*args, 224, 1344, p0, p0 + nb, p0 + 2 * nb, p0 + 3 * nb, st) != 0
    assert lib.dd_mlp_train_pack_narrow(*args, C, HID - 32, p0, p0 + nb, p0 + 2 * nb, p0 + 3 * nb, st) != 0
    torch.cuda.synchronize()
    # every refusal came before a launch: nothing was written
    assert bool(torch.isnan(pbuf).all())
    for k, (buf, view) in bufs.items():
        assert bool(torch.isnan(buf).all()), "a refused call wrote %s" % k


class _Block(torch.nn.Module):
    def __init__(self, C):
        super().__init__()
        self.pwconv1 = torch.nn.Linear(C, 6 * C)
        self.act = torch.nn.GELU()
        self.pwconv2 = torch.nn.Linear(6 * C, C)

    def forward(self, y):
        return self.pwconv2(self.act(self.pwconv1(y)))


@pytest.mark.parametrize("C", WIDTHS)
def test_the_module_path_takes_it_and_counts_it(C, monkeypatch):
    """mlp_train_narrow_ok / mlp_train_narrow (what networks/depth_encoder.py:_mlp_residual calls with a tape, behind the opt-ins) at
    (1, 5, 7, C): output and all five gradients against float64 beside the stock module, the output gradient arriving NON-contiguous; the
    path counts itself and leaves the other four counters alone; it is off without a tape, under autocast, under DD_STOCK_MLP=1, with its
    own switch at 0 and below the default gate; DD_MLP=1 keeps precedence in _mlp_residual"""
    from hipops import functions as HF
    import networks.depth_encoder as DE
    for k in ("DD_MLP", "DD_MLP_RECOMPUTE", "DD_STOCK_MLP", "DD_MLP_TRAIN_NARROW", "DD_MLP_TRAIN_NARROW_MIN_ROWS", "DD_STOCK_LINEAR_GRAD"):
        monkeypatch.delenv(k, raising=False)
    torch.manual_seed(7)
    blk = _Block(C).cuda()
    with torch.no_grad():
        blk.pwconv1.bias.mul_(3.0)
    y = (torch.randn(1, 5, 7, C, device="cuda") * 1.5).requires_grad_(True)
    gout = torch.randn(1, C, 5, 7, device="cuda")                  # the gradient reaches the block through a permute: not contiguous
    assert not HF.mlp_train_narrow_ok(y, blk)                      # 35 rows are below every default gate
    if C in HF._MLP_TRAIN_NARROW_MIN_ROWS:                         # a width that ships on takes the workload's shape (batch 12 at 192x640)
        big = torch.empty((12, 48, 160, 64) if C == 64 else (12, 24, 80, 128), device="cuda")
        assert HF.mlp_train_narrow_ok(big, blk)
    monkeypatch.setenv("DD_MLP_TRAIN_NARROW_MIN_ROWS", "1")
    assert HF.mlp_train_narrow_ok(y, blk) and not HF.mlp_train_ok(y, blk)
    with torch.no_grad():
        assert not HF.mlp_train_narrow_ok(y, blk)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        assert not HF.mlp_train_narrow_ok(y, blk)
    assert not HF.mlp_train_narrow_ok(y.detach().permute(0, 2, 1, 3), blk) and not HF.mlp_train_narrow_ok(y.detach().half(), blk)
    monkeypatch.setenv("DD_STOCK_MLP", "1")
    assert not HF.mlp_train_narrow_ok(y, blk)
    monkeypatch.delenv("DD_STOCK_MLP")
    monkeypatch.setenv("DD_MLP_TRAIN_NARROW", "0")
    assert not HF.mlp_train_narrow_ok(y, blk)
    monkeypatch.delenv("DD_MLP_TRAIN_NARROW")

    def grads(module, inp, run, g):
        module.zero_grad()
        inp.grad = None
        out = run(inp)
        (out.permute(0, 3, 1, 2) * g).sum().backward()
        return [out.detach()] + [t.grad.detach().clone() for t in (inp, module.pwconv1.weight, module.pwconv1.bias, module.pwconv2.weight, module.pwconv2.bias)]

    def counters():
        return (HF.mlp_calls(), HF.mlp_recompute_calls(), HF.mlp_fused_calls(), HF.mlp_train_calls())

    others, before = counters(), HF.mlp_train_narrow_calls()
    own = grads(blk, y, lambda t: HF.mlp_train_narrow(t, blk), gout)
    assert HF.mlp_train_narrow_calls() == before + 1 and counters() == others
    lib = grads(blk, y, blk, gout)
    blk.double()
    y64 = y.detach().double().requires_grad_(True)
    ref = grads(blk, y64, blk, gout.double())
    blk.float()
    bad = []
    for name, o, l, r in zip(("out", "dy", "dW1", "db1", "dW2", "db2"), own, lib, ref):
        e_own, e_lib = _err(o, r), _err(l, r)
        print("mlp narrow train module C %-3d %-3s own %.2e  torch fp32 %.2e" % (C, name, e_own, e_lib))
        if not (o.shape == r.shape and e_own <= max(2.0 * e_lib, 2e-6)):
            bad.append((name, e_own, e_lib))
    assert not bad, bad

    # _mlp_residual: this path with nothing set, dd_pw_gemm's (mlp_calls) under the explicit opt-in DD_MLP=1
    blk.gamma, blk.drop_path = None, torch.nn.Identity()
    res = torch.zeros(1, 5, 7, C, device="cuda")
    before = HF.mlp_train_narrow_calls()
    DE._mlp_residual(blk, y, res)
    assert HF.mlp_train_narrow_calls() == before + 1
    monkeypatch.setenv("DD_MLP", "1")
    monkeypatch.setenv("DD_MLP_MIN_ROWS", "1")
    before, before_mlp = HF.mlp_train_narrow_calls(), HF.mlp_calls()
    DE._mlp_residual(blk, y, res)
    assert HF.mlp_train_narrow_calls() == before and HF.mlp_calls() == before_mlp + 1


def test_litemono_step_runs_the_stage1_and_stage2_training_blocks_through_it(monkeypatch):
    """One LiteMono step at batch 2 (192x640) with the row gate lowered, twice, the legs differing in DD_STOCK_MLP only (test_trainer_gpu's
    hooks_against_stock forces DD_MLP=1, which keeps precedence over this path): the four + four blocks of stages 1 and 2 of the training
    pass run through dd_mlp_train_fwd / dd_mlp_train_bwd in the hooked leg and none in the stock leg; losses and gradient norms agree
    inside hooks_against_stock's tolerances (2e-3 and 2e-2)."""
    import numpy as np
    from torch.utils.data import DataLoader
    from Trainer import Trainer
    from hipops import functions as HF
    from test_trainer_gpu import fill_state, make_opt
    for k in ("DD_MLP", "DD_MLP_RECOMPUTE", "DD_MLP_TRAIN_NARROW"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("DD_MLP_TRAIN_NARROW_MIN_ROWS", "256")
    monkeypatch.setenv("DD_STOCK_DROP_PATH", "1")                  # per-block draws in both legs: identical masks
    B, results, calls = 2, {}, {}
    for stock in ("1", "0"):
        monkeypatch.setenv("DD_STOCK_MLP", stock)
        torch.manual_seed(5)
        opt = make_opt("litemono", ["--synthetic", "--channels_last"])
        opt.batch_size = B
        tr = Trainer(opt)
        for name in sorted(tr.base_model.module_names):
            fill_state(getattr(tr.base_model, name), seed=3)
        tr.base_model.to(tr.device)
        tr.num_steps_per_epoch = 100
        tr.setup_phase("fine_tune")
        tr.bool_automask = False
        tr.step = 50
        tr.set_train()
        ds = tr.get_dataset(["s {}".format(i) for i in range(B)])
        batch = next(iter(DataLoader(ds, batch_size=B)))
        rs = np.random.RandomState(1)
        tr.rand_idx_override = {s: rs.randint(0, int(0.4 * (opt.height >> s)) * (opt.width >> s), (B, 500)).astype(np.int64) for s in opt.scales}
        torch.manual_seed(9)
        before = HF.mlp_train_narrow_calls()
        _, losses = tr.process_batch(batch)
        losses["loss"].backward()
        torch.cuda.synchronize()
        calls[stock] = HF.mlp_train_narrow_calls() - before
        norms = {n: sum(float((p.grad.double() ** 2).sum()) for p in getattr(tr.base_model, n).parameters() if p.grad is not None) ** 0.5
                 for n in sorted(tr.base_model.module_names)}
        results[stock] = ({k: float(v) for k, v in losses.items()}, norms)
    assert calls == {"1": 0, "0": 8}, calls
    (l1, n1), (l0, n0) = results["1"], results["0"]
    bad = [k for k in l1 if abs(l1[k] - l0[k]) > 2e-3 * max(abs(l1[k]), 1e-3)]
    bad += ["gradnorm " + k for k in n1 if abs(n1[k] - n0[k]) > 2e-2 * max(n1[k], 1e-6)]
    print({k: (l1[k], l0[k]) for k in l1}, {k: (n1[k], n0[k]) for k in n1})
    assert not bad, bad
