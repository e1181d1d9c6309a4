"""Trainer.process_batch on the GPU (networks via MIOpen, loss via the fused HIP path AND via the operator path)
against the reference's full-step goldens on tiny_kitti (MD2, train mode, identical key-addressed weights)."""
import os

import numpy as np
import pytest
import torch

from fill import fill_state
from test_networks import batch_from_golden, make_opt

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def z(golden_dir):
    return np.load(os.path.join(golden_dir, "net_tiny_kitti.npz"))


def build(z, phase, fused, channels_last=False, depth_model="monodepthv2"):
    from Trainer import Trainer
    opt = make_opt(depth_model, ["--synthetic"] + ([] if fused else ["--no_fused_loss"]) + (["--channels_last"] if channels_last else []))
    tr = Trainer(opt)
    for name in sorted(tr.base_model.module_names):
        fill_state(getattr(tr.base_model, name), seed=3)
    tr.base_model.to(tr.device)
    tr.num_steps_per_epoch = 100
    tr.setup_phase(phase)
    tr.bool_automask = phase == "disp_init"
    tr.step = 50
    tr.set_train()
    if phase == "disp_init":
        torch.manual_seed(77)
        tr.noise_override = {s: torch.randn(2, 2, opt.height, opt.width) for s in opt.scales}
    else:
        tr.rand_idx_override = {s: z["{}/fine_tune/rand_idx|{}".format(depth_model, s)] for s in opt.scales}
    return tr, opt


# Tolerances: a MEASURED yardstick instead of fixed per cents.  tests/golden/yardstick_step.npz holds this step --
# this tree's networks on the CPU + the oracle loss, same weights / RANSAC draws / tie-break noise as the reference golden -- in
# float64 and in float32 (tests/golden/make_golden_yardstick.py).  The GPU step is held to the FLOAT64 values, in units of what fp32
# arithmetic costs on the same quantity:
#   a loss term:      yard = max(|float32 CPU - float64|, |reference golden - float64|)   (1e-6 .. 6e-5 of the term)
#   a gradient norm:  yard = max(|g32 - g64| of the gradient VECTORS, |reference golden - float64|)   (0.1 .. 1.7 % of the norm, 7 % for
#                     MonoDepth2's pose decoder in fine_tune: a sum over all pixels with heavy cancellation) -- the vectors' distance,
#                     because a norm is one number and |norm32 - norm64| is small by chance where the vectors are not (it bounds the
#                     norm's error: | |a| - |b| | <= |a - b|)
# within LOSS_K / GRAD_K x yard (+ a rounding floor on the losses).  Measured on MI355X over the ten steps below
# (profiles/r06_step_yardstick.txt): every loss term within 4.4e-6 of float64 (0.9 x yard at most; the ground term 4e-6, old
# tolerance 5e-2), every gradient norm within 1.6 x the vectors' distance.  The fixed tolerances this replaces were 2e-3 on the
# losses, 2e-2 / 6e-2 on the norms.  The reference golden itself sits inside the yardstick by construction;
# tests/test_networks.py::test_yardstick_float32_run_is_the_reference_step pins the float32 CPU run to it without a GPU.
LOSS_K, GRAD_K = 4.0, 4.0
LOSS_FLOOR = 2e-6


def compare_step(z, tr, losses, phase, depth_model, golden_dir=None):
    y = np.load(os.path.join(golden_dir or os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"), "yardstick_step.npz"))
    lines, fails, worst = [], [], {"loss": 0.0, "grad": 0.0}
    pfx = "{}/{}/".format(depth_model, phase)

    def judge(key, got, kind):
        f64, ref = float(y[pfx + "f64/" + key]), float(z[pfx + key])
        if kind == "loss":
            yard, k, floor = max(abs(float(y[pfx + "f32/" + key]) - f64), abs(ref - f64)), LOSS_K, LOSS_FLOOR * max(abs(f64), 1e-3)
        else:
            yard, k, floor = max(float(y[pfx + "gradvec_dist|" + key.split("|")[1]]), abs(ref - f64)), GRAD_K, 1e-7 * max(abs(f64), 1e-3)
        err = abs(got - f64)
        ok = err <= k * yard + floor
        worst[kind] = max(worst[kind], err / (yard + floor / k))
        lines.append("%-44s got %.7e  float64 %.7e  reference %.7e  |err| %.1e (%.1e of it) = %5.2f x yard (%.1e)  %s" % (
            key, got, f64, ref, err, err / max(abs(f64), 1e-30), err / yard if yard > 0 else 0.0, yard, "" if ok else "<-- FAIL"))
        if not ok:
            fails.append(key)

    for name in z.files:
        if name.startswith(pfx + "losses/") and "loss_coef" not in name:
            judge(name[len(pfx):], float(losses[name[len(pfx) + 7:]]), "loss")
    for name in sorted(tr.base_model.module_names):
        sq = sum(float((p.grad.double() ** 2).sum()) for p in getattr(tr.base_model, name).parameters() if p.grad is not None)
        judge("gradnorm|" + name, sq ** 0.5, "grad")
    print("\n".join(lines))
    print("worst of %s %s: losses %.2f x (yard + floor / K) of %.1f allowed, gradient norms %.2f of %.1f" % (depth_model, phase, worst["loss"], LOSS_K, worst["grad"], GRAD_K))
    return fails


@pytest.mark.parametrize("phase", ["disp_init", "fine_tune"])
@pytest.mark.parametrize("channels_last", [True, False])
def test_litemono_train_step_matches_reference(golden_dir, phase, channels_last):
    """The benchmark's network in the mode the benchmark runs it: LiteMono, TRAIN mode (batch-statistics BatchNorm, layer
    scale, XCA, dilated depth-wise convs), channels-last with every network-side HIP hook (and NCHW on the stock operators),
    fused HIP loss -- against the unmodified reference's step on tiny_kitti with identical key-addressed weights
    (tests/golden/make_golden_net.py::gen_litemono_train).  Stochastic depth is switched off on both sides (p = 0)."""
    from networks.depth_encoder import DropPath
    z = np.load(os.path.join(golden_dir, "net_litemono_train.npz"))
    tr, opt = build(z, phase, True, channels_last, depth_model="litemono")
    n = 0
    for m in tr.base_model.modules():
        if isinstance(m, DropPath):
            m.drop_prob = 0.0
            n += 1
    assert n > 0
    tr.base_model.depth_enc._drop_layers = None          # the cached list of active stochastic-depth layers is rebuilt (now empty)
    inputs = batch_from_golden(np.load(os.path.join(golden_dir, "net_tiny_kitti.npz")), opt.scales)
    outputs, losses = tr.process_batch(inputs)
    losses["loss"].backward()
    torch.cuda.synchronize()
    fails = compare_step(z, tr, losses, phase, "litemono")
    assert not fails, fails


@pytest.mark.parametrize("phase", ["disp_init", "fine_tune"])
@pytest.mark.parametrize("fused,channels_last", [(True, False), (False, False), (True, True)])
def test_process_batch_matches_reference(z, phase, fused, channels_last):
    """channels_last=True additionally routes the networks through the NHWC HIP hooks (reflection pad, fused BatchNorm+ReLU
    +residual, conv bias gradients, aligned cat+conv, split reductions, disparity-head gradient)."""
    tr, opt = build(z, phase, fused, channels_last)
    inputs = batch_from_golden(z, opt.scales)
    outputs, losses = tr.process_batch(inputs)
    losses["loss"].backward()
    torch.cuda.synchronize()
    fails = compare_step(z, tr, losses, phase, "monodepthv2")
    assert not fails, fails


@pytest.mark.parametrize("precision", ["high", pytest.param("medium", marks=pytest.mark.gpu_slow)])     # (medium at step level: DD_GPU_SLOW=1; its kernels are in test_conv_mfma_gpu.py)
def test_fewer_partial_products_stay_within_a_stated_distance_of_the_reference_step(z, precision):
    """--matmul_precision high / medium (torch.set_float32_matmul_precision: the 3x3 convolutions of dd_conv3x3_mfma from three / one bf16
    partial products instead of six) is NOT the fp32 step and is not held to its yardstick; it is held to a stated distance from the
    reference's golden step: 'high' (bf16x3, 2^-16 per product) every loss term within 2e-4 and every gradient norm within 2e-2 of the
    reference (or GRAD_K fp32 yardsticks where that is more) -- the fixed tolerances rounds 1-5 granted the fp32 step itself; 'medium'
    (bf16 operands) 2e-2 on the loss terms (the ground term, which holds a discrete RANSAC choice, to a factor); its gradient norms are printed, not judged (1.5x off on the pose decoder, whose gradient is
    a sum that cancels: 7 % between two fp32 arithmetics).  MonoDepth2,
    fine_tune, channels-last: the configuration with the most convolutions on that kernel."""
    from hipops.functions import mfma_conv_calls, mfma_products
    before = torch.get_float32_matmul_precision()
    try:
        from Trainer import Trainer
        opt = make_opt("monodepthv2", ["--synthetic", "--channels_last", "--matmul_precision", precision])
        tr = Trainer(opt)
        assert torch.get_float32_matmul_precision() == precision and mfma_products() == {"high": 3, "medium": 1}[precision]
        for name in sorted(tr.base_model.module_names):
            fill_state(getattr(tr.base_model, name), seed=3)
        tr.base_model.to(tr.device)
        tr.num_steps_per_epoch = 100
        tr.setup_phase("fine_tune")
        tr.bool_automask = False
        tr.step = 50
        tr.set_train()
        tr.rand_idx_override = {s: z["monodepthv2/fine_tune/rand_idx|{}".format(s)] for s in opt.scales}
        n0 = mfma_conv_calls()
        outputs, losses = tr.process_batch(batch_from_golden(z, opt.scales))
        losses["loss"].backward()
        torch.cuda.synchronize()
        assert mfma_conv_calls() > n0 + 10
    finally:
        torch.set_float32_matmul_precision(before)
    tol_loss, tol_grad = {"high": (2e-4, 2e-2), "medium": (2e-2, 0.3)}[precision]
    pfx, worst, fails = "monodepthv2/fine_tune/", [0.0, 0.0], []
    y = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "yardstick_step.npz"))
    for name in z.files:
        if name.startswith(pfx + "losses/") and "loss_coef" not in name:
            ref, got = float(z[name]), float(torch.as_tensor(losses[name[len(pfx) + 7:]]).detach())
            rel = abs(got - ref) / max(abs(ref), 1e-3)
            if precision == "medium" and name.endswith("d_ground"):
                # a DISCRETE choice sits in this term (which RANSAC candidate plane wins): under bf16-rounded operands it flips from run to
                # run (7.7e-4, 8.5e-3, 2.1e-2 off in three runs) -- judged as tests/test_zz_half_precision_gpu.py judges it: same sign, same size
                if not 0.4 <= got / ref <= 2.5:
                    fails.append((name, got, ref))
                continue
            worst[0] = max(worst[0], rel)
            if rel > tol_loss:
                fails.append((name, got, ref))
    for name in sorted(tr.base_model.module_names):
        sq = sum(float((p.grad.double() ** 2).sum()) for p in getattr(tr.base_model, name).parameters() if p.grad is not None)
        ref = float(z[pfx + "gradnorm|" + name])
        # (where fp32 itself is ill-conditioned -- the pose decoder's gradient is a sum over all pixels with heavy cancellation: the fp32
        # gradient VECTORS of two arithmetics are 7 % of the norm apart, compare_step's yardstick -- GRAD_K of that yardstick is granted)
        yard = float(y[pfx + "gradvec_dist|" + name]) / max(ref, 1e-12)
        rel = abs(sq ** 0.5 - ref) / max(ref, 1e-12)
        worst[1] = max(worst[1], rel / max(tol_grad, GRAD_K * yard))
        print("  gradient norm %-12s %.6e  reference %.6e  (%.2e of it; fp32 yardstick %.2e)" % (name, sq ** 0.5, ref, rel, yard))
        if precision == "high" and rel > max(tol_grad, GRAD_K * yard):       # ('medium': printed, not judged -- bf16 operands in a sum that cancels)
            fails.append((name, sq ** 0.5, ref))
    if precision == "high":
        # measured, and stated in DESIGN 4.10: bf16x3 also sits inside the fp32 step's own yardstick test
        print("the fp32 yardstick test on the bf16x3 step:", compare_step(z, tr, losses, "fine_tune", "monodepthv2") or "passes")
    print("matmul precision %s: worst loss term %.2e of the reference's (allowed %.0e), worst gradient norm %.2f of its allowance" % (precision, worst[0], tol_loss, worst[1]))
    assert not fails, fails


@pytest.mark.parametrize("multi_stream", [False, True])
def test_train_steps_reduce_loss_and_graph_matches_eager(multi_stream):
    """A few optimisation steps on synthetic triplets: loss finite and decreasing-ish; the hipGraph step replays -- also with
    the network branches on separate streams (parallel branches of the captured graph)."""
    from Trainer import Trainer
    from torch.utils.data import DataLoader
    losses = {}
    for graph in (False, True):
        torch.manual_seed(0)
        opt = make_opt("litemono", ["--synthetic", "--height", "96", "--width", "160"] + (["--hip_graph"] if graph else []) +
                       (["--multi_stream"] if multi_stream else []))
        opt.batch_size = 2
        tr = Trainer(opt)
        tr.num_steps_per_epoch = 10
        tr.setup_phase("disp_init")
        tr.bool_automask = True
        tr.set_eval()           # no stochastic depth: both runs see the same function
        ds = tr.get_dataset(["s {}".format(i) for i in range(2)])
        batch = next(iter(DataLoader(ds, batch_size=2)))
        tr.noise_override = {s: torch.zeros(2, 2, 96, 160, device="cuda") for s in opt.scales}    # device tensor: graph-capturable
        vals = []
        for i in range(6):
            _, l = tr.train_step({k: (v.clone() if torch.is_tensor(v) else v) for k, v in batch.items()})
            vals.append(float(l["loss"]))
        losses[graph] = vals
        assert all(np.isfinite(vals)), vals
    print(losses)
    assert min(losses[False][-3:]) < losses[False][0] and min(losses[True][-3:]) < losses[True][0]
    # Every step of the replayed graph must track the eager run: step k sees the result of k captured Adam updates.  A capture
    # that swallowed Adam's lazy state initialisation would replay the zero-fills (every update lr*sign(g)) and be off by tens
    # of per cent after five updates.  What remains between the two runs (measured 1e-4 after one update, 5e-3 after five) is
    # the sign-like first Adam updates acting on last-bit gradient differences of weights whose gradient is ~0.
    assert abs(losses[True][0] - losses[False][0]) < 1e-6 * abs(losses[False][0]), losses
    for k in range(1, 6):
        assert abs(losses[True][k] - losses[False][k]) < 2e-2 * abs(losses[False][k]), (k, losses)


# three times what the final code of round 5 measures (printed by the test); round 4 accepted 0.6
RATE_CHANGE_RATIO = 0.36         # measured 0.119 (gpurun_out/r5a)


def test_replayed_steps_follow_a_learning_rate_change():
    """StepLR halves the rate at an epoch boundary; run_epoch has just called optimizer.zero_grad() (every .grad is
    None) when segments.SegmentedStep re-captures its fused-Adam graph for the new rate.  Adam skips parameters without a
    gradient, so a re-capture that does not put the flat-buffer views back records an EMPTY graph and the replayed steps stop
    training.  Replayed run against the eager run through the same schedule: weights keep moving and end on the eager run's."""
    from Trainer import Trainer
    from torch.utils.data import DataLoader
    ends, fracs = {}, {}
    for graph in (False, True):
        torch.manual_seed(0)
        opt = make_opt("litemono", ["--synthetic", "--height", "96", "--width", "160", "--scheduler_step_size", "1"] + (["--hip_graph", "--multi_stream"] if graph else []))
        opt.batch_size = 2
        tr = Trainer(opt)
        tr.num_steps_per_epoch = 10
        tr.setup_phase("disp_init")
        tr.bool_automask = True
        tr.set_eval()           # no stochastic depth: both runs see the same function
        batch = next(iter(DataLoader(tr.get_dataset(["s {}".format(i) for i in range(2)]), batch_size=2)))
        tr.noise_override = {s: torch.zeros(2, 2, 96, 160, device="cuda") for s in opt.scales}

        def step():
            return tr.train_step({k: (v.clone() if torch.is_tensor(v) else v) for k, v in batch.items()})

        def weights():
            return torch.cat([p.detach().double().flatten() for p in tr.base_model.parameters() if p.requires_grad]).clone()
        for _ in range(3):
            step()
        lr0 = tr.optim["optimizer"].param_groups[0]["lr"]
        tr.step_lr_scheduler()                               # end of the epoch (Trainer.run_epoch)
        assert tr.optim["optimizer"].param_groups[0]["lr"] == 0.5 * lr0
        tr.optim["optimizer"].zero_grad()                    # start of the next epoch
        tr.materialise = True                                # its first step is a log step: eager, ends with zero_grad()
        step()
        tr.materialise = False
        torch.cuda.synchronize()
        w_before = weights()
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        if graph:
            assert tr._graph is not None and tr._graph.replays >= 5
            # the replayed step updates through dd_adam_multi (hipops.adam); a silent fall-back to torch's kernel would pass every
            # numerical check of this file
            assert tr._graph.one_launch_adam is not None, tr._graph.adam_fallback
        delta = weights() - w_before
        moved = float(delta.abs().max())
        assert moved > 0.5 * 3 * 0.5 * lr0, ("the steps after the rate change did not train", graph, moved, lr0)
        ends[graph] = delta
        fracs[graph] = float((delta.abs() > 0.05 * lr0).double().mean())       # share of the weights the three steps moved at all
    # what the three steps behind the rate change did to the weights, replayed against eager (an empty Adam graph: ratio 1.0; the
    # sign-like early Adam updates of weights whose gradient is ~0 differ between any two runs)
    ratio = float((ends[True] - ends[False]).norm() / ends[False].norm())
    print("replayed vs eager, update of the three steps behind the rate change: relative L2 %.3e; share of weights moved: replayed %.4f eager %.4f"
          % (ratio, fracs[True], fracs[False]))
    # a replay that froze part of the parameters (an incomplete Adam graph) moves a smaller share of the weights than the eager run
    assert abs(fracs[True] - fracs[False]) < 0.02 and fracs[True] > 0.5, fracs
    assert ratio < RATE_CHANGE_RATIO, ratio


def test_replayed_steps_stay_finite_with_the_host_ahead(monkeypatch):
    """Forty replayed steps at the bench shape (KITTI 192x640, LiteMono, batch 12, fine_tune) WITHOUT a host sync between them, a
    finiteness flag per buffer written on the device every step (segments.SegmentedStep._probe).  With ROCm 7.2's graph packet
    capture on (the runtime's default) the depth network's gradients were non-finite at the fifth replay of exactly this run,
    every time, out of finite inputs; conftest.py / Trainer.py / miopen_env.py switch it off."""
    from Trainer import Trainer
    from torch.utils.data import DataLoader
    assert os.environ.get("DEBUG_CLR_GRAPH_PACKET_CAPTURE") == "0"
    monkeypatch.setenv("DD_SEG_PROBE", "1")
    torch.manual_seed(0)
    opt = make_opt("litemono", ["--synthetic", "--hip_graph", "--multi_stream", "--channels_last"])
    opt.batch_size = 12
    tr = Trainer(opt)
    tr.num_steps_per_epoch = 10
    tr.setup_phase("fine_tune")
    tr.bool_automask = False
    tr.step = 10
    tr.set_train()
    ds = tr.get_dataset(["s {}".format(i) for i in range(12)])
    batch = next(iter(DataLoader(ds, batch_size=12)))
    tr.upload_inputs(batch)
    for _ in range(40):
        _, losses = tr.train_step(dict(batch))
    torch.cuda.synchronize()
    report = tr._graph.probe_report()
    print(report, float(losses["loss"]))
    assert tr._graph.replays >= 39 and report.startswith("no non-finite buffer"), report
    assert np.isfinite(float(losses["loss"]))
    for n, p in tr.base_model.named_parameters():
        assert bool(torch.isfinite(p).all()), n


REPLAY_ORDER = {
    "fine_tune": ["inputs fwd", "menc fwd", "pose fwd", "motion fwd", "side fwd", "depth fwd", "fold fwd", "loss fwd",
                  "motion bwd", "menc bwd", "pose bwd", "depth bwd", "optim optim"],
    "disp_init": ["inputs fwd", "pose fwd", "side fwd", "depth fwd", "fold fwd", "loss fwd", "pose bwd", "depth bwd", "optim optim"],
}


@pytest.mark.parametrize("phase", ["fine_tune", "disp_init"])
def test_replayed_step_launches_its_graphs_in_the_recorded_order(phase, monkeypatch):
    """Which graphs a replayed step launches, in which host order (segments.SegmentedStep.run; DD_SEG_TIMING=1 brackets every launch
    with events, timeline() names them).  The lists were recorded from the step as it stood before the placement switches of
    rounds 3 and 4 were retired: a segment that is dropped, added or issued at another point of the step changes them."""
    from Trainer import Trainer
    from torch.utils.data import DataLoader
    monkeypatch.setenv("DD_SEG_TIMING", "1")
    torch.manual_seed(0)
    opt = make_opt("litemono", ["--synthetic", "--hip_graph", "--multi_stream", "--channels_last", "--height", "96", "--width", "160"])
    opt.batch_size = 2
    tr = Trainer(opt)
    tr.num_steps_per_epoch = 10
    tr.setup_phase(phase)
    tr.bool_automask = False
    tr.step = 10
    tr.set_train()
    batch = next(iter(DataLoader(tr.get_dataset(["s {}".format(i) for i in range(2)]), batch_size=2)))
    tr.upload_inputs(batch)
    for _ in range(3):
        tr.train_step(dict(batch))
    assert tr._graph is not None and tr._graph.replays == 3
    order = [name for name, _, _ in tr._graph.timeline()]
    print(phase, order)
    assert order == REPLAY_ORDER[phase]


STOCK_SWITCHES = ("DD_STOCK_CONV_BIAS_GRAD", "DD_STOCK_REFLECT_PAD", "DD_STOCK_DWCONV", "DD_STOCK_LINEAR_GRAD", "DD_STOCK_BATCHNORM",
                  "DD_STOCK_XCA", "DD_STOCK_LAYERNORM", "DD_STOCK_CAT_CONV", "DD_STOCK_REDU_CAT", "DD_STOCK_LAYER_SCALE", "DD_STOCK_SLICES", "DD_STOCK_SMALL_CONV", "DD_STOCK_HEAD_CONV", "DD_STOCK_REDU", "DD_STOCK_MFMA_CONV", "DD_STOCK_MLP", "DD_STOCK_MLP_FUSED")


def hooks_against_stock(extra, B):
    """One LiteMono training step (train-mode BatchNorm, stochastic depth on, channels-last) with every network-side HIP hook
    against the same step on the stock torch operators: same weights, inputs and random stream -> same losses and gradients.
    Returns how often hipops.functions.SmallConvFn ran in the hooked step."""
    from Trainer import Trainer
    from torch.utils.data import DataLoader
    from hipops import functions as HF
    results, small, mfma, mlps, fused = {}, {}, {}, {}, {}
    old = {k: os.environ.get(k) for k in STOCK_SWITCHES + ("DD_STOCK_DROP_PATH", "DD_MLP_MIN_ROWS", "DD_MLP")}
    try:
        os.environ["DD_STOCK_DROP_PATH"] = "1"                    # per-block draws in both runs: identical masks
        os.environ["DD_MLP"] = "1"                                # the opt-in dd_pw_gemm path (csrc/dd_pw_gemm.hip) is part of the hooked step here
        os.environ["DD_MLP_MIN_ROWS"] = "1024"                    # ... on every stage at these small batches too (its few-rows dispatch)
        for stock in ("1", "0"):
            for k in STOCK_SWITCHES:
                os.environ[k] = stock
            torch.manual_seed(5)
            opt = make_opt("litemono", ["--synthetic", "--channels_last"] + list(extra))
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
            before, before_mfma, before_mlp, before_fused = HF.small_conv_calls(), HF.mfma_conv_calls(), HF.mlp_calls(), HF.mlp_fused_calls()
            _, losses = tr.process_batch(batch)
            losses["loss"].backward()
            torch.cuda.synchronize()
            small[stock] = HF.small_conv_calls() - before
            mfma[stock] = HF.mfma_conv_calls() - before_mfma
            mlps[stock] = HF.mlp_calls() - before_mlp
            fused[stock] = HF.mlp_fused_calls() - before_fused
            norms = {n: sum(float((p.grad.double() ** 2).sum()) for p in getattr(tr.base_model, n).parameters() if p.grad is not None) ** 0.5
                     for n in sorted(tr.base_model.module_names)}
            results[stock] = ({k: float(v) for k, v in losses.items()}, norms)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    (l1, n1), (l0, n0) = results["1"], results["0"]
    bad = [k for k in l1 if abs(l1[k] - l0[k]) > 2e-3 * max(abs(l1[k]), 1e-3)]
    bad += ["gradnorm " + k for k in n1 if abs(n1[k] - n0[k]) > 2e-2 * max(n1[k], 1e-6)]
    print({k: (l1[k], l0[k]) for k in l1}, {k: (n1[k], n0[k]) for k in n1}, "dd_conv_small launches (stock, hooked):", small["1"], small["0"])
    print("dd_conv3x3_mfma forward launches (stock, hooked):", mfma["1"], mfma["0"])
    assert not bad, bad
    print("dd_pw_gemm MLP blocks (stock, hooked):", mlps["1"], mlps["0"])
    assert small["1"] == 0 and mfma["1"] == 0 and mlps["1"] == 0
    assert mlps["0"] > 0            # LiteMono's pwconv1 -> GELU -> pwconv2 ran through csrc/dd_pw_gemm.hip
    print("dd_mlp_fwd block forwards of the statistics-only side batch (stock, hooked):", fused["1"], fused["0"])
    assert fused["1"] == 0 and fused["0"] > 0
    assert mfma["0"] > 0            # the 3x3 stride-1 convolutions of the hooked step ran on the bf16 matrix pipe (csrc/dd_conv_mfma.hip)
    return small["0"]


def test_litemono_step_hooks_match_stock_operators():
    """KITTI shape 192x640, batch 2 (below dd_conv_small's 64k-pixel threshold... 2 x 192 x 640 = 245 760 pixels: above it)."""
    assert hooks_against_stock([], 2) > 0


def test_waymo_shape_step_hooks_match_stock_operators():
    """BASELINE.json config 4's network at ITS shape and batch (VERDICT r4 missing #4): LiteMono + motion networks at 320x480,
    batch 8, fine_tune -- dd_conv_small's tile grid at 15 x 20 tiles, the 300-tile XCD remap of the photometric kernel, the motion
    decoders' full-resolution level at 1.2 M pixels (reference networks/motion_decoder.py:48-91, options.py:274-294)."""
    assert hooks_against_stock(["-d", "waymo"], 8) > 0


@pytest.mark.parametrize("phase", ["disp_init", "fine_tune"])
def test_logging_rows_agree_between_loss_paths(z, phase):
    """the image rows of Trainer.log (reconstruction, L1, disparity / mask / depth, ego / independent / total
    flow through vis_motion) built from what the FUSED path materialises on a log step equal the rows built from the
    operator-by-operator path's outputs (which keeps the full-resolution ('independ_flow', f, 0) like the reference)."""
    rows = {}
    for fused in (True, False):
        tr, opt = build(z, phase, fused)
        tr.materialise = True
        inputs = batch_from_golden(z, opt.scales)
        with torch.no_grad():
            outputs, losses = tr.process_batch(inputs)
        r = tr.vis_rows(inputs, outputs)
        H, W = opt.height, opt.width
        assert r.shape == (2, 3, 3 * H, 3 * W) and bool(torch.isfinite(r).all()) and float(r.min()) >= 0 and float(r.max()) <= 1.0 + 1e-6
        rows[fused] = r
        package = tr.log("train", inputs, outputs, losses)
        assert isinstance(package["train_loss"], float)
    err = (rows[True] - rows[False]).abs()
    # identical network outputs; the warp differs by sub-pixel rounding, the flow wheel is normalised by its own maximum
    assert float(err.mean()) < 1e-4 and float((err > 2e-2).float().mean()) < 1e-3, (float(err.mean()), float(err.max()))


@pytest.mark.parametrize("depth_model,phase", [("litemono", "fine_tune"), ("monodepthv2", "disp_init")])
def test_multi_stream_forward_is_the_same_step(z, depth_model, phase):
    """--multi_stream only changes WHERE the independent branches of the forward (and, through autograd, of the backward) are
    enqueued: same kernels, same inputs -> the same losses, gradients and BatchNorm statistics up to the run-to-run noise the
    single-stream step has itself."""
    from networks.depth_encoder import DropPath
    seen = []
    for multi in (False, False, True, True):
        torch.manual_seed(5)
        tr, opt = build(z, phase, True, True, depth_model=depth_model) if depth_model == "monodepthv2" else build(
            np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "net_litemono_train.npz")), phase, True, True, depth_model=depth_model)
        for m in tr.base_model.modules():
            if isinstance(m, DropPath):
                m.drop_prob = 0.0
        opt.multi_stream = multi
        inputs = batch_from_golden(z, opt.scales)
        _, losses = tr.process_batch(inputs)
        losses["loss"].backward()
        torch.cuda.synchronize()
        grads = torch.cat([p.grad.flatten() for p in tr.base_model.parameters() if p.grad is not None])
        stats = torch.cat([b.flatten().float() for n, b in tr.base_model.named_buffers() if "running" in n])
        seen.append((float(losses["loss"]), grads.double().clone(), stats.double().clone()))

    def dist(a, b):
        return (abs(a[0] - b[0]) / abs(a[0]), float((a[1] - b[1]).norm() / a[1].norm()), float((a[2] - b[2]).norm() / a[2].norm()))
    single, multi, cross = dist(seen[0], seen[1]), dist(seen[2], seen[3]), dist(seen[0], seen[2])
    print("single vs single", single, "multi vs multi", multi, "single vs multi", cross)
    # The convolution library's split-K kernels accumulate with atomics, so two runs of the SAME configuration already differ in
    # the last bits; the multi-stream step has to stay inside that band (a missing inter-stream dependency reads half-written
    # tensors and is off by orders of magnitude more).
    for k in range(3):
        floor = max(single[k], multi[k], 2.5e-7)         # statistics: a deferred update rounds (1-m)*r and the sum separately (1 ulp)
        assert cross[k] <= 4 * floor, (k, single, multi, cross)
        assert multi[k] <= max(4 * single[k], 1e-6), (k, single, multi)


def test_multi_stream_training_run_tracks_the_single_stream_run():
    """Four optimizer steps with library kernels that use no atomics: the multi-stream run must end on the single-stream
    run's weights to within what two single-stream runs differ by (a few 1e-6; an Adam step is 1e-4).  Catches a permuted
    random stream (the stochastic-depth draws of the three depth passes: 3.6e-4 before they were drawn up front) as well
    as a missing cross-stream dependency."""
    import importlib.util
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "check_ms_determinism.py")
    spec = importlib.util.spec_from_file_location("check_ms_determinism", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    bench, det = torch.backends.cudnn.benchmark, torch.backends.cudnn.deterministic
    try:
        eager = ["--no_hip_graph"]          # (the replayed step has its own test; this one is about the host-issued streams)
        single, again, multi = mod.run(False, extra=eager), mod.run(False, extra=eager), mod.run(True, extra=eager)
    finally:
        torch.backends.cudnn.benchmark, torch.backends.cudnn.deterministic = bench, det
    noise = float((single[0] - again[0]).abs().max())
    diff = float((single[0] - multi[0]).abs().max())
    print("single vs single %.3e, multi vs single %.3e" % (noise, diff))
    assert diff <= max(1.5e-4, 20.0 * noise), (diff, noise)
    assert max(abs(a - b) for a, b in zip(single[2], multi[2])) < 1e-4, (single[2], multi[2])


def test_stats_only_side_frames_leave_the_run_unchanged():
    """--stats_only_side_frames (opt-in): frames -1/+1 stop after the depth encoder.  The decoders hold no BatchNorm and no
    training step reads those disparities (reference Trainer.py:222-230,357,371,428), so four optimizer steps must end on the
    same weights AND the same running statistics as the full passes, to within what two identical runs differ by."""
    import importlib.util
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "check_ms_determinism.py")
    spec = importlib.util.spec_from_file_location("check_ms_determinism", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    bench, det = torch.backends.cudnn.benchmark, torch.backends.cudnn.deterministic
    try:
        full, again, lean = mod.run(True), mod.run(True), mod.run(True, extra=["--stats_only_side_frames"])
    finally:
        torch.backends.cudnn.benchmark, torch.backends.cudnn.deterministic = bench, det
    for what, i in (("weights", 0), ("buffers", 1)):
        noise, diff = float((full[i] - again[i]).abs().max()), float((full[i] - lean[i]).abs().max())
        print("%s: full vs full %.3e, encoder-only side frames vs full %.3e" % (what, noise, diff))
        assert diff <= max(2e-5, 20.0 * noise), (what, diff, noise)
    assert max(abs(a - b) for a, b in zip(full[2], lean[2])) < 1e-4, (full[2], lean[2])


@pytest.mark.parametrize("phase", ["disp_init", "fine_tune"])
def test_packed_source_frames_leave_the_losses_unchanged(z, phase, monkeypatch):
    """Trainer.pack_sources (default on): the input side hands the photometric kernel pixel-interleaved copies of the two source frames
    (DDPhotoArgs.source_packed).  Same weights, same batch: every entry of the losses dict is the one of the planar run (the kernel's own
    outputs are bit-identical, tests/test_photo_gpu.py; the networks in front of it are the same launches)."""
    from hipops import fused_loss as FL
    res = {}
    for on in ("1", "0"):
        monkeypatch.setenv("DD_PACK_SOURCES", on)
        tr, opt = build(z, phase, True, channels_last=True)
        inputs = batch_from_golden(z, opt.scales)
        before = FL.PACKED_CALLS[0]
        outputs, losses = tr.process_batch(inputs)
        torch.cuda.synchronize()
        took = FL.PACKED_CALLS[0] - before
        assert took == (1 if on == "1" else 0), (on, took)
        assert (("color_packed", -1) in inputs) == (on == "1") and (("color_packed", 1) in inputs) == (on == "1")
        if on == "1":
            for f in (-1, 1):
                assert torch.equal(inputs[("color_packed", f)], inputs[("color", f, 0)].permute(0, 2, 3, 1).contiguous())
        res[on] = {k: float(v.detach()) for k, v in losses.items() if torch.is_tensor(v) and v.numel() == 1}
    assert res["1"].keys() == res["0"].keys() and "loss" in res["1"]
    worst = max(abs(res["1"][k] - res["0"][k]) / max(abs(res["0"][k]), 1e-6) for k in res["1"])
    print("packed vs planar source frames, %s: worst relative difference over %d loss entries %.2e" % (phase, len(res["1"]), worst))
    assert worst <= 1e-6, (worst, res)
