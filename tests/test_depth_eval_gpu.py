"""dd_depth_metrics_accumulate and tools.DepthMetricsAccumulator on the device: the accumulation against a sequential float64 loop
on the host (exact: same operations, same order), independence of how the samples are cut into batches (bit for bit), the totals
against tools.DepthMetrics aggregated the way the reference's eval/depth.py does it (within the rounding of that path, derived in
place), a sample without a LiDAR point inside the bounds, and eval/depth.py end to end on generated samples."""
import glob
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NAMES = ["de:abs_rel", "de:sq_rel", "de:rms", "de:log_rms", "da:a1", "da:a2", "da:a3"]
BOUND, MIN_DEPTH, MAX_DEPTH = [0, 1, 0, 1], 1e-3, 75.0
H, W, M, GH, GW = 24, 40, 300, 48, 80


# ---- the entry point alone ---------------------------------------------------------------------------------------------------
def _rows(B, seed):
    """per_sample (B,8) with NaN rows of count 0, per_label (B,256,8) with most labels absent (zero rows), as the metrics kernels write them."""
    g = torch.Generator().manual_seed(seed)
    per = torch.rand(B, 8, generator=g) * 3
    per[:, 7] = torch.randint(1, 25000, (B,), generator=g).float()
    empty = torch.rand(B, generator=g) < 0.3
    if B >= 3:
        empty[1] = True
    per[empty, :7] = float("nan")
    per[empty, 7] = 0
    lab = torch.rand(B, 256, 8, generator=g) * 3
    lab[:, :, 7] = torch.randint(1, 25000, (B, 256), generator=g).float()
    lab[torch.rand(B, 256, generator=g) < 0.7] = 0
    lab[:, 200:] = 0                                          # labels no sample shows
    return per, lab


def _host_accumulate(per, lab, totals, label_totals):
    """The contract of dd_depth_metrics_accumulate, one addition at a time in float64, in batch order."""
    per, lab = per.numpy(), lab.numpy()
    for b in range(per.shape[0]):
        if per[b, 7] > 0:
            for j in range(7):
                totals[j] += np.float64(per[b, j])
            totals[7] += 1
        else:
            totals[8] += 1
        cnt = lab[b, :, 7].astype(np.float64)
        label_totals[:, :7] += lab[b, :, :7].astype(np.float64) * cnt[:, None]      # one label per row: no sum across rows
        label_totals[:, 7] += cnt


def _device_accumulate(batches):
    from hipops import abi, lib as L
    lib = L.load()
    totals = torch.zeros(9, dtype=torch.float64, device="cuda")
    label_totals = torch.zeros(256, 8, dtype=torch.float64, device="cuda")
    for per, lab in batches:
        per, lab = per.cuda(), lab.cuda()
        L.check(lib.dd_depth_metrics_accumulate(abi.ptr(per), abi.ptr(lab), per.shape[0], abi.ptr(totals), abi.ptr(label_totals), L.current_stream()),
                "dd_depth_metrics_accumulate")
    return totals.cpu(), label_totals.cpu()


@pytest.mark.parametrize("B", [1, 3, 7])
def test_accumulate_is_the_sequential_float64_sum(B):
    batches = [_rows(B, seed=10 * B), _rows(B, seed=10 * B + 1)]           # two calls in a row into the same totals
    want_t, want_l = np.zeros(9), np.zeros((256, 8))
    for per, lab in batches:
        _host_accumulate(per, lab, want_t, want_l)
    got_t, got_l = _device_accumulate(batches)
    assert np.isfinite(want_t).all() and want_t[7] + want_t[8] == 2 * B
    assert np.array_equal(got_t.numpy(), want_t), (got_t.numpy() - want_t)
    assert np.array_equal(got_l.numpy(), want_l), np.abs(got_l.numpy() - want_l).max()
    assert (want_l[200:] == 0).all() and (want_l[:200, 7] > 0).any()
    again_t, again_l = _device_accumulate(batches)
    assert torch.equal(again_t, got_t) and torch.equal(again_l, got_l)     # bit-identical from run to run


def test_accumulate_without_labels_and_bad_arguments():
    from hipops import abi, lib as L
    lib = L.load()
    per, lab = (t.cuda() for t in _rows(3, seed=5))
    totals = torch.full((9,), 7.0, dtype=torch.float64, device="cuda")
    label_totals = torch.full((256, 8), 7.0, dtype=torch.float64, device="cuda")
    s = L.current_stream()
    bad = [(None, abi.ptr(lab), 3, abi.ptr(totals), abi.ptr(label_totals)),        # no per_sample
           (abi.ptr(per), abi.ptr(lab), 3, None, abi.ptr(label_totals)),           # no totals
           (abi.ptr(per), abi.ptr(lab), 0, abi.ptr(totals), abi.ptr(label_totals)),  # B < 1
           (abi.ptr(per), abi.ptr(lab), 3, abi.ptr(totals), None),                 # per_label without label_totals
           (abi.ptr(per), None, 3, abi.ptr(totals), abi.ptr(label_totals))]        # label_totals without per_label
    for args in bad:
        assert lib.dd_depth_metrics_accumulate(*args, s) == 1
    torch.cuda.synchronize()
    assert bool((totals == 7).all()) and bool((label_totals == 7).all())
    # no labels at all: only `totals` moves
    assert lib.dd_depth_metrics_accumulate(abi.ptr(per), None, 3, abi.ptr(totals), None, s) == 0
    want_t, want_l = np.full(9, 7.0), np.zeros((256, 8))
    _host_accumulate(per.cpu(), torch.zeros_like(lab).cpu(), want_t, want_l)
    assert np.array_equal(totals.cpu().numpy(), want_t) and bool((label_totals == 7).all())


# ---- the accumulator class ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def samples():
    """Seven samples: disparity 24 x 40, 300 LiDAR points (some invalid, some outside the depth range) in 48 x 80 ground-truth pixels,
    motion-mask labels 0..3 at 48 x 80."""
    g = torch.Generator().manual_seed(0)
    n = 7
    disp = 0.02 + 0.5 * torch.rand(n, 1, H, W, generator=g)
    rows = torch.randint(0, GH, (n, M), generator=g).float()
    cols = torch.randint(0, GW, (n, M), generator=g).float()
    z = 0.5 + 90 * torch.rand(n, M, generator=g)             # some beyond the 75 m bound
    inputs = {"depth_gt": torch.stack([rows, cols, z], 2), "depth_valid": (torch.rand(n, M, generator=g) < 0.9).float(),
              "gt_dim": torch.tensor([[GH, GW]] * n, dtype=torch.int32)}
    mask = torch.randint(0, 4, (n, GH // 8, GW // 8), generator=g, dtype=torch.uint8).repeat_interleave(8, 1).repeat_interleave(8, 2).contiguous()
    return {k: v.cuda() for k, v in inputs.items()}, disp.cuda(), mask.cuda()


def _cut(samples, sizes):
    inputs, disp, mask = samples
    at = 0
    for b in sizes:
        yield {k: v[at:at + b] for k, v in inputs.items()}, disp[at:at + b], mask[at:at + b]
        at += b
    assert at == disp.shape[0]


def _accumulate(samples, sizes, masked, bound=BOUND):
    from tools import DepthMetricsAccumulator
    acc = DepthMetricsAccumulator(bound, MIN_DEPTH, MAX_DEPTH)
    for inputs, disp, mask in _cut(samples, sizes):
        assert acc.update(inputs, disp, mask if masked else None) is None
    return acc


@pytest.mark.parametrize("masked", [False, True])
def test_totals_do_not_depend_on_the_batch_cut(samples, masked):
    whole = _accumulate(samples, [7], masked)
    assert whole.totals.is_cuda and whole.totals.dtype == torch.float64
    for sizes in ([3, 3, 1], [1] * 7):
        cut = _accumulate(samples, sizes, masked)
        assert torch.equal(cut.totals, whole.totals), (sizes, cut.totals - whole.totals)
        if masked:
            assert torch.equal(cut.label_totals, whole.label_totals), sizes
    res = whole.compute()
    assert res["num"] == 7 and res["skipped"] == 0 and all(np.isfinite(res["overall"][m]) for m in NAMES)
    if masked:
        assert sorted(res["by_label"]) == [0, 1, 2, 3] and all(c > 0 for c in res["label_counts"].values())
    else:
        assert "by_label" not in res


def test_totals_against_depth_metrics_aggregated_as_the_reference_does(samples):
    """The existing path, per batch of 3 (3 + 3 + 1), summed the way eval/depth.py sums it.  Overall row: that path rounds each batch mean
    to fp32 (B - 1 fp32 additions and a division) before the script multiplies by B, so the sums may differ by
    sum_batches B * (B * 2**-24) * mean|x|, plus (n - 1) * 2**-53 * sum|term| for the float64 additions in another order.  Per label:
    the same fp32 values times integer counts summed in float64 in another order, (n - 1) * 2**-53 * sum|term|."""
    from tools import DepthMetrics
    dm = DepthMetrics(BOUND, MIN_DEPTH, MAX_DEPTH)
    sizes, n = [3, 3, 1], 7
    want = {m: 0.0 for m in NAMES}
    want_l = {l: {m: [0.0, 0] for m in NAMES} for l in range(4)}
    slack = np.zeros(7)
    total = 0
    for inputs, disp, mask in _cut(samples, sizes):
        B = disp.shape[0]
        met = dm(inputs, {("disp_scaled", 0, 0): disp})
        met_m = dm(inputs, {("disp_scaled", 0, 0): disp}, mask=mask)
        per = dm.device_metrics(inputs, disp)[0].double().cpu().numpy()
        slack += B * (B * 2.0 ** -24) * np.abs(per[:, :7]).mean(0)
        for m in NAMES:
            want[m] += met[m].item() * B
            for l in range(4):
                if l in met_m["{}_mask".format(m)]:
                    want_l[l][m][0] += met_m["{}_mask".format(m)][l][0]
                    want_l[l][m][1] += met_m["{}_mask".format(m)][l][1]
        total += B
    acc = _accumulate(samples, sizes, masked=True)
    totals, label_totals = acc.totals.cpu().numpy(), acc.label_totals.cpu().numpy()
    assert total == n and totals[7] == n
    for j, m in enumerate(NAMES):
        bound = slack[j] + (n - 1) * 2.0 ** -53 * abs(totals[j])              # every term is non-negative: sum|term| is the sum
        print("{:10s} sum {:.9f} reference-style {:.9f} diff {:.3e} bound {:.3e}".format(m, totals[j], want[m], abs(totals[j] - want[m]), bound))
        assert abs(totals[j] - want[m]) <= bound, (m, totals[j], want[m], bound)
        for l in range(4):
            bound_l = (n - 1) * 2.0 ** -53 * abs(label_totals[l, j])
            assert label_totals[l, 7] == want_l[l][m][1] > 0
            assert abs(label_totals[l, j] - want_l[l][m][0]) <= bound_l, (m, l, label_totals[l, j], want_l[l][m][0], bound_l)
    res = acc.compute()
    for j, m in enumerate(NAMES):
        assert res["overall"][m] == totals[j] / totals[7] and res["by_label"][2][m] == label_totals[2, j] / label_totals[2, 7]


def test_sample_without_a_point_inside_the_bounds_is_skipped(samples):
    """eval_img_bound keeps the lower half of the image; sample 1's points all lie in the upper half."""
    inputs, disp, mask = samples
    inputs = {k: v[:3].clone() for k, v in inputs.items()}
    inputs["depth_gt"][1, :, 0] = inputs["depth_gt"][1, :, 0] % (GH // 2)
    for masked in (False, True):
        acc = _accumulate((inputs, disp[:3], mask[:3]), [2, 1], masked, bound=[0.5, 1, 0, 1])
        res = acc.compute()
        assert res["num"] == 2 and res["skipped"] == 1
        assert all(np.isfinite(res["overall"][m]) for m in NAMES)
        if masked:
            assert all(np.isfinite(v) for row in res["by_label"].values() for v in row.values())
    # the two samples that count, alone, give the same totals bit for bit
    two = {k: v[[0, 2]] for k, v in inputs.items()}
    alone = _accumulate((two, disp[:3][[0, 2]], mask[:3][[0, 2]]), [2], True, bound=[0.5, 1, 0, 1])
    assert torch.equal(alone.totals[:8], acc.totals[:8]) and torch.equal(alone.label_totals, acc.label_totals)


def test_refuses_cpu_tensors(samples):
    from hipops.lib import DynamoHipError
    from tools import DepthMetricsAccumulator
    inputs, disp, _ = samples
    with pytest.raises(DynamoHipError):
        DepthMetricsAccumulator(BOUND, MIN_DEPTH, MAX_DEPTH).update({k: v.cpu() for k, v in inputs.items()}, disp.cpu())


# ---- the script --------------------------------------------------------------------------------------------------------------
def test_end_to_end_evaluation(tmp_path):
    from eval import depth as dp
    from options import DynamoOptions
    from Trainer import Trainer
    args = ["-d", "nuscenes", "--synthetic", "--depth_model", "litemono", "--height", "64", "--width", "96", "-b", "2", "--weights_init", "scratch",
            "--num_workers", "0", "--log_dir", str(tmp_path / "logs"), "--eval_dir", str(tmp_path / "out")]
    torch.manual_seed(0)
    opt = DynamoOptions().parse(args=args)
    opt.print_opt = False
    opt.frame_ids = [0]
    trainer = Trainer(opt)
    trainer.base_model.bool_CmpFlow = trainer.base_model.bool_MotMask = False
    trainer.set_eval()
    loader = dp.eval_loader(trainer, "test_mask_files.txt", load_mask=True)
    assert len(loader.dataset) % 2 == 1                       # a ragged last batch
    acc = dp.evaluate(trainer, loader, masked=True)
    assert acc.totals.is_cuda and acc.label_totals.is_cuda
    res = acc.compute()
    assert res["num"] + res["skipped"] == len(loader.dataset) and res["skipped"] == 0 and {0, 1, 2} <= set(res["by_label"])
    assert [dp.metric_row(s.upper(), [res["by_label"][l][m] for m in NAMES]) for s, l in dp.SPLIT_LABELS] == dp.split_rows(res, NAMES)

    torch.manual_seed(0)
    out = dp.main(args)
    files = glob.glob(str(tmp_path / "out" / "*_nuscenes" / "depth" / "*.txt"))
    assert files == [out["path"]]
    lines = open(files[0]).read().splitlines()
    num = r"-?\d+\.\d{3}"
    rows = {name: [l for l in lines if re.fullmatch(r" *{} *(& {} *){{7}}".format(name, num), l)] for name in ("OVERALL", "BG", "STATIC", "MOT")}
    assert all(len(v) == 1 for v in rows.values()), rows
    assert rows["OVERALL"][0] == dp.overall_row(out["overall"], NAMES)
    assert [rows[k][0] for k in ("BG", "STATIC", "MOT")] == dp.split_rows(out["by_mask"], NAMES)
    assert lines.index(rows["OVERALL"][0]) < lines.index(rows["BG"][0]) < lines.index(rows["STATIC"][0]) < lines.index(rows["MOT"][0])
    assert dp.display_str(["Split"] + NAMES) in lines and "====== Depth Eval on Overall Test Set ======" in lines
