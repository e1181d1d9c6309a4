"""dd_motion_pr on the device (through tools.MotionSegMetrics) against the reference's scan written out in tests/motion_pr_case.py,
evaluated on the same device tensors: exact where the interpolation is exact (dyadic values at integer scale factors, identity
size), decision-masked at general scale factors, and end to end through eval/motion_segmentation.py."""
import glob

import numpy as np
import pytest
import torch

import motion_pr_case as mc

pytestmark = pytest.mark.gpu


def _run(pred, mot, sem, num_sem, thrds=None, counts=None):
    from tools import MotionSegMetrics
    T = 150 if thrds is None else thrds.numel()
    m = MotionSegMetrics(num_thrd=T, num_sem=num_sem, thrds=thrds)
    if counts is not None:
        m.counts = counts
    m.update(pred, mot, sem if num_sem > 0 else None)
    return m


def _check_exact(pred, mot, sem, num_sem, thrds=None):
    pred, mot, sem = pred.cuda(), mot.cuda(), sem.cuda()
    m = _run(pred, mot, sem, num_sem, thrds)
    want = mc.expected_counts(pred, mot, sem, m.thrds, num_sem)
    got = m.counts.cpu()
    assert got.dtype == torch.int64 and got.shape == want.shape
    assert torch.equal(got, want), (got - want).nonzero()[:8]
    return got


@pytest.mark.parametrize("num_sem", [0, 29])
@pytest.mark.parametrize("h,w,H,W", [(9, 20, 36, 80),        # x4
                                     (17, 23, 34, 46),       # x2, odd sizes: 8-pixel runs cross rows and samples, ragged tail
                                     (33, 70, 33, 70)])      # identity
def test_exact_on_dyadic_inputs(h, w, H, W, num_sem):
    pred, mot, sem = mc.dyadic_case(3, h, w, H, W, seed=h)
    up = mc.upsample(pred, (H, W))
    assert torch.equal(up.double(), mc.upsample(pred.double(), (H, W)))             # the premise: the fp32 interpolation is exact
    _check_exact(pred, mot, sem, num_sem)


def _tables():
    return {"reference": mc.reference_thrds(150), "non_uniform": torch.linspace(0, 1, 152)[1:-1] ** 2,
            "T1": torch.tensor([0.25]), "T256": torch.linspace(-0.01, 1.01, 256)}


@pytest.mark.parametrize("table", ["reference", "non_uniform", "T1", "T256"])
def test_strict_comparison_at_the_table_entries(table):
    """Pixels exactly on a table entry do not exceed it; the next float up does, the next float down does not exceed the entry
    before either."""
    thrds = _tables()[table]
    vals = torch.cat([thrds, torch.nextafter(thrds, torch.tensor(2.0)), torch.nextafter(thrds, torch.tensor(-2.0)), torch.tensor([0.0, 1.0, -1.0, 2.0])])
    h, w = 11, (vals.numel() + 10) // 11
    g = torch.Generator().manual_seed(7)
    pred = torch.zeros(h * w)
    pred[:vals.numel()] = vals
    pred = pred[torch.randperm(h * w, generator=g)].reshape(1, 1, h, w).repeat(2, 1, 1, 1)
    mot = torch.randint(0, 4, (2, h, w), generator=g, dtype=torch.uint8)
    sem = torch.randint(0, 29, (2, h, w), generator=g, dtype=torch.uint8)
    got = _check_exact(pred, mot, sem, 29, thrds)
    # and spelled out without the interpolation (identity size copies the values)
    bins = (pred[:, 0, :, :, None] > thrds).sum(-1)
    assert torch.equal(got[1], torch.bincount(bins[mot != 3], minlength=thrds.numel() + 1))


def _extreme(name):
    pred, mot, sem = mc.dyadic_case(3, 17, 23, 34, 46, seed=11, sem_max=29)
    if name == "pred_zeros":
        pred = torch.zeros_like(pred)
    elif name == "pred_ones":
        pred = torch.ones_like(pred)
    elif name == "labels_all_3":
        mot = torch.full_like(mot, 3)
    elif name == "labels_all_1":
        mot = torch.ones_like(mot)
    elif name == "sem_beyond_num_sem":
        sem = torch.randint(0, 256, sem.shape, generator=torch.Generator().manual_seed(12), dtype=torch.uint8)
    return pred, mot, sem


@pytest.mark.parametrize("name", ["pred_zeros", "pred_ones", "labels_all_3", "labels_all_1", "sem_beyond_num_sem"])
def test_contention_and_extremes(name):
    """Whole waves on one (row, bin) -- the wave-aggregated path -- and the labels that fall in no row."""
    pred, mot, sem = _extreme(name)
    got = _check_exact(pred, mot, sem, 29)
    n = mot.numel()
    if name == "pred_zeros":                                 # every pixel in the one bin of the value 0
        b0 = int((0.0 > mc.reference_thrds(150)).sum())
        assert b0 >= 1 and int(got[1, b0]) == int((mot != 3).sum()) and int(got.sum()) == int(got[:, b0].sum())
    if name == "pred_ones":                                  # 1 exceeds all 150 entries
        assert int(got[0, 150]) == int((mot == 1).sum()) and int(got[:, :150].sum()) == 0
    if name == "labels_all_3":
        assert int(got.sum()) == 0
    if name == "labels_all_1":
        assert int(got[0].sum()) == int(got[1].sum()) == n and int(got[2:].sum()) == 0
    if name == "sem_beyond_num_sem":
        assert int(got[2:].sum()) == int(((mot != 1) & (mot != 3) & (sem < 29)).sum()) < int(((mot != 1) & (mot != 3)).sum())


def test_nan_pixel_lands_in_bin_zero():
    pred = torch.ones(2, 1, 33, 70)
    pred[1, 0, 20, 31] = float("nan")
    mot = torch.ones(2, 33, 70, dtype=torch.uint8)
    got = _check_exact(pred, mot, mot, 0)
    # at equal sizes F.interpolate copies: the NaN stays one pixel (a tap of weight 0 does not spread it), and it is in bin 0
    assert int(torch.isnan(mc.upsample(pred.cuda(), (33, 70))).sum()) == 1
    assert int(got[0, 0]) == 1 and int(got[0, 150]) == mot.numel() - 1


def test_nan_spreads_as_in_the_interpolation():
    """x2: every output that has the NaN among its four taps is NaN in F.interpolate and here, and lands in bin 0."""
    pred = torch.ones(2, 1, 17, 23)
    pred[1, 0, 9, 11] = float("nan")
    mot = torch.ones(2, 34, 46, dtype=torch.uint8)
    got = _check_exact(pred, mot, mot, 0)
    n_nan = int(torch.isnan(mc.upsample(pred.cuda(), (34, 46))).sum())
    assert n_nan == 16 and int(got[0, 0]) == n_nan and int(got[0, 150]) == mot.numel() - n_nan


def test_accumulation_and_64_bit_counters():
    pred, mot, sem = (t.cuda() for t in mc.dyadic_case(3, 17, 23, 34, 46, seed=13, sem_max=29))
    single = _run(pred, mot, sem, 29).counts
    again = _run(pred, mot, sem, 29).counts
    assert torch.equal(single, again)                        # integer atomics: run-to-run identical
    prefill = 2 ** 32 - 5
    m = _run(pred, mot, sem, 29, counts=torch.full((31, 151), prefill, dtype=torch.int64, device="cuda"))
    m.update(pred, mot, sem)
    assert torch.equal(m.counts, prefill + 2 * single)
    assert int(m.counts.max()) > 2 ** 32                     # a carry past 32 bits happened


def test_unaligned_label_pointers():
    """Label maps that do not start on an 8-byte boundary take the byte-wise loads."""
    pred, mot, sem = (t.cuda() for t in mc.dyadic_case(3, 17, 23, 34, 46, seed=14, sem_max=29))
    want = _run(pred, mot, sem, 29).counts
    from hipops import abi, lib as L
    from tools import MotionSegMetrics
    m = MotionSegMetrics(num_sem=29)
    thr = m.thrds.cuda()
    shifted_mot, shifted_sem = torch.empty(mot.numel() + 8, dtype=torch.uint8, device="cuda"), torch.empty(sem.numel() + 8, dtype=torch.uint8, device="cuda")
    shifted_mot[3:3 + mot.numel()] = mot.reshape(-1)
    shifted_sem[5:5 + sem.numel()] = sem.reshape(-1)
    counts = torch.zeros((31, 151), dtype=torch.int64, device="cuda")
    lib = L.load()
    L.check(lib.dd_motion_pr(abi.ptr(pred), 3, 17, 23, shifted_mot.data_ptr() + 3, shifted_sem.data_ptr() + 5, 34, 46, abi.ptr(thr), 150, 29,
                             abi.ptr(counts), L.current_stream()), "dd_motion_pr")
    assert torch.equal(counts, want)
    # argument checks: hipErrorInvalidValue (1), nothing launched
    for T, num_sem, sem_ptr in ((0, 29, shifted_sem.data_ptr()), (257, 29, shifted_sem.data_ptr()), (150, 33, shifted_sem.data_ptr()), (150, 29, None)):
        assert lib.dd_motion_pr(abi.ptr(pred), 3, 17, 23, abi.ptr(mot), sem_ptr, 34, 46, abi.ptr(thr), T, num_sem, abi.ptr(counts), L.current_stream()) == 1
    torch.cuda.synchronize()
    assert torch.equal(counts, want)


def _smooth_case(B, lh, lw, h, w, H, W, seed=0):
    g = torch.Generator().manual_seed(seed)
    pred = torch.sigmoid(4 * mc.upsample(torch.randn(B, 1, lh, lw, generator=g), (h, w)) - 2)
    mot = torch.randint(0, 4, (B, H, W), generator=g, dtype=torch.uint8)
    return pred.cuda(), mot.cuda()


def test_general_scale_factor_decision_masked():
    """72x128 -> 225x400 (nuScenes' 3.125): the products are no longer exact, so a pixel within 1e-6 of a threshold may fall on either
    side of it; every count must agree up to the number of such pixels, and those must be rare (<= 1e-3 of all) for the test to say
    anything."""
    pred, mot = _smooth_case(2, 9, 16, 72, 128, 225, 400)
    m = _run(pred, mot, None, 0)
    mc.assert_decision_masked(m.counts, pred, mot, m.thrds)
    assert int(m.counts[1].sum()) == int((mot != 3).sum())


def test_full_size_decision_masked():
    """nuScenes evaluation shape, 288x512 -> 900x1600, against the per-sample scan."""
    pred, mot = _smooth_case(2, 36, 64, 288, 512, 900, 1600)
    m = _run(pred, mot, None, 0)
    mc.assert_decision_masked(m.counts, pred, mot, m.thrds)
    assert int(m.counts[1].sum()) == int((mot != 3).sum())


def test_end_to_end_evaluation(tmp_path):
    from eval import motion_segmentation as ms
    from options import DynamoOptions
    from tools import MotionSegMetrics
    from Trainer import Trainer
    from torch.utils.data import DataLoader
    args = ["-d", "kitti", "--synthetic", "--depth_model", "litemono", "--height", "64", "--width", "96", "-b", "2", "--weights_init", "scratch",
            "--num_workers", "0", "--log_dir", str(tmp_path / "logs"), "--eval_dir", str(tmp_path / "out")]
    torch.manual_seed(0)
    opt = DynamoOptions().parse(args=args)
    opt.print_opt = False
    trainer = Trainer(opt)
    trainer.set_eval()
    dataset = trainer.get_dataset(["synthetic {}".format(i) for i in range(4)], is_train=False, load_depth=False, load_mask=True)
    loader = DataLoader(dataset, 2, False, num_workers=0)
    seen = []
    model = trainer.model

    def tapped(inputs):                                      # the same outputs, copied to the host for the second metrics object
        outputs = model(inputs)
        seen.append((outputs[("motion_mask", -1, 0)].float().cpu(), inputs["mot_mask"].cpu(), inputs["sem_mask"].cpu()))
        return outputs

    trainer.model = tapped
    on_device = ms.evaluate(trainer, loader, num_thrd=150, num_sem=29)
    trainer.model = model
    assert len(seen) == 2 and on_device.counts.is_cuda and tuple(seen[0][1].shape) == (2, 128, 192)
    on_host = MotionSegMetrics(num_thrd=150, num_sem=29)
    for pred, mot, sem in seen:
        on_host.update(pred, mot, sem)
    assert not on_host.counts.is_cuda
    pred, mot = torch.cat([s[0] for s in seen]), torch.cat([s[1] for s in seen])
    mc.assert_decision_masked(on_device.counts, pred, mot, on_host.thrds, max_share=1.0)
    mc.assert_decision_masked(on_host.counts, pred, mot, on_host.thrds, max_share=1.0)
    n, _ = mc.near_threshold_counts(mc.upsample(pred, (128, 192)), on_host.thrds)
    diff = (mc.above_from_counts(on_device.counts) - mc.above_from_counts(on_host.counts)).abs()
    assert bool((diff <= n).all()), diff.max()
    assert torch.equal(on_device.counts.sum(1).cpu(), on_host.counts.sum(1))        # the row totals do not depend on the prediction
    res = on_device.compute()
    assert res["fp_tally"]["total"] == int(res["fp"][res["best_thrd_idx"]])            # every synthetic class label is below 29

    ms.main(args)
    files = glob.glob(str(tmp_path / "out" / "*_kitti" / "mot_seg" / "pr_record_*.npz"))
    assert len(files) == 1
    rec = np.load(files[0])
    assert sorted(rec.files) == ["f1", "precision", "recall", "thrds"] and all(rec[k].shape == (150,) for k in rec.files)
    assert np.array_equal(rec["thrds"], mc.reference_thrds(150).numpy())
