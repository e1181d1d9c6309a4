"""Motion-segmentation evaluation without a GPU: tools.MotionSegMetrics' torch path against the reference's scan written out in
tests/motion_pr_case.py, the compute() identities, the nuScenes reader on the tiny fixture, and the synthetic masks."""
import os

import numpy as np
import pytest
import torch

import motion_pr_case as mc

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
NUSC = os.path.join(ROOT, "tests", "golden", "tiny_nuscenes")


def _metrics(pred, mot, sem, num_sem, thrds=None, num_thrd=150):
    from tools import MotionSegMetrics
    m = MotionSegMetrics(num_thrd=num_thrd, num_sem=num_sem, thrds=thrds)
    m.update(pred, mot, sem if num_sem > 0 else None)
    return m


@pytest.mark.parametrize("num_sem", [0, 29])
def test_torch_path_equals_scan_on_dyadic_inputs(num_sem):
    pred, mot, sem = mc.dyadic_case(2, 18, 32, 72, 128, seed=1)
    # the premise: with dyadic values at an integer scale factor the fp32 interpolation is exact
    assert torch.equal(mc.upsample(pred, (72, 128)).double(), mc.upsample(pred.double(), (72, 128)))
    m = _metrics(pred, mot, sem, num_sem)
    assert torch.equal(m.thrds, mc.reference_thrds(150))
    want = mc.expected_counts(pred, mot, sem, m.thrds, num_sem)
    assert m.counts.dtype == torch.int64 and tuple(m.counts.shape) == (2 + num_sem, 151)
    assert torch.equal(m.counts, want)
    assert int(m.counts[0].sum()) == int((mot == 1).sum()) and int(m.counts[1].sum()) == int((mot != 3).sum())


@pytest.mark.parametrize("num_thrd", [1, 37, 256])
def test_torch_path_equals_scan_on_a_non_uniform_table(num_thrd):
    pred, mot, sem = mc.dyadic_case(2, 18, 32, 72, 128, seed=2)
    thrds = torch.linspace(0, 1, num_thrd + 2)[1:-1] ** 2       # ascending, unevenly spaced
    m = _metrics(pred, mot, sem, 29, thrds=thrds, num_thrd=num_thrd)
    assert torch.equal(m.counts, mc.expected_counts(pred, mot, sem, thrds, 29))


def test_values_on_a_threshold_do_not_exceed_it_and_nan_exceeds_nothing():
    thrds = mc.reference_thrds(150)
    vals = torch.cat([thrds, torch.nextafter(thrds, torch.tensor(2.0)), torch.nextafter(thrds, torch.tensor(-2.0)),
                      torch.tensor([float("nan"), 0.0, 1.0])])
    pred = vals.reshape(1, 1, 1, -1)
    mot = (torch.arange(vals.numel()) % 4).to(torch.uint8).reshape(1, 1, -1)
    m = _metrics(pred, mot, mot, 0)
    assert torch.equal(m.counts, mc.expected_counts(pred, mot, mot, thrds, 0))


def test_two_updates_equal_one_update_on_the_concatenation():
    pred, mot, sem = mc.dyadic_case(4, 18, 32, 72, 128, seed=3)
    one = _metrics(pred, mot, sem, 29)
    two = _metrics(pred[:1], mot[:1], sem[:1], 29)
    two.update(pred[1:], mot[1:], sem[1:])
    assert torch.equal(one.counts, two.counts)


def test_compute_identities():
    g = torch.Generator().manual_seed(4)
    pred, mot, _ = mc.dyadic_case(2, 18, 32, 72, 128, seed=4)
    sem = torch.randint(0, 29, (2, 72, 128), generator=g, dtype=torch.uint8)         # every label < num_sem
    m = _metrics(pred, mot, sem, 29)
    res = m.compute()
    s = mc.scan(pred, mot, sem, m.thrds, 29)
    for name in ("tp", "fp", "fn"):
        assert res[name].dtype == torch.int64 and tuple(res[name].shape) == (150,)
    assert torch.equal(res["tp"], s["tp"]) and torch.equal(res["fp"], s["p_sum"] - s["tp"]) and torch.equal(res["fn"], s["g_sum"] - s["tp"])
    assert bool((res["tp"] + res["fn"] == int((mot == 1).sum())).all())
    for name in ("precision", "recall", "f1"):
        assert res[name].dtype == torch.float32 and tuple(res[name].shape) == (150,)
    tp, fp, fn = res["tp"].double(), res["fp"].double(), res["fn"].double()
    p, r = tp / (tp + fp + 1e-10), tp / (tp + fn + 1e-10)
    assert torch.equal(res["precision"], p.float()) and torch.equal(res["recall"], r.float())
    assert torch.equal(res["f1"], (2 * p * r / (p + r + 1e-10)).float())
    best = res["best_thrd_idx"]
    assert best == int(torch.argmax(res["f1"])) and torch.equal(res["thrds"], m.thrds)
    tally = res["fp_tally"]
    assert tally["total"] == int(res["fp"][best]) == sum(c for l, c in tally.items() if l != "total")
    # ... and it is the reference's second pass: false positives at the best threshold by class
    up = mc.upsample(pred, (72, 128))[:, 0]
    fp_b = (up > m.thrds[best]) & (mot != 1) & (mot != 3)
    labels, cnts = np.unique(sem[fp_b].numpy(), return_counts=True)
    assert {int(l): int(c) for l, c in zip(labels, cnts)} == {l: c for l, c in tally.items() if l != "total"}


def test_labels_at_or_above_num_sem_are_counted_in_no_class_row():
    pred, mot, sem = mc.dyadic_case(2, 18, 32, 72, 128, seed=5, sem_max=40)
    m = _metrics(pred, mot, sem, 29)
    assert torch.equal(m.counts, mc.expected_counts(pred, mot, sem, m.thrds, 29))
    assert int(m.counts[2:].sum()) < int(((mot != 1) & (mot != 3)).sum())


def _nusc_dataset(**kw):
    import datasets
    args = dict(data_path=NUSC, filenames=["scenes/scene-0001 0", "scenes/scene-0001 1"], height=288, width=512, cam_name="FRONT",
                img_type="downsample", frame_idxs=[0], num_scales=4, is_train=False, img_ext=".jpg", load_depth=True, load_mask=True)
    args.update(kw)
    return datasets.nuScenesDataset(**args)


def test_nuscenes_reader_on_the_fixture():
    base = os.path.join(NUSC, "scenes", "scene-0001", "FRONT")
    import json
    cam = json.load(open(os.path.join(base, "rgb", "cam.json")))
    ts = json.load(open(os.path.join(base, "rgb", "ts.json")))
    raw = np.load(os.path.join(base, "depth", "000000.npy"))                       # [col, row, z]
    labels = np.load(os.path.join(base, "mask", "000000.npz"))["motion_label"]
    ds = _nusc_dataset()
    assert ds.full_res_shape == (1600, 900)
    item = ds[0]
    assert tuple(item[("color", 0, 0)].shape) == (3, 288, 512)
    assert item["gt_dim"].tolist() == [900, 1600]

    mot = item["mot_mask"]
    assert mot.dtype == torch.uint8 and tuple(mot.shape) == (900, 1600)
    assert set(torch.unique(mot).tolist()) <= {0, 1, 2, 3}
    assert item["sem_mask"].dtype == torch.uint8 and bool((item["sem_mask"] == 1).all())
    rows, cols = (raw[:, 1] // 5).astype(int), (raw[:, 0] // 5).astype(int)
    assert rows.min() >= 0 and rows.max() < 180 and cols.min() >= 0 and cols.max() < 320
    assert len(set(zip(rows.tolist(), cols.tolist()))) == len(raw) == 3356        # distinct cells: no last-wins ambiguity here
    cells = mot.reshape(180, 5, 320, 5).permute(0, 2, 1, 3).reshape(180, 320, 25)
    assert bool((cells == cells[:, :, :1]).all())                                   # every 5x5 cell is uniform
    grid = cells[:, :, 0].numpy()
    assert np.array_equal(grid[rows, cols], labels)
    occupied = np.zeros((180, 320), dtype=bool)
    occupied[rows, cols] = True
    assert bool((grid[~occupied] == 3).all())

    K = item[("K", 0)].numpy()
    want = np.array(cam["intrinsic_mat"], dtype=np.float32)
    assert np.allclose(K[0, :3], want[0] * 512) and np.allclose(K[1, :3], want[1] * 288) and np.allclose(K[2, :3], want[2])
    assert np.array_equal(ds.get_intrinsic("scenes/scene-0001")[:3, :3], want)

    n = len(raw)
    assert torch.equal(item["depth_gt"][:n], torch.from_numpy(raw[:, [1, 0, 2]].astype(np.float32)))
    assert float(item["depth_valid"].sum()) == n


def test_nuscenes_timestep_and_missing_mask():
    base = os.path.join(NUSC, "scenes", "scene-0001", "FRONT")
    import json
    ts = json.load(open(os.path.join(base, "rgb", "ts.json")))
    ds = _nusc_dataset(frame_idxs=[0, 1], load_depth=False, load_mask=False)
    item = ds[0]
    assert item[("ts", 0)] == 0 and item[("ts", 1)] == ts[0] / 100.0
    assert ds.get_timestep("scenes/scene-0001", 3, -1) == ts[2] / 100.0 and ds.get_timestep("scenes/scene-0001", 1, 2) == (ts[1] + ts[2]) / 100.0
    sem, mot = ds.get_mask("scenes/scene-0001", 1, "l", False)                      # frame 1 has no mask file
    assert sem.shape == mot.shape == (900, 1600) and (sem == 0).all() and (mot == 3).all()
    with open(os.path.join(base, "rgb", "downsample", "000001.jpg"), "rb") as fh:
        assert ds.get_color_bytes("scenes/scene-0001", 1, "l") == fh.read()


def test_scatter_keeps_the_last_point_of_a_cell(tmp_path):
    """Two points in one cell, points outside the image: the later point labels the cell, coordinates are clamped into the grid."""
    import json
    import shutil
    cam_dir = tmp_path / "s" / "FRONT"
    (cam_dir / "rgb").mkdir(parents=True)
    (cam_dir / "depth").mkdir()
    (cam_dir / "mask").mkdir()
    shutil.copy(os.path.join(NUSC, "scenes", "scene-0001", "FRONT", "rgb", "cam.json"), cam_dir / "rgb" / "cam.json")
    json.dump([100, 100], open(cam_dir / "rgb" / "ts.json", "w"))
    pts = np.array([[11.0, 22.0, 5.0], [14.9, 24.9, 6.0], [1700.0, 950.0, 7.0], [-3.0, -2.0, 8.0]])      # [col, row, z]
    np.save(cam_dir / "depth" / "000000.npy", pts)
    np.savez(cam_dir / "mask" / "000000.npz", motion_label=np.array([1, 2, 1, 2], dtype=np.uint8))
    ds = _nusc_dataset(data_path=str(tmp_path), filenames=["s 0"])
    _, mot = ds.get_mask("s", 0, "l", False)
    assert (mot[20:25, 10:15] == 2).all() and (mot[895:, 1595:] == 1).all() and (mot[:5, :5] == 2).all()
    assert int((mot != 3).sum()) == 75


def _current_synthetic_item(index, height, width, frame_idxs, num_scales, load_depth, seed=0):
    """The generator's recipe as it stood before masks were added, restated: load_mask=False must keep producing exactly this."""
    import torch.nn.functional as F
    K0 = np.array([[0.58, 0, 0.5, 0], [0, 1.92, 0.5, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=np.float32)
    gen = torch.Generator().manual_seed(seed * 1000003 + index)
    base = torch.rand(1, 3, height // 8 + 2, width // 8 + 2, generator=gen)
    big = F.interpolate(base, (height + 16, width + 16), mode="bilinear", align_corners=False)[0]
    item = {}
    for f in frame_idxs:
        x0 = 8 + 2 * f
        img = (big[:, 8:8 + height, x0:x0 + width] + 0.05 * torch.rand(3, height, width, generator=gen)).clamp(0, 1).contiguous()
        item[("color", f, 0)] = img
        item[("color_aug", f, 0)] = img
        item[("ts", f)] = 1
    for s in range(num_scales):
        K = K0.copy()
        K[0, :] *= width // (2 ** s)
        K[1, :] *= height // (2 ** s)
        item[("K", s)] = torch.from_numpy(K)
        item[("inv_K", s)] = torch.from_numpy(np.linalg.pinv(K))
    item["gt_dim"] = torch.tensor([height, width]).type(torch.int)
    if load_depth:
        n = 2000
        rows = torch.randint(0, height, (n,), generator=gen).float()
        cols = torch.randint(0, width, (n,), generator=gen).float()
        z = 2 + 40 * torch.rand(n, generator=gen)
        item["depth_gt"] = torch.cat((torch.stack([rows, cols, z], 1), torch.zeros(25000 - n, 3)))
        item["depth_valid"] = torch.cat((torch.ones(n), torch.zeros(25000 - n)))
    item["index"] = index
    return item


def _same(a, b):
    return torch.equal(a, b) if torch.is_tensor(a) else a == b


@pytest.mark.parametrize("load_depth", [False, True])
def test_synthetic_items_are_unchanged_and_masks_come_on_top(load_depth):
    from datasets import SyntheticTriplets
    kw = dict(height=64, width=96, frame_idxs=[0, -1, 1], num_scales=3, load_depth=load_depth, length=8)
    plain, masked = SyntheticTriplets(load_mask=False, **kw), SyntheticTriplets(load_mask=True, **kw)
    assert masked.full_res_shape == (192, 128) and set(masked.categories) == set(range(29))
    for index in (0, 5):
        want = _current_synthetic_item(index, 64, 96, [0, -1, 1], 3, load_depth)
        got, got_m = plain[index], masked[index]
        assert set(got) == set(want) and all(_same(got[k], want[k]) for k in want)
        assert set(got_m) == set(want) | {"mot_mask", "sem_mask"} and all(_same(got_m[k], want[k]) for k in want)
        mot, sem = got_m["mot_mask"], got_m["sem_mask"]
        assert mot.dtype == sem.dtype == torch.uint8 and tuple(mot.shape) == tuple(sem.shape) == (128, 192)
        assert set(torch.unique(mot).tolist()) == {0, 1, 2, 3} and int(sem.max()) < 29
        assert _same(masked[index]["mot_mask"], mot)                                # deterministic per index
    assert not torch.equal(masked[0]["mot_mask"], masked[5]["mot_mask"])
