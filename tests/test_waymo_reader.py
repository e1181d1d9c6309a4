"""The Waymo reader on the tiny_waymo fixture without a GPU: item contract, the motion mask against the frame's panoptic labels (an
independent ground truth for the contour fill), the numpy fill against the brute-force definition of tests/contour_fill_case.py,
the record packer, and the items that must not change."""
import json
import os
import pickle

import numpy as np
import pytest
import torch

import contour_fill_case as cc

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
WAYMO = os.path.join(ROOT, "tests", "golden", "tiny_waymo")
NUSC = os.path.join(ROOT, "tests", "golden", "tiny_nuscenes")
FOLDER = "val/segment-1024360143612057520_3580_000_3600_000"
BASE = os.path.join(WAYMO, FOLDER, "FRONT")
LABEL_COUNTS = {0: 2299491, 1: 66220, 2: 86122, 3: 5767}        # recorded when the definition was checked against the panoptic labels


def waymo_dataset(**kw):
    import datasets
    args = dict(data_path=WAYMO, filenames=[FOLDER + " 1"], height=320, width=480, cam_name="FRONT", img_type="downsample", frame_idxs=[0, -1, 1],
                num_scales=4, is_train=False, img_ext=".jpg", load_depth=True, load_mask=True)
    args.update(kw)
    return datasets.WaymoDataset(**args)


def motion_label(obj):
    if obj["box_label"] is None:
        return 3
    return 1 if np.sqrt(np.sum(np.array(obj["speed"]) ** 2)) > 1.0 else 2


_panoptic = {}


def panoptic_objects():
    """[(motion label, expected object mask (1280, 1920) bool), ...] in the pickle's order, rebuilt from the panoptic labels stored
    beside the contours: `(instance + 1) * (semantic == c) == i` over the sorted classes, i = 1 .. max."""
    if not _panoptic:
        npz = np.load(os.path.join(BASE, "mask", "000001.npz"))
        sem, inst = npz["semantic"].reshape(1280, 1920), npz["instance"].reshape(1280, 1920).astype(np.int64)
        with open(os.path.join(BASE, "mask", "000001.pickle"), "rb") as fh:
            entries = pickle.load(fh)
        masks, k = [], 0
        for c in sorted({obj["mask_label"] for obj in entries}):
            ids = (inst + 1) * (sem == c)
            for i in range(1, int(ids.max()) + 1):
                assert entries[k]["mask_label"] == c
                masks.append((motion_label(entries[k]), ids == i))
                k += 1
        assert k == len(entries) == 65
        _panoptic["objects"], _panoptic["entries"], _panoptic["sem"] = masks, entries, sem
    return _panoptic["objects"]


def panoptic_motion_mask():
    if "mot" not in _panoptic:
        mot = np.zeros((1280, 1920), dtype=np.uint8)
        for label, m in panoptic_objects():
            mot[m] = label
        _panoptic["mot"] = mot
    return _panoptic["mot"]


def fixture_objects():
    panoptic_objects()
    return [(motion_label(obj), [np.asarray(c).reshape(-1, 2) for c in obj["mask"]]) for obj in _panoptic["entries"]]


def test_reader_on_the_fixture():
    cam = json.load(open(os.path.join(BASE, "rgb", "cam.json")))
    raw = np.load(os.path.join(BASE, "depth", "000001.npy"))                        # [col, row, z]
    ds = waymo_dataset()
    assert ds.full_res_shape == (1920, 1280)
    assert sorted(ds.categories) == list(range(29)) and ds.categories[2] == "car" and ds.categories[28] == "static"
    item = ds[0]
    for f in (0, -1, 1):
        assert tuple(item[("color", f, 0)].shape) == (3, 320, 480) and item[("color", f, 0)].dtype == torch.float32
        assert item[("ts", f)] == 1
    assert item["gt_dim"].tolist() == [1280, 1920]
    K = item[("K", 0)].numpy()
    want = np.array(cam["intrinsic_mat"], dtype=np.float32)
    assert np.allclose(K[0, :3], want[0] * 480) and np.allclose(K[1, :3], want[1] * 320) and np.allclose(K[2, :3], want[2])
    assert np.array_equal(ds.get_intrinsic(FOLDER)[:3, :3], want)
    sem, mot = item["sem_mask"], item["mot_mask"]
    assert sem.dtype == mot.dtype == torch.uint8 and tuple(sem.shape) == tuple(mot.shape) == (1280, 1920)
    assert np.array_equal(sem.numpy(), np.load(os.path.join(BASE, "mask", "000001.npz"))["semantic"].reshape(1280, 1920))
    assert "mask_contours" not in item and "mask_vertices" not in item
    n = len(raw)
    assert torch.equal(item["depth_gt"][:n], torch.from_numpy(raw[:, [1, 0, 2]].astype(np.float32)))
    assert float(item["depth_valid"].sum()) == n
    flipped = ds.get_depth(FOLDER, 1, "l", True)
    assert np.array_equal(flipped[:, 1], 1920 - raw[:, 0]) and np.array_equal(flipped[:, [0, 2]], raw[:, [1, 2]])
    with open(os.path.join(BASE, "rgb", "downsample", "000002.jpg"), "rb") as fh:
        assert ds.get_color_bytes(FOLDER, 2, "l") == fh.read()


def test_motion_mask_equals_the_panoptic_labels():
    want = panoptic_motion_mask()
    assert {int(l): int(c) for l, c in zip(*np.unique(want, return_counts=True))} == LABEL_COUNTS
    sem, mot = waymo_dataset().get_mask(FOLDER, 1, "l", False)
    assert mot.dtype == np.uint8 and mot.shape == (1280, 1920)
    assert np.array_equal(mot, want), int((mot != want).sum())
    # ... and object by object
    from hipops import contours
    for (label, contour_list), (want_label, want_mask) in zip(fixture_objects(), panoptic_objects()):
        assert label == want_label
        assert np.array_equal(contours.fill_host([(label, contour_list)], 1280, 1920) == label, want_mask)


def test_masks_are_not_flipped_and_a_missing_file_gives_zeros():
    ds = waymo_dataset()
    a, b = ds.get_mask(FOLDER, 1, "l", False), ds.get_mask(FOLDER, 1, "l", True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    sem, mot = ds.get_mask(FOLDER, 2, "l", False)                                  # frame 2 has no mask files
    assert sem.shape == mot.shape == (1280, 1920) and sem.dtype == mot.dtype == np.uint8 and not sem.any() and not mot.any()


@pytest.mark.parametrize("height,width", cc.CANVASES)
def test_numpy_fill_equals_the_brute_force_definition(height, width):
    from hipops import contours
    for name, objects in cc.cases(height, width).items():
        got = contours.fill_host(objects, height, width, name)
        want = np.array(cc.expected(name, height, width), dtype=np.uint8)
        assert got.dtype == np.uint8 and np.array_equal(got, want), (name, np.argwhere(got != want)[:8])
    assert np.array(cc.expected("ring_hole_island", height, width))[9, width - 70 + 10] == 0           # the hole is a hole ...
    assert np.array(cc.expected("ring_hole_island", height, width))[9, width - 70 + 30] == 3           # ... and the island is filled


def test_packer_round_trip_of_the_fixture():
    from hipops import contours
    objects = fixture_objects()
    vertices, records = contours.pack(objects, 1280, 1920)
    assert vertices.dtype == np.int16 and vertices.shape == (contours.V_CAP, 2)
    assert records.dtype == np.int32 and records.shape == (contours.C_CAP, contours.REC_WORDS)
    used = records[records[:, 1] > 0]
    assert len(used) == 43 and int(used[:, 1].sum()) == 4307 and int(used[:, 1].max()) == 1013 and not records[43:].any()
    assert np.array_equal(used[:, 0], np.cumsum(used[:, 1]) - used[:, 1]) and bool((np.diff(used[:, 2]) >= 0).all())
    assert contours.V_CAP >= 3 * 4307 and contours.C_CAP >= 3 * 43                  # the stated headroom over this frame
    with_contours = [(l, c) for l, c in objects if c]
    assert len(with_contours) == 22 and max(len(c) for _, c in with_contours) == 11
    back = contours.unpack(vertices, records)
    assert len(back) == 22
    for (l0, c0), (l1, c1) in zip(with_contours, back):
        assert l0 == l1 and len(c0) == len(c1) and all(np.array_equal(a, b) for a, b in zip(c0, c1))
    for r in used:                                                                  # the row range the kernel skips by
        ys = vertices[r[0]:r[0] + r[1], 1]
        assert r[4] == ys.min() and r[5] == ys.max()
    assert np.array_equal(contours.fill_host(back, 1280, 1920), panoptic_motion_mask())


def test_packer_refuses_what_has_no_defined_fill():
    from hipops import contours
    with pytest.raises(ValueError, match="frame_7"):
        contours.pack([(1, [[(3, 3), (5, 4), (3, 8)]])], 20, 20, "frame_7")         # a knight's move
    with pytest.raises(ValueError, match="frame_7"):
        contours.fill_host([(1, [[(3, 3), (5, 4), (3, 8)]])], 20, 20, "frame_7")
    for bad in ([(3, 3), (20, 3)], [(3, 3), (3, -1)], [(3, 20)]):
        with pytest.raises(ValueError, match="frame_8"):
            contours.pack([(1, [bad])], 20, 20, "frame_8")
    with pytest.raises(ValueError):
        contours.pack([(0, [[(3, 3)]])], 20, 20)
    with pytest.raises(ValueError):
        contours.pack([(1, [[(3, 3)]])], 20, 40000)                                 # beyond int16 vertices
    with pytest.raises(contours.OverCap):
        contours.pack([(1, [[(3, 3)], [(4, 4)], [(5, 5)]])], 20, 20, v_cap=16, c_cap=2)
    with pytest.raises(contours.OverCap):
        contours.pack([(1, [[(3, 3), (4, 4), (5, 5)]])], 20, 20, v_cap=2, c_cap=2)


def test_device_items_carry_records_and_an_over_cap_sample_travels_filled():
    from hipops import contours
    ds = waymo_dataset(device_preprocess=True, load_depth=False, frame_idxs=[0])
    item = ds[0]
    assert "mot_mask" not in item and item["sem_mask"].dtype == torch.uint8
    assert item["mask_vertices"].dtype == torch.int16 and tuple(item["mask_vertices"].shape) == (contours.V_CAP, 2)
    assert item["mask_contours"].dtype == torch.int32 and tuple(item["mask_contours"].shape) == (contours.C_CAP, contours.REC_WORDS)
    v, r = contours.pack(fixture_objects(), 1280, 1920)
    assert np.array_equal(item["mask_vertices"].numpy(), v) and np.array_equal(item["mask_contours"].numpy(), r)
    batch = ds.collate([ds[0], ds[0]])
    assert tuple(batch["mask_contours"].shape) == (2, contours.C_CAP, contours.REC_WORDS) and "mot_mask" not in batch

    small = waymo_dataset(device_preprocess=True, load_depth=False, frame_idxs=[0])
    small.mask_caps = (4000, 64)                                                     # the frame has 4 307 vertices
    over = small[0]
    assert "mask_contours" not in over and "mask_vertices" not in over
    want = torch.from_numpy(panoptic_motion_mask())
    assert torch.equal(over["mot_mask"], want)
    batch = ds.collate([ds[0], over, ds[0]])                                         # the rest of the batch is filled on the host
    assert "mask_contours" not in batch and "mask_vertices" not in batch
    assert tuple(batch["mot_mask"].shape) == (3, 1280, 1920) and all(torch.equal(m, want) for m in batch["mot_mask"])
    tiny = waymo_dataset(device_preprocess=True, load_depth=False, frame_idxs=[0])
    tiny.mask_caps = (8192, 42)                                                      # ... and 43 contours
    assert "mot_mask" in tiny[0]


def test_items_without_device_masks_are_unchanged(monkeypatch):
    host = waymo_dataset(load_depth=False, frame_idxs=[0])[0]                       # device_preprocess=False
    assert "mot_mask" in host and "mask_contours" not in host
    monkeypatch.setenv("DD_DEVICE_MASKS", "0")
    off = waymo_dataset(device_preprocess=True, load_depth=False, frame_idxs=[0])[0]
    assert "mask_contours" not in off and "mask_vertices" not in off
    assert torch.equal(off["mot_mask"], host["mot_mask"]) and torch.equal(off["sem_mask"], host["sem_mask"])
    monkeypatch.delenv("DD_DEVICE_MASKS")
    # a missing annotation: records without a used slot
    none = waymo_dataset(device_preprocess=True, load_depth=False, frame_idxs=[0], filenames=[FOLDER + " 2"], load_mask=True)
    # frame 2 has no neighbours on disk for a triplet, frame_idxs=[0] reads only itself
    item = none[0]
    assert not item["mask_contours"].any() and not item["sem_mask"].any()

    import datasets
    kw = dict(data_path=NUSC, filenames=["scenes/scene-0001 0"], height=288, width=512, cam_name="FRONT", img_type="downsample", frame_idxs=[0],
              num_scales=4, is_train=False, img_ext=".jpg", load_depth=True, load_mask=True)
    keys = {("K", s) for s in range(4)} | {("inv_K", s) for s in range(4)} | {("ts", 0), "gt_dim", "depth_gt", "depth_valid", "sem_mask", "mot_mask", "index"}
    assert set(datasets.nuScenesDataset(**kw)[0]) == keys | {("color", 0, 0), ("color_aug", 0, 0)}
    assert set(datasets.nuScenesDataset(device_preprocess=True, **kw)[0]) == keys | {"frames_u8", "jitter", "flip"}


def test_synthetic_still_serves_the_waymo_shape():
    import datasets
    from options import DynamoOptions
    opt = DynamoOptions().parse(args=["-d", "waymo", "--synthetic"])
    assert (opt.height, opt.width) == (320, 480)
    item = datasets.SyntheticTriplets(height=opt.height, width=opt.width, load_mask=True, length=2)[1]
    assert tuple(item[("color", 0, 0)].shape) == (3, 320, 480) and tuple(item["mot_mask"].shape) == (640, 960)
    assert not hasattr(datasets.synthetic, "WaymoDataset") and datasets.WaymoDataset.__module__ == "datasets.waymo_dataset"
