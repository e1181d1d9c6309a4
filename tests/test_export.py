"""Depth export on the host: the numpy definition of csrc/dd_export.hip (hipops/export.py) against a float64 evaluation of the same
formulas, the flip post-processing, the 16-bit quantisation at its edges, the folder reader, and the 16-bit PNG round trip.
No GPU."""
import os
import shutil

import numpy as np
import pytest
from PIL import Image

import export_case as EC

GOLDEN_FRAMES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tiny_kitti_jpeg")


# ---- the definition ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("shape", EC.SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_host_definition_against_float64(shape, flip):
    """export_depth_host is the fp32 evaluation; the same formulas in float64 on the same fp32 inputs and constants differ from it by
    fp32 rounding alone.  The bound is derived in export_case.depth64 / depth_bound: 3 EPS (w dx + h dy) from the rounded source
    coordinate (in_size * 2**-23 in the tap weight times the tap difference, as far as three roundings go), 8 EPS S for the taps and
    the blend, the fuse step's 17 EPS D per tap scaled by span, then the division's relative EPS.  Where a NaN tap reaches an output
    pixel both evaluations are NaN."""
    from hipops.export import export_depth_host
    B, h, w, H, W = shape
    disp, flipped = EC.disparities(B, h, w)
    got = export_depth_host(disp, H, W, disp_flipped=flipped if flip else None, min_depth=EC.MIN_DEPTH, max_depth=EC.MAX_DEPTH, want=("depth",))["depth"]
    assert got.dtype == np.float32 and got.shape == (B, H, W)
    with np.errstate(all="ignore"):
        want, u, u_bound = EC.depth64(disp, H, W, flipped if flip else None)
        tol = EC.depth_bound(want, u, u_bound)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan) and not nan.all()
    err = np.abs(got.astype(np.float64) - want)
    print("shape {} flip {}: worst error {:.3e}, worst error / bound {:.3f}".format(shape, flip, np.nanmax(err), np.nanmax(err / tol)))
    assert (err[~nan] <= tol[~nan]).all(), (np.nanmax(err / tol))
    assert np.nanmedian(tol / np.abs(want)) < 1e-4                 # a rounding bound: the typical pixel is held to a few 1e-6 of its value


def test_definition_differs_from_a_wrong_one():
    """The bound separates the definition from its nearest wrong neighbour: align_corners=True taps."""
    from hipops.export import export_depth_host
    B, h, w, H, W = EC.SHAPES[4]
    disp, _ = EC.disparities(B, h, w, values=False)
    got = export_depth_host(disp, H, W, min_depth=EC.MIN_DEPTH, max_depth=EC.MAX_DEPTH, want=("depth",))["depth"]
    want, u, u_bound = EC.depth64(disp, H, W)
    wrong = 1.0 / EC.blend64(0.01 + 9.99 * disp.astype(np.float64), H, W + 1)[:, :, :W]
    assert (np.abs(got - want) <= EC.depth_bound(want, u, u_bound)).all()
    assert (np.abs(got - wrong) > EC.depth_bound(want, u, u_bound)).mean() > 0.5


@pytest.mark.parametrize("shape", EC.SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_post_processing_against_float64(shape):
    """The fuse step alone, fp32 against the float64 transcription in the pinned order: export_case.fuse_bound."""
    from hipops.export import fuse_host
    B, h, w, _, _ = shape
    disp, flipped = EC.disparities(B, h, w, values=False)
    got, want, tol = fuse_host(disp, flipped), EC.fuse64(disp, flipped), EC.fuse_bound(disp, flipped)
    assert got.dtype == np.float32
    assert (np.abs(got - want) <= tol).all(), np.max(np.abs(got - want) / tol)
    # the plain mean where neither mask reaches, the left image's own value at the left border of the fused map, the mirrored one's at the right
    from hipops.export import l_mask_table
    lm = l_mask_table(w)
    rm = lm[::-1]
    mean = 0.5 * (disp.astype(np.float64) + flipped.astype(np.float64)[:, :, ::-1])
    inner = (lm == 0) & (rm == 0)
    assert np.allclose(got[:, :, inner], mean[:, :, inner], rtol=4 * EC.EPS, atol=0)
    if w >= 20:
        assert inner.any() and lm[0] == 1 and rm[-1] == 1 and rm[0] == 0
        assert np.array_equal(got[:, :, 0], flipped[:, :, -1]) and np.array_equal(got[:, :, -1], disp[:, :, -1])


@pytest.mark.parametrize("shape", EC.SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_symmetric_pair_fuses_to_itself(shape):
    """disp_flipped == flip(disp): l == r, so m == l exactly, and wherever lm + rm is 0 or 1 the fused value is l bit for bit."""
    from hipops.export import export_depth_host, fuse_host, l_mask_table
    B, h, w, H, W = shape
    disp, _ = EC.disparities(B, h, w, values=False)
    mirror = np.ascontiguousarray(disp[:, :, ::-1])
    lm = l_mask_table(w)
    total = lm + lm[::-1]
    exact = (total == 0) | (total == 1)
    fused = fuse_host(disp, mirror)
    assert np.array_equal(fused[:, :, exact], disp[:, :, exact])
    if w >= 3:
        assert exact.any()
    if exact.all():
        a = export_depth_host(disp, H, W, disp_flipped=mirror, min_depth=EC.MIN_DEPTH, max_depth=EC.MAX_DEPTH)
        b = export_depth_host(disp, H, W, min_depth=EC.MIN_DEPTH, max_depth=EC.MAX_DEPTH)
        assert all(np.array_equal(a[k], b[k]) for k in a)


# ---- quantisation ----------------------------------------------------------------------------------------------------------------
def _same_size(values, **kwargs):
    """Same-size export of a (1, 1, n) map: every weight is 0, the value passes through the blend unchanged."""
    from hipops.export import export_depth_host
    v = np.asarray(values, dtype=np.float32).reshape(1, 1, -1)
    kwargs.setdefault("min_depth", EC.MIN_DEPTH)
    kwargs.setdefault("max_depth", EC.MAX_DEPTH)
    return {k: o[0, 0] for k, o in export_depth_host(v, 1, v.shape[2], **kwargs).items()}


def test_ties_round_to_even():
    cases = EC.ties()
    ks = np.array([k for _, k in cases])
    assert (ks % 2 == 0).sum() >= 6 and (ks % 2 == 1).sum() >= 6
    out = _same_size([d for d, _ in cases])
    assert np.array_equal(out["depth"].astype(np.float64) * 256.0, ks + 0.5)            # exact ties, as constructed
    assert np.array_equal(out["depth16"], np.where(ks % 2 == 0, ks, ks + 1))
    assert (out["depth16"] % 2 == 0).all()


def test_disparity_bounds_give_the_depth_bounds():
    """disp 0 -> s = lo, disp 1 -> s = lo + span: two roundings in s and the division's, 3 EPS relative; 4 for the second order."""
    out = _same_size([0.0, 1.0])
    for got, want in zip(out["depth"], (EC.MAX_DEPTH, EC.MIN_DEPTH)):
        assert abs(float(got) - want) <= 4 * EC.EPS * want, (got, want)
    assert out["depth16"].tolist() == [25600, 26]                                     # 100 * 256 and rint(25.6)
    from hipops.vis import cmap_bytes
    assert np.array_equal(out["rgb"], cmap_bytes("plasma")[[0, 255]])


def test_nan_negative_and_saturation():
    out = _same_size([np.nan, 0.5])                         # the NaN is the first element: nobody else's right-hand tap (0 * NaN is NaN)
    assert np.isnan(out["depth"][0]) and out["depth16"][0] == 0 and out["rgb"][0].tolist() == [0, 0, 0]
    assert np.isfinite(out["depth"][1]) and out["depth16"][1] > 0 and out["rgb"][1].any()
    neg = _same_size([0.25, 0.0], depth_scale=-256.0)
    assert neg["depth16"].tolist() == [0, 0] and (neg["depth"] > 0).all()
    sat = _same_size([0.0, 0.0005, 1.0], depth_scale=1000.0)
    assert sat["depth"][0] * 1000.0 > 65535 and sat["depth16"].tolist()[0] == 65535 and sat["depth16"][1] == 65535 and sat["depth16"][2] == 100
    inf = _same_size([-0.01 / 9.99, 0.5])                    # s == 0 within rounding: a huge or infinite depth saturates
    assert inf["depth16"][0] in (0, 65535) and (not np.isfinite(inf["depth"][0]) or abs(inf["depth"][0]) > 1e6)


def test_plane_bytes():
    from hipops.export import export_plane_u8_host
    v = np.array([[[-0.5, 0.0, 0.2, 0.999, 1.0, 7.0, np.nan]]], dtype=np.float32)
    got = export_plane_u8_host(v[:, :, :6], 1, 6)[0, 0]
    assert got.tolist() == [0, 0, 51, 254, 255, 255] and got.dtype == np.uint8
    assert export_plane_u8_host(v, 1, 7)[0, 0, 6] == 0      # fmaxf(NaN, 0) == 0
    up = export_plane_u8_host(np.array([[[0.0, 1.0]]], dtype=np.float32), 3, 8)
    assert up.shape == (1, 3, 8) and (np.diff(up[0, 0].astype(int)) >= 0).all() and up[0, 0, 0] == 0 and up[0, 0, -1] == 255


def test_sixteen_bit_png_round_trip(tmp_path):
    """Every 16-bit value survives Image.fromarray(...).save(...png) and Image.open: mode I;16."""
    values = np.arange(65536, dtype=np.uint16).reshape(256, 256)
    path = str(tmp_path / "all.png")
    Image.fromarray(values).save(path)
    with Image.open(path) as img:
        assert img.mode == "I;16" and img.size == (256, 256)
        assert np.array_equal(np.asarray(img, dtype=np.uint16), values)
    from hipops.export import export_depth_host
    disp, _ = EC.disparities(1, 9, 16)
    d16 = export_depth_host(disp, 21, 33, min_depth=EC.MIN_DEPTH, max_depth=EC.MAX_DEPTH, want=("depth16",))["depth16"][0]
    Image.fromarray(d16).save(path)
    with Image.open(path) as img:
        assert np.array_equal(np.asarray(img, dtype=np.uint16), d16)


# ---- the reader -----------------------------------------------------------------------------------------------------------------
def _dataset(folder, **kwargs):
    from datasets.folder_dataset import FolderDataset
    kwargs.setdefault("frame_idxs", [0])
    return FolderDataset(folder, None, height=64, width=96, cam_name=None, img_type=None, num_scales=3, is_train=False, path=True, **kwargs)


def test_folder_dataset_items():
    import torch
    ds = _dataset(GOLDEN_FRAMES)
    names = sorted(os.listdir(GOLDEN_FRAMES))
    assert ds.frames == names and len(ds) == 6 == len(names)
    assert ds.filenames[4] == "{} 4".format(GOLDEN_FRAMES)
    for i in (0, 5):
        item = ds[i]
        assert item["paths"] == os.path.splitext(names[i])[0] and item["index"] == i
        assert item["gt_dim"].tolist() == [192, 640] and item["gt_dim"].dtype == torch.int32
        assert {("color", 0, 0), ("color_aug", 0, 0), ("K", 0), ("inv_K", 2), ("ts", 0), "gt_dim", "paths", "index"} <= set(item)
        assert "depth_gt" not in item and "mot_mask" not in item
        color = item[("color", 0, 0)]
        assert color.shape == (3, 64, 96) and color.dtype == torch.float32
        with Image.open(os.path.join(GOLDEN_FRAMES, names[i])) as img:
            want = np.asarray(img.convert("RGB").resize((96, 64), Image.BICUBIC), dtype=np.uint8)
        assert np.array_equal((color * 255).round().to(torch.uint8).permute(1, 2, 0).numpy(), want)
    # KITTI's intrinsics by default, scaled to the network resolution; --intrinsics normalised by the frame's own size
    assert np.allclose(ds[0][("K", 0)].numpy()[:2, :3], [[0.58 * 96, 0, 48], [0, 1.92 * 64, 32]])
    own = _dataset(GOLDEN_FRAMES, intrinsics=(320.0, 96.0, 160.0, 48.0))
    assert np.allclose(own[0][("K", 0)].numpy()[:2, :3], [[0.5 * 96, 0, 0.25 * 96], [0, 0.5 * 64, 0.25 * 64]])
    # the triplet of an interior frame goes by position in the sorted list
    tri = _dataset(GOLDEN_FRAMES, frame_idxs=[0, -1, 1])
    from datasets.folder_dataset import sample_lines
    tri.filenames = sample_lines(GOLDEN_FRAMES, [1])
    item = tri[0]
    assert item["paths"] == "image_02_1" and torch.equal(item[("color", -1, 0)], ds[0][("color", 0, 0)]) and torch.equal(item[("color", 1, 0)], ds[2][("color", 0, 0)])


def test_folder_dataset_mixed_folder(tmp_path):
    import torch
    names = sorted(os.listdir(GOLDEN_FRAMES))[:3]
    for n in names[:2]:
        shutil.copy(os.path.join(GOLDEN_FRAMES, n), str(tmp_path / n))
    with Image.open(os.path.join(GOLDEN_FRAMES, names[2])) as img:
        img.convert("RGB").resize((50, 30)).save(str(tmp_path / "image_02_1b.png"))            # another size, another format, sorts in between
    (tmp_path / "notes.txt").write_text("not a frame")
    ds = _dataset(str(tmp_path))
    assert ds.frames == [names[0], names[1], "image_02_1b.png"] == sorted(ds.frames) and len(ds) == 3
    assert [ds[i]["gt_dim"].tolist() for i in range(3)] == [[192, 640], [192, 640], [30, 50]]
    item = ds[2]
    assert item["paths"] == "image_02_1b"
    with Image.open(str(tmp_path / "image_02_1b.png")) as img:
        want = np.asarray(img.convert("RGB").resize((96, 64), Image.BICUBIC), dtype=np.uint8)
    assert np.array_equal((item[("color", 0, 0)] * 255).round().to(torch.uint8).permute(1, 2, 0).numpy(), want)
    # the compressed-frame path takes the JPEGs and hands the PNG to the host
    dev = _dataset(str(tmp_path), device_preprocess=True, device_decode=True)
    assert dev.device_decode and "jpeg_bytes" in dev[0] and "frames_u8" in dev[2]
    assert np.array_equal(dev[2]["frames_u8"][0].numpy(), want)
    batch = dev.collate([dev[0], dev[2]])
    assert "frames_u8" in batch and "jpeg_bytes" not in batch and batch["paths"] == [os.path.splitext(names[0])[0], "image_02_1b"]
    with pytest.raises(FileNotFoundError):
        _dataset(str(tmp_path / "nothing"))
