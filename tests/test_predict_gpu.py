"""predict.py end to end on the six golden frames with untrained networks: the files it writes against the host definition of the
export (hipops/export.py) applied to the disparities predict_batch returned in that very run."""
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

FRAMES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tiny_kitti_jpeg")
STEMS = sorted(os.path.splitext(f)[0] for f in os.listdir(FRAMES))
H, W = 192, 640                      # the golden frames' own size
NET = ["--weights_init", "scratch", "--depth_model", "litemono", "--height", "64", "--width", "96", "--num_workers", "0"]


def _run(tmp_path, monkeypatch, extra):
    """predict.main over the golden frames -> (written paths, out dir, {stem: predict_batch's tensors for that frame, on the host})."""
    import predict
    seen = {}
    inner = predict.predict_batch

    def recording(opt, trainer, inputs, **kwargs):
        res = inner(opt, trainer, inputs, **kwargs)
        for b, stem in enumerate(inputs["paths"]):
            seen[stem] = {k: v[b].float().cpu().numpy() for k, v in res.items()}
        recording.batches += 1
        return res

    recording.batches = 0
    monkeypatch.setattr(predict, "predict_batch", recording)
    out = str(tmp_path / "out")
    torch.manual_seed(0)
    written = predict.main([FRAMES] + NET + ["--log_dir", str(tmp_path / "logs"), "--out", out] + extra)
    return written, out, seen, recording.batches


def _png(path):
    with Image.open(path) as img:
        return img.mode, np.asarray(img).copy()


def test_default_mode(tmp_path, monkeypatch):
    from hipops.export import export_depth_host
    written, out, seen, batches = _run(tmp_path, monkeypatch, ["-b", "2", "--save", "depth16", "npy", "color"])
    assert batches == 3 and sorted(seen) == STEMS and len(STEMS) == 6
    assert sorted(os.listdir(out)) == ["color", "depth", "depth_npy", "predict.json"]
    assert sorted(written) == sorted([os.path.join(out, d, s + e) for s in STEMS for d, e in (("depth", ".png"), ("depth_npy", ".npy"), ("color", ".png"))]
                                     + [os.path.join(out, "predict.json")])
    for stem in STEMS:
        disp = seen[stem]["disp"]
        assert disp.shape == (1, 64, 96) and set(seen[stem]) == {"disp"}
        want = export_depth_host(disp, H, W, min_depth=0.1, max_depth=100.0)
        mode, d16 = _png(os.path.join(out, "depth", stem + ".png"))
        assert mode == "I;16" and d16.shape == (H, W) and np.array_equal(d16.astype(np.uint16), want["depth16"][0])
        npy = np.load(os.path.join(out, "depth_npy", stem + ".npy"))
        assert npy.dtype == np.float32 and npy.shape == (H, W) and np.array_equal(npy, want["depth"][0])
        mode, rgb = _png(os.path.join(out, "color", stem + ".png"))
        assert mode == "RGB" and rgb.shape == (H, W, 3) and np.array_equal(rgb, want["rgb"][0])
        assert 0 < d16.min() and d16.max() < 65535 and len(np.unique(npy)) > 1       # (an untrained network's depth hardly moves: one 16-bit level)
    meta = json.load(open(os.path.join(out, "predict.json")))
    assert (meta["min_depth"], meta["max_depth"], meta["depth_scale"], meta["height"], meta["width"]) == (0.1, 100.0, 256.0, 64, 96)
    assert "up to scale" in meta["note"]


def test_post_processing(tmp_path, monkeypatch):
    from hipops.export import export_depth_host, l_mask_table
    written, out, seen, batches = _run(tmp_path, monkeypatch, ["-b", "4", "--save", "depth16", "npy", "--post_process", "--depth_scale", "50000"])   # a scale at which
    # the untrained network's nearly constant depth (about 0.2) spreads over many 16-bit levels
    assert batches == 2 and sorted(seen) == STEMS
    lm = l_mask_table(96)
    inner = (lm == 0) & (lm[::-1] == 0)
    assert inner.sum() == 76                # columns 10 .. 85 of 96
    for stem in STEMS:
        l, r = seen[stem]["disp"], seen[stem]["disp_flipped"]
        assert r.shape == l.shape == (1, 64, 96) and not np.array_equal(l, r[:, :, ::-1])
        want = export_depth_host(l, H, W, disp_flipped=r, min_depth=0.1, max_depth=100.0, depth_scale=50000.0)
        npy = np.load(os.path.join(out, "depth_npy", stem + ".npy"))
        assert np.array_equal(npy, want["depth"][0])
        d16 = _png(os.path.join(out, "depth", stem + ".png"))[1].astype(np.uint16)
        assert np.array_equal(d16, want["depth16"][0]) and len(np.unique(d16)) > 4 and d16.max() < 65535
        # where neither border mask reaches a tap, the fused disparity is the plain mean of the two passes: the output columns whose taps
        # all lie inside that band carry exactly the depth of the mean
        mean = (np.float32(0.5) * (l + r[:, :, ::-1])).astype(np.float32)
        of_mean = export_depth_host(mean, H, W, min_depth=0.1, max_depth=100.0, want=("depth",))["depth"][0]
        cols = np.arange(W)
        src = np.maximum((96 / W) * (cols + 0.5) - 0.5, 0)
        band = inner[np.floor(src).astype(int)] & inner[np.minimum(np.floor(src).astype(int) + 1, 95)] & (np.abs(src - np.round(src)) > 1e-3)
        assert band.sum() > W // 2 and np.array_equal(npy[:, band], of_mean[:, band])
        assert not np.array_equal(npy, of_mean)                                    # the borders differ from the mean


def test_motion_mode(tmp_path, monkeypatch):
    from hipops.export import export_depth_host, export_plane_u8_host
    import shutil
    frames = tmp_path / "frames"
    frames.mkdir()
    for stem in STEMS[:3]:
        shutil.copy(os.path.join(FRAMES, stem + ".jpg"), str(frames / (stem + ".jpg")))
    import predict
    seen = {}
    inner = predict.predict_batch

    def recording(opt, trainer, inputs, **kwargs):
        res = inner(opt, trainer, inputs, **kwargs)
        seen.update({stem: {k: v[b].float().cpu().numpy() for k, v in res.items()} for b, stem in enumerate(inputs["paths"])})
        return res

    monkeypatch.setattr(predict, "predict_batch", recording)
    out = str(tmp_path / "out")
    torch.manual_seed(0)
    written = predict.main([str(frames)] + NET + ["--log_dir", str(tmp_path / "logs"), "--out", out, "-b", "2", "--motion"])
    stem = STEMS[1]
    assert list(seen) == [stem] and stem == "image_02_1"
    assert sorted(os.listdir(out)) == ["depth", "motion_mask", "poses.txt", "predict.json"]
    assert os.listdir(os.path.join(out, "depth")) == [stem + ".png"] == os.listdir(os.path.join(out, "motion_mask")) and len(written) == 4
    mask = seen[stem]["motion_mask"]
    assert mask.shape == (1, 64, 96)
    mode, got = _png(os.path.join(out, "motion_mask", stem + ".png"))
    assert mode == "L" and got.shape == (H, W) and np.array_equal(got, export_plane_u8_host(mask, H, W)[0])
    d16 = _png(os.path.join(out, "depth", stem + ".png"))[1].astype(np.uint16)
    assert np.array_equal(d16, export_depth_host(seen[stem]["disp"], H, W, min_depth=0.1, max_depth=100.0, want=("depth16",))["depth16"][0])
    lines = open(os.path.join(out, "poses.txt")).read().splitlines()
    assert len(lines) == 1
    fields = lines[0].split()
    assert len(fields) == 17 and fields[0] == stem
    T = np.array([float(v) for v in fields[1:]]).reshape(4, 4)
    assert T[3].tolist() == [0, 0, 0, 1] and np.allclose(T, seen[stem]["cam_T_cam"], rtol=1e-7, atol=1e-9)
    assert np.allclose(T[:3, :3] @ T[:3, :3].T, np.eye(3), atol=1e-5)
