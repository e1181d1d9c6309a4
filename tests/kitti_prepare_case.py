"""Shared by tests/test_kitti_prepare.py (host callables) and tests/test_lidar_depth_gpu.py (the device path): the golden cases of
tests/golden/kitti_prepare.npz, a generated raw KITTI tree, and what prepare_data/kitti.py has to make of it."""
import io
import os

import numpy as np
from PIL import Image

CASES = ("real_calib", "dense", "alias", "ties")
CAMS = (2, 3)
DATE, DRIVE = "2011_09_26", "2011_09_26_drive_0001_sync"
FRAMES = ("0000000000", "0000000001", "0000000002")
NO_SCAN = "0000000001"                                              # the frame without a .bin
SRC_H, SRC_W, OUT_H, OUT_W = 62, 200, 31, 100

_golden = {}


def golden(golden_dir):
    """The npz as a dict, loaded once and shared read-only."""
    if not _golden:
        with np.load(os.path.join(golden_dir, "kitti_prepare.npz")) as z:
            for k in z.files:
                v = z[k]
                v.setflags(write=False)
                _golden[k] = v
    return _golden


def write_raw_tree(root, g):
    """One date, one drive, three 62x200 RGB frames per camera, `dense`'s calibration (24x40) and two scans cut from its points."""
    date_dir = os.path.join(root, DATE)
    drive_dir = os.path.join(date_dir, DRIVE)
    os.makedirs(os.path.join(drive_dir, "velodyne_points", "data"))
    for name, key in (("calib_cam_to_cam.txt", "dense/cam2cam"), ("calib_velo_to_cam.txt", "dense/velo2cam")):
        with open(os.path.join(date_dir, name), "w") as fh:
            fh.write(str(g[key]))
    with open(os.path.join(date_dir, "calib_imu_to_velo.txt"), "w") as fh:
        fh.write("calib_time: 25-May-2012 16:47:16\nR: 1 0 0 0 1 0 0 0 1\nT: 0 0 0\n")
    rng = np.random.default_rng(62200)
    for cam in ("image_02", "image_03"):
        os.makedirs(os.path.join(drive_dir, cam, "data"))
        for name in FRAMES:
            yy, xx = np.mgrid[0:SRC_H, 0:SRC_W]
            img = np.stack([xx * 255 // SRC_W, yy * 255 // SRC_H, (xx + yy) % 256], axis=-1) + rng.integers(-20, 21, (SRC_H, SRC_W, 3))
            Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(os.path.join(drive_dir, cam, "data", name + ".png"))
    pts = g["dense/points"]
    scans = {"0000000000": pts[:3500], "0000000002": pts[2500:]}
    for name, scan in scans.items():
        np.ascontiguousarray(scan).tofile(os.path.join(drive_dir, "velodyne_points", "data", name + ".bin"))
    return scans


def pillow_line(png, height, width):
    """The bytes `Image.open(png).resize((width, height)).save(jpg)` writes (reference prepare_data/kitti.py:101-102)."""
    buf = io.BytesIO()
    Image.open(png).resize((width, height)).save(buf, format="JPEG")
    return buf.getvalue()


def check_tree(raw, out, scans, g, printed):
    """The prepared tree against the raw one, file by file."""
    from hipops import lidar
    raw_date, out_drive = os.path.join(raw, DATE), os.path.join(out, DATE, DRIVE)
    for txt in ("calib_cam_to_cam.txt", "calib_velo_to_cam.txt", "calib_imu_to_velo.txt"):
        path = os.path.join(out_drive, txt)
        assert os.path.islink(path) and os.path.realpath(path) == os.path.realpath(os.path.join(raw_date, txt)), txt
    H, W = (int(v) for v in g["dense/HW"])
    for c, cam in enumerate(("image_02", "image_03")):
        for name in FRAMES:
            png = os.path.join(raw_date, DRIVE, cam, "data", name + ".png")
            link = os.path.join(out_drive, cam, "rgb", "original", name + ".png")
            assert os.path.islink(link) and os.path.realpath(link) == os.path.realpath(png), link
            with open(os.path.join(out_drive, cam, "rgb", "downsample", name + ".jpg"), "rb") as fh:
                assert fh.read() == pillow_line(png, OUT_H, OUT_W), (cam, name)
            npy = os.path.join(out_drive, cam, "depth", name + ".npy")
            if name == NO_SCAN:
                assert not os.path.exists(npy)
                continue
            got = np.load(npy)
            want, _ = lidar.depth_points_host(scans[name], g["dense/P"][c], H, W)
            assert want.shape[0] > 100
            assert got.dtype == np.float64 and got.shape == want.shape and np.array_equal(got, want), (cam, name)
        assert sorted(os.listdir(os.path.join(out_drive, cam, "depth"))) == sorted(n + ".npy" for n in FRAMES if n != NO_SCAN)
    missing = os.path.join(raw_date, DRIVE, "velodyne_points", "data", NO_SCAN + ".bin")
    assert printed.count("Depth Data {} Not Found - Skipped".format(missing)) == 2, printed


def check_reader(out, scans, g):
    """datasets.KITTIDataset reads the prepared tree."""
    from datasets import KITTIDataset
    from hipops import lidar
    folder = "{}/{}".format(DATE, DRIVE)
    ds = KITTIDataset(data_path=out, filenames=["{} 0 l".format(folder)], cam_name="image_02", img_type="downsample", frame_idxs=[0], num_scales=1,
                      is_train=False, img_ext=".jpg", height=OUT_H, width=OUT_W)
    H, W = (int(v) for v in g["dense/HW"])
    assert ds.get_gt_dim(folder, 0, "l") == (H, W)
    for c, side in enumerate(("l", "r")):
        want, _ = lidar.depth_points_host(scans["0000000002"], g["dense/P"][c], H, W)
        assert np.array_equal(ds.get_depth(folder, 2, side, False), want)
        img = ds.get_color(folder, 2, side, False)
        assert img.size == (OUT_W, OUT_H) and img.mode == "RGB"
