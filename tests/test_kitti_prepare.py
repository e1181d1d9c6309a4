"""KITTI preparation on the host (prepare_data/kitti.py, hipops/lidar.py): the numpy definition of the LiDAR depth list
against the reference's own rows (tests/golden/kitti_prepare.npz, written by the unmodified prepare_data/kitti_util.py), the
projection matrix from the calibration texts, and the script's tree walk driven with the host callables.  Equality throughout;
the one slack is projection()'s 1e-12 max|P| for another machine's BLAS.  CPU."""
import os

import numpy as np
import pytest

import kitti_prepare_case as kc
from oracle.ref_resize import resize_bicubic


@pytest.mark.parametrize("cam", kc.CAMS)
@pytest.mark.parametrize("case", kc.CASES)
def test_host_definition_equals_the_reference(golden_dir, case, cam):
    from hipops import lidar
    g = kc.golden(golden_dir)
    H, W = (int(v) for v in g[case + "/HW"])
    want = g["{}/rows{}".format(case, cam)]
    rows, depth = lidar.depth_points_host(g[case + "/points"], g[case + "/P"][kc.CAMS.index(cam)], H, W)
    assert rows.dtype == np.float64 and want.dtype == np.float64 and rows.shape == want.shape
    assert np.array_equal(rows, want)
    assert depth.dtype == np.float32 and depth.shape == (H, W) and int((depth > 0).sum()) == want.shape[0]
    for scan in (g["empty/points_a"], g["empty/points_b"]):
        none, blank = lidar.depth_points_host(scan, g[case + "/P"][kc.CAMS.index(cam)], H, W)
        assert none.dtype == np.float64 and none.shape == g["empty/rows"].shape == (0, 3) and not blank.any()


def test_the_golden_cases_hold_what_they_are_for(golden_dir):
    """The fixture's own claims: shared buckets listed in `dense` and `alias`, bucket -1 in `alias`, four crowded pixels in `ties`."""
    g = kc.golden(golden_dir)
    for case in ("dense", "alias"):
        H, W = (int(v) for v in g[case + "/HW"])
        rows = g[case + "/rows2"]
        shared = np.bincount((rows[:, 0] * (W - 1) + rows[:, 1]).astype(np.int64))
        assert int((shared > 1).sum()) >= 5
    assert g["alias/rows2"][0].tolist() == [0.0, 0.0, 8.0]
    assert g["ties/rows2"][:, :2].tolist() == [[1.0, 1.0], [1.0, 11.0], [7.0, 1.0], [7.0, 11.0]]
    assert g["real_calib/points"].shape[0] > 30000 and g["real_calib/rows2"].shape[0] > 10000


@pytest.mark.parametrize("case", kc.CASES)
def test_projection_reads_the_calibration_texts(golden_dir, tmp_path, case):
    from hipops import lidar
    g = kc.golden(golden_dir)
    for name, key in (("calib_cam_to_cam.txt", "/cam2cam"), ("calib_velo_to_cam.txt", "/velo2cam")):
        (tmp_path / name).write_text(str(g[case + key]))
    for c, cam in enumerate(kc.CAMS):
        P, H, W = lidar.projection(str(tmp_path), cam)
        want = g[case + "/P"][c]
        assert (H, W) == tuple(int(v) for v in g[case + "/HW"])
        assert P.dtype == np.float64 and P.shape == (3, 4)
        assert float(np.abs(P - want).max()) <= 1e-12 * float(np.abs(want).max())


def host_resize(frames, height, width):
    return np.stack([resize_bicubic(f, height, width) for f in frames])


def test_script_prepares_the_layout(golden_dir, tmp_path, capsys):
    from prepare_data import kitti
    g = kc.golden(golden_dir)
    raw, out = str(tmp_path / "raw"), str(tmp_path / "out")
    scans = kc.write_raw_tree(raw, g)
    kw = dict(height=kc.OUT_H, width=kc.OUT_W, batch=2, num_workers=3, depth_rows=kitti.host_depth_rows, resize=host_resize)
    kitti.prepare(raw, out, **kw)
    kc.check_tree(raw, out, scans, g, capsys.readouterr().out)
    kc.check_reader(out, scans, g)
    jpgs = [os.path.join(out, kc.DATE, kc.DRIVE, cam, "rgb", "downsample", n + ".jpg") for cam in ("image_02", "image_03") for n in kc.FRAMES]
    npy = os.path.join(out, kc.DATE, kc.DRIVE, "image_02", "depth", "0000000000.npy")
    before = [os.stat(p).st_mtime_ns for p in jpgs]
    np.save(npy, np.zeros((1, 3)))                                  # the depth lists are always rewritten ...
    kitti.prepare(raw, out, **dict(kw, resize=None))                # ... and no frame reaches the resize
    assert [os.stat(p).st_mtime_ns for p in jpgs] == before
    kc.check_tree(raw, out, scans, g, capsys.readouterr().out)


def test_script_flags_and_odd_frames(golden_dir, tmp_path, capsys):
    """--skip_rgb / --skip_depth, dates that do not start with 2011, and a PNG that is not 8-bit RGB (Pillow's own line on the host)."""
    from PIL import Image
    from prepare_data import kitti
    g = kc.golden(golden_dir)
    raw, out = str(tmp_path / "raw"), str(tmp_path / "out")
    kc.write_raw_tree(raw, g)
    os.makedirs(os.path.join(raw, "2012_01_01", "2012_01_01_drive_0001_sync"))
    gray = os.path.join(raw, kc.DATE, kc.DRIVE, "image_03", "data", "0000000002.png")
    Image.open(gray).convert("L").save(gray)
    drive = os.path.join(out, kc.DATE, kc.DRIVE)

    def nothing(*args):
        raise AssertionError("a skipped step ran")

    kitti.prepare(raw, out, height=kc.OUT_H, width=kc.OUT_W, skip_depth=True, depth_rows=nothing, resize=host_resize)
    assert os.listdir(out) == [kc.DATE] and os.listdir(os.path.join(drive, "image_02", "depth")) == []
    for cam in ("image_02", "image_03"):
        for name in kc.FRAMES:
            with open(os.path.join(drive, cam, "rgb", "downsample", name + ".jpg"), "rb") as fh:
                assert fh.read() == kc.pillow_line(os.path.join(raw, kc.DATE, kc.DRIVE, cam, "data", name + ".png"), kc.OUT_H, kc.OUT_W)
    out2 = str(tmp_path / "out2")
    kitti.prepare(raw, out2, skip_rgb=True, depth_rows=kitti.host_depth_rows, resize=nothing)
    drive2 = os.path.join(out2, kc.DATE, kc.DRIVE)
    assert os.listdir(os.path.join(drive2, "image_02", "rgb", "original")) == [] and len(os.listdir(os.path.join(drive2, "image_03", "depth"))) == 2
    assert capsys.readouterr().out.count("Not Found - Skipped") == 2


def test_thread_pool_is_capped(monkeypatch, tmp_path):
    from prepare_data import kitti
    seen = []

    class Pool(kitti.ThreadPoolExecutor):
        def __init__(self, max_workers=None):
            seen.append(max_workers)
            super().__init__(max_workers=max_workers)

    monkeypatch.setattr(kitti, "ThreadPoolExecutor", Pool)
    os.makedirs(str(tmp_path / "raw"))
    for asked in (0, 8, 500):
        kitti.prepare(str(tmp_path / "raw"), str(tmp_path / "out"), num_workers=asked)
    assert seen == [1, 8, 16]


def test_abi_lists_the_lidar_entry_points():
    import ctypes

    from hipops import abi, lib
    assert abi.DD_ABI_VERSION == 2
    assert "dd_lidar_depth_points" in abi.EXPORTED and "dd_lidar_depth_points_workspace_bytes" in abi.EXPORTED
    lib.build()
    so = ctypes.CDLL(lib.LIB_PATH)
    assert "dd_lidar_depth_points" in abi.declare(so) and "dd_lidar_depth_points_workspace_bytes" in abi.declare(so)
    # sized on the host: per job last[HW] + 3 x bucket[H (W - 1) + 1] + value[HW] + one count per 256 pixels, 4 bytes each; 16 scans at a time
    assert so.dd_lidar_depth_points_workspace_bytes(1, 2, 8, 6) == 2 * (2 * 48 + 3 * 41 + 1) * 4
    assert so.dd_lidar_depth_points_workspace_bytes(40, 2, 375, 1242) == 32 * (2 * 465750 + 3 * 465376 + 1820) * 4
    for bad in ((0, 2, 8, 6), (1, 0, 8, 6), (1, 2, 0, 6), (1, 2, 8, 1), (1, 2, 65536, 32768)):
        assert so.dd_lidar_depth_points_workspace_bytes(*bad) == 0
