"""nuScenes preparation on the host (prepare_data/nuScenes.py, prepare_data/nuscenes_tables.py, hipops/resize.py, hipops/lidar.py;
DESIGN 4.22): the area-weighted down-sample against the reference's own down-samples (tests/golden/nuscenes_prepare, written by the
unmodified prepare_data/nuScenes.py), the weight tables, the pose chain against the composed 4x4 matrices and on the mask's
thresholds, the formats of the reference's output files, the box fit's rules, and the script's walk over a generated raw tree with
the host callables.  CPU."""
import io
import json
import os
import os.path as osp

import numpy as np
import pytest
from PIL import Image

import nuscenes_prepare_case as nc

GOLDEN = "nuscenes_prepare"
ROUNDTRIP_MARGIN = 1.05


def _mean_abs(a, b):
    return float(np.abs(a.astype(np.float64) - b.astype(np.float64)).mean())


@pytest.mark.parametrize("frame", (0, 1, 2))
def test_area_definition_is_the_reference_downsample(golden_dir, frame):
    """The reference's down-sample is cv2.resize(INTER_AREA) saved as a JPEG at quality 95, so its decoded pixels carry JPEG noise.
    Measured on the three frames of scene-0001 (1600x900 -> 512x288), mean absolute difference to the decoded down-sample:
    resize_area_host 1.388 / 1.376 / 1.380, Pillow BOX 1.751 / 1.734 / 1.735, Pillow BILINEAR 1.589 / 1.570 / 1.574; the JPEG
    round trip of resize_area_host's own result (Pillow, quality 95) costs 1.388 / 1.376 / 1.380 -- and decodes to the very pixels of
    the reference's file (difference 0), which is asserted too.  The bound is that round-trip noise times 1.05: room for another
    JPEG encoder's rounding, none for another filter (BILINEAR is 14 % off, BOX 26 %)."""
    from hipops import resize
    g = osp.join(golden_dir, GOLDEN)
    with Image.open(osp.join(g, "original", "{:06}.jpg".format(frame))) as img:
        original = np.asarray(img.convert("RGB"))
    with Image.open(osp.join(g, "downsample", "{:06}.jpg".format(frame))) as img:
        want = np.asarray(img.convert("RGB"))
    h, w = int(original.shape[0] / 3.125), int(original.shape[1] / 3.125)
    assert want.shape == (h, w, 3) == (288, 512, 3)
    got = resize.resize_area_host(original[None], h, w)[0]
    buf = io.BytesIO()
    Image.fromarray(got).save(buf, format="JPEG", quality=95)
    with Image.open(io.BytesIO(buf.getvalue())) as img:
        again = np.asarray(img)
    pil = Image.fromarray(original)
    area, box, bilinear = _mean_abs(got, want), _mean_abs(np.asarray(pil.resize((w, h), Image.BOX)), want), _mean_abs(np.asarray(pil.resize((w, h), Image.BILINEAR)), want)
    noise = _mean_abs(again, got)
    print("frame {}: area {:.4f} box {:.4f} bilinear {:.4f} round trip {:.4f} saved-and-decoded against the reference {:.4f}".format(
        frame, area, box, bilinear, noise, _mean_abs(again, want)))
    assert area < box and area < bilinear
    assert area <= ROUNDTRIP_MARGIN * noise
    assert np.array_equal(again, want)


@pytest.mark.parametrize("S,D", ((1600, 512), (900, 288), (1920, 480), (7, 3), (5, 5), (9, 2)))
def test_weight_tables(S, D):
    from hipops import resize
    start, count, weight = resize.area_table(S, D)
    assert start.dtype == count.dtype == np.int32 and weight.dtype == np.float32 and weight.shape[0] == D
    assert float(np.abs(weight.astype(np.float64).sum(axis=1) - 1.0).max()) <= 1e-6
    assert (start >= 0).all() and (count >= 1).all() and (start + count <= S).all() and (np.diff(start) >= 0).all()
    assert start[0] == 0 and start[-1] + count[-1] == S
    for d in range(D):
        assert (weight[d, :count[d]] > 0).all() and not weight[d, count[d]:].any()
    if S % D == 0:                                                  # an integer factor is the plain box mean
        f = S // D
        assert (count == f).all() and np.array_equal(start, np.arange(D) * f) and np.array_equal(weight, np.full((D, f), np.float32(1.0 / f)))
        x = np.random.default_rng(S).integers(0, 256, size=(1, S, S, 3), dtype=np.uint8)
        mean = x.reshape(1, D, f, D, f, 3).astype(np.float64).mean(axis=(2, 4))
        assert float(np.abs(resize.resize_area_sums(x, D, D) - mean).max()) <= 256 * 2.0 ** -23      # fp32 weights: 1/f rounded once per axis


def test_pose_points_equal_the_composed_matrices():
    from hipops import lidar
    rng = np.random.default_rng(3)
    lidar_pose, cam_pose = nc.ego_pose(1, 0.3), nc.ego_pose(1, 0.9)
    scan = nc.scan_points(rng, 1, lidar_pose)
    params = lidar.pose_params(nc.LIDAR_CS, lidar_pose, cam_pose, nc.CAM_CS, nc.K, nc.W, nc.H)
    rows, full, kept = lidar.pose_points_host(scan, params)
    want, keep = nc.direct_rows(scan, lidar_pose, cam_pose)
    assert rows.dtype == np.float64 and rows.shape == (int(kept.sum()), 6) and np.array_equal(kept, keep) and 20 < rows.shape[0] < scan.shape[0]
    assert np.allclose(rows[:, :3], want, rtol=0, atol=1e-8)        # coordinates up to 1e3 in float64, two orders of summation
    glob = np.concatenate([scan[:, :3].astype(np.float64), np.ones((scan.shape[0], 1))], axis=1) @ (nc.rigid(lidar_pose) @ nc.rigid(nc.LIDAR_CS)).T
    assert np.allclose(full[:, 3:], glob[:, :3], rtol=0, atol=1e-9)
    # pyquaternion's matrix: orthonormal, the quaternion normalised first, the known quarter turn about z
    R = lidar.quaternion_matrix([2.0, 0.0, 0.0, 2.0])
    assert np.allclose(R, [[0, -1, 0], [1, 0, 0], [0, 0, 1]], atol=1e-15)
    R = lidar.quaternion_matrix(nc.CAM_CS["rotation"])
    assert np.allclose(R @ R.T, np.eye(3), atol=1e-15) and abs(np.linalg.det(R) - 1) < 1e-15


BOUNDARY_KEPT = [False, False, False, False, False, True, False, True, False, True, False, False]


def test_pose_points_on_the_mask_thresholds():
    """With identity poses and power-of-two intrinsics the images are exact: u = 1, u = W - 1, v = 1, v = H - 1 and depth = 1 fall out
    (strict inequalities), as do points behind the camera and at depth 0 (u is not a number)."""
    from hipops import lidar
    params = nc.exact_params()
    scan = nc.boundary_scan(params)
    rows, full, kept = lidar.pose_points_host(scan, params)
    assert full[0, 0] == 1.0 and full[1, 0] == 31.0 and full[2, 1] == 1.0 and full[3, 1] == 15.0 and full[4, 2] == 1.0 and full[6, 2] == -3.0
    assert kept.tolist() == BOUNDARY_KEPT and rows.shape == (3, 6)
    none = lidar.pose_points_host(np.zeros((0, 5), dtype=np.float32), params)
    assert none[0].shape == (0, 6) and none[2].shape == (0,)


def test_reference_files_pin_the_formats(golden_dir):
    """dtypes, shapes, keys and text formats of what the reference wrote for scene-0001.  The values cannot be reproduced here: the raw
    scans, tables and panoptic files they were computed from are not part of the fixture."""
    g = osp.join(golden_dir, GOLDEN)
    depth = np.load(osp.join(g, "depth_000000.npy"))
    assert depth.dtype == np.float64 and depth.ndim == 2 and depth.shape[1] == 3
    assert (depth[:, 2] > 1.0).all() and (depth[:, 0] > 1).all() and (depth[:, 0] < 1599).all() and (depth[:, 1] > 1).all() and (depth[:, 1] < 899).all()
    with np.load(osp.join(g, "mask_000000.npz"), allow_pickle=True) as z:
        assert sorted(z.files) == ["motion_label", "panoptic2ann", "panoptic_label"]
        assert z["panoptic_label"].dtype == np.uint16 and z["motion_label"].dtype == np.uint8
        assert z["panoptic_label"].shape == z["motion_label"].shape == (depth.shape[0],)
        assert set(np.unique(z["motion_label"]).tolist()) <= {0, 1, 2, 3}
        p2a = z["panoptic2ann"].item()
    assert isinstance(p2a, dict) and all(sorted(v) == ["fit", "token"] for v in p2a.values())
    assert all(int(k) in np.load(osp.join(g, "mask_000000.npz"), allow_pickle=True)["panoptic_label"] for k in p2a)
    with open(osp.join(g, "cam.json")) as fh:
        cam = json.load(fh)
    assert list(cam) == ["camera_intrinsic", "translation", "rotation", "dim", "intrinsic_mat"] and cam["dim"] == [900, 1600]
    assert np.allclose(np.array(cam["intrinsic_mat"])[:2] * np.array([[1600.0], [900.0]]), np.array(cam["camera_intrinsic"])[:2], rtol=1e-15)
    with open(osp.join(g, "ts.json")) as fh:
        ts = json.load(fh)
    assert isinstance(ts, list) and all(isinstance(t, int) and 0 <= t < 256 for t in ts)
    with open(osp.join(g, "odometry.txt")) as fh:
        lines = fh.read().split("\n")
    assert lines[-1] == "" and len(lines) == len(ts) + 2
    from hipops import lidar
    for line in lines[:-1]:
        vals = line.split(" ")
        assert len(vals) == 16 and vals[12:] == ["0.0", "0.0", "0.0", "1.0"]
        assert all(v == str(np.float64(float(v))) for v in vals)           # str() of a float64, as the script writes it
        R = np.array([float(v) for v in vals]).reshape(4, 4)[:3, :3]
        assert np.allclose(R @ R.T, np.eye(3), atol=1e-12)
    # a pose the script would write has the same text form
    text = " ".join(str(x) for x in lidar.transform_matrix([1010.1102882349232, 610.6567106479714, 0.0], [0.75, 0.0, 0.0, 0.66]).flatten())
    assert len(text.split(" ")) == 16 and text.split(" ")[3] == "1010.1102882349232" and text.endswith(" 0.0 0.0 0.0 1.0")


def unit_box(centre):
    from hipops import lidar
    return lidar.box_corners(centre, [2.0, 2.0, 2.0], [1.0, 0.0, 0.0, 0.0])


def test_box_fit_rules_on_the_host():
    from hipops import lidar
    corners = lidar.box_corners([1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [1.0, 0.0, 0.0, 0.0])          # w = 2 along y, l = 4 along x, h = 6 along z
    assert corners.shape == (8, 3) and corners[0].tolist() == [3.0, 3.0, 6.0] and corners[1].tolist() == [3.0, 1.0, 6.0]
    assert corners[3].tolist() == [3.0, 3.0, 0.0] and corners[4].tolist() == [-1.0, 3.0, 6.0] and corners[6].tolist() == [-1.0, 1.0, 0.0]
    # labels: 17001 two points in boxes a and b alike (a tie: the first), 17002 half in box c, 17003 in no box, 2001 a pedestrian with
    # car boxes only, 24000 the road, 17004 on a face of box a (strict inequalities: outside)
    pan = np.array([17001, 17001, 17002, 17002, 17003, 2001, 24000, 17004], dtype=np.uint16)
    pts = np.array([[0.1, 0, 0], [-0.1, 0, 0], [10, 0, 0], [30, 0, 0], [50, 0, 0], [0, 0, 0], [0.2, 0, 0], [1.0, 0, 0]], dtype=np.float64)
    boxes = [("a", 17, unit_box([0, 0, 0]), False), ("b", 17, unit_box([0, 0, 0]), True), ("c", 17, unit_box([10, 0, 0]), True), ("d", 9, unit_box([0, 0, 0]), True)]
    motion, p2a = lidar.motion_labels(pan, pts, boxes, {2, 9, 17})
    assert motion.dtype == np.uint8 and motion.tolist() == [2, 2, 1, 1, 3, 3, 0, 3]
    assert p2a == {17001: {"token": "a", "fit": 1.0}, 17002: {"token": "c", "fit": 0.5}, 17003: {"token": None, "fit": 0}, 2001: {"token": None, "fit": 0},
                   17004: {"token": None, "fit": 0}}
    counts, best = lidar.box_fit_host(pts[:2], [0, 2, 2], [17, 17], lidar.box_params(np.stack([b[2] for b in boxes])), [b[1] for b in boxes])
    assert counts.tolist() == [[2, 2, 0, -1], [0, 0, 0, -1]] and best.tolist() == [[0, 2], [-1, 0]]      # an empty point set: fraction 0, no box
    motion, p2a = lidar.motion_labels(pan[:2], pts[:2], [], {17})                                        # no boxes at all
    assert motion.tolist() == [3, 3] and p2a == {17001: {"token": None, "fit": 0}}


def snapshot(root):
    out = {}
    for d, _, files in os.walk(osp.join(root, "scenes")):
        for f in files:
            p = osp.join(d, f)
            out[osp.relpath(p, root)] = (os.stat(p).st_mtime_ns, open(p, "rb").read())
    return out


def test_script_prepares_the_layout(tmp_path):
    from hipops import resize
    from prepare_data import nuScenes
    root = str(tmp_path / "nuscenes")
    expect = nc.write_tree(root)
    logged = []
    nuScenes.prepare(root, batch=2, num_workers=3, log=logged.append, **nc.host_steps())
    assert logged == ["Processing " + s for s in nc.SCENES]
    nc.check_tree(root, expect)
    for name in nc.SCENES:                                            # the down-samples are the definition's bytes through Pillow at quality 95
        for ii, rel in enumerate(expect[name]["cams"]):
            with Image.open(osp.join(root, rel)) as img:
                small = resize.resize_area_host(np.asarray(img.convert("RGB"))[None], nc.DOWN_H, nc.DOWN_W)[0]
            buf = io.BytesIO()
            Image.fromarray(small).save(buf, format="JPEG", quality=95)
            assert open(osp.join(root, "scenes", name, "FRONT", "rgb", "downsample", "{:06}.jpg".format(ii)), "rb").read() == buf.getvalue()
    # a second run keeps every down-sample, depth list and mask (it compares the depth lists) and rewrites only the texts
    before = snapshot(root)
    marker = osp.join(root, "scenes", nc.SCENES[0], "FRONT", "rgb", "downsample", "000001.jpg")
    open(marker, "wb").write(b"kept")
    nuScenes.prepare(root, batch=16, num_workers=1, log=logged.append, **nc.host_steps())
    after = snapshot(root)
    assert open(marker, "rb").read() == b"kept"
    for rel, (mtime, data) in before.items():
        if rel.endswith((".jpg", ".npy", ".npz", "cam.json")) and not osp.islink(osp.join(root, rel)) and osp.join(root, rel) != marker:
            assert after[rel] == (mtime, data), rel
        elif osp.join(root, rel) != marker:
            assert after[rel][1] == data, rel
    # a depth list that differs from the new one stops the run, as in the reference
    dpath = osp.join(root, "scenes", nc.SCENES[1], "FRONT", "depth", "000002.npy")
    np.save(dpath, np.load(dpath) + 1.0)
    with pytest.raises(AssertionError):
        nuScenes.prepare(root, scenes=[nc.SCENES[1]], log=logged.append, **nc.host_steps())


@pytest.mark.parametrize("skip", ("rgb", "depth", "mask"))
def test_script_skip_switches_and_scene_choice(tmp_path, skip):
    from prepare_data import nuScenes
    root = str(tmp_path / "nuscenes")
    expect = nc.write_tree(root)
    nuScenes.prepare(root, scenes=[nc.SCENES[1]], log=lambda s: None, **{"skip_" + skip: True}, **nc.host_steps())
    nc.check_tree(root, expect, scenes=[nc.SCENES[1]], rgb=skip != "rgb", depth=skip != "depth", mask=skip != "mask")
    with pytest.raises(ValueError):
        nuScenes.prepare(root, scenes=["scene-9999"], log=lambda s: None, **nc.host_steps())


def test_tables_need_the_panoptic_category_index(tmp_path):
    from prepare_data import nuscenes_tables
    root = str(tmp_path / "nuscenes")
    nc.write_tree(root)
    path = osp.join(root, "v1.0-trainval", "category.json")
    rows = json.load(open(path))
    for r in rows:
        del r["index"]
    json.dump(rows, open(path, "w"))
    with pytest.raises(KeyError, match="index"):
        nuscenes_tables.Tables(root)
    os.remove(osp.join(root, "v1.0-trainval", "panoptic.json"))
    with pytest.raises(FileNotFoundError, match="panoptic"):
        nuscenes_tables.Tables(root)


def test_entry_points_are_declared():
    from hipops import abi
    for name in ("dd_resize_area", "dd_lidar_pose_points", "dd_lidar_pose_points_workspace_bytes", "dd_box_fit"):
        assert name in abi.EXPORTED


@pytest.mark.parametrize("kind,seed", (("noise", 11), ("white", 0), ("checker", 0)))
@pytest.mark.parametrize("shape", ((2, 900, 1600, 288, 512), (1, 7, 9, 3, 2), (3, 25, 50, 8, 16), (1, 10, 16, 10, 16), (2, 33, 47, 8, 12)))
def test_gpu_resize_cases_stay_under_the_exclusion_cap(shape, kind, seed):
    """The device comparison (tests/test_nuscenes_prepare_gpu.py) leaves out the bytes whose float64 sum lies within 1e-4 of a
    half-integer; with these seeds the numpy definition alone excludes at most 0.1 % of a case's bytes."""
    from hipops import resize
    n, hs, ws, hd, wd = shape
    if kind != "noise" and hs * ws > 10000:
        n = 1
    sums = resize.resize_area_sums(nc.resize_frames(kind, n, hs, ws, seed), hd, wd)
    near = np.abs(sums - np.floor(sums) - 0.5) < 1e-4
    assert float(near.mean()) <= 1e-3, float(near.mean())
