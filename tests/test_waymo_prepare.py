"""Waymo preparation on the host (prepare_data/waymo.py, prepare_data/waymo_records.py, hipops/contours.py trace, hipops/lidar.py
range_image_points_host, hipops/undistort.py).

Against real data from the reference's own run (the tiny_waymo fixture and one original / down-sample pair of it): the contour
tracer array for array, the object list, cam.json, the area down-sample.  The definitions of the two new kernels against the
restatements of tests/waymo_prepare_case.py: nothing of Waymo's can be executed here, so those guard against transcription errors,
not against a misremembered convention.  And the whole script with the host steps on a generated segment, read back by
datasets/waymo_dataset.py."""
import io
import json
import os
import os.path as osp
import pickle

import numpy as np
import pytest
from PIL import Image

import waymo_prepare_case as wc


def key(a):
    return a.dtype.str, a.shape, a.tobytes()


_fixture = {}


def fixture_masks():
    if not _fixture:
        with np.load(osp.join(wc.FIXTURE, "mask", "000001.npz")) as z:
            _fixture["semantic"], _fixture["instance"] = z["semantic"], z["instance"]
        with open(osp.join(wc.FIXTURE, "mask", "000001.pickle"), "rb") as fh:
            _fixture["entries"] = pickle.load(fh)
    return _fixture["semantic"], _fixture["instance"], _fixture["entries"]


def signed_area(c):
    p = c.reshape(-1, 2).astype(np.int64)
    q = np.roll(p, -1, axis=0)
    return int((p[:, 0] * q[:, 1] - q[:, 0] * p[:, 1]).sum())


def test_trace_equals_the_stored_contours_of_the_fixture():
    """Array for array: vertices, start vertex, direction, dtype; 43 contours with 4 307 vertices, 32 of them of negative signed
    area, [] for the 43 objects without a pixel."""
    from hipops import contours
    from prepare_data import waymo
    semantic, instance, entries = fixture_masks()
    objects, labels = waymo.object_image(semantic, instance)
    assert len(labels) == len(entries) == 65
    n_contours = n_vertices = negative = empty = 0
    for o, entry in enumerate(entries):
        got = contours.trace(objects == o)
        want = list(entry["mask"])
        assert all(g.dtype == np.int32 and g.ndim == 3 and g.shape[1:] == (1, 2) for g in got)
        assert sorted(map(key, got)) == sorted(map(key, want)), o
        n_contours, n_vertices, empty = n_contours + len(got), n_vertices + sum(len(g) for g in got), empty + (got == [])
        negative += sum(signed_area(g) < 0 for g in got)
    assert (n_contours, n_vertices, negative, empty) == (43, 4307, 32, 43)
    # the script's own path, on bounding boxes, gives the same arrays
    for outlines, entry in zip(waymo.object_contours(objects, len(labels)), entries):
        assert sorted(map(key, outlines)) == sorted(map(key, entry["mask"]))


def generated_masks():
    yy, xx = np.mgrid[0:40, 0:50]
    r2 = (yy - 20) ** 2 + (xx - 25) ** 2
    ring = (r2 <= 15 ** 2) & (r2 >= 8 ** 2)
    island = ring | (r2 <= 3 ** 2)
    dot = np.zeros((9, 9), dtype=bool)
    dot[4, 4] = True
    full = np.ones((6, 7), dtype=bool)
    full[2:4, 3] = False
    diagonal = np.eye(12, dtype=bool)
    noise = np.random.default_rng(2).uniform(size=(30, 31)) < 0.55
    return {"ring": ring, "island in a hole": island, "one pixel": dot, "touching all borders": full, "diagonal": diagonal,
            "anti-diagonal": diagonal[::-1].copy(), "noise": noise, "empty": np.zeros((5, 5), dtype=bool)}


@pytest.mark.parametrize("name", sorted(generated_masks()))
def test_fill_of_the_traced_contours_rebuilds_the_mask(name):
    from hipops import contours
    mask = generated_masks()[name]
    found = contours.trace(mask)
    h, w = mask.shape
    filled = contours.fill_host([(1, [c.reshape(-1, 2) for c in found])], h, w)
    assert np.array_equal(filled.astype(bool), mask)
    assert np.array_equal(mask, generated_masks()[name]), "trace changed its input"
    for three_d in (mask[:, :, None].astype(np.uint8) * 255,):
        assert list(map(key, contours.trace(three_d))) == list(map(key, found))
    if name == "ring":
        assert len(found) == 2 and sorted(np.sign(signed_area(c)) for c in found) == [-1, 1]
        outer = max(found, key=lambda c: abs(signed_area(c)))
        assert tuple(outer[0, 0]) == (25, 5)                        # its first pixel in raster order
    if name == "one pixel":
        assert len(found) == 1 and found[0].tolist() == [[[4, 4]]]
    if name == "empty":
        assert found == []


def test_object_list_of_the_fixture():
    from prepare_data import waymo
    semantic, instance, entries = fixture_masks()
    objects, labels = waymo.object_image(semantic, instance)
    assert labels == [e["mask_label"] for e in entries] and len(labels) == 65
    assert sum(1 for e in entries if len(e["mask"])) == 22 == len(np.unique(objects[objects >= 0]))
    assert objects.dtype == np.int32 and objects.shape == (1280, 1920)
    # the + 1 in the stored dtype: instance 255 of uint8 wraps to 0 and names no object
    sem = np.full((2, 3, 1), 2, dtype=np.uint8)
    ins = np.array([[0, 1, 255], [255, 1, 0]], dtype=np.uint8)[:, :, None]
    objects, labels = waymo.object_image(sem, ins)
    assert labels == [2, 2] and objects[:, :, ].tolist() == [[0, 1, -1], [-1, 1, 0]]


def test_cam_json_equals_the_fixture(tmp_path):
    from prepare_data import waymo
    want = json.load(open(osp.join(wc.FIXTURE, "rgb", "cam.json")))
    path = str(tmp_path / "cam.json")
    waymo.write_cam(path, want["intrinsic"], want["extrinsic"], want["dim"])
    got = json.load(open(path))
    assert got == want and list(got) == list(want)


def test_area_downsample_against_the_reference_on_a_real_frame():
    """decode(downsample) against resize_area_host(decode(original)) saved at quality 95 and decoded: mean absolute difference in
    grey levels, beside Pillow's BOX and BILINEAR.  The original is itself a JPEG of the frame the reference down-sampled, so
    equality is not expected: ours is the smallest of the three and no larger than the nuScenes figure of DESIGN 4.22."""
    from hipops import resize
    original = np.asarray(Image.open(osp.join(wc.PAIR, "original_000001.jpg")).convert("RGB"))
    want = np.asarray(Image.open(osp.join(wc.PAIR, "downsample_000001.jpg")).convert("RGB")).astype(np.int64)
    assert original.shape == (1280, 1920, 3) and want.shape == (320, 480, 3)

    def round_trip(a):
        buf = io.BytesIO()
        Image.fromarray(a).save(buf, format="JPEG", quality=95)
        return np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert("RGB")).astype(np.int64)

    figures = {"area": float(np.abs(round_trip(resize.resize_area_host(original[None], 320, 480)[0]) - want).mean())}
    for name, kind in (("BOX", Image.BOX), ("BILINEAR", Image.BILINEAR)):
        figures[name] = float(np.abs(round_trip(np.asarray(Image.fromarray(original).resize((480, 320), kind))) - want).mean())
    print(figures)
    assert figures["area"] < figures["BOX"] and figures["area"] < figures["BILINEAR"]
    assert figures["area"] <= wc.NUSCENES_AREA_FIGURE


def test_records(tmp_path):
    from prepare_data import waymo_records as wr
    payloads = [b"first", b"", bytes(range(256)) * 5, b"last one"]
    path = str(tmp_path / "a.tfrecord")
    offsets = wc.write_tfrecord(path, payloads)
    assert list(wr.read_records(path)) == payloads == list(wr.read_records(path, check_data=True))
    assert wr.crc32c(b"123456789") == 0xE3069283 == wc._crc32c_bitwise(b"123456789")
    data = open(path, "rb").read()

    def damaged(name, change):
        p = str(tmp_path / name)
        open(p, "wb").write(change(bytearray(data)))
        return p

    def flip(at):
        def change(b):
            b[at] ^= 0x40
            return bytes(b)
        return change

    p = damaged("length.tfrecord", flip(offsets[2] + 1))
    with pytest.raises(ValueError, match=r"length\.tfrecord.*offset {}\b".format(offsets[2])):
        list(wr.read_records(p))
    p = damaged("payload.tfrecord", flip(offsets[2] + 12 + 700))
    assert list(wr.read_records(p))[3] == payloads[3]                # not checked by default
    with pytest.raises(ValueError, match=r"payload\.tfrecord.*offset {}\b".format(offsets[2])):
        list(wr.read_records(p, check_data=True))
    for cut in (3, 12 + 4, 20):                                      # inside the last record's trailer, payload and header
        p = damaged("cut{}.tfrecord".format(cut), lambda b: bytes(b[:len(b) - cut]))
        got = []
        with pytest.raises(ValueError, match=r"truncated.*offset {}\b".format(offsets[3])):
            for payload in wr.read_records(p):
                got.append(payload)
        assert got == payloads[:3]


def test_a_missing_waymo_package_is_one_clear_sentence():
    from prepare_data import waymo_records as wr
    try:
        import waymo_open_dataset  # noqa: F401
    except ImportError:
        with pytest.raises(RuntimeError, match="waymo_open_dataset.dataset_pb2.*not installed"):
            wr.message_classes()


_lidar = {}


def lidar_case():
    """The generated frames, the definition's output and the restatement's, computed once."""
    if not _lidar:
        from hipops import lidar
        frames = [wc.lidar_frame(seed) for seed in (0, 1, 2)]
        inputs = wc.definition_inputs(frames)
        _lidar["frames"], _lidar["inputs"] = frames, inputs
        _lidar["host"] = lidar.range_image_points_host(*inputs)
        _lidar["restated"] = [r for f in frames for r in wc.restate_points(f)]
    return _lidar


def test_range_image_points_host_equals_the_restatement():
    case = lidar_case()
    found, counts = case["host"]
    bound = wc.points_bound()
    f, n_rows = wc.CAM_INTRINSIC[1], 0
    assert counts.shape == (15, 2) and counts.dtype == np.int32
    for s, ((points, cp, rows), (want_points, want_cp, want_rows)) in enumerate(zip(found, case["restated"])):
        assert points.dtype == rows.dtype == np.float64 and cp.dtype == np.int32
        assert counts[s].tolist() == [points.shape[0], rows.shape[0]] == [want_points.shape[0], want_rows.shape[0]], s
        assert np.array_equal(cp, want_cp)
        # the restatement rounds differently (composed matrices at the global magnitude): the same derived bound, times 8
        assert np.abs(points - want_points).max(initial=0) <= 8 * bound
        if rows.shape[0]:
            z_min = rows[:, 2].min()
            assert np.abs(rows[:, 2] - want_rows[:, 2]).max() <= 8 * bound
            assert np.abs(rows[:, :2] - want_rows[:, :2]).max() <= 8 * bound * f / z_min
        n_rows += rows.shape[0]
    valid = sum(int(c[0]) for c in counts)
    pixels = 3 * (8 * 40 + 4 * 5 * 12)
    assert 0.4 * pixels < valid < 0.7 * pixels and n_rows > 30
    for k in range(3):                                               # image 4 entirely invalid, image 5 without a point in view
        assert counts[5 * k + 3].tolist() == [0, 0] and counts[5 * k + 4, 0] == 20 and counts[5 * k + 4, 1] == 0


def test_generated_depth_list_shows_the_orderings_of_the_real_one():
    """In the fixture's depth/000001.npy 99.3 % of consecutive rows have increasing u and its runs descend the image; the generated
    TOP image shows the same: u increases within a range-image row, and the rows' mean v increases."""
    real = np.load(osp.join(wc.FIXTURE, "depth", "000001.npy"))
    up = np.diff(real[:, 0]) > 0
    assert abs(up.mean() - 0.993) < 5e-4
    rows = lidar_case()["host"][0][0][2]                              # frame 0, TOP
    breaks = np.flatnonzero(np.diff(rows[:, 0]) <= 0) + 1
    runs = np.split(rows, breaks)
    assert len(runs) == 8 and all(len(r) >= 3 for r in runs)
    means = [r[:, 1].mean() for r in runs]
    assert all(b > a for a, b in zip(means[:-1], means[1:]))


def test_the_lidar_case_keeps_clear_of_every_threshold():
    """No point of the case within 1000 times the comparison's bound of rho = 0, z = 0 or an image edge: the tolerance of the device
    test cannot move a decision."""
    case = lidar_case()
    ranges, cps, poses, trigs, params = case["inputs"]
    bound = 1000 * wc.points_bound()
    f = max(wc.CAM_INTRINSIC[:2])
    from hipops import lidar
    for s, rng in enumerate(ranges):
        assert not ((rng > 0) & (rng < 1.0)).any()
        # every valid pixel's camera values, kept or not: open the window
        wide = params[s].copy()
        (points, _, _), = lidar.range_image_points_host([rng], [cps[s]], [poses[s]], [trigs[s]], wide[None])[0]
        q = points @ wide[25:34].reshape(3, 3).T + wide[34:37]
        a = q @ wide[37:46].reshape(3, 3).T
        z = a[:, 2]
        assert (np.abs(z) > bound).all()
        front = z > 0
        u, v = a[front, 0] / z[front], a[front, 1] / z[front]
        edge = bound * f / np.abs(z[front])
        for value, limit in ((u, 0.0), (u, wc.CAM_W), (v, 0.0), (v, wc.CAM_H)):
            assert (np.abs(value - limit) > edge).all()


def test_range_image_points_host_on_the_exact_thresholds():
    from hipops import lidar
    inputs, expected = wc.exact_case()
    found, counts = lidar.range_image_points_host(*inputs)
    for s, want in enumerate(expected):
        assert counts[s].tolist() == [0 if want is None else 1, 1 if want else 0], (s, counts[s])
    assert found[0][2].tolist() == [[0.0, 16.0, 4.0]] and found[2][2].tolist() == [[32.0, 0.0, 4.0]]
    assert found[7][2].tolist() == [[32.0, 16.0, 2.0 ** -127]] and found[9][2].tolist() == [[60.0, 16.0, 4.0]]
    assert found[1][0].tolist() == [[4.0, -4.0, 0.0]] and found[1][1].tolist() == [[3, 4, 5]]


def test_inclination_table_and_refusals():
    from hipops import lidar
    assert lidar.inclination_table(3, [0.1, 0.2, 0.4], -1, 1).tolist() == [0.4, 0.2, 0.1]
    assert np.allclose(lidar.inclination_table(4, [], -1.0, 1.0), [0.75, 0.25, -0.25, -0.75])
    with pytest.raises(ValueError):
        lidar.inclination_table(4, [0.1, 0.2], -1, 1)
    corners = lidar.upright_box_corners([1.0, 2.0, 3.0, 4.0, 2.0, 1.0, 0.0])
    assert corners[0].tolist() == [3.0, 3.0, 2.5] and corners[1].tolist() == [-1.0, 3.0, 2.5]
    assert corners[3].tolist() == [3.0, 1.0, 2.5] and corners[4].tolist() == [3.0, 3.0, 3.5]
    turned = lidar.upright_box_corners([0.0, 0.0, 0.0, 4.0, 2.0, 1.0, np.pi / 2])
    assert np.allclose(turned[0], [-1.0, 2.0, -0.5])


def test_frame_to_arrays_refuses_what_does_not_look_right():
    from prepare_data import waymo_records as wr
    frames, _, _, _ = wc.script_frames()

    def arrays(frame):
        return wr.frame_to_arrays(frame, ("FRONT",), wc.MatrixFloat, wc.MatrixInt32)

    fa = arrays(frames[1])
    assert [l["name"] for l in fa.lasers] == [1, 2, 3, 4, 5] and fa.lasers[0]["pose"] is not None and fa.lasers[1]["pose"] is None
    assert fa.lasers[0]["range"].shape == (8, 40) and fa.lasers[0]["cp"].shape == (8, 40, 3) and fa.lasers[0]["cp"].dtype == np.int32
    assert fa.cameras["FRONT"]["code"] == 1 and fa.cameras["FRONT"]["panoptic"] is not None and len(fa.labels) == 2
    assert arrays(frames[0]).cameras["FRONT"]["panoptic"] is None
    import copy
    bad = copy.deepcopy(frames[0])
    bad.lasers[0].ri_return1.range_image_compressed = wc._compressed(np.zeros((5, 12, 3), dtype=np.float32))
    with pytest.raises(ValueError, match="range image"):
        arrays(bad)
    bad = copy.deepcopy(frames[0])
    bad.lasers[0].ri_return1.camera_projection_compressed = wc._compressed(np.zeros((5, 12, 5), dtype=np.int32))
    with pytest.raises(ValueError, match="camera projection"):
        arrays(bad)
    bad = copy.deepcopy(frames[0])
    del bad.context.camera_calibrations[0].intrinsic[-1]
    with pytest.raises(ValueError, match="intrinsic"):
        arrays(bad)
    bad = copy.deepcopy(frames[0])
    del bad.context.laser_calibrations[2]
    with pytest.raises(ValueError, match="no calibration"):
        arrays(bad)


def test_undistort_host_without_distortion_is_the_identity():
    from hipops import undistort
    frames = wc.checkerboard(2, 21, 30)
    assert np.array_equal(undistort.undistort_host(frames, wc.calibration(21, 30, "none")), frames)


@pytest.mark.parametrize("strength", ("k1", "strong"))
def test_undistort_host_equals_the_scalar_restatement(strength):
    from hipops import undistort
    H, W = 22, 31
    frames = wc.checkerboard(2, H, W)
    cal = wc.calibration(H, W, strength)
    got = undistort.undistort_host(frames, cal)
    assert got.shape == frames.shape and got.dtype == np.uint8
    for n in range(2):
        for v in range(H):
            for u in range(W):
                assert got[n, v, u].tolist() == wc.restate_undistort_pixel(frames[n], cal, u, v), (n, v, u)
    assert not np.array_equal(got, frames)
    if strength == "strong":                                         # border taps leave the image on all four sides
        ix, iy = undistort.source_grid(cal, H, W)
        assert (ix >> 5).min() < 0 and (ix >> 5).max() + 1 >= W and (iy >> 5).min() < 0 and (iy >> 5).max() + 1 >= H


def test_script_with_the_host_steps(tmp_path):
    """Three generated 64 x 96 frames, the second with a panoptic label and two laser labels: every file of the layout, the logged
    segment-count warnings, and datasets/waymo_dataset.py reading the result."""
    import datasets
    from hipops import lidar, resize, undistort
    from prepare_data import waymo
    records, out = str(tmp_path / "records"), str(tmp_path / "out")
    frames, plain, images, (sem, ins, objects) = wc.write_records(records)
    logged = []
    waymo.prepare(records, out, batch=2, num_workers=3, log=logged.append, **wc.host_steps())
    assert sum("Warning" in line and "798" in line for line in logged) == 1 and sum("Warning" in line and "202" in line for line in logged) == 1
    base = osp.join(out, "val", wc.SEGMENT_NAME, "FRONT")
    files = sorted(osp.relpath(osp.join(d, f), base) for d, _, fs in os.walk(base) for f in fs)
    assert files == sorted(["odometry.txt", "rgb/cam.json", "mask/000001.npz", "mask/000001.pickle"] +
                           ["{}/{:06}.{}".format(d, k, e) for d, e in (("rgb/original", "jpg"), ("rgb/downsample", "jpg"), ("depth", "npy")) for k in range(3)])
    # frames: the JPEG as Pillow decodes it, undistorted, and its quarter-size area down-sample
    from prepare_data import common
    decoded = np.stack([common.pil_decode(f.images[1].image) for f in frames])
    flat = undistort.undistort_host(decoded, wc.SCRIPT_INTRINSIC)
    small = resize.resize_area_host(flat, 16, 24)
    for k in range(3):
        for kind, want in (("original", flat[k]), ("downsample", small[k])):
            buf = io.BytesIO()
            Image.fromarray(want).save(buf, format="JPEG", quality=95)
            assert open(osp.join(base, "rgb", kind, "{:06}.jpg".format(k)), "rb").read() == buf.getvalue()
    cam = json.load(open(osp.join(base, "rgb", "cam.json")))
    assert cam["intrinsic"] == wc.SCRIPT_INTRINSIC and cam["dim"] == [64, 96] and cam["extrinsic"] == wc.CAM_EXTRINSIC.reshape(-1).tolist()
    assert cam["intrinsic_mat"] == [[40.0 / 96, 0.0, 47.3 / 96], [0.0, 41.0 / 64, 31.6 / 64], [0.0, 0.0, 1.0]]
    lines = open(osp.join(base, "odometry.txt")).read().splitlines()
    assert lines == [" ".join(str(x) for x in f.images[1].pose.transform) for f in frames]
    # depth lists: the five lasers' rows, in ascending laser name
    for k in range(3):
        found, _ = lidar.range_image_points_host(*wc.definition_inputs([plain[k]], intrinsic=wc.SCRIPT_INTRINSIC))
        depth = np.load(osp.join(base, "depth", "{:06}.npy".format(k)))
        assert depth.dtype == np.float64 and depth.shape[1] == 3 and depth.shape[0] > 10
        assert np.array_equal(depth, np.concatenate([f[2] for f in found]))
    # labels
    with np.load(osp.join(base, "mask", "000001.npz")) as z:
        assert sorted(z.files) == ["instance", "semantic"] and z["semantic"].dtype == z["instance"].dtype == np.uint8
        assert np.array_equal(z["semantic"], sem[:, :, None]) and np.array_equal(z["instance"], ins[:, :, None])
    entries = pickle.load(open(osp.join(base, "mask", "000001.pickle"), "rb"))
    assert [e["mask_label"] for e in entries] == [c for c, _ in objects]
    assert [e["box_label"] for e in entries] == [1, None, 2] and entries[1]["match"] == 0 and entries[1]["speed"] == [None] * 3
    assert entries[0]["speed"] == [3.0, 0.0, 0.0] and entries[0]["dim"] == [4.0, 2.0, 1.5] and entries[0]["heading"] == 0.4
    assert 0 < entries[0]["match"] <= 1 and isinstance(entries[0]["match"], np.float64) and len(entries[0]["mask"]) == 2
    # the reader on the result
    ds = datasets.WaymoDataset(data_path=out, filenames=["val/{} 1".format(wc.SEGMENT_NAME)], height=16, width=24, cam_name="FRONT", img_type="downsample",
                               frame_idxs=[0, -1, 1], num_scales=2, is_train=False, img_ext=".jpg", load_depth=True, load_mask=True)
    ds.full_res_shape = (wc.CAM_W, wc.CAM_H)
    item = ds[0]
    want = np.zeros((wc.CAM_H, wc.CAM_W), dtype=np.uint8)
    for label, (_, mask) in zip(wc.OBJECT_LABELS, objects):
        want[mask] = label
    assert np.array_equal(item["mot_mask"].numpy(), want) and np.array_equal(item["sem_mask"].numpy(), sem.astype(np.uint8))
    assert tuple(item[("color", 0, 0)].shape) == (3, 16, 24)
    # a second run with the skips writes nothing new and keeps the odometry
    waymo.prepare(records, str(tmp_path / "skipped"), skip_rgb=True, skip_depth=True, skip_mask=True, log=lambda s: None, **wc.host_steps())
    skipped = osp.join(str(tmp_path / "skipped"), "val", wc.SEGMENT_NAME, "FRONT")
    assert sorted(f for _, _, fs in os.walk(skipped) for f in fs) == ["odometry.txt"]
    assert open(osp.join(skipped, "odometry.txt")).read().splitlines() == lines
    with pytest.raises(ValueError, match="no such segments"):
        waymo.prepare(records, str(tmp_path / "none"), segments=["segment-9"], log=lambda s: None, **wc.host_steps())
