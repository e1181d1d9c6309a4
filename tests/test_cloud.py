"""Point clouds on the host: the numpy definition of csrc/dd_cloud.hip (hipops/cloud.py) against a float64 evaluation of the same
formulas, the keep rule's decisions at their exact bounds, order and offsets, the PLY files, the scene's pose chain and the parser.
No GPU."""
import numpy as np
import pytest

import cloud_case as CC

_f32 = np.float32


def _dense(shape, flip, with_mask, with_pose, **change):
    from hipops.cloud import cloud_candidates_host
    B, h, w, H, W, stride = shape
    x = CC.inputs(B, h, w)
    kw = CC.host_kwargs(B, h, w, flip, with_mask, with_pose, stride)
    kw.update(change)
    return cloud_candidates_host(x["disp"], x["color"], H, W, CC.intrinsics(H, W), **kw)


# ---- the definition ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_pose", [False, True], ids=["camera", "pose"])
@pytest.mark.parametrize("flip", [False, True], ids=["plain", "pp"])
@pytest.mark.parametrize("shape", CC.SHAPES, ids=CC.IDS)
def test_host_definition_against_float64(shape, flip, with_pose):
    """The fp32 coordinates of every fp32-kept point against the same formulas in float64 on the same fp32 inputs and constants, within
    the per-point bound cloud_case.cloud64 derives: the depth's bound of export_case, three roundings of the back-projection, four
    per term of the pose.  No point is excluded; a kept point is finite in both evaluations."""
    B, h, w, H, W, stride = shape
    x = CC.inputs(B, h, w)
    keep, xyz, _ = _dense(shape, flip, False, with_pose)
    with np.errstate(all="ignore"):
        want, bound = CC.cloud64(x["disp"], H, W, CC.intrinsics(H, W), x["flipped"] if flip else None, x["pose"] if with_pose else None, stride)
    assert xyz.dtype == np.float32 and xyz.shape == want.shape == keep.shape + (3,) and keep.any()
    got, want, bound = xyz[keep].astype(np.float64), want[keep], bound[keep]
    assert np.isfinite(got).all() and np.isfinite(want).all() and np.isfinite(bound).all()
    err = np.abs(got - want)
    print("shape {} flip {} pose {}: {} points, worst error {:.3e}, worst error / bound {:.3f}".format(shape, flip, with_pose, len(got), err.max(), (err / bound).max()))
    assert (err <= bound).all(), (err / bound).max()
    scale = np.abs(want).max(axis=1, keepdims=True) + (np.abs(x["pose"][:, :, 3]).max() if with_pose else 0.0)
    assert np.median(bound / scale) < 1e-4                         # a rounding bound: the typical point is held to a few 1e-6 of its size


def test_bound_separates_the_definition_from_a_wrong_one():
    """Pixel centres at half-integer coordinates (the other common convention) lie outside the bound."""
    shape = CC.SHAPES[4]
    B, h, w, H, W, stride = shape
    x = CC.inputs(B, h, w)
    keep, xyz, _ = _dense(shape, False, False, False)
    fx, fy, cx, cy = CC.intrinsics(H, W)
    want, bound = CC.cloud64(x["disp"], H, W, (fx, fy, cx - 0.5, cy - 0.5), None, None, stride)
    assert (np.abs(xyz[keep] - want[keep]) > bound[keep])[:, :2].mean() > 0.9


def test_records_are_the_dense_candidates_compacted():
    from hipops.cloud import unpack_records
    shape = CC.SHAPES[4]
    keep, xyz, rgb = _dense(shape, True, True, True)
    records, offsets = CC.host_reference(shape, True, True, True)
    got_xyz, rgba = unpack_records(records)
    assert records.dtype == np.uint8 and records.shape == (keep.sum(), 16) and offsets.dtype == np.int64
    assert np.array_equal(got_xyz.view(np.uint32), xyz[keep].view(np.uint32)) and np.array_equal(rgba[:, :3], rgb[keep]) and (rgba[:, 3] == 255).all()
    assert offsets.tolist() == [0] + np.cumsum(keep.reshape(keep.shape[0], -1).sum(1)).tolist()
    assert 0 < keep.sum() < keep.size and rgb.min() == 0 and rgb.max() == 255          # something kept, something dropped, both clamps of the colour byte
    assert records[0, :4].tobytes() == np.array([xyz[keep][0, 0]], dtype="<f4").tobytes()


# ---- decisions -------------------------------------------------------------------------------------------------------------------
def test_decisions_at_their_bounds():
    """The same-size case: the blend passes a tap through, so the hand-laid frame 0 of cloud_case.inputs meets every bound exactly."""
    from hipops.export import depth_params
    shape = CC.SAME_SIZE
    B, h, w, H, W, _ = shape
    x = CC.inputs(B, h, w)
    lo, span = depth_params(CC.MIN_DEPTH, CC.MAX_DEPTH)
    s = (lo + span * x["disp"]).astype(np.float32)
    max_range, d_at, d_above = CC.range_case()
    d_low, e_at, e_above = CC.edge_case()
    one, edge = _f32(1), _f32(CC.EDGE)
    # what the searches promise
    assert one / CC._s(d_at) == _f32(max_range) and one / CC._s(d_above) == np.nextafter(_f32(max_range), _f32(np.inf))
    assert CC._s(e_at) - CC._s(d_low) == edge * CC._s(d_low) and CC._s(e_above) == np.nextafter(CC._s(e_at), _f32(np.inf))
    assert CC._s(e_above) - CC._s(d_low) > edge * CC._s(d_low)
    keep, xyz, _ = _dense(shape, False, True, False)
    assert xyz[0, 3, 0, 2] == _f32(max_range) and xyz[0, 3, 3, 2] == np.nextafter(_f32(max_range), _f32(np.inf))
    assert np.array_equal(xyz[0, :, :, 2], one / s[0])                       # same size: depth is 1 / s of the pixel itself
    for (Y, X), (kept, why) in CC.DECISIONS.items():
        assert bool(keep[0, Y, X]) == kept, ((Y, X), why)
    # each rule alone decides its cases: without the edge rule the edge cases are all kept, without the mask the mask cases, and
    # beyond the range bound the range case
    assert _dense(shape, False, True, False, edge=0.0)[0][0, :2, :6].all()
    assert _dense(shape, False, False, False)[0][0, 2, 6:].all()
    assert _dense(shape, False, True, False, max_range=float(np.nextafter(_f32(max_range), _f32(np.inf))))[0][0, 3, 3]
    assert not _dense(shape, False, True, False, max_range=float(np.nextafter(_f32(max_range), _f32(0))))[0][0, 3, 0]
    # NaN disparity (every candidate that reads it as a tap), depth <= 0, NaN mask
    k1 = keep[1]
    assert not k1[1:3, 1:3].any() and not k1[0, 5:7].any() and not k1[3:5, 4:6].any()
    assert np.isnan(xyz[1, 2, 2, 2]) and xyz[1, 0, 6, 2] < 0
    assert keep[1].any() and keep[2].any()


def test_nan_compares_false_everywhere():
    from hipops.cloud import export_cloud_host
    disp = np.full((1, 2, 2), 0.5, dtype=np.float32)
    color = np.full((1, 3, 2, 2), np.nan, dtype=np.float32)
    cam = (2.0, 2.0, 0.5, 0.5)
    kw = dict(min_depth=0.1, max_depth=100.0)
    rec, off = export_cloud_host(disp, color, 2, 2, cam, **kw)
    assert off.tolist() == [0, 4] and (rec[:, 12:15] == 0).all() and (rec[:, 15] == 255).all()            # fmaxf(NaN, 0) == 0
    assert export_cloud_host(disp, color, 2, 2, cam, max_range=float("nan"), **kw)[1].tolist() == [0, 0]
    assert export_cloud_host(disp, color, 2, 2, cam, motion_mask=np.zeros((1, 2, 2), np.float32), motion_thresh=float("nan"), **kw)[1].tolist() == [0, 0]
    assert export_cloud_host(disp * 0 - 0.01 / 9.99, color, 2, 2, cam, max_range=float("inf"), **kw)[1][1] in (0, 4)     # s about 0: depth huge, infinite or negative
    with pytest.raises(ValueError):
        export_cloud_host(disp, color[:, :2], 2, 2, cam, **kw)
    with pytest.raises(ValueError):
        export_cloud_host(disp, color, 2, 2, cam, stride=0, **kw)


# ---- order and offsets -----------------------------------------------------------------------------------------------------------
def _pixels(records, offsets, H, W):
    """(b, Y, X) of every record of a pose-free cloud: X = x / z * fx + cx within rounding of an integer."""
    from hipops.cloud import unpack_records
    fx, fy, cx, cy = CC.intrinsics(H, W)
    xyz = unpack_records(records)[0].astype(np.float64)
    X, Y = xyz[:, 0] / xyz[:, 2] * fx + cx, xyz[:, 1] / xyz[:, 2] * fy + cy
    assert np.abs(X - np.rint(X)).max() < 1e-2 and np.abs(Y - np.rint(Y)).max() < 1e-2
    b = np.searchsorted(offsets, np.arange(len(records)), side="right") - 1
    return b, np.rint(Y).astype(int), np.rint(X).astype(int)


def test_order_all_kept_and_none_kept():
    from hipops.cloud import export_cloud_host
    B, h, w, H, W, _ = CC.SHAPES[1]
    x = CC.inputs(B, h, w)
    disp = np.abs(np.nan_to_num(x["disp"], nan=0.3))                     # no NaN, no negative depth
    kw = dict(min_depth=CC.MIN_DEPTH, max_depth=CC.MAX_DEPTH, edge=0.0)
    rec, off = export_cloud_host(disp, x["color"], H, W, CC.intrinsics(H, W), **kw)
    assert off.tolist() == [0, H * W, 2 * H * W] and rec.shape == (2 * H * W, 16)
    b, Y, X = _pixels(rec, off, H, W)
    assert np.array_equal(b * H * W + Y * W + X, np.arange(2 * H * W))              # frame by frame, row-major
    rec, off = export_cloud_host(disp, x["color"], H, W, CC.intrinsics(H, W), max_range=1e-3, **kw)
    assert off.tolist() == [0, 0, 0] and rec.shape == (0, 16) and rec.dtype == np.uint8


def test_a_frame_without_points_between_two_others():
    from hipops.cloud import export_cloud_host
    B, h, w, H, W, _ = CC.SAME_SIZE
    x = CC.inputs(B, h, w)
    mask = np.nan_to_num(x["mask"], nan=0.0).copy()
    mask[1] = 1.0
    kw = dict(CC.params(), motion_mask=mask)
    rec, off = export_cloud_host(x["disp"], x["color"], H, W, CC.intrinsics(H, W), **kw)
    assert 0 < off[1] == off[2] < off[3] == len(rec)
    whole, _ = export_cloud_host(x["disp"][[0, 2]], x["color"][[0, 2]], H, W, CC.intrinsics(H, W), **dict(kw, motion_mask=mask[[0, 2]]))
    assert np.array_equal(rec, whole)


@pytest.mark.parametrize("stride", [1, 2, 3])
def test_strides_against_a_filtered_stride_one_result(stride):
    from hipops.cloud import export_cloud_host
    B, h, w, H, W, _ = CC.SHAPES[4]
    x = CC.inputs(B, h, w)
    kw = dict(CC.params(), disp_flipped=x["flipped"], motion_mask=x["mask"])
    cam = CC.intrinsics(H, W)
    full, off = export_cloud_host(x["disp"], x["color"], H, W, cam, stride=1, **kw)
    b, Y, X = _pixels(full, off, H, W)
    sel = (Y % stride == 0) & (X % stride == 0)
    rec, got = export_cloud_host(x["disp"], x["color"], H, W, cam, stride=stride, **kw)
    assert np.array_equal(rec, full[sel]) and got.tolist() == [0] + np.cumsum(np.bincount(b[sel], minlength=B)).tolist()
    assert 0 < len(rec) and (stride == 1 or len(rec) < len(full))


# ---- PLY -------------------------------------------------------------------------------------------------------------------------
HEADER = """ply
format binary_little_endian 1.0
comment camera coordinates: x right, y down, z forward; depth is up to scale (one unknown factor per model)
element vertex {}
property float x
property float y
property float z
property uchar red
property uchar green
property uchar blue
property uchar alpha
end_header
"""


def test_ply_round_trip_and_header(tmp_path):
    from hipops.cloud import ply_header, read_ply, unpack_records, write_ply
    records, _ = CC.host_reference(CC.SHAPES[4], False, False, True)
    path = write_ply(str(tmp_path / "a.ply"), records)
    raw = open(path, "rb").read()
    assert raw == HEADER.format(len(records)).encode("ascii") + records.tobytes() and ply_header(len(records)) == raw[:len(raw) - records.nbytes]
    xyz, rgba, back = read_ply(path)
    assert np.array_equal(back, records) and xyz.dtype == np.float32 and xyz.shape == (len(records), 3) and rgba.shape == (len(records), 4)
    assert all(np.array_equal(a, b) for a, b in zip((xyz, rgba), unpack_records(records)))
    assert np.array_equal(xyz[:, 0], records[:, :4].copy().view("<f4")[:, 0]) and (rgba[:, 3] == 255).all()
    # a slice of a batch's bytes, as predict.py hands it over; an empty cloud
    assert open(write_ply(str(tmp_path / "b.ply"), records.reshape(-1)[16:48]), "rb").read() == HEADER.format(2).encode("ascii") + records[1:3].tobytes()
    assert read_ply(write_ply(str(tmp_path / "c.ply"), records[:0]))[2].shape == (0, 16)
    with pytest.raises(ValueError):
        write_ply(str(tmp_path / "d.ply"), records.reshape(-1)[:17])
    (tmp_path / "e.ply").write_bytes(raw[:-3])
    with pytest.raises(ValueError):
        read_ply(str(tmp_path / "e.ply"))
    (tmp_path / "f.ply").write_bytes(raw.replace(b"property uchar alpha\n", b""))
    with pytest.raises(ValueError):
        read_ply(str(tmp_path / "f.ply"))


def test_scene_header_has_one_length(tmp_path):
    from hipops.cloud import COUNT_DIGITS, ScenePly, ply_header, read_ply
    lengths = {len(ply_header(n, fixed=True)) for n in (0, 7, 10 ** 9, 2 ** 63 - 1, 10 ** COUNT_DIGITS - 1)}
    assert len(lengths) == 1
    zero, big = ply_header(0, fixed=True).decode(), ply_header(10 ** 9, fixed=True).decode()
    assert zero.replace("comment " + "-" * (COUNT_DIGITS - 1) + "\n", "") == HEADER.format(0)
    assert big.replace("comment " + "-" * (COUNT_DIGITS - 10) + "\n", "") == HEADER.format(10 ** 9)
    with pytest.raises(ValueError):
        ply_header(10 ** COUNT_DIGITS, fixed=True)
    records, offsets = CC.host_reference(CC.SHAPES[4], False, False, True)
    path = str(tmp_path / "scene.ply")
    with ScenePly(path) as scene:
        scene.append(records[:offsets[1]])
        scene.append(records[:0])
        scene.append(records[offsets[1]:].reshape(-1))
    assert scene.count == len(records) and np.array_equal(read_ply(path)[2], records)
    assert open(path, "rb").read() == ply_header(len(records), fixed=True) + records.tobytes()
    empty = ScenePly(str(tmp_path / "empty.ply")).close()
    assert read_ply(empty)[2].shape == (0, 16)


# ---- predict.py ------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def predict():
    """The predict module for the tests of its host logic.  predict.py prepares MIOpen's environment when it is imported, as a
    command-line tool does; in the test process that would reach every test file behind this one (the solvers their library
    convolutions get), so the environment is put back and the module is dropped again."""
    import importlib
    import os
    import sys
    saved = dict(os.environ)
    had = sys.modules.get("predict")
    try:
        yield importlib.import_module("predict")
    finally:
        os.environ.clear()
        os.environ.update(saved)
        if had is None:
            sys.modules.pop("predict", None)


def _transform(axis, angle, t):
    axis = np.asarray(axis, dtype=np.float64)
    axis /= np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)
    T[:3, 3] = t
    return T.astype(np.float32)


def test_scene_poses_are_the_float64_product(predict):
    T = np.stack([_transform((1, 2, 3), 0.7, (5, 6, 7)), _transform((0, 1, 0.1), 0.02, (0.01, -0.02, 1.3)), _transform((1, 0, 0.3), -0.05, (0.2, 0.0, 0.9))])
    G = predict.chain_poses(T)
    assert G.dtype == np.float64 and G.shape == (3, 4, 4)
    T64 = T.astype(np.float64)
    assert np.array_equal(G[0], np.eye(4))                                  # the first frame opens the chain: its own transform is not used
    assert np.array_equal(G[1], T64[1]) and np.array_equal(G[2], T64[1] @ T64[2])
    # split over two batches: the chain goes on from the last frame of the first
    first, second = predict.chain_poses(T[:2]), predict.chain_poses(T[2:], start=G[1])
    assert np.array_equal(np.concatenate([first, second]), G)
    assert np.array_equal(predict.chain_poses(T.reshape(3, 16)), G)
    # a point of frame 2 lands where two steps take it
    p = np.array([0.3, -0.2, 4.0, 1.0])
    assert np.allclose(G[2] @ p, T64[1] @ (T64[2] @ p), rtol=1e-15, atol=1e-15)


def test_scene_needs_frames_of_one_size(tmp_path, predict):
    """The check comes before any network runs: a stand-in trainer that only names the device is enough."""
    import os
    import shutil
    import types
    import torch
    from PIL import Image
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tiny_kitti_jpeg")
    names = sorted(os.listdir(golden))[:3]
    frames = tmp_path / "frames"
    frames.mkdir()
    for n in names:
        shutil.copy(os.path.join(golden, n), str(frames / n))
    with Image.open(os.path.join(golden, names[1])) as img:
        img.convert("RGB").resize((50, 30)).save(str(frames / (os.path.splitext(names[1])[0] + "b.png")))       # a second interior frame of another size
    opt = predict.parse([str(frames), "--weights_init", "scratch", "--log_dir", str(tmp_path / "logs"), "--motion", "--scene"])
    trainer = types.SimpleNamespace(device=torch.device("cpu"))
    with pytest.raises(ValueError, match="frames of one size"):
        predict.predict_folder(opt, trainer, str(frames), str(tmp_path / "out"), motion=True, scene=True)
    with pytest.raises(ValueError, match="--motion"):
        predict.predict_folder(opt, trainer, str(frames), str(tmp_path / "out"), motion=False, scene=True)
    assert not os.path.exists(str(tmp_path / "out" / "scene.ply"))


def test_scene_without_motion_is_refused_by_the_parser(tmp_path, capsys, predict):
    base = [str(tmp_path), "--weights_init", "scratch", "--log_dir", str(tmp_path / "logs")]
    with pytest.raises(SystemExit) as stop:
        predict.parse(base + ["--scene"])
    assert stop.value.code == 2 and "--scene needs --motion" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        predict.parse(base + ["--save", "cloud", "--cloud_stride", "0"])
    opt = predict.parse(base + ["--scene", "--motion", "--save", "cloud", "depth16"])
    assert opt.scene and opt.motion and opt.save == ["cloud", "depth16"]
    assert predict.cloud_parameters(opt) == {"stride": 1, "max_range": opt.max_depth, "edge": 0.05, "motion_thresh": 0.5}
    opt = predict.parse(base + ["--cloud_stride", "3", "--cloud_max_range", "40", "--cloud_edge", "0", "--cloud_motion_thresh", "2"])
    assert predict.cloud_parameters(opt) == {"stride": 3, "max_range": 40.0, "edge": 0.0, "motion_thresh": 2.0} and opt.save == ["depth16"]
    assert predict.cloud_intrinsics(np.array([[0.58, 0, 0.5, 0], [0, 1.92, 0.5, 0]], dtype=np.float32), 192, 640) == \
        (float(np.float32(0.58)) * 640, float(np.float32(1.92)) * 192, 320.0, 96.0)
