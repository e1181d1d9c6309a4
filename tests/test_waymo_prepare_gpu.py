"""The device steps of the Waymo preparation (csrc/dd_range_image.hip, csrc/dd_undistort.hip through hipops.lidar and
hipops.undistort) against their numpy definitions, and prepare_data/waymo.py with the device callables against the
host callables.

dd_range_image_points reads the host's trigonometric tables and computes the definition's float64 operations in the definition's
order; only the pose image's six sines and cosines come from another library.  counts and cp are exact; points agree within
64 * 2^-52 * (G + 75) m (G the case's largest pose translation: a few float64 roundings at the global magnitude; derived, not
measured), the rows' depth within the same bound and u, v within it times f / z_min.  tests/test_waymo_prepare.py asserts on the host
that no point of the case lies within 1000 times that bound of a threshold, so the tolerance cannot move a decision; a second case
puts points on the thresholds with exact arithmetic and asks for equality.  dd_undistort is bit for bit the definition."""
import ctypes
import os
import os.path as osp

import numpy as np
import pytest
import torch

import waymo_prepare_case as wc

pytestmark = pytest.mark.gpu

_case = {}


def lidar_case():
    if not _case:
        from hipops import lidar
        _case["inputs"] = wc.definition_inputs([wc.lidar_frame(seed) for seed in (0, 1, 2)])
        _case["host"] = lidar.range_image_points_host(*_case["inputs"])
    return _case["inputs"], _case["host"]


def test_range_image_points_equal_the_definition():
    from hipops import lidar
    inputs, (want, want_counts) = lidar_case()
    got, counts = lidar.range_image_points(*inputs)
    assert counts.dtype == np.int32 and np.array_equal(counts, want_counts)
    bound, f = wc.points_bound(), max(wc.CAM_INTRINSIC[:2])
    worst = [0.0, 0.0, 0.0]
    for s, ((points, cp, rows), (w_points, w_cp, w_rows)) in enumerate(zip(got, want)):
        assert points.dtype == rows.dtype == np.float64 and cp.dtype == np.int32
        assert points.shape == w_points.shape and rows.shape == w_rows.shape and np.array_equal(cp, w_cp), s
        if points.size:
            worst[0] = max(worst[0], float(np.abs(points - w_points).max()))
        if rows.size:
            worst[1] = max(worst[1], float(np.abs(rows[:, 2] - w_rows[:, 2]).max()))
            worst[2] = max(worst[2], float((np.abs(rows[:, :2] - w_rows[:, :2]).max(axis=1) * w_rows[:, 2]).max()) / f)
            if inputs[2][s] is None:                                # no pose: the same tables, the same operations
                assert np.array_equal(rows, w_rows) and np.array_equal(points, w_points), s
    print("points {:.3e} m, depth {:.3e} m, pixels times z / f {:.3e} m against the bound {:.3e} m".format(*worst, bound))
    assert worst[0] <= bound and worst[1] <= bound
    for (points, cp, rows), (w_points, w_cp, w_rows) in zip(got, want):
        if rows.size:
            assert (np.abs(rows[:, :2] - w_rows[:, :2]) <= bound * f / w_rows[:, 2].min()).all()


def test_range_image_points_on_the_exact_thresholds():
    from hipops import lidar
    inputs, expected = wc.exact_case()
    want, want_counts = lidar.range_image_points_host(*inputs)
    got, counts = lidar.range_image_points(*inputs)
    assert np.array_equal(counts, want_counts)
    assert counts.tolist() == [[0 if e is None else 1, 1 if e else 0] for e in expected]
    for g, w in zip(got, want):
        for a, b in zip(g, w):
            assert a.shape == b.shape and a.tobytes() == b.tobytes()


def test_range_image_points_at_the_real_image_sizes():
    """One frame's five images at the real sizes (64 x 2650 with a pose, four of 200 x 600): many blocks per image, blocks that end
    inside a row, images of different sizes in one chunk."""
    from hipops import lidar
    rng = np.random.default_rng(9)
    frame_pose = wc.rigid(0.4, 0.01, -0.02, [wc.GLOBAL, -wc.GLOBAL, 20.0])
    K = np.array([[2044.5, 0, 949.6], [0, 2044.5, 633.2], [0, 0, 1.0]])
    e2c = lidar.vehicle_to_camera(wc.CAM_EXTRINSIC)
    ranges, cps, poses, trigs, params = [], [], [], [], []
    for name, (H, W) in enumerate([(64, 2650)] + [(200, 600)] * 4):
        rho = rng.uniform(2.0, 70.0, size=(H, W)).astype(np.float32)
        rho[rng.uniform(size=(H, W)) < 0.3] = -1.0
        pose = None
        if name == 0:
            pose = np.zeros((H, W, 6), dtype=np.float32)
            pose[:, :, :3], pose[:, :, 3:] = [-0.02, 0.01, 0.4], frame_pose[:3, 3]
        extrinsic = wc.rigid(0.5 * name, 0.0, 0.0, [1.4, 0.0, 2.0 - 0.2 * name])
        ranges.append(rho), poses.append(pose)
        cps.append(rng.integers(0, 1000, size=(H, W, 3)).astype(np.int32))
        trigs.append(lidar.range_image_trig(lidar.inclination_table(H, [], -0.31, 0.04), W, extrinsic))
        params.append(lidar.range_image_params(extrinsic, frame_pose if pose is not None else None, e2c, K, 1920, 1280))
    inputs = (ranges, cps, poses, trigs, np.stack(params))
    want, want_counts = lidar.range_image_points_host(*inputs)
    got, counts = lidar.range_image_points(*inputs)
    assert np.array_equal(counts, want_counts)
    assert want_counts[:, 1].min() > 100
    for s in range(5):
        assert np.array_equal(got[s][1], want[s][1])
        assert np.abs(got[s][0] - want[s][0]).max() <= wc.points_bound()
        if s:
            assert np.array_equal(got[s][2], want[s][2]) and np.array_equal(got[s][0], want[s][0])


def test_range_image_points_refuses_what_it_cannot_do():
    from hipops import lidar
    from hipops import lib as L
    inputs, _ = lidar_case()
    rng, cp, pose, trig, desc = lidar.range_image_pack(*inputs[:4])
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (rng, cp, pose, trig, inputs[4])]
    with pytest.raises(L.DynamoHipError):
        lidar.range_image_points_device(dev[0].double(), dev[1], dev[2], dev[3], desc, dev[4])
    with pytest.raises(L.DynamoHipError):
        lidar.range_image_points_device(dev[0].cpu(), dev[1], dev[2], dev[3], desc, dev[4])
    for column, value in ((0, 5), (1, 9), (3, 100000), (4, trig.size), (2, -1)):      # overlap, past the end, pose and table out of range, a size
        bad = desc.copy()
        bad[1, column] = value
        with pytest.raises(L.DynamoHipError, match="dd_range_image_points"):
            lidar.range_image_points_device(dev[0], dev[1], dev[2], dev[3], bad, dev[4])
    lib = L.load()
    assert lib.dd_range_image_points_workspace_bytes(0, 10) == 0 and lib.dd_range_image_points_workspace_bytes(3, 0) == 0
    assert lib.dd_range_image_points_workspace_bytes(40, 257) == 2 * 16 * 2 * 4


UNDISTORT_CASES = [(1, 22, 31, "none"), (2, 22, 31, "k1"), (3, 22, 31, "strong"), (2, 9, 260, "strong"), (3, 37, 516, "k1"), (1, 5, 3, "strong"),
                   (1, 1280, 1920, "real")]


@pytest.mark.parametrize("n,H,W,strength", UNDISTORT_CASES)
def test_undistort_equals_the_definition(n, H, W, strength):
    """Bit for bit: widths that are and are not multiples of four (dword and byte stores), more than one block per row, one pixel
    rows, taps outside on every side, and one frame of the real size with the fixture's calibration."""
    from hipops import undistort
    frames = wc.checkerboard(n, H, W, cell=5, seed=H + W)
    cal = [2044.5083584358413, 2044.5083584358413, 949.5746451352071, 633.2422462156501, 0.040358363932006036, -0.33001662226602974,
           0.0010402702690110032, -0.0015669020781401406, 0.0] if strength == "real" else wc.calibration(H, W, strength)
    want = undistort.undistort_host(frames, cal)
    got = undistort.undistort_batch(torch.from_numpy(frames).cuda(), cal)
    assert got.dtype == torch.uint8 and tuple(got.shape) == frames.shape
    got = got.cpu().numpy()
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    if strength == "none":
        assert np.array_equal(got, frames)
    else:
        assert not np.array_equal(got, frames)


def test_undistort_refuses_what_it_cannot_do():
    from hipops import undistort
    from hipops import lib as L
    x = torch.zeros((1, 4, 4, 3), dtype=torch.uint8, device="cuda")
    cal = wc.calibration(4, 4, "k1")
    for bad in (lambda: undistort.undistort_batch(x.cpu(), cal), lambda: undistort.undistort_batch(x.float(), cal),
                lambda: undistort.undistort_batch(x, cal[:8]), lambda: undistort.undistort_batch(x, [float("nan")] + cal[1:]),
                lambda: undistort.undistort_batch(x, [0.0] + cal[1:])):
        with pytest.raises(L.DynamoHipError):
            bad()
    lib = L.load()
    arr = (ctypes.c_double * 9)(*cal)
    assert lib.dd_undistort(None, 1, 4, 4, arr, ctypes.c_void_p(x.data_ptr()), None) == 1
    assert lib.dd_undistort(ctypes.c_void_p(x.data_ptr()), 0, 4, 4, arr, ctypes.c_void_p(x.data_ptr()), None) == 1
    assert lib.dd_undistort(ctypes.c_void_p(x.data_ptr() + 1), 1, 2, 2, arr, ctypes.c_void_p(x.data_ptr()), None) == 1


def tree_files(root):
    return {osp.relpath(osp.join(d, f), root): osp.join(d, f) for d, _, files in os.walk(root) for f in files}


def test_script_with_the_device_steps_writes_the_host_steps_files(tmp_path):
    import pickle

    from prepare_data import waymo
    records = str(tmp_path / "records")
    wc.write_records(records)
    roots = [str(tmp_path / "host"), str(tmp_path / "device")]
    waymo.prepare(records, roots[0], batch=2, num_workers=3, log=lambda s: None, **wc.host_steps())
    waymo.prepare(records, roots[1], batch=2, num_workers=3, log=lambda s: None, messages=wc.MESSAGES)
    a, b = tree_files(roots[0]), tree_files(roots[1])
    assert sorted(a) == sorted(b) and len(a) == 3 + 3 + 3 + 2 + 2
    bound = wc.points_bound()
    for rel in a:
        if rel.endswith(".npy"):
            x, y = np.load(a[rel]), np.load(b[rel])
            assert x.shape == y.shape and np.abs(x[:, 2] - y[:, 2]).max() <= bound
            assert (np.abs(x[:, :2] - y[:, :2]).max(axis=1) <= bound * 41.0 / x[:, 2].min()).all()
        elif rel.endswith(".npz"):
            with np.load(a[rel]) as x, np.load(b[rel]) as y:
                assert np.array_equal(x["semantic"], y["semantic"]) and np.array_equal(x["instance"], y["instance"])
        elif rel.endswith(".pickle"):
            x, y = pickle.load(open(a[rel], "rb")), pickle.load(open(b[rel], "rb"))
            assert len(x) == len(y) == 3
            for p, q in zip(x, y):
                assert list(p) == list(q)
                assert all(p[k] == q[k] for k in p if k != "mask") and [c.tobytes() for c in p["mask"]] == [c.tobytes() for c in q["mask"]]
        else:
            assert open(a[rel], "rb").read() == open(b[rel], "rb").read(), rel
