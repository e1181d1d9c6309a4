"""dd_export_cloud on the device against the numpy definition (hipops/cloud.py), bit for bit: records and offsets at the shapes of
cloud_case.SHAPES with and without the flip fuse, the motion mask and the pose; nothing written outside the kept records; the same
bytes from run to run; the arguments the wrapper and the entry point refuse; predict.py --save cloud and --scene end to end."""
import json
import os

import numpy as np
import pytest
import torch

import cloud_case as CC

pytestmark = pytest.mark.gpu

FRAMES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tiny_kitti_jpeg")
STEMS = sorted(os.path.splitext(f)[0] for f in os.listdir(FRAMES))
H, W = 192, 640                      # the golden frames' own size
NET = ["--weights_init", "scratch", "--depth_model", "litemono", "--height", "64", "--width", "96", "--num_workers", "0"]
POISON = 0xA5


def _device(B, h, w):
    return {k: torch.from_numpy(v.copy()).cuda() for k, v in CC.inputs(B, h, w).items()}


def _export(shape, flip, with_mask, with_pose):
    from hipops.cloud import export_cloud
    B, h, w, H_, W_, stride = shape
    x = _device(B, h, w)
    kw = dict(CC.params(), disp_flipped=x["flipped"] if flip else None, motion_mask=x["mask"] if with_mask else None,
              pose=x["pose"] if with_pose else None, stride=stride)
    return export_cloud(x["disp"].unsqueeze(1), x["color"], H_, W_, CC.intrinsics(H_, W_), **kw)


@pytest.mark.parametrize("flip", [False, True], ids=["plain", "pp"])
@pytest.mark.parametrize("shape", CC.SHAPES, ids=CC.IDS)
def test_export_cloud_is_the_host_definition(shape, flip):
    """Bytes, not values: a kept point is finite (its depth is in (0, max_range]), so no NaN payload can differ."""
    from hipops.cloud import candidates
    B, h, w, H_, W_, stride = shape
    for with_mask, with_pose in CC.VARIANTS:
        want, want_off = CC.host_reference(shape, flip, with_mask, with_pose)
        records, offsets = _export(shape, flip, with_mask, with_pose)
        assert records.is_cuda and records.dtype == torch.uint8 and tuple(records.shape) == (candidates(B, H_, W_, stride), 16)
        assert offsets.is_cuda and offsets.dtype == torch.int64 and np.array_equal(offsets.cpu().numpy(), want_off), (shape, flip, with_mask, with_pose)
        got = records[:int(want_off[-1])].cpu().numpy()
        assert np.array_equal(got, want), (shape, flip, with_mask, with_pose, int(np.argmax((got != want).any(1))))
    if h * w > 1:
        assert 0 < CC.host_reference(shape, flip, False, False)[1][-1] < candidates(B, H_, W_, stride)                # something kept, something dropped


def test_decisions_on_the_device():
    """The same-size case alone, decoded: the candidates of cloud_case.DECISIONS are in the cloud or not, as constructed."""
    from hipops.cloud import unpack_records
    B, h, w, H_, W_, _ = CC.SAME_SIZE
    records, offsets = _export(CC.SAME_SIZE, False, True, False)
    off = offsets.cpu().numpy()
    xyz = unpack_records(records[:off[1]].cpu().numpy())[0].astype(np.float64)
    fx, fy, cx, cy = CC.intrinsics(H_, W_)
    present = {(int(round(y / z * fy + cy)), int(round(x / z * fx + cx))) for x, y, z in xyz}
    for at, (kept, why) in CC.DECISIONS.items():
        assert (at in present) == kept, (at, why)


@pytest.mark.parametrize("shape", [CC.SHAPES[1], CC.SHAPES[4], CC.SHAPES[6]], ids=[CC.IDS[1], CC.IDS[4], CC.IDS[6]])
def test_nothing_is_written_outside_the_kept_records(shape):
    """The raw entry point on a records buffer and an offsets vector inside poisoned arenas: every byte in front of the records, every
    byte past offsets[B] * 16 (the rest of the caller's buffer included) and every byte around the offsets keeps the poison."""
    from hipops import abi, lib as L
    from hipops.cloud import candidates
    from hipops.export import _table
    B, h, w, H_, W_, stride = shape
    lib, s = L.load(), L.current_stream()
    x = _device(B, h, w)
    want, want_off = CC.host_reference(shape, True, True, True)
    room, lead = candidates(B, H_, W_, stride) * 16, 48
    arena = torch.full((lead + room + 64,), POISON, dtype=torch.uint8, device="cuda")
    oarena = torch.full((8 + 8 * (B + 1) + 8,), POISON, dtype=torch.uint8, device="cuda")
    need = lib.dd_export_cloud_workspace_bytes(B, H_, W_, stride)
    assert need > 0 and need % 8 == 0 and arena.data_ptr() % 16 == 0 and oarena.data_ptr() % 8 == 0
    ws = torch.empty(need // 8, dtype=torch.int64, device="cuda")
    p = CC.params()
    code = lib.dd_export_cloud(abi.ptr(x["disp"]), abi.ptr(x["flipped"]), abi.ptr(_table("l_mask", w, x["disp"].device)), abi.ptr(x["color"]), abi.ptr(x["mask"]),
                               abi.ptr(x["pose"]), B, h, w, H_, W_, *CC.intrinsics(H_, W_), p["min_depth"], p["max_depth"], p["max_range"], p["edge"],
                               p["motion_thresh"], stride, abi.C.c_void_p(arena.data_ptr() + lead), abi.C.c_void_p(oarena.data_ptr() + 8), abi.ptr(ws), need, s)
    assert code == 0
    host, ohost = arena.cpu().numpy(), oarena.cpu().numpy()
    arena.zero_(), oarena.zero_()           # the poison does not stay in the blocks that go back to the allocator
    used = int(want_off[-1]) * 16
    assert 0 < used < room
    assert (host[:lead] == POISON).all() and (host[lead + used:] == POISON).all()
    assert np.array_equal(host[lead:lead + used].reshape(-1, 16), want)
    assert (ohost[:8] == POISON).all() and (ohost[-8:] == POISON).all() and np.array_equal(ohost[8:-8].copy().view(np.int64), want_off)


def test_two_runs_give_the_same_bytes():
    shape = CC.SHAPES[4]
    a, b = _export(shape, True, True, True), _export(shape, True, True, True)
    n = int(a[1][-1])
    assert n > 0 and torch.equal(a[1], b[1]) and torch.equal(a[0][:n], b[0][:n])


def test_bad_arguments_are_refused():
    from hipops import abi, lib as L
    from hipops.cloud import export_cloud
    from hipops.lib import DynamoHipError
    disp = torch.rand(2, 1, 4, 6, device="cuda")
    color = torch.rand(2, 3, 4, 6, device="cuda")
    cam = (5.0, 5.0, 6.0, 4.0)
    kw = dict(min_depth=0.1, max_depth=100.0)
    for bad in (lambda: export_cloud(disp.cpu(), color, 8, 12, cam, **kw),
                lambda: export_cloud(disp, color.cpu(), 8, 12, cam, **kw),
                lambda: export_cloud(disp, color[:, :2], 8, 12, cam, **kw),
                lambda: export_cloud(disp, color[:1], 8, 12, cam, **kw),
                lambda: export_cloud(disp, color.double(), 8, 12, cam, **kw),
                lambda: export_cloud(disp.double(), color, 8, 12, cam, **kw),
                lambda: export_cloud(disp[0, 0, 0], color, 8, 12, cam, **kw),
                lambda: export_cloud(disp, color, 8, 12, cam, disp_flipped=disp.cpu(), **kw),
                lambda: export_cloud(disp, color, 8, 12, cam, disp_flipped=disp[:, :, :, :5], **kw),
                lambda: export_cloud(disp, color, 8, 12, cam, motion_mask=disp[:1], **kw),
                lambda: export_cloud(disp, color, 8, 12, cam, motion_mask=disp.cpu(), **kw),
                lambda: export_cloud(disp, color, 8, 12, cam, pose=torch.zeros(2, 3, 3, device="cuda"), **kw),
                lambda: export_cloud(disp, color, 8, 12, cam, pose=torch.zeros(2, 3, 4), **kw),
                lambda: export_cloud(disp, color, 8, 12, cam, pose=torch.zeros(2, 3, 4, dtype=torch.float64, device="cuda"), **kw),
                lambda: export_cloud(disp, color, 0, 12, cam, **kw),
                lambda: export_cloud(disp, color, 8, 0, cam, **kw),
                lambda: export_cloud(disp, color, 8, 12, cam, stride=0, **kw),
                lambda: export_cloud(disp, color, 8, 12, (0.0, 5.0, 6.0, 4.0), **kw),
                lambda: export_cloud(disp, color, 8, 12, (5.0, float("inf"), 6.0, 4.0), **kw),
                lambda: export_cloud(disp, color, 8, 12, cam, min_depth=0.0, max_depth=100.0)):
        with pytest.raises(DynamoHipError):
            bad()
    # the entry point itself: every refusal returns hipErrorInvalidValue and leaves the poisoned outputs alone
    lib, s = L.load(), L.current_stream()
    d = disp[:, 0].contiguous()
    mask, lmask, pose = torch.zeros(2, 4, 6, device="cuda"), torch.zeros(6, device="cuda"), torch.zeros(2, 3, 4, device="cuda")
    records = torch.full((2 * 8 * 12, 16), POISON, dtype=torch.uint8, device="cuda")
    offsets = torch.full((3,), 7, dtype=torch.int64, device="cuda")
    need = lib.dd_export_cloud_workspace_bytes(2, 8, 12, 1)
    assert need == 2 * 8 * 8
    ws = torch.full((need // 8 + 1,), 7, dtype=torch.int64, device="cuda")
    P = abi.ptr
    names = ["disp", "flip", "lmask", "color", "mask", "pose", "B", "h", "w", "H", "W", "fx", "fy", "cx", "cy", "min_depth", "max_depth", "max_range", "edge",
             "thresh", "stride", "records", "offsets", "ws", "ws_bytes"]
    good = [P(d), None, None, P(color), P(mask), P(pose), 2, 4, 6, 8, 12, 5.0, 5.0, 6.0, 4.0, 0.1, 100.0, 100.0, 0.05, 0.5, 1, P(records), P(offsets), P(ws), need]

    def call(**change):
        args = list(good)
        for k, v in change.items():
            args[names.index(k)] = v
        return lib.dd_export_cloud(*args, s)

    off = lambda t, n: abi.C.c_void_p(t.data_ptr() + n)           # noqa: E731
    assert all(call(**{k: None}) == 1 for k in ("disp", "color", "records", "offsets", "ws"))
    assert call(flip=P(d)) == 1 and call(lmask=P(lmask)) == 1
    assert all(call(**{k: 0}) == 1 for k in ("B", "h", "w", "H", "W", "stride")) and call(H=-3) == 1 and call(stride=-1) == 1
    assert call(H=65536, W=32768) == 1 and call(h=65536, w=32768) == 1            # 2**31 pixels
    assert all(call(**{k: v}) == 1 for k in ("fx", "fy") for v in (0.0, float("inf"), float("-inf"), float("nan")))
    assert call(min_depth=0.0) == 1 and call(max_depth=-1.0) == 1 and call(max_depth=float("nan")) == 1
    assert all(call(**{k: off(t, 2)}) == 1 for k, t in (("disp", d), ("color", color), ("mask", mask), ("pose", pose)))
    assert call(flip=off(d, 2), lmask=P(lmask)) == 1 and call(flip=P(d), lmask=off(lmask, 2)) == 1
    assert call(records=off(records, 8)) == 1 and call(records=off(records, 4)) == 1 and call(offsets=off(offsets, 4)) == 1 and call(ws=off(ws, 4)) == 1
    assert call(ws_bytes=need - 1) == 1
    assert lib.dd_export_cloud_workspace_bytes(0, 8, 12, 1) == 0 and lib.dd_export_cloud_workspace_bytes(2, 8, 12, 0) == 0
    assert lib.dd_export_cloud_workspace_bytes(1, 65536, 32768, 1) == 0
    torch.cuda.synchronize()
    assert bool((records == POISON).all()) and bool((offsets == 7).all()) and bool((ws == 7).all())
    assert call(stride=5) == 0 and call() == 0            # what stride 5 keeps, stride 1 keeps too: the second call overwrites the first from the front
    torch.cuda.synchronize()
    n = int(offsets[2])
    clean = bool((records[n:] == POISON).all()) and int(ws[-1]) == 7          # one word past the workspace's size is not touched
    records.zero_(), ws.zero_(), offsets.zero_()        # the poison does not stay in the blocks that go back to the allocator
    assert 0 < n <= 192 and clean


def test_the_wrapper_does_not_synchronise():
    """Under torch.cuda.set_sync_debug_mode("error") any host synchronisation of the wrapper raises."""
    shape = CC.SHAPES[4]
    B, h, w, H_, W_, stride = shape
    x = _device(B, h, w)
    from hipops.cloud import export_cloud
    kw = dict(CC.params(), disp_flipped=x["flipped"], motion_mask=x["mask"], pose=x["pose"], stride=stride)
    export_cloud(x["disp"], x["color"], H_, W_, CC.intrinsics(H_, W_), **kw)       # the tables are made on the first call
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        records, offsets = export_cloud(x["disp"], x["color"], H_, W_, CC.intrinsics(H_, W_), **kw)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    want, want_off = CC.host_reference(shape, True, True, True)
    assert np.array_equal(offsets.cpu().numpy(), want_off) and np.array_equal(records[:int(want_off[-1])].cpu().numpy(), want)


# ---- predict.py ------------------------------------------------------------------------------------------------------------------
RUNS = {
    "cloud": ["-b", "2", "--save", "depth16", "cloud", "--cloud_stride", "3", "--post_process"],
    "scene2": ["-b", "3", "--motion", "--scene", "--cloud_stride", "2", "--cloud_motion_thresh", "2"],
    "scene": ["-b", "3", "--motion", "--scene", "--cloud_stride", "2"],
}


@pytest.fixture(scope="module")
def predict_runs(tmp_path_factory):
    """predict.main over the golden frames, once per entry of RUNS, all in ONE child process (tests/cloud_predict_worker.py says why
    not in this one) -> {name: (written paths, out dir, {stem: predict_batch's tensors for that frame, on the host})}."""
    import subprocess
    import sys
    root = tmp_path_factory.mktemp("predict_cloud")
    job = root / "job.json"
    job.write_text(json.dumps({"frames": FRAMES, "out": str(root), "runs": {name: NET + extra for name, extra in RUNS.items()}}))
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cloud_predict_worker.py")
    done = subprocess.run([sys.executable, worker, str(job)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=240)
    assert done.returncode == 0, done.stdout[-4000:]
    runs = {}
    for name in RUNS:
        seen = {}
        with np.load(str(root / (name + "_seen.npz"))) as data:
            for key in data.files:                                  # in the order the frames were seen
                stem, what = key.split("/")
                seen.setdefault(stem, {})[what] = data[key]
        runs[name] = (json.loads((root / (name + "_written.json")).read_text()), str(root / name), seen)
    return runs


def _host_cloud(frame, camera, params, pose=None, static=False):
    from hipops.cloud import export_cloud_host
    return export_cloud_host(frame["disp"], frame["color"][None], H, W, camera, disp_flipped=frame.get("disp_flipped"),
                             motion_mask=frame["motion_mask"] if static else None, pose=None if pose is None else pose[None], min_depth=0.1, max_depth=100.0,
                             max_range=params["max_range"], edge=params["edge"], motion_thresh=params["motion_thresh"], stride=params["stride"])[0]


def test_predict_save_cloud(predict_runs):
    from PIL import Image
    from hipops.cloud import read_ply
    from hipops.export import export_depth_host
    written, out, seen = predict_runs["cloud"]
    assert sorted(seen) == STEMS and sorted(os.listdir(out)) == ["cloud", "depth", "predict.json"]
    assert sorted(written) == sorted([os.path.join(out, d, s + e) for s in STEMS for d, e in (("depth", ".png"), ("cloud", ".ply"))] + [os.path.join(out, "predict.json")])
    meta = json.load(open(os.path.join(out, "predict.json")))
    cloud = meta["cloud"]
    assert (cloud["stride"], cloud["max_range"], cloud["edge"], cloud["motion_thresh"]) == (3, 100.0, 0.05, 0.5) and "up to scale" in cloud["note"]
    camera = cloud["intrinsics"]["{}x{}".format(H, W)]
    assert np.allclose(camera, [0.58 * W, 1.92 * H, 0.5 * W, 0.5 * H], rtol=1e-6) and list(cloud["points"]) == STEMS and "scene_points" not in cloud
    for stem in STEMS:
        frame = seen[stem]
        assert set(frame) == {"disp", "disp_flipped", "color"} and frame["color"].shape == (3, 64, 96) and frame["disp"].shape == (1, 64, 96)
        want = _host_cloud(frame, camera, cloud)
        xyz, rgba, got = read_ply(os.path.join(out, "cloud", stem + ".ply"))
        assert np.array_equal(got, want) and cloud["points"][stem] == len(want) and 0 < len(want) <= 64 * 214
        assert (xyz[:, 2] > 0).all() and len(np.unique(rgba[:, :3], axis=0)) > 16                     # a picture's colours, not one value
        # the other outputs of the run are what they are without the clouds
        with Image.open(os.path.join(out, "depth", stem + ".png")) as img:
            d16 = np.asarray(img).astype(np.uint16)
        assert np.array_equal(d16, export_depth_host(frame["disp"], H, W, disp_flipped=frame["disp_flipped"], min_depth=0.1, max_depth=100.0)["depth16"][0])


@pytest.mark.parametrize("run", ["scene2", "scene"], ids=["thresh2", "default"])
def test_predict_scene(predict_runs, run):
    """--scene: the static points of the four interior frames in the first one's coordinates.  With a threshold of 2 an untrained mask
    (a sigmoid, at most 1) drops nothing, so the file is not empty; at the default threshold the file is the host definition whatever
    the untrained mask yields."""
    from hipops.cloud import chain_poses, read_ply
    written, out, seen = predict_runs[run]
    interior = STEMS[1:-1]
    assert list(seen) == interior and len(interior) == 4
    assert sorted(os.listdir(out)) == ["depth", "motion_mask", "poses.txt", "predict.json", "scene.ply"] and os.path.join(out, "scene.ply") in written
    meta = json.load(open(os.path.join(out, "predict.json")))
    cloud = meta["cloud"]
    camera = cloud["intrinsics"]["{}x{}".format(H, W)]
    assert cloud["motion_thresh"] == (2.0 if run == "scene2" else 0.5) and "points" not in cloud and list(cloud["scene_points"]) == interior
    assert all(set(seen[s]) == {"disp", "motion_mask", "cam_T_cam", "color"} for s in interior)
    G = chain_poses(np.stack([seen[s]["cam_T_cam"] for s in interior]))      # two batches in the run (3 + 1), one chain here
    assert np.array_equal(G[0], np.eye(4)) and not np.array_equal(G[3], G[2])
    parts = [_host_cloud(seen[s], camera, cloud, pose=G[i, :3].astype(np.float32), static=True) for i, s in enumerate(interior)]
    xyz, rgba, got = read_ply(os.path.join(out, "scene.ply"))
    assert np.array_equal(got, np.concatenate(parts))
    assert len(got) == cloud["scene_total"] == sum(cloud["scene_points"].values()) and [cloud["scene_points"][s] for s in interior] == [len(p) for p in parts]
    first = _host_cloud(seen[interior[0]], camera, cloud, static=True)                       # the first frame is its own pose-free cloud
    assert np.array_equal(got[:len(first)], first) and len(first) == len(parts[0])
    if run == "scene2":
        assert all(len(p) > 0 for p in parts) and (seen[interior[0]]["motion_mask"] <= 1).all()
        unfiltered = _host_cloud(seen[interior[1]], camera, cloud, pose=G[1, :3].astype(np.float32), static=False)
        assert np.array_equal(parts[1], unfiltered)                                          # nothing dropped by the mask
