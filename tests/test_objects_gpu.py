"""dd_objects on the device against the numpy definition (hipops/objects.py): labels, counts and the integer and depth-range columns
exactly, the seven float64 sums within the bound of two orders of one sum (objects_case.sum_bound), for every shape, mask and both
connectivities of objects_case; min_pixels, the cap, two runs, nothing written outside the outputs, a workspace full of garbage, the
arguments that are refused, the label image, and predict.py --save objects end to end."""
import json
import os

import numpy as np
import pytest
import torch

import objects_case as OC

pytestmark = pytest.mark.gpu

FRAMES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tiny_kitti_jpeg")
STEMS = sorted(os.path.splitext(f)[0] for f in os.listdir(FRAMES))
H, W = 192, 640                      # the golden frames' own size
NET = ["--weights_init", "scratch", "--depth_model", "litemono", "--height", "64", "--width", "96", "--num_workers", "0"]
POISON = 0xA5
SHAPE_IDS = ["x".join(map(str, s)) for s in OC.SHAPES]


def _device(shape, name):
    return {k: torch.from_numpy(v.copy()).cuda() for k, v in OC.inputs(shape, name).items()}


def _find(shape, name, connectivity, min_pixels=1, max_objects=OC.CAP):
    from hipops.objects import find_objects
    x = _device(shape, name)
    out = find_objects(x["mask"], x["disp"], x["flow"], x["ts"], x["pose"], OC.intrinsics(*shape), disp_flipped=x["flipped"] if OC.uses_flip(shape, name) else None,
                       min_depth=OC.MIN_DEPTH, max_depth=OC.MAX_DEPTH, thresh=OC.THRESH, connectivity=connectivity, min_pixels=min_pixels, max_objects=max_objects)
    return tuple(t.cpu().numpy() for t in out)


def _check(shape, name, connectivity, min_pixels=1, max_objects=OC.CAP, got=None):
    want = OC.reference(shape, name, connectivity, min_pixels, max_objects)
    bound = OC.sum_bound(want[0], OC.quantities(shape, name), max_objects)
    got = _find(shape, name, connectivity, min_pixels, max_objects) if got is None else got
    OC.compare(*got, want, bound, (shape, name, connectivity, min_pixels, max_objects))
    return got, want, bound


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("shape", OC.SHAPES, ids=SHAPE_IDS)
def test_objects_are_the_host_definition(shape, connectivity):
    from hipops.objects import ROW
    for name in OC.NAMES:
        (labels, table, counts), _, _ = _check(shape, name, connectivity)
        assert labels.dtype == np.int32 and labels.shape == (OC.B,) + shape and table.shape == (OC.B, OC.CAP, ROW) and counts.shape == (OC.B, 3)


@pytest.mark.parametrize("min_pixels", [1, 2, 16])
@pytest.mark.parametrize("name", ["bernoulli50", "blobs"])
def test_min_pixels(name, min_pixels):
    for connectivity in (4, 8):
        _, want, _ = _check((37, 53), name, connectivity, min_pixels)
        if min_pixels > 1 and name == "bernoulli50":        # a random field has single pixels and small groups; a smooth one need not
            assert (want[2][:, 1] < OC.reference((37, 53), name, connectivity)[2][:, 1]).all()            # the rule dropped something


def test_truncation_on_the_checkerboard():
    shape, name, connectivity, components = OC.TRUNCATED
    (labels, table, counts), _, _ = _check(shape, name, connectivity, 1, OC.DEFAULT_CAP)
    assert counts[0].tolist() == [256, 981, 1] and labels[0].max() == 256
    full = OC.reference(shape, name, connectivity)[0][0]
    assert (labels[0][full > 256] == 0).all() and np.array_equal(labels[0][full <= 256], full[full <= 256])        # labels above the cap are 0


def test_two_runs_agree():
    """Labels and integer columns identical; the sums of both runs are orders of the same terms, so the same bound holds between them."""
    from hipops.objects import rows
    shape, name = (130, 67), "bernoulli60"
    a, want, bound = _check(shape, name, 8)
    b = _find(shape, name, 8)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]) and np.array_equal(a[1][:, :, :8], b[1][:, :, :8])
    sa, sb = rows(a[1])["sums"], rows(b[1])["sums"]
    finite = np.isfinite(sa)
    assert np.array_equal(finite, np.isfinite(sb)) and (np.abs(sa[finite] - sb[finite]) <= bound[finite]).all()


def _raw(shape, name, connectivity, min_pixels, max_objects, labels, table, counts, ws, ws_bytes, **change):
    """The entry point itself on caller-made buffers (addresses); `change`: arguments replaced by name."""
    from hipops import abi, lib as L
    from hipops.export import _table, depth_params
    h, w = shape
    x = _device(shape, name)
    flip = OC.uses_flip(shape, name)
    lo, span = depth_params(OC.MIN_DEPTH, OC.MAX_DEPTH)
    fx, fy, cx, cy = OC.intrinsics(h, w)
    args = dict(mask=abi.ptr(x["mask"]), disp=abi.ptr(x["disp"]), flip=abi.ptr(x["flipped"]) if flip else None,
                lmask=abi.ptr(_table("l_mask", w, "cuda:0")) if flip else None, flow=abi.ptr(x["flow"]), ts=abi.ptr(x["ts"]), pose=abi.ptr(x["pose"]), B=OC.B, h=h, w=w,
                fx=fx, fy=fy, cx=cx, cy=cy, lo=float(lo), span=float(span), thresh=OC.THRESH, connectivity=connectivity, min_pixels=min_pixels,
                max_objects=max_objects, labels=labels, table=table, counts=counts, ws=ws, ws_bytes=ws_bytes)
    assert set(change) <= set(args)
    args.update(change)
    code = L.load().dd_objects(*args.values(), L.current_stream())
    torch.cuda.synchronize()
    return code


@pytest.mark.parametrize("shape,name,connectivity,max_objects", [((37, 53), "blobs", 8, 40), ((5, 7), "bernoulli50", 4, 9), ((64, 96), "checker", 4, 256)],
                         ids=["blobs", "small", "truncated"])
def test_nothing_is_written_outside_the_outputs(shape, name, connectivity, max_objects):
    """labels, table and counts inside poisoned arenas: every byte around them keeps the poison, and the table's rows at and past the
    kept count read as zero (the reference's rows there are zero, and the whole table is compared)."""
    from hipops import abi, lib as L
    from hipops.objects import ROW
    h, w = shape
    n = OC.B * h * w
    sizes = {"labels": 4 * n, "table": 4 * OC.B * max_objects * ROW, "counts": 4 * OC.B * 3}
    lead = 64
    arenas = {k: torch.full((lead + v + 64,), POISON, dtype=torch.uint8, device="cuda") for k, v in sizes.items()}
    assert all(a.data_ptr() % 8 == 0 for a in arenas.values())
    need = L.load().dd_objects_workspace_bytes(OC.B, h, w, max_objects)
    assert need == 8 * n
    ws = torch.empty(need // 8 + 1, dtype=torch.int64, device="cuda")
    ws[-1] = 7
    at = {k: abi.C.c_void_p(a.data_ptr() + lead) for k, a in arenas.items()}
    assert _raw(shape, name, connectivity, 1, max_objects, at["labels"], at["table"], at["counts"], abi.ptr(ws), need) == 0
    host = {k: a.cpu().numpy() for k, a in arenas.items()}
    past = int(ws[-1])
    for a in arenas.values():
        a.zero_()               # the poison does not stay in the blocks that go back to the allocator
    assert past == 7            # one word past the workspace's size is not touched
    for k, v in sizes.items():
        assert (host[k][:lead] == POISON).all() and (host[k][lead + v:] == POISON).all(), k
    got = (host["labels"][lead:lead + sizes["labels"]].copy().view(np.int32).reshape(OC.B, h, w),
           host["table"][lead:lead + sizes["table"]].copy().view(np.int32).reshape(OC.B, max_objects, ROW),
           host["counts"][lead:lead + sizes["counts"]].copy().view(np.int32).reshape(OC.B, 3))
    _, want, _ = _check(shape, name, connectivity, 1, max_objects, got=got)
    kept = want[2][:, 0]
    assert all(not got[1][b, kept[b]:].any() for b in range(OC.B)) and ((kept < max_objects).any() or want[2][:, 2].all())


def test_the_workspace_need_not_be_cleared():
    from hipops import abi, lib as L
    from hipops.objects import ROW
    shape, name, connectivity = (37, 53), "bernoulli50", 8
    h, w = shape
    need = L.load().dd_objects_workspace_bytes(OC.B, h, w, OC.CAP)
    results = []
    for fill in (POISON, 0):
        ws = torch.full((need,), fill, dtype=torch.uint8, device="cuda")
        labels = torch.empty((OC.B, h, w), dtype=torch.int32, device="cuda")
        table = torch.empty((OC.B, OC.CAP, ROW), dtype=torch.int32, device="cuda")
        counts = torch.empty((OC.B, 3), dtype=torch.int32, device="cuda")
        assert _raw(shape, name, connectivity, 1, OC.CAP, abi.ptr(labels), abi.ptr(table), abi.ptr(counts), abi.ptr(ws), need) == 0
        results.append((labels.cpu().numpy(), table.cpu().numpy(), counts.cpu().numpy()))
        ws.zero_()
        _check(shape, name, connectivity, got=results[-1])
    assert np.array_equal(results[0][0], results[1][0]) and np.array_equal(results[0][2], results[1][2])
    assert np.array_equal(results[0][1][:, :, :8], results[1][1][:, :, :8])


def test_bad_arguments_are_refused():
    from hipops import abi, lib as L
    from hipops.lib import DynamoHipError
    from hipops.objects import ROW, find_objects, labels_u16
    mask, disp = torch.rand(2, 1, 4, 6, device="cuda"), torch.rand(2, 1, 4, 6, device="cuda")
    flow, ts, pose = torch.rand(2, 3, 4, 6, device="cuda"), torch.ones(2, device="cuda"), torch.zeros(2, 3, 4, device="cuda")
    cam = (5.0, 5.0, 3.0, 2.0)
    kw = dict(min_depth=0.1, max_depth=100.0)
    assert find_objects(mask, disp, flow, ts, pose, cam, **kw)[0].shape == (2, 4, 6)
    for bad in (lambda: find_objects(mask, disp, flow, ts, pose, cam, connectivity=6, **kw),
                lambda: find_objects(mask, disp, flow, ts, pose, cam, connectivity=0, **kw),
                lambda: find_objects(mask, disp, flow, ts, pose, cam, min_pixels=0, **kw),
                lambda: find_objects(mask, disp, flow, ts, pose, cam, max_objects=0, **kw),
                lambda: find_objects(mask, disp, flow, ts, pose, cam, max_objects=65536, **kw),
                lambda: find_objects(mask.cpu(), disp, flow, ts, pose, cam, **kw),
                lambda: find_objects(mask, disp.cpu(), flow, ts, pose, cam, **kw),
                lambda: find_objects(mask, disp, flow.cpu(), ts, pose, cam, **kw),
                lambda: find_objects(mask, disp, flow, ts.cpu(), pose, cam, **kw),
                lambda: find_objects(mask, disp, flow, ts, pose.cpu(), cam, **kw),
                lambda: find_objects(mask, disp, flow, ts, pose, cam, disp_flipped=disp.cpu(), **kw),
                lambda: find_objects(mask, disp[:, :, :3], flow, ts, pose, cam, **kw),
                lambda: find_objects(mask, disp[:1], flow, ts, pose, cam, **kw),
                lambda: find_objects(mask, disp, flow[:, :2], ts, pose, cam, **kw),
                lambda: find_objects(mask, disp, flow[:, :, :, :5], ts, pose, cam, **kw),
                lambda: find_objects(mask, disp, flow, ts[:1], pose, cam, **kw),
                lambda: find_objects(mask, disp, flow, ts, pose[:, :, :3], cam, **kw),
                lambda: find_objects(mask, disp, flow, ts, pose, cam, disp_flipped=disp[:, :, :, :5], **kw),
                lambda: find_objects(mask.double(), disp, flow, ts, pose, cam, **kw),
                lambda: find_objects(mask, disp, flow, ts, pose, (0.0, 5.0, 3.0, 2.0), **kw),
                lambda: find_objects(mask, disp, flow, ts, pose, cam, min_depth=0.0, max_depth=100.0),
                lambda: labels_u16(torch.zeros(2, 4, 6, dtype=torch.int32), 8, 12),
                lambda: labels_u16(torch.zeros(2, 4, 6, device="cuda"), 8, 12),
                lambda: labels_u16(torch.zeros(2, 4, 6, dtype=torch.int32, device="cuda"), 0, 12)):
        with pytest.raises(DynamoHipError):
            bad()
    # the entry point itself: every refusal returns hipErrorInvalidValue and leaves the poisoned outputs alone
    lib = L.load()
    shape, name = (5, 7), "bernoulli50"
    n = OC.B * 5 * 7
    labels = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    table = torch.full((OC.B * 9 * ROW + 2,), 7, dtype=torch.int32, device="cuda")
    counts = torch.full((OC.B * 3,), 7, dtype=torch.int32, device="cuda")
    need = lib.dd_objects_workspace_bytes(OC.B, 5, 7, 9)
    ws = torch.full((need // 8 + 1,), 7, dtype=torch.int64, device="cuda")
    P = abi.ptr
    off = lambda t, k: abi.C.c_void_p(t.data_ptr() + k)           # noqa: E731

    def call(**change):
        buffers = dict(labels=P(labels), table=P(table), counts=P(counts), ws=P(ws), ws_bytes=need)
        buffers.update({k: change.pop(k) for k in list(change) if k in buffers})
        return _raw(shape, name, change.pop("connectivity", 8), change.pop("min_pixels", 1), change.pop("max_objects", 9), *buffers.values(), **change)

    x = _device(shape, name)
    assert all(call(**{k: None}) == 1 for k in ("mask", "disp", "flow", "ts", "pose", "labels", "table", "counts", "ws"))
    assert call(lmask=P(x["ts"])) == 1 if not OC.uses_flip(shape, name) else call(lmask=None) == 1
    assert all(call(**{k: 0}) == 1 for k in ("B", "h", "w")) and call(h=-5) == 1 and call(h=65536, w=32768) == 1
    assert all(call(connectivity=c) == 1 for c in (0, 1, 6, 9, -4)) and call(min_pixels=0) == 1 and call(min_pixels=-3) == 1
    assert all(call(max_objects=m) == 1 for m in (0, -1, 65536, 1 << 20))
    assert all(call(**{k: v}) == 1 for k in ("fx", "fy") for v in (0.0, float("inf"), float("nan")))
    assert all(call(**{k: off(x[t], 2)}) == 1 for k, t in (("mask", "mask"), ("disp", "disp"), ("flow", "flow"), ("ts", "ts"), ("pose", "pose")))
    assert call(labels=off(labels, 2)) == 1 and call(counts=off(counts, 2)) == 1 and call(table=off(table, 4)) == 1 and call(ws=off(ws, 4)) == 1
    assert call(ws_bytes=need - 1) == 1
    assert lib.dd_objects_workspace_bytes(0, 5, 7, 9) == 0 and lib.dd_objects_workspace_bytes(2, 5, 7, 0) == 0 and lib.dd_objects_workspace_bytes(2, 5, 7, 65536) == 0
    assert lib.dd_objects_workspace_bytes(1, 65536, 32768, 9) == 0 and lib.dd_objects_workspace_bytes(2, 5, 7, 65535) == 8 * n
    out = torch.full((OC.B * 10 * 14,), 7, dtype=torch.int16, device="cuda")
    u16 = lambda *a: lib.dd_export_labels_u16(*a, L.current_stream())       # noqa: E731
    assert u16(None, 2, 5, 7, 10, 14, P(out)) == 1 and u16(P(labels), 2, 5, 7, 10, 14, None) == 1 and u16(P(labels), 2, 5, 7, 0, 14, P(out)) == 1
    assert u16(P(labels), 2, 5, 7, 65536, 32768, P(out)) == 1 and u16(P(labels), 2, 5, 7, 10, 14, off(out, 1)) == 1 and u16(off(labels, 2), 2, 5, 7, 10, 14, P(out)) == 1
    torch.cuda.synchronize()
    assert bool((labels == 7).all()) and bool((table == 7).all()) and bool((counts == 7).all()) and bool((ws == 7).all()) and bool((out == 7).all())
    assert call() == 0
    clean = bool((table[-2:] == 7).all()) and int(ws[-1]) == 7
    want = OC.reference(shape, name, 8, 1, 9)
    ok = np.array_equal(labels.cpu().numpy().reshape(OC.B, 5, 7), want[0]) and np.array_equal(counts.cpu().numpy().reshape(OC.B, 3), want[2])
    assert clean and ok


@pytest.mark.parametrize("sizes", [((5, 7), (11, 20)), ((64, 96), (192, 640))], ids=["5x7", "64x96"])
def test_label_image(sizes):
    from hipops.objects import labels_u16, labels_u16_host
    (h, w), (H_, W_) = sizes
    labels = np.random.default_rng(3).integers(0, 70000, (2, h, w)).astype(np.int32)            # some above 65535: they saturate
    got = labels_u16(torch.from_numpy(labels).cuda(), H_, W_)
    assert got.is_cuda and got.dtype == torch.uint16 and tuple(got.shape) == (2, H_, W_)
    assert np.array_equal(got.cpu().numpy(), labels_u16_host(labels, H_, W_)) and (got.cpu().numpy() == 65535).any()


def test_the_wrapper_does_not_synchronise():
    from hipops.objects import find_objects
    shape, name = (37, 53), "blobs"
    x = _device(shape, name)
    args = (x["mask"], x["disp"], x["flow"], x["ts"], x["pose"], OC.intrinsics(*shape))
    kw = dict(disp_flipped=x["flipped"], min_depth=OC.MIN_DEPTH, max_depth=OC.MAX_DEPTH, min_pixels=1)
    find_objects(*args, **kw)           # the table of the flip fuse and the workspace are made on the first call
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        labels, table, counts = find_objects(*args, **kw)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert int(counts[0, 1]) == OC.reference(shape, name, 8)[2][0, 1]


# ---- predict.py ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def predict_runs(tmp_path_factory):
    """predict.main over the golden frames in ONE child process (tests/cloud_predict_worker.py says why not in this one): first without
    the objects, then with them at a threshold taken from the untrained network's own mask -- the median of the first batch's."""
    import subprocess
    import sys
    root = tmp_path_factory.mktemp("predict_objects")
    job = root / "job.json"
    job.write_text(json.dumps({"frames": FRAMES, "out": str(root), "base": NET + ["-b", "3", "--motion"], "min_pixels": 4}))
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "objects_predict_worker.py")
    done = subprocess.run([sys.executable, worker, str(job)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=240)
    assert done.returncode == 0, done.stdout[-4000:]
    runs = {"thresh": json.loads((root / "thresh.json").read_text())}
    for name in ("plain", "objects"):
        seen = {}
        with np.load(str(root / (name + "_seen.npz"))) as data:
            for key in data.files:
                stem, what = key.split("/")
                seen.setdefault(stem, {})[what] = data[key]
        runs[name] = (json.loads((root / (name + "_written.json")).read_text()), str(root / name), seen)
    return runs


def test_predict_save_objects(predict_runs):
    from PIL import Image
    from hipops.objects import objects_host, pixel_quantities_host, unpack_table
    thresh = predict_runs["thresh"]
    written, out, seen = predict_runs["objects"]
    _, plain_out, plain_seen = predict_runs["plain"]
    interior = STEMS[1:-1]
    assert list(seen) == interior and sorted(os.listdir(out)) == ["depth", "motion_mask", "objects", "poses.txt", "predict.json"]
    assert sorted(os.listdir(os.path.join(out, "objects"))) == sorted(s + e for s in interior for e in (".json", ".png"))
    assert all(os.path.join(out, "objects", s + e) in written for s in interior for e in (".json", ".png"))
    assert all(set(plain_seen[s]) == {"disp", "motion_mask", "cam_T_cam"} for s in interior)            # without the option the batch is what it was
    assert all(set(seen[s]) == {"disp", "motion_mask", "cam_T_cam", "complete_flow", "ts"} for s in interior)
    meta = json.load(open(os.path.join(out, "predict.json")))["objects"]
    assert (meta["motion_thresh"], meta["connectivity"], meta["min_pixels"], meta["max_objects"]) == (thresh, 8, 4, 256)
    assert "up to scale" in meta["note"] and "ts" in meta["motion_note"] and list(meta["frames"]) == interior
    assert "objects" not in json.load(open(os.path.join(plain_out, "predict.json")))
    camera = (float(np.float32(0.58)) * 96, float(np.float32(1.92)) * 64, 48.0, 32.0)
    some = 0
    for stem in interior:
        f = seen[stem]
        mask = f["motion_mask"][None]
        assert 0 < (mask >= np.float32(thresh)).sum() < mask.size           # some, not all, foreground
        args = (mask, f["disp"][None], f["complete_flow"][None], f["ts"].reshape(1), f["cam_T_cam"][None, :3], camera)
        labels, table, counts = objects_host(*args, min_depth=0.1, max_depth=100.0, thresh=thresh, connectivity=8, min_pixels=4, max_objects=256)
        want = unpack_table(table, counts, size=(64, 96, H, W))[0]
        got = json.load(open(os.path.join(out, "objects", stem + ".json")))
        assert meta["frames"][stem] == {"kept": len(want["objects"]), "found": want["found"], "truncated": want["truncated"]}
        assert got["found"] == want["found"] and got["truncated"] == want["truncated"] and len(got["objects"]) == len(want["objects"])
        bound = OC.sum_bound(labels, pixel_quantities_host(*args, min_depth=0.1, max_depth=100.0), 256)[0]
        for n, (g, r) in enumerate(zip(got["objects"], want["objects"])):
            assert all(g[k] == r[k] for k in ("id", "pixels", "box", "anchor", "z_min", "z_max")), (stem, n, g, r)
            b = bound[n] / r["pixels"]              # the derived means: the sums' bound divided by pixels
            for k, (lo, hi) in (("centroid", (0, 3)), ("motion", (3, 6))):
                assert all(abs(gv - rv) <= bv for gv, rv, bv in zip(g[k], r[k], b[lo:hi])), (stem, n, k)
            assert abs(g["confidence"] - r["confidence"]) <= b[6] and abs(g["speed"] - r["speed"]) <= np.sqrt((b[3:6] ** 2).sum()) + 4e-16 * r["speed"]
            assert 0 <= g["box"][0] <= g["box"][2] < W and 0 <= g["box"][1] <= g["box"][3] < H
        some += len(got["objects"])
        with Image.open(os.path.join(out, "objects", stem + ".png")) as img:
            assert img.mode == "I;16" and img.size == (W, H)
            image = np.asarray(img).astype(np.int64)
        assert set(np.unique(image)) - {0} == {g["id"] for g in got["objects"]}
        from hipops.objects import labels_u16_host
        assert np.array_equal(image, labels_u16_host(labels, H, W)[0])
        # the other outputs are what they are without the objects
        for folder in ("depth", "motion_mask"):
            assert open(os.path.join(out, folder, stem + ".png"), "rb").read() == open(os.path.join(plain_out, folder, stem + ".png"), "rb").read()
    assert some > 0
    assert open(os.path.join(out, "poses.txt")).read() == open(os.path.join(plain_out, "poses.txt")).read()
