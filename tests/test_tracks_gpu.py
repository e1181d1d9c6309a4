"""dd_tracks_link on the device against the numpy definition (hipops/tracks.py): votes and links EQUAL to link_host for every case of
tracks_case with the flip fuse off and on -- everything is an integer, there is no tolerance; nothing written outside the outputs,
two runs, labels out of range, the arguments that are refused, no host synchronisation; a synthetic sequence through find_objects,
link_objects and TrackBuilder across a batch boundary; and predict.py --save tracks end to end."""
import json
import os

import numpy as np
import pytest
import torch

import objects_case as OC
import tracks_case as TC

pytestmark = pytest.mark.gpu

FRAMES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tiny_kitti_jpeg")
STEMS = sorted(os.path.splitext(f)[0] for f in os.listdir(FRAMES))
H, W = 192, 640                      # the golden frames' own size
NET = ["--weights_init", "scratch", "--depth_model", "litemono", "--height", "64", "--width", "96", "--num_workers", "0"]
POISON = 0xA5


def _device(x):
    return {k: torch.from_numpy(v.copy()).cuda() for k, v in x.items() if isinstance(v, np.ndarray)}


def _link(x, shape, flip, M):
    from hipops.tracks import link_objects
    d = _device(x)
    votes, links = link_objects(d["src"], d["dst"], d["disp"], d["flow"], d["ts"], OC.intrinsics(*shape), disp_flipped=d["flipped"] if flip else None,
                                min_depth=OC.MIN_DEPTH, max_depth=OC.MAX_DEPTH, max_objects=M)
    return votes.cpu().numpy(), links.cpu().numpy()


@pytest.mark.parametrize("flip", [False, True], ids=["plain", "pp"])
@pytest.mark.parametrize("case", TC.CASES, ids=TC.CASE_IDS)
def test_links_are_the_host_definition(case, flip):
    shape, M = case[0], case[5]
    votes, links = _link(TC.inputs(case), shape, flip, M)
    want_votes, want_links = TC.reference(case, flip)
    assert votes.dtype == np.int32 and votes.shape == (TC.B, M, M + 2) and links.dtype == np.int32 and links.shape == (TC.B, M, 6)
    assert np.array_equal(votes, want_votes), (case, flip, int((votes != want_votes).sum()))
    assert np.array_equal(links, want_links), (case, flip)


def _raw(x, shape, fused, M, votes, links, **change):
    """The entry point itself on caller-made buffers (addresses); `change`: arguments replaced by name."""
    from hipops import abi, lib as L
    from hipops.export import _table, depth_params
    h, w = shape
    d = _device(x)
    lo, span = depth_params(OC.MIN_DEPTH, OC.MAX_DEPTH)
    fx, fy, cx, cy = OC.intrinsics(h, w)
    args = dict(src=abi.ptr(d["src"]), dst=abi.ptr(d["dst"]), disp=abi.ptr(d["disp"]), flip=abi.ptr(d["flipped"]) if fused else None,
                lmask=abi.ptr(_table("l_mask", w, "cuda:0")) if fused else None, flow=abi.ptr(d["flow"]), ts=abi.ptr(d["ts"]), B=TC.B, h=h, w=w,
                fx=fx, fy=fy, cx=cx, cy=cy, lo=float(lo), span=float(span), M=M, votes=votes, links=links)
    assert set(change) <= set(args)
    args.update(change)
    code = L.load().dd_tracks_link(*args.values(), L.current_stream())
    torch.cuda.synchronize()
    return code


def _in_arenas(x, shape, flip, M):
    """One call with votes and links inside arenas full of 0xA5, the outputs' own bytes included: (votes, links) on the host after
    the check that every byte around them kept the poison."""
    from hipops import abi
    sizes = {"votes": 4 * TC.B * M * (M + 2), "links": 4 * TC.B * M * 6}
    lead = 64
    arenas = {k: torch.full((lead + v + 64,), POISON, dtype=torch.uint8, device="cuda") for k, v in sizes.items()}
    assert all(a.data_ptr() % 4 == 0 for a in arenas.values())
    at = {k: abi.C.c_void_p(a.data_ptr() + lead) for k, a in arenas.items()}
    assert _raw(x, shape, flip, M, at["votes"], at["links"]) == 0
    host = {k: a.cpu().numpy() for k, a in arenas.items()}
    for a in arenas.values():
        a.zero_()               # the poison does not stay in the blocks that go back to the allocator
    for k, v in sizes.items():
        assert (host[k][:lead] == POISON).all() and (host[k][lead + v:] == POISON).all(), k
    return (host["votes"][lead:lead + sizes["votes"]].copy().view(np.int32).reshape(TC.B, M, M + 2),
            host["links"][lead:lead + sizes["links"]].copy().view(np.int32).reshape(TC.B, M, 6))


ARENA_CASES = [((37, 53), "smooth", "blobs", "rings", 8, 256), ((5, 7), "shift", "checker", "blobs", 4, 4), ((130, 67), "smooth", "checker", "checker", 4, 4)]


@pytest.mark.parametrize("case", ARENA_CASES, ids=["blobs", "small", "above-the-cap"])
def test_nothing_is_written_outside_the_outputs(case):
    """Every word of the outputs is written by the call (they start as 0xA5 and the caller clears nothing), none around them."""
    for flip in (False, True):
        votes, links = _in_arenas(TC.inputs(case), case[0], flip, case[5])
        want = TC.reference(case, flip)
        assert np.array_equal(votes, want[0]) and np.array_equal(links, want[1])


def test_two_runs_are_byte_identical():
    case = ((130, 67), "smooth", "checker", "checker", 4, 1024)
    first, second = _link(TC.inputs(case), case[0], True, 1024), _link(TC.inputs(case), case[0], True, 1024)
    assert first[0].tobytes() == second[0].tobytes() and first[1].tobytes() == second[1].tobytes() and first[0].sum() > 0


@pytest.mark.parametrize("M", [4, 256])
def test_labels_out_of_range(M):
    """-1, M+1, 2^30 and the most negative int in both maps: such a source pixel votes nowhere, such a destination pixel is background,
    and nothing outside the outputs is touched."""
    from hipops.tracks import link_host
    case = ((37, 53), "smooth", "blobs", "blobs", 8, M)
    x = dict(TC.inputs(case))
    bad = np.array([-1, M + 1, 1 << 30, -(1 << 31)], dtype=np.int64)
    rng = np.random.default_rng(M)
    for key in ("src", "dst"):
        m = x[key].copy()
        at = rng.random(m.shape) < 0.2
        m[at] = bad[rng.integers(0, len(bad), int(at.sum()))].astype(np.int32)
        x[key] = m
    args, kw = TC.host_args(x, case[0], False, M)
    want = link_host(*args, **kw)
    votes, links = _in_arenas(x, case[0], False, M)
    assert np.array_equal(votes, want[0]) and np.array_equal(links, want[1]) and votes.sum() > 0
    assert not np.array_equal(want[0], TC.reference(case, False)[0])


def test_bad_arguments_are_refused():
    from hipops import abi
    from hipops.lib import DynamoHipError
    from hipops.tracks import link_objects
    case = ((5, 7), "smooth", "blobs", "rings", 8, 9)
    x = dict(TC.inputs(((5, 7), "smooth", "blobs", "rings", 8, 4)))
    d = _device(x)
    cam = OC.intrinsics(5, 7)
    kw = dict(min_depth=0.1, max_depth=100.0, max_objects=9)
    assert link_objects(d["src"], d["dst"], d["disp"], d["flow"], d["ts"], cam, **kw)[1].shape == (2, 9, 6)
    for bad in (lambda: link_objects(d["src"].cpu(), d["dst"], d["disp"], d["flow"], d["ts"], cam, **kw),
                lambda: link_objects(d["src"], d["dst"].float(), d["disp"], d["flow"], d["ts"], cam, **kw),
                lambda: link_objects(d["src"], d["dst"][:1], d["disp"], d["flow"], d["ts"], cam, **kw),
                lambda: link_objects(d["src"], d["dst"], d["disp"].cpu(), d["flow"], d["ts"], cam, **kw),
                lambda: link_objects(d["src"], d["dst"], d["disp"], d["flow"][:, :2], d["ts"], cam, **kw),
                lambda: link_objects(d["src"], d["dst"], d["disp"], d["flow"], d["ts"][:1], cam, **kw),
                lambda: link_objects(d["src"], d["dst"], d["disp"], d["flow"], d["ts"], cam, disp_flipped=d["disp"][:, :, :, :5], **kw),
                lambda: link_objects(d["src"], d["dst"], d["disp"], d["flow"], d["ts"], (0.0, 5.0, 3.0, 2.0), **kw),
                lambda: link_objects(d["src"], d["dst"], d["disp"], d["flow"], d["ts"], cam, min_depth=0.0, max_depth=100.0),
                lambda: link_objects(d["src"], d["dst"], d["disp"], d["flow"], d["ts"], cam, min_depth=0.1, max_depth=100.0, max_objects=0),
                lambda: link_objects(d["src"], d["dst"], d["disp"], d["flow"], d["ts"], cam, min_depth=0.1, max_depth=100.0, max_objects=1025)):
        with pytest.raises(DynamoHipError):
            bad()
    # the entry point itself: every refusal returns hipErrorInvalidValue and leaves the outputs alone
    M = case[5]
    votes = torch.full((TC.B * M * (M + 2) + 2,), 7, dtype=torch.int32, device="cuda")
    links = torch.full((TC.B * M * 6 + 2,), 7, dtype=torch.int32, device="cuda")
    P = abi.ptr
    off = lambda t, k: abi.C.c_void_p(t.data_ptr() + k)           # noqa: E731

    def call(fused=False, **change):
        buffers = dict(votes=P(votes), links=P(links))
        buffers.update({k: change.pop(k) for k in list(change) if k in buffers})
        return _raw(x, case[0], fused, change.pop("M", M), buffers["votes"], buffers["links"], **change)

    assert all(call(**{k: None}) == 1 for k in ("src", "dst", "disp", "flow", "ts", "votes", "links"))
    assert call(lmask=P(d["ts"])) == 1 and call(flip=P(d["flipped"])) == 1              # one of the flip fuse's two without the other
    assert call(fused=True, lmask=None) == 1 and call(fused=True, flip=None) == 1
    assert all(call(**{k: v}) == 1 for k in ("B", "h", "w", "M") for v in (0, -1)) and call(h=65536, w=32768) == 1
    assert call(M=1025) == 1 and call(M=1 << 20) == 1 and call(B=2048, M=1024) == 1         # the cap; B * M * (M + 2) above 2^31 - 1
    assert all(call(**{k: v}) == 1 for k in ("fx", "fy") for v in (0.0, float("inf"), float("-inf"), float("nan")))
    assert all(call(**{k: off(d[t], 2)}) == 1 for k, t in (("src", "src"), ("dst", "dst"), ("disp", "disp"), ("flow", "flow"), ("ts", "ts")))
    assert call(votes=off(votes, 2)) == 1 and call(links=off(links, 2)) == 1
    torch.cuda.synchronize()
    assert bool((votes == 7).all()) and bool((links == 7).all())
    assert call() == 0
    from hipops.tracks import link_host
    args, hkw = TC.host_args(x, case[0], False, M)
    want = link_host(*args, **hkw)
    assert bool((votes[-2:] == 7).all()) and bool((links[-2:] == 7).all())
    assert np.array_equal(votes[:-2].cpu().numpy().reshape(TC.B, M, M + 2), want[0]) and np.array_equal(links[:-2].cpu().numpy().reshape(TC.B, M, 6), want[1])


def test_the_wrapper_does_not_synchronise():
    from hipops.tracks import link_objects
    case = ((37, 53), "shift", "blobs", "blobs", 8, 256)
    d = _device(TC.inputs(case))
    args = (d["src"], d["dst"], d["disp"], d["flow"], d["ts"], OC.intrinsics(*case[0]))
    kw = dict(disp_flipped=d["flipped"], min_depth=OC.MIN_DEPTH, max_depth=OC.MAX_DEPTH, max_objects=256)
    link_objects(*args, **kw)           # the table of the flip fuse is made on the first call
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        votes, links = link_objects(*args, **kw)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert np.array_equal(links.cpu().numpy(), TC.reference(case, True)[1])


# ---- a synthetic sequence --------------------------------------------------------------------------------------------------------
def test_a_moving_blob_is_one_track_across_the_batch_boundary():
    """A 9 x 7 blob moves two pixels to the right per frame over six 37 x 53 frames; the disparity is constant, the flow carries every
    pixel two pixels back (c = -2 * z / fx) onto the blob of the frame in front, the pose chain adds 0.5 along x per frame.  Fed in
    batches of 4 and 2 with the last label map carried over: one track of length six, its positions the constructed ones.
    A position is the float64 mean of fp32 terms ((x - cx) * ifx) * z with x - cx exact: at most six roundings of 2^-24 relative lie
    on the way to a term (three into z, one in ifx, two products), so a term, and with it the mean, is within 6 * 2^-24 of the largest
    term to first order; the exact offset of the chain is added in float64.  The tolerance is 8 * 2^-24 of the largest coordinate."""
    from hipops.cloud import chain_poses
    from hipops.export import depth_params
    from hipops.objects import find_objects, unpack_table
    from hipops.tracks import TrackBuilder, link_objects
    h, w, n = 37, 53, 6
    cam = OC.intrinsics(h, w)
    fx, fy, cx, cy = (float(np.float32(v)) for v in cam)
    disp = 0.37
    lo, span = depth_params(OC.MIN_DEPTH, OC.MAX_DEPTH)
    z = 1.0 / (float(lo) + float(span) * float(np.float32(disp)))
    mask = np.zeros((n, 1, h, w), dtype=np.float32)
    for i in range(n):
        mask[i, 0, 11:18, 5 + 2 * i:14 + 2 * i] = 1.0
    flow = np.zeros((n, 3, h, w), dtype=np.float32)
    flow[:, 0] = -2.0 * z / fx
    pose = np.tile(np.eye(4, dtype=np.float32), (n, 1, 1))
    pose[:, 0, 3] = 0.5
    builder, carry, chain, start = TrackBuilder(0.25), None, None, 0
    kw = dict(min_depth=OC.MIN_DEPTH, max_depth=OC.MAX_DEPTH)
    for size in (4, 2):
        sl = slice(start, start + size)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a[sl])).cuda()          # noqa: E731
        d, f, ts, T = torch.full((size, 1, h, w), disp, device="cuda"), dev(flow), torch.ones(size, device="cuda"), dev(pose)
        labels, table, counts = find_objects(dev(mask), d, f, ts, T, cam, min_pixels=4, max_objects=8, **kw)
        before = torch.zeros_like(labels[:1]) if carry is None else carry
        votes, links = link_objects(labels, torch.cat([before, labels[:-1]]), d, f, ts, cam, max_objects=8, **kw)
        frames = unpack_table(table.cpu().numpy(), counts.cpu().numpy())
        G = chain_poses(pose[sl], chain)
        rows = links.cpu().numpy()
        for b in range(size):
            builder.add("f%d" % (start + b), frames[b]["objects"], None if carry is None and b == 0 else rows[b], G[b])
        if start:
            assert rows[0, 0].tolist() == [1, 63, 0, 0, 0, 0]           # the first frame of the second batch links into the carried map
        carry, chain, start = labels[-1:], G[-1], start + size
    tracks = builder.summary()
    assert len(tracks) == 1 and tracks[0]["length"] == n and (builder.accepted, builder.refused) == (n - 1, 0)
    assert [f["stem"] for f in tracks[0]["frames"]] == ["f%d" % i for i in range(n)]
    want = np.array([[((9 + 2 * i) - cx) / fx * z + 0.5 * i, (14 - cy) / fy * z, z] for i in range(n)])
    got = np.array([f["position"] for f in tracks[0]["frames"]])
    assert np.abs(got - want).max() <= 8 * 2.0 ** -24 * np.abs(want).max(), np.abs(got - want).max()
    assert all(f["iou"] == 1.0 for f in tracks[0]["frames"][1:])          # every pixel lands on the predecessor's blob
    steps = np.linalg.norm(np.diff(got, axis=0), axis=1).sum()
    assert abs(tracks[0]["path_length"] - steps) <= 1e-15 * steps


# ---- predict.py ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def predict_runs(tmp_path_factory):
    """predict.main over the golden frames in ONE child process (tests/tracks_predict_worker.py): without the objects, with them, and
    with them and the tracks, at a threshold taken from the untrained network's own mask."""
    import subprocess
    import sys
    root = tmp_path_factory.mktemp("predict_tracks")
    job = root / "job.json"
    job.write_text(json.dumps({"frames": FRAMES, "out": str(root), "base": NET + ["-b", "3", "--motion"], "min_pixels": 4}))
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tracks_predict_worker.py")
    done = subprocess.run([sys.executable, worker, str(job)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert done.returncode == 0, done.stdout[-4000:]
    runs = {"thresh": json.loads((root / "thresh.json").read_text())}
    for name in ("objects", "tracks"):
        seen = {}
        with np.load(str(root / (name + "_seen.npz"))) as data:
            for key in data.files:
                stem, what = key.split("/")
                seen.setdefault(stem, {})[what] = data[key]
        runs[name] = (json.loads((root / (name + "_written.json")).read_text()), str(root / name), seen)
    return runs


def test_predict_save_tracks(predict_runs):
    """tracks.json and tracks/*.png are what link_host + TrackBuilder give from the tensors the worker recorded.  Equality with the
    definition, not a number of tracks: an untrained network owes nobody a link.  Integers, stems and the iou (a quotient of
    integers) are equal; centroids and positions are means of float64 sums that the device adds in another order than the host, held
    to objects_case.sum_bound as tests/test_objects_gpu.py holds them."""
    from PIL import Image
    from hipops.cloud import chain_poses
    from hipops.objects import labels_u16_host, objects_host, pixel_quantities_host, unpack_table
    from hipops.tracks import TrackBuilder, link_host, track_image
    thresh = predict_runs["thresh"]
    written, out, seen = predict_runs["tracks"]
    _, objects_out, objects_seen = predict_runs["objects"]
    interior = STEMS[1:-1]
    assert list(seen) == interior and sorted(os.listdir(out)) == ["depth", "motion_mask", "objects", "poses.txt", "predict.json", "tracks", "tracks.json"]
    assert sorted(os.listdir(os.path.join(out, "tracks"))) == [s + ".png" for s in interior]
    assert os.path.join(out, "tracks.json") in written and all(os.path.join(out, "tracks", s + ".png") in written for s in interior)
    assert sorted(os.listdir(objects_out)) == ["depth", "motion_mask", "objects", "poses.txt", "predict.json"]
    # the other outputs are, byte for byte, what they are without the tracks
    for folder in ("depth", "motion_mask", "objects"):
        names = sorted(os.listdir(os.path.join(objects_out, folder)))
        assert names == sorted(os.listdir(os.path.join(out, folder))) and len(names) >= len(interior)
        for name in names:
            assert open(os.path.join(out, folder, name), "rb").read() == open(os.path.join(objects_out, folder, name), "rb").read(), (folder, name)
    assert open(os.path.join(out, "poses.txt")).read() == open(os.path.join(objects_out, "poses.txt")).read()
    assert all(set(objects_seen[s]) == set(seen[s]) == {"disp", "motion_mask", "cam_T_cam", "complete_flow", "ts"} for s in interior)
    meta, plain_meta = json.load(open(os.path.join(out, "predict.json"))), json.load(open(os.path.join(objects_out, "predict.json")))
    assert "tracks" not in plain_meta and {k: v for k, v in meta.items() if k != "tracks"} == plain_meta
    # the definition on the recorded tensors
    camera = (float(np.float32(0.58)) * 96, float(np.float32(1.92)) * 64, 48.0, 32.0)
    kw = dict(min_depth=0.1, max_depth=100.0)
    builder, before, labels_of, bounds = TrackBuilder(0.25), None, {}, {}
    G = chain_poses(np.stack([seen[s]["cam_T_cam"] for s in interior]))
    for i, stem in enumerate(interior):
        f = seen[stem]
        args = (f["motion_mask"][None], f["disp"][None], f["complete_flow"][None], f["ts"].reshape(1), f["cam_T_cam"][None, :3], camera)
        labels, table, counts = objects_host(*args, thresh=thresh, connectivity=8, min_pixels=4, max_objects=256, **kw)
        frame = unpack_table(table, counts, size=(64, 96, H, W))[0]
        links = None
        if before is not None:
            links = link_host(labels, before, f["disp"][None], f["complete_flow"][None], f["ts"].reshape(1), camera, max_objects=256, **kw)[1][0]
        ids = builder.add(stem, frame["objects"], links, G[i])
        with Image.open(os.path.join(out, "tracks", stem + ".png")) as img:
            assert img.mode == "I;16" and img.size == (W, H)
            assert np.array_equal(np.asarray(img).astype(np.uint16), track_image(labels_u16_host(labels, H, W)[0], ids)), stem
        bound = OC.sum_bound(labels, pixel_quantities_host(*args, **kw), 256)[0]
        bounds[stem] = {n + 1: bound[n, :3] / o["pixels"] for n, o in enumerate(frame["objects"])}
        before = labels
    want, got = builder.summary(), json.load(open(os.path.join(out, "tracks.json")))
    assert got["parameters"] == {"motion_thresh": thresh, "connectivity": 8, "min_pixels": 4, "max_objects": 256, "min_iou": 0.25}
    assert got["count"] == len(want) == len(got["tracks"]) and got["longest"] == max(t["length"] for t in want)
    assert (got["links_accepted"], got["links_refused"]) == (builder.accepted, builder.refused)
    notes = " ".join(got["notes"])
    assert "up to scale" in notes and "ts" in notes and "gap" in notes
    assert meta["tracks"] == {k: got[k] for k in ("parameters", "count", "longest", "links_accepted", "links_refused", "notes")}
    assert sum(t["length"] for t in want) == sum(len(b) for b in bounds.values()) > 0          # every object of every frame is in one track
    for g, r in zip(got["tracks"], want):
        assert all(g[k] == r[k] for k in ("id", "first", "last", "length")) and len(g["frames"]) == len(r["frames"])
        for gf, rf in zip(g["frames"], r["frames"]):
            assert all(gf[k] == rf[k] for k in ("stem", "object", "pixels", "box", "iou")), (g["id"], gf, rf)
            b = bounds[rf["stem"]][rf["object"]]
            Gi = np.abs(G[interior.index(rf["stem"])][:3, :3])
            assert all(abs(u - v) <= e for u, v, e in zip(gf["centroid"], rf["centroid"], b)), (g["id"], rf["stem"])
            assert all(abs(u - v) <= e + 4e-16 * abs(v) for u, v, e in zip(gf["position"], rf["position"], Gi @ b)), (g["id"], rf["stem"])
        steps = 2 * sum(float(np.sqrt(((np.abs(G[interior.index(f["stem"])][:3, :3]) @ bounds[f["stem"]][f["object"]]) ** 2).sum())) for f in r["frames"])
        assert abs(g["path_length"] - r["path_length"]) <= steps + 1e-15 * r["path_length"]
