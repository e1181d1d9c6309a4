"""Tracks on the host (hipops/tracks.py): the numpy definition of the link against a plain triple loop, the selection of links from
votes, TrackBuilder on hand-written tables, positions against the pose chain, the track image, the parser and predict_folder's
refusals.  No GPU."""
import json

import numpy as np
import pytest

import objects_case as OC
import tracks_case as TC

_f32 = np.float32


# ---- the definition ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", TC.SHAPES[:3], ids=["1x1", "1x70", "5x7"])
def test_link_host_is_the_triple_loop(shape):
    from hipops.export import depth_params
    from hipops.tracks import links_from_votes
    lo, span = depth_params(OC.MIN_DEPTH, OC.MAX_DEPTH)
    seen = 0
    for case in TC.CASES:
        if case[0] != shape:
            continue
        x = TC.inputs(case)
        votes, links = TC.reference(case, False)
        M = case[5]
        assert votes.dtype == np.int32 and votes.shape == (TC.B, M, M + 2) and links.dtype == np.int32 and links.shape == (TC.B, M, 6)
        want = TC.link_loops(x["src"], x["dst"], x["disp"], x["flow"], x["ts"], OC.intrinsics(*shape), lo, span, M)
        assert np.array_equal(votes, want), case
        assert np.array_equal(links, links_from_votes(want))
        voters = ((x["src"] >= 1) & (x["src"] <= M)).reshape(TC.B, -1).sum(1)
        assert np.array_equal(votes.reshape(TC.B, -1).sum(1), voters)         # every voting pixel votes once
        seen += 1
    assert seen == len(TC.FLOWS)


def test_the_cases_hold_what_they_promise():
    """On the host alone: exact ties exist, the shift moves labels, `outside` and `behind` send every vote to the last column, labels
    above the cap are present, and the flip fuse changes the result somewhere."""
    by = {(c[0], c[1]): c for c in TC.CASES[:len(TC.SHAPES) * len(TC.FLOWS)]}
    for shape in ((37, 53), (130, 67)):
        assert TC.inputs(by[shape, "ties"])["exact"] >= 3, shape
        for kind in ("outside", "behind"):
            case = by[shape, kind]
            votes, links = TC.reference(case, False)
            M = case[5]
            assert votes.sum() > 0 and votes[:, :, :M + 1].sum() == 0 and (links[:, :, :5] == 0).all() and links[:, :, 5].sum() == votes.sum()
    same = ((37, 53), "zero", "checker", "checker", 4, 4)
    votes, links = TC.reference(same, False)
    x = TC.inputs(same)
    assert x["src"].max() > 256 and TC.labels((130, 67), "checker", 4).max() > 1024     # labels above every cap
    assert links[0, :, 0].tolist() == [1, 2, 3, 4] and (links[0, :, 1] == 1).all()      # zero flow: every object lands on itself
    shift = ((37, 53), "shift", "blobs", "blobs", 8, 256)
    assert not np.array_equal(TC.reference(shift, False)[0], TC.reference(shift, True)[0])


def test_links_from_votes():
    from hipops.tracks import links_from_votes
    M = 5
    votes = np.zeros((1, M, M + 2), dtype=np.int32)
    votes[0, 0] = [9, 3, 7, 7, 0, 1, 4]          # the largest twice: the smaller column is dst, the other dst2
    votes[0, 1] = [2, 0, 0, 0, 0, 0, 8]          # only background and outside: no link
    votes[0, 2] = [0, 0, 0, 0, 0, 6, 0]          # one column: no second
    votes[0, 3] = [0, 4, 4, 4, 4, 4, 0]          # all equal
    links = links_from_votes(votes)
    assert links[0].tolist() == [[2, 7, 3, 7, 9, 4], [0, 0, 0, 0, 2, 8], [5, 6, 0, 0, 0, 0], [1, 4, 2, 4, 0, 0], [0, 0, 0, 0, 0, 0]]
    with pytest.raises(ValueError):
        links_from_votes(np.zeros((1, 5, 6), dtype=np.int32))


# ---- TrackBuilder ----------------------------------------------------------------------------------------------------------------
def _object(n, pixels, centroid=(0.0, 0.0, 1.0)):
    return {"id": n, "pixels": pixels, "box": [0, 0, 1, 1], "anchor": 0, "centroid": list(centroid), "motion": [0.0, 0.0, 0.0], "speed": 0.0, "confidence": 0.9,
            "z_min": 1.0, "z_max": 1.0}


def _rows(*rows, M=4):
    out = np.zeros((M, 6), dtype=np.int32)
    for k, row in enumerate(rows):
        out[k, :len(row)] = row
    return out


def test_one_object_through_four_frames_is_one_track():
    from hipops.tracks import TrackBuilder
    b = TrackBuilder(0.25)
    ids = [b.add("f0", [_object(1, 100)], None, np.eye(4))]
    for k in range(1, 4):
        ids.append(b.add("f%d" % k, [_object(1, 100)], _rows([1, 80]), np.eye(4)))
    assert ids == [[1]] * 4 and len(b.tracks) == 1 and (b.accepted, b.refused) == (3, 0)
    t = b.summary()[0]
    assert (t["id"], t["first"], t["last"], t["length"], t["path_length"]) == (1, "f0", "f3", 4, 0.0)
    assert t["frames"][0]["iou"] is None and all(f["iou"] == 80 / 120 for f in t["frames"][1:])
    assert list(t["frames"][1]) == ["stem", "object", "pixels", "box", "centroid", "position", "motion", "speed", "confidence", "iou"]


def test_two_objects_claim_one_predecessor():
    from hipops.tracks import TrackBuilder
    # the larger vote wins; the other takes dst2
    b = TrackBuilder(0.25)
    assert b.add("f0", [_object(1, 100), _object(2, 100)], None, np.eye(4)) == [1, 2]
    ids = b.add("f1", [_object(1, 100), _object(2, 100)], _rows([1, 60, 2, 50], [1, 70, 2, 10]), np.eye(4))
    assert ids == [2, 1] and (b.accepted, b.refused) == (2, 0)
    assert b.tracks[1]["frames"][1]["iou"] == 50 / 150 and b.tracks[0]["frames"][1]["iou"] == 70 / 130
    # ... or opens a track when dst2 is not eligible; equal votes: the smaller object number goes first
    b = TrackBuilder(0.25)
    b.add("f0", [_object(1, 100), _object(2, 100)], None, np.eye(4))
    ids = b.add("f1", [_object(1, 100), _object(2, 100)], _rows([1, 70, 2, 10], [1, 70, 0, 0]), np.eye(4))
    assert ids == [1, 3] and (b.accepted, b.refused) == (1, 1) and [t["length"] for t in b.summary()] == [2, 1, 1]
    # new tracks are opened after the links, in increasing object number
    b = TrackBuilder(0.25)
    b.add("f0", [_object(1, 100)], None, np.eye(4))
    assert b.add("f1", [_object(1, 50), _object(2, 50), _object(3, 100)], _rows([0, 0], [0, 0], [1, 90]), np.eye(4)) == [2, 3, 1]


def test_min_iou_is_inclusive():
    from hipops.tracks import TrackBuilder
    for votes, linked in ((40, True), (39, False)):          # 40 / (100 + 100 - 40) == 0.25 exactly; 39 / 161 is below
        b = TrackBuilder(0.25)
        b.add("f0", [_object(1, 100)], None, np.eye(4))
        assert b.add("f1", [_object(1, 100)], _rows([1, votes]), np.eye(4)) == [1 if linked else 2]
        assert (b.accepted, b.refused) == ((1, 0) if linked else (0, 1))


def test_an_empty_frame_ends_everything():
    from hipops.tracks import TrackBuilder
    b = TrackBuilder(0.25)
    b.add("f0", [_object(1, 100), _object(2, 30)], None, np.eye(4))
    assert b.add("f1", [], _rows(), np.eye(4)) == []
    assert b.add("f2", [_object(1, 100)], _rows([1, 100]), np.eye(4)) == [3]          # a link into an empty frame links to nothing
    assert [(t["first"], t["last"], t["length"]) for t in b.summary()] == [("f0", "f0", 1), ("f0", "f0", 1), ("f2", "f2", 1)]


def _run():
    from hipops.tracks import TrackBuilder, tracks_json
    rng = np.random.default_rng(5)
    b = TrackBuilder(0.25)
    for k in range(6):
        n = int(rng.integers(0, 5))
        objects = [_object(i + 1, int(rng.integers(20, 200)), rng.standard_normal(3)) for i in range(n)]
        rows = _rows(*[[int(rng.integers(0, 5)), int(rng.integers(0, 20)), int(rng.integers(0, 5)), int(rng.integers(0, 10))] for _ in range(n)])
        G = np.eye(4)
        G[:3, 3] = rng.standard_normal(3)
        b.add("f%d" % k, objects, None if k == 0 else rows, G)
    return json.dumps(tracks_json(b, {"min_iou": 0.25}, notes=("n",)), sort_keys=True)


def test_two_runs_give_the_same_json():
    first = _run()
    assert first == _run()
    record = json.loads(first)
    assert record["count"] == len(record["tracks"]) and [t["id"] for t in record["tracks"]] == list(range(1, record["count"] + 1))
    assert record["longest"] == max(t["length"] for t in record["tracks"]) and "gap" in " ".join(record["notes"])


def test_position_is_the_chained_pose_times_the_centroid():
    from hipops.cloud import chain_poses
    from hipops.tracks import TrackBuilder
    rng = np.random.default_rng(9)
    T = np.tile(np.eye(4, dtype=np.float32), (3, 1, 1))
    T[:, :3, 3] = rng.standard_normal((3, 3)).astype(np.float32)
    T[1, :3, :3] = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], dtype=np.float32)
    G = np.concatenate([chain_poses(T[:2]), chain_poses(T[2:], start=chain_poses(T[:2])[-1])])        # across a batch boundary
    centroids = rng.standard_normal((3, 3))
    b = TrackBuilder(0.25)
    for k in range(3):
        b.add("f%d" % k, [_object(1, 100, centroids[k])], None if k == 0 else _rows([1, 100]), G[k])
    t = b.summary()[0]
    T64 = T.astype(np.float64)
    want = [centroids[0], (T64[1] @ np.append(centroids[1], 1.0))[:3], (T64[1] @ T64[2] @ np.append(centroids[2], 1.0))[:3]]
    for f, w in zip(t["frames"], want):
        assert np.allclose(f["position"], w, rtol=1e-14, atol=1e-14)
    assert t["frames"][0]["position"] == centroids[0].tolist()
    steps = [np.linalg.norm(np.array(t["frames"][k + 1]["position"]) - np.array(t["frames"][k]["position"])) for k in range(2)]
    assert t["length"] == 3 and abs(t["path_length"] - sum(steps)) <= 1e-15 * sum(steps)
    b = TrackBuilder(0.25)              # a centroid that is not finite (None in the table's JSON) has no position and adds no path
    b.add("f0", [_object(1, 100, (None, None, None))], None, G[0])
    b.add("f1", [_object(1, 100)], _rows([1, 100]), G[1])
    assert b.summary()[0]["frames"][0]["position"] == [None, None, None] and b.summary()[0]["path_length"] == 0.0


def test_track_image():
    from hipops.tracks import track_image
    labels = np.array([[0, 1, 2], [3, 2, 9]], dtype=np.uint16)
    assert track_image(labels, [7, 70000, 65535]).tolist() == [[0, 7, 65535], [65535, 65535, 0]]      # saturated; past the list: 0
    assert track_image(labels, []).tolist() == [[0, 0, 0], [0, 0, 0]] and track_image(labels, [5]).dtype == np.uint16
    with pytest.raises(ValueError):
        track_image(labels.astype(np.int32), [1])


# ---- predict.py ------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def predict():
    """The predict module with the environment put back afterwards (tests/test_cloud.py says why)."""
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


def test_the_parser(tmp_path, capsys, predict):
    base = [str(tmp_path), "--weights_init", "scratch", "--log_dir", str(tmp_path / "logs")]
    with pytest.raises(SystemExit) as stop:
        predict.parse(base + ["--save", "tracks"])
    assert stop.value.code == 2 and "--save tracks needs --motion" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        predict.parse(base + ["--save", "tracks", "--motion", "--frame_ids", "0", "1", "-1"])
    assert "frame_ids[1] == -1" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        predict.parse(base + ["--save", "tracks", "--motion", "--object_max", "1025"])
    opt = predict.parse(base + ["--save", "depth16", "tracks", "--motion"])
    assert opt.save == ["depth16", "tracks"] and opt.track_min_iou == 0.25 and predict.track_parameters(opt) == {"min_iou": 0.25}
    opt = predict.parse(base + ["--save", "tracks", "objects", "--motion", "--track_min_iou", "0.5", "--object_max", "1024"])
    assert predict.track_parameters(opt) == {"min_iou": 0.5} and predict.object_parameters(opt)["max_objects"] == 1024
    assert predict.parse(base).track_min_iou == 0.25


def test_predict_folder_refuses(tmp_path, predict):
    """The checks come before any network runs: a stand-in trainer that only names the device is enough."""
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
    opt = predict.parse([str(frames), "--weights_init", "scratch", "--log_dir", str(tmp_path / "logs"), "--motion", "--save", "tracks"])
    trainer = types.SimpleNamespace(device=torch.device("cpu"))
    out = str(tmp_path / "out")
    with pytest.raises(ValueError, match="--motion"):
        predict.predict_folder(opt, trainer, str(frames), out, save=("tracks",), motion=False)
    with pytest.raises(ValueError, match="frames of one size"):
        predict.predict_folder(opt, trainer, str(frames), out, save=("tracks",), motion=True)
    opt.frame_ids = [0, 1, -1]
    with pytest.raises(ValueError, match=r"frame_ids\[1\] == -1"):
        predict.predict_folder(opt, trainer, str(frames), out, save=("tracks",), motion=True)
    assert not os.path.exists(os.path.join(out, "tracks.json")) and not os.path.exists(os.path.join(out, "tracks"))
