"""hipops/objects.py on the host: the labelling against scipy.ndimage.label on every mask of objects_case, the min_pixels and
max_objects rules on hand-built cases, the table and what goes to JSON, the label image's index formula, predict.py's parser."""
import json

import numpy as np
import pytest

import objects_case as OC
from hipops import objects as O


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("shape", OC.SHAPES, ids=["x".join(map(str, s)) for s in OC.SHAPES])
def test_labelling_is_scipys(shape, connectivity):
    ndimage = pytest.importorskip("scipy.ndimage")
    structure = np.ones((3, 3), dtype=int) if connectivity == 8 else None
    for name in OC.NAMES:
        fg = OC.pattern(shape, name)
        labels, found, truncated = O.label_components_host(OC.inputs(shape, name)["mask"], thresh=OC.THRESH, connectivity=connectivity, min_pixels=1,
                                                           max_objects=O.MAX_OBJECTS)
        assert labels.dtype == np.int32 and labels.shape == fg.shape and not truncated.any()
        for b in range(OC.B):
            want, n = ndimage.label(fg[b], structure=structure)
            assert n == found[b] and np.array_equal(labels[b], want), (shape, name, connectivity, b)


def test_masks_are_what_their_names_say():
    """The properties the cases are there for, from the reference alone."""
    shape = (37, 53)
    count = lambda name, c: OC.reference(shape, name, c)[2][0, 1]           # noqa: E731
    assert count("empty", 8) == 0 and OC.reference(shape, "empty", 8)[2][1, 1] == 1             # image 1 of `empty` is full
    assert count("full", 4) == 1 and OC.reference(shape, "full", 4)[2][1, 1] == 0
    assert count("checker", 4) == 981 and count("checker", 8) == 1
    assert count("serpentine", 4) == 1 and count("spiral", 4) == 1
    assert count("rings", 8) == count("rings", 4) == 10                     # min(37, 53) = 37 -> rings 0, 2, ..., 18: nested, none merged
    assert count("comb", 4) == 13 + 1                                       # 13 whole Us and the single column 52
    assert count("diagonals", 8) == 1 and count("diagonals", 4) == 2 * 37 - 1                   # 37 pixels each, crossing in the one pixel (26, 26)
    assert count("corners", 8) == 4
    assert OC.reference((64, 96), "blobs", 8)[2][0, 1] == 22                # a few dozen objects at the network size
    labels = OC.reference(shape, "nan_thresh", 8)[0]
    mask = OC.inputs(shape, "nan_thresh")["mask"][:, 0]
    assert np.isnan(mask).any() and (mask == np.float32(OC.THRESH)).any() and (labels[mask == np.float32(OC.THRESH)] > 0).all() and (labels[np.isnan(mask)] == 0).all()


def test_caps():
    OC.check_caps()


def test_min_pixels_and_max_objects():
    m = np.zeros((1, 6, 9), dtype=np.float32)
    m[0, 0, 0:3] = 1            # 3 pixels, anchor 0
    m[0, 0, 5] = 1              # 1 pixel, anchor 5
    m[0, 2:4, 4:6] = 1          # 4 pixels, anchor 22
    m[0, 5, 0:2] = 1            # 2 pixels, anchor 45
    m[0, 4, 2] = 1              # joins the pair under 8-connectivity only: 3 pixels, anchor 38
    kw = dict(thresh=0.5)
    labels, found, truncated = O.label_components_host(m, connectivity=4, min_pixels=1, max_objects=10, **kw)
    assert found[0] == 5 and not truncated[0] and [labels[0].reshape(-1)[i] for i in (0, 5, 22, 38, 45)] == [1, 2, 3, 4, 5]
    labels, found, truncated = O.label_components_host(m, connectivity=4, min_pixels=2, max_objects=10, **kw)
    assert found[0] == 3 and [labels[0].reshape(-1)[i] for i in (0, 5, 22, 38, 45)] == [1, 0, 2, 0, 3]          # the numbering closes up
    labels, found, truncated = O.label_components_host(m, connectivity=8, min_pixels=3, max_objects=10, **kw)
    assert found[0] == 3 and [labels[0].reshape(-1)[i] for i in (0, 5, 22, 38, 45)] == [1, 0, 2, 3, 3]
    labels, found, truncated = O.label_components_host(m, connectivity=4, min_pixels=1, max_objects=2, **kw)
    assert found[0] == 5 and truncated[0] and labels.max() == 2 and (labels[0, 2:] == 0).all()                  # cut components read as background
    labels, found, truncated = O.label_components_host(m, connectivity=4, min_pixels=1, max_objects=5, **kw)
    assert found[0] == 5 and not truncated[0] and labels.max() == 5
    for bad in (dict(connectivity=6), dict(min_pixels=0), dict(max_objects=0), dict(max_objects=65536)):
        with pytest.raises(ValueError):
            O.label_components_host(m, **dict(dict(connectivity=8, min_pixels=1, max_objects=4), **bad))


def test_table_of_a_hand_built_case():
    """One 2 x 2 object at a constant disparity under the identity pose and zero flow: the numbers by hand."""
    h, w = 4, 5
    mask = np.zeros((1, 1, h, w), dtype=np.float32)
    mask[0, 0, 1:3, 2:4] = 0.75
    disp = np.full((1, 1, h, w), 0.5, dtype=np.float32)
    flow = np.zeros((1, 3, h, w), dtype=np.float32)
    pose = np.eye(4, dtype=np.float32)[None, :3].copy()
    pose[0, 0, 3] = 0.25        # the camera's motion shifts every point by +0.25 in x: ego = (0.25, 0, 0)
    labels, table, counts = O.objects_host(mask, disp, flow, np.ones(1, np.float32), pose, (2.0, 4.0, 2.5, 1.5), min_depth=0.1, max_depth=100.0,
                                           min_pixels=1, max_objects=3)
    assert counts.tolist() == [[1, 1, 0]] and table.shape == (1, 3, O.ROW) and table.dtype == np.int32 and not table[0, 1:].any()
    row = O.rows(table)[0, 0]
    lo, span = O.depth_params(0.1, 100.0)
    z = np.float32(1) / np.float32(lo + span * np.float32(0.5))
    assert row["pixels"] == 4 and row["box"].tolist() == [2, 1, 3, 2] and row["anchor"] == 7 and row["z"].tolist() == [z, z]
    assert np.allclose(row["sums"], [4 * 0.0 * z, 4 * 0.0 * z, 4 * z, -1.0, 0, 0, 3.0], atol=1e-6)          # xc = -0.25, +0.25; yc = -0.125, +0.125
    frame = O.unpack_table(table, counts, size=(h, w, 8, 15))[0]
    assert frame["found"] == 1 and frame["truncated"] is False and len(frame["objects"]) == 1
    obj = frame["objects"][0]
    assert obj["id"] == 1 and obj["pixels"] == 4 and obj["box"] == [6, 2, 11, 5] and obj["confidence"] == 0.75
    assert np.allclose(obj["motion"], [-0.25, 0, 0], atol=1e-6) and abs(obj["speed"] - 0.25) < 1e-6 and abs(obj["centroid"][2] - z) < 1e-7


def test_unpack_table_round_trips_through_json():
    shape, name = (37, 53), "blobs"
    labels, table, counts = OC.reference(shape, name, 8)
    frames = O.unpack_table(table, counts)
    assert json.loads(json.dumps(frames, allow_nan=False)) == frames            # plain values, no NaN: what a strict reader accepts
    r = O.rows(table)
    keys = {"id", "pixels", "box", "anchor", "centroid", "motion", "speed", "confidence", "z_min", "z_max"}
    for b, frame in enumerate(frames):
        assert set(frame) == {"found", "truncated", "objects"} and frame["found"] == counts[b, 1] and len(frame["objects"]) == counts[b, 0]
        for n, obj in enumerate(frame["objects"]):
            row = r[b, n]
            assert set(obj) == keys and obj["id"] == n + 1 and obj["pixels"] == row["pixels"] == (labels[b] == n + 1).sum()
            assert obj["box"] == row["box"].tolist() and obj["anchor"] == row["anchor"] == np.flatnonzero(labels[b].reshape(-1) == n + 1)[0]
            if np.isfinite(row["sums"]).all():
                assert np.array_equal(np.array(obj["centroid"] + obj["motion"] + [obj["confidence"]]) * obj["pixels"], row["sums"] / row["pixels"] * row["pixels"])
                assert obj["z_min"] == float(row["z"][0]) and obj["z_max"] == float(row["z"][1]) and 0 < obj["z_min"] <= obj["z_max"]
            else:
                assert None in obj["centroid"] and obj["speed"] is None
    # the NaN disparity of image 0 sits in exactly one row, and in none of image 1
    bad = ~np.isfinite(r["sums"]).all(axis=2)
    assert bad[0].sum() == 1 and bad[1].sum() == 0


def test_scale_box_and_label_image_formula():
    assert O.scale_box([0, 0, 95, 63], 64, 96, 192, 640) == [0, 0, 639, 191]
    assert O.scale_box([1, 2, 1, 2], 64, 96, 192, 640) == [6, 6, 13, 8]              # x: 6.67 .. 13.33, y: 6 .. 9
    assert O.scale_box([3, 1, 4, 2], 5, 7, 5, 7) == [3, 1, 4, 2]
    rng = np.random.default_rng(5)
    for (h, w), (H, W) in (((5, 7), (11, 20)), ((64, 96), (192, 640)), ((4, 6), (2, 3)), ((3, 3), (3, 3))):
        labels = rng.integers(0, 70000, (2, h, w)).astype(np.int32)
        got = O.labels_u16_host(labels, H, W)
        assert got.dtype == np.uint16 and got.shape == (2, H, W)
        for Y in range(H):
            for X in range(0, W, max(1, W // 7)):
                y, x = min(h - 1, int((Y + 0.5) * h / H)), min(w - 1, int((X + 0.5) * w / W))           # the pixel under the destination's centre
                assert got[0, Y, X] == min(labels[0, y, x], 65535)
    assert np.array_equal(O.labels_u16_host(labels, 3, 3), np.minimum(labels, 65535).astype(np.uint16))


@pytest.fixture
def predict():
    """The predict module with the environment it prepares put back afterwards (tests/test_cloud.py says why)."""
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


def test_objects_without_motion_are_refused_by_the_parser(tmp_path, capsys, predict):
    base = [str(tmp_path), "--weights_init", "scratch", "--log_dir", str(tmp_path / "logs")]
    with pytest.raises(SystemExit) as stop:
        predict.parse(base + ["--save", "depth16", "objects"])
    assert stop.value.code == 2 and "--save objects needs --motion" in capsys.readouterr().err
    for bad in (["--object_connectivity", "6"], ["--object_min_pixels", "0"], ["--object_max", "0"], ["--object_max", "65536"]):
        with pytest.raises(SystemExit):
            predict.parse(base + ["--motion", "--save", "objects"] + bad)
    opt = predict.parse(base + ["--motion", "--save", "depth16", "objects"])
    assert opt.save == ["depth16", "objects"]
    assert predict.object_parameters(opt) == {"motion_thresh": 0.5, "connectivity": 8, "min_pixels": 16, "max_objects": 256}
    opt = predict.parse(base + ["--motion", "--save", "objects", "--object_motion_thresh", "0.25", "--object_connectivity", "4", "--object_min_pixels", "3",
                                "--object_max", "7"])
    assert predict.object_parameters(opt) == {"motion_thresh": 0.25, "connectivity": 4, "min_pixels": 3, "max_objects": 7}
    opt = predict.parse(base)           # nothing changes without the option
    assert opt.save == ["depth16"] and not opt.motion
