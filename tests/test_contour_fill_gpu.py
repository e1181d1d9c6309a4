"""dd_fill_contours on the device: hand-made contours against the brute-force definition of tests/contour_fill_case.py, the
tiny_waymo frame against its panoptic labels.  Equality is exact everywhere.  (The loader -> Trainer -> evaluation path on the
fixture: tests/test_waymo_eval_gpu.py.)"""
import numpy as np
import pytest
import torch

import contour_fill_case as cc
import test_waymo_reader as wr

pytestmark = pytest.mark.gpu


def _records(batch, height, width, v_cap=512, c_cap=128):
    """Device records of a batch of object lists.  c_cap = 128: two rounds of 64 records in the kernel."""
    from hipops import contours
    packed = [contours.pack(objects, height, width, "sample {}".format(i), v_cap, c_cap) for i, objects in enumerate(batch)]
    return torch.from_numpy(np.stack([p[0] for p in packed])).cuda(), torch.from_numpy(np.stack([p[1] for p in packed])).cuda()


def _fill(batch, height, width, **caps):
    from hipops.contours import fill_contours
    vertices, records = _records(batch, height, width, **caps)
    out = torch.full((len(batch), height, width), 0xFF, dtype=torch.uint8, device="cuda")       # every byte must be written
    assert fill_contours(vertices, records, height, width, out=out) is out
    return out.cpu().numpy()


def _batches():
    """Three samples each, with different object counts; the first batch of a canvas has the sample without objects."""
    names = list(cc.cases(*cc.CANVASES[0]))
    names.remove("no_objects")
    triples = [("border_rectangle", "no_objects", "many_contours")]
    rest = [n for n in names if n not in triples[0]]
    triples += [tuple(rest[i:i + 3]) for i in range(0, len(rest), 3)]
    return [(h, w, t) for h, w in cc.CANVASES for t in triples]


@pytest.mark.parametrize("height,width,names", _batches(), ids=lambda v: "+".join(v) if isinstance(v, tuple) else str(v))
def test_hand_made_contours_equal_the_brute_force_definition(height, width, names):
    table = cc.cases(height, width)
    got = _fill([table[n] for n in names], height, width)
    for i, name in enumerate(names):
        want = np.array(cc.expected(name, height, width), dtype=np.uint8)
        assert np.array_equal(got[i], want), (name, np.argwhere(got[i] != want)[:8])
        if name == "no_objects":
            assert not got[i].any()


def test_every_hand_made_case_is_covered():
    used = {n for _, _, t in _batches() for n in t}
    assert used == set(cc.cases(*cc.CANVASES[0])) and all(len(t) == 3 for _, _, t in _batches())


def test_real_contours_on_a_small_canvas():
    """The fixture's objects whose bounding box fits 64x64, translated to a 67x70 canvas: the translated crop of their panoptic mask."""
    height, width, oy, ox = 67, 70, 2, 5
    batch, wants = [], []
    for (label, contours), (_, mask) in zip(wr.fixture_objects(), wr.panoptic_objects()):
        if not contours:
            continue
        pts = np.concatenate(contours)
        x0, y0, x1, y1 = pts[:, 0].min(), pts[:, 1].min(), pts[:, 0].max(), pts[:, 1].max()
        if x1 - x0 >= 64 or y1 - y0 >= 64:
            continue
        batch.append([(label, [c - np.array([x0 - ox, y0 - oy]) for c in contours])])
        want = np.zeros((height, width), dtype=np.uint8)
        want[oy:oy + y1 - y0 + 1, ox:ox + x1 - x0 + 1] = mask[y0:y1 + 1, x0:x1 + 1] * label
        assert int(mask.sum()) == int(mask[y0:y1 + 1, x0:x1 + 1].sum())
        wants.append(want)
    assert len(batch) >= 5
    got = _fill(batch, height, width, v_cap=1024, c_cap=16)
    for i, want in enumerate(wants):
        assert np.array_equal(got[i], want), (i, np.argwhere(got[i] != want)[:8])


def test_fixture_frame_at_full_size():
    """The 1920-wide path: the frame twice with a sample without objects between them, one launch."""
    from hipops import contours
    objects = wr.fixture_objects()
    got = _fill([objects, [], objects], 1280, 1920, v_cap=contours.V_CAP, c_cap=contours.C_CAP)
    want = wr.panoptic_motion_mask()
    assert np.array_equal(got[0], want), int((got[0] != want).sum())
    assert np.array_equal(got[2], want) and not got[1].any()
    assert {int(l): int(c) for l, c in zip(*np.unique(got[0], return_counts=True))} == wr.LABEL_COUNTS


def test_unaligned_output_base_and_argument_checks():
    from hipops import abi, lib as L
    height, width = cc.CANVASES[0]
    names = ("ring_hole_island", "no_objects", "staircase")
    table = cc.cases(height, width)
    vertices, records = _records([table[n] for n in names], height, width)
    n = 3 * height * width
    buf = torch.full((n + 16,), 0xEE, dtype=torch.uint8, device="cuda")
    lib = L.load()
    args = (abi.ptr(vertices), 512, abi.ptr(records), 128, 3, height, width)
    L.check(lib.dd_fill_contours(*args, buf.data_ptr() + 3, L.current_stream()), "dd_fill_contours")
    host = buf.cpu().numpy()
    assert (host[:3] == 0xEE).all() and (host[3 + n:] == 0xEE).all()                # the bytes around the output are untouched
    got = host[3:3 + n].reshape(3, height, width)
    for i, name in enumerate(names):
        assert np.array_equal(got[i], np.array(cc.expected(name, height, width), dtype=np.uint8)), name
    # hipErrorInvalidValue (1), nothing launched
    out = buf.data_ptr()
    assert lib.dd_fill_contours(None, 512, abi.ptr(records), 128, 3, height, width, out, L.current_stream()) == 1
    assert lib.dd_fill_contours(abi.ptr(vertices), 512, None, 128, 3, height, width, out, L.current_stream()) == 1
    assert lib.dd_fill_contours(*args, None, L.current_stream()) == 1
    assert lib.dd_fill_contours(abi.ptr(vertices), 512, abi.ptr(records), 128, 3, 0, width, out, L.current_stream()) == 1
    assert lib.dd_fill_contours(abi.ptr(vertices), 512, abi.ptr(records), 128, 3, height, 40000, out, L.current_stream()) == 1
    assert lib.dd_fill_contours(abi.ptr(vertices), 0, abi.ptr(records), 128, 3, height, width, out, L.current_stream()) == 1
    assert lib.dd_fill_contours(abi.ptr(vertices), 512, abi.ptr(records), 128, 0, height, width, out, L.current_stream()) == 1
    torch.cuda.synchronize()
    assert np.array_equal(buf.cpu().numpy(), host)


def test_two_launches_give_identical_bytes():
    height, width = cc.CANVASES[1]
    table = cc.cases(height, width)
    batch = [table["many_contours"], table["run_touching_a_diamond_tip"], table["label_255"]]
    assert np.array_equal(_fill(batch, height, width), _fill(batch, height, width))
