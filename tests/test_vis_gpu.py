"""dd_vis_frame / dd_vis_flow_tiles on the device (through hipops.vis.SegmentRenderer) against the fp64 definition on the host
(tests/vis_case.py), held to the caps that tests/test_vis.py shows the reference's own fp32 arithmetic to sit far inside: no byte
off by more than 1 level, at most 1 % of the flow-tile bytes off at all, image and colour-map tiles identical; and end to end
through eval/visualize.py.

The shapes are the smallest that take every path: 13 x 37 (W % 4 = 1: a scalar tail in every row, row starts on every byte
alignment, three workgroups with a ragged last one) and 24 x 40 (whole groups of four, rows that start on dword boundaries in
some tiles and not in others, a partial fourth workgroup)."""
import glob
import os

import numpy as np
import pytest
import torch

import vis_case as vc

pytestmark = pytest.mark.gpu

SHAPES = [(13, 37), (24, 40)]
ALL_FLOWS = [["ego_flow", "ind_flow"], ["comp_flow", "samp_flow"]]


def _renderer(arrangement, H, W, n, **kw):
    from hipops.vis import SegmentRenderer
    return SegmentRenderer(arrangement, H, W, n, **kw)


def _render(frames, arrangement, renderer=None, **kw):
    H, W = frames[0]["disp"].shape[-2:]
    r = renderer if renderer is not None else _renderer(arrangement, H, W, len(frames), **kw)
    r.reset()
    for fr in vc.to_device(frames):
        r.add_frame(min_depth=vc.MIN_DEPTH, max_depth=vc.MAX_DEPTH, **fr)
    panel = r.finish()
    assert panel.is_cuda and panel.dtype == torch.uint8 and tuple(panel.shape) == (len(frames), r.R * H, r.C * W, 3)
    return panel.cpu(), r.maxima.cpu()


@pytest.fixture(scope="module")
def cases():
    """Per shape: the scene and its fp64 / fp32 definitions for the arrangements used below, computed once."""
    out = {}
    for H, W in SHAPES:
        frames = vc.scene(3, H, W, seed=H)
        out[H, W] = {"frames": frames,
                     "golden64": vc.render(frames, vc.GOLDEN_ARRANGEMENT, dtype=torch.float64),
                     "golden32": vc.render(frames, vc.GOLDEN_ARRANGEMENT, dtype=torch.float32),
                     "second64": vc.render(frames, vc.SECOND_ARRANGEMENT, dtype=torch.float64)}
    return out


def _assert_within_caps(got, want, arrangement, H, W, what):
    worst, share, rest_equal = vc.compare(got, want, arrangement, H, W)
    print("{} {}x{}: worst level {}, share of flow bytes off {:.5f}, other tiles equal {}".format(what, H, W, worst, share, rest_equal))
    assert worst <= 1 and share <= 1e-2 and rest_equal, (what, worst, share, rest_equal)


@pytest.mark.parametrize("H,W", SHAPES)
def test_kernel_against_fp64_definition(cases, H, W):
    case = cases[H, W]
    panel, maxima = _render(case["frames"], vc.GOLDEN_ARRANGEMENT)
    want, max64 = case["golden64"]
    _assert_within_caps(panel, want, vc.GOLDEN_ARRANGEMENT, H, W, "kernel against fp64")
    assert int(max64[1:].argmax()) == 1                                  # the segment's maximum is the middle frame's
    # the device maxima: within ten times the distance the fp32 definition keeps from the fp64 one (1e-6 at the least)
    max32 = case["golden32"][1]
    bound = max(10 * float((max32.double() - max64).abs().max()), 1e-6)
    dist = float((maxima.double() - max64).abs().max())
    print("maxima {}x{}: device {:.9f}, fp64 {:.9f}, distance {:.2e}, bound {:.2e}".format(H, W, float(maxima[0]), float(max64[0]), dist, bound))
    assert maxima.shape == max64.shape and dist <= bound


@pytest.mark.parametrize("H,W", SHAPES)
def test_second_arrangement(cases, H, W):
    """2 x 3 with ref_img, comp_flow and samp_flow: tile addressing in both directions, the transform and motion-map flags."""
    case = cases[H, W]
    panel, _ = _render(case["frames"], vc.SECOND_ARRANGEMENT)
    _assert_within_caps(panel, case["second64"][0], vc.SECOND_ARRANGEMENT, H, W, "2x3 arrangement against fp64")
    # the four flow tiles are four different pictures
    tiles = [vc.tile_of(panel, vc.SECOND_ARRANGEMENT, n, H, W) for n in ("ego_flow", "ind_flow", "comp_flow", "samp_flow")]
    assert all(not torch.equal(a, b) for i, a in enumerate(tiles) for b in tiles[i + 1:])


def test_colour_map_special_values_on_the_device():
    """Every k / 256 and its two fp32 neighbours, 0, 1, -0.1, 1.5 and NaN through both colour maps, and a mask range other than (0, 1)."""
    k = torch.arange(257, dtype=torch.float32) / 256
    vals = torch.cat([torch.tensor([0.0, 1.0, -0.1, 1.5, float("nan")]), k, torch.nextafter(k, torch.tensor(2.0)), torch.nextafter(k, torch.tensor(-2.0))])
    H, W = 8, 97
    arrangement = [["disp", "mask"]]
    fr = {"disp": vals.reshape(1, H, W), "motion_mask": (0.7 * vals).reshape(1, H, W)}
    want, _ = vc.render([fr], arrangement, mask_max_mag=0.7)
    r = _renderer(arrangement, H, W, 1, mask_max_mag=0.7)
    r.add_frame(disp=fr["disp"].cuda(), motion_mask=fr["motion_mask"].cuda())
    got = r.finish().cpu()
    assert torch.equal(got, want)
    assert torch.equal(got[0, 0, 4], torch.zeros(3, dtype=torch.uint8)) and torch.equal(got[0, 0, W + 4], torch.zeros(3, dtype=torch.uint8))     # NaN: black


def test_static_scene_is_white():
    """cam_T_cam = I and no motion: both projections are the same arithmetic, every flow tile is 255 everywhere (0 / 0 in the
    angle does not show as black); a static first frame of a moving segment has a white ego tile."""
    H, W = 13, 37
    frames = vc.scene(3, H, W, seed=5)
    still = [dict(fr, cam_T_cam=torch.eye(4), complete_flow=torch.zeros(3, H, W)) for fr in frames]
    panel, maxima = _render(still, ALL_FLOWS)
    assert bool((panel == 255).all()) and float(maxima.max()) == 0.0
    frames[0]["cam_T_cam"] = torch.eye(4)
    panel, maxima = _render(frames, vc.GOLDEN_ARRANGEMENT)
    ego = vc.tile_of(panel, vc.GOLDEN_ARRANGEMENT, "ego_flow", H, W)
    assert bool((ego[0] == 255).all()) and not bool((ego[1] == 255).all()) and float(maxima[0]) > 0


def test_reuse_after_reset_and_per_frame_maxima():
    H, W = 13, 37
    big = vc.scene(3, H, W, seed=6, flow=0.5, step=0.2)
    small = vc.scene(2, H, W, seed=7, flow=0.01, step=0.002)
    r = _renderer(vc.GOLDEN_ARRANGEMENT, H, W, 3)
    a, max_a = _render(big, vc.GOLDEN_ARRANGEMENT, renderer=r)
    a, max_a = a.clone(), max_a.clone()
    b, max_b = _render(small, vc.GOLDEN_ARRANGEMENT, renderer=r)             # reset() inside: nothing of segment A is left
    fresh, max_fresh = _render(small, vc.GOLDEN_ARRANGEMENT)
    assert float(max_a[0]) > 10 * float(max_fresh[0]) > 0
    assert torch.equal(b, fresh) and torch.equal(max_b, max_fresh) and tuple(b.shape) == (2, H, 5 * W, 3)
    # consistent_flow=False: every frame normalised by its own maximum = every frame rendered as its own segment
    per_frame, maxima = _render(big, vc.GOLDEN_ARRANGEMENT, consistent_flow=False)
    for n, fr in enumerate(big):
        alone, max_alone = _render([fr], vc.GOLDEN_ARRANGEMENT)
        assert torch.equal(per_frame[n], alone[0]) and float(maxima[1 + n]) == float(max_alone[0])
    assert not torch.equal(per_frame, a) and torch.equal(maxima, max_a)
    # flow_mag_factor scales the normalisation
    half, _ = _render(big, vc.GOLDEN_ARRANGEMENT, flow_mag_factor=0.5)
    want, _ = vc.render(big, vc.GOLDEN_ARRANGEMENT, dtype=torch.float64, flow_mag_factor=0.5)
    _assert_within_caps(half, want, vc.GOLDEN_ARRANGEMENT, H, W, "flow_mag_factor 0.5")


def test_two_runs_are_byte_identical(cases):
    frames = cases[24, 40]["frames"]
    a, max_a = _render(frames, vc.SECOND_ARRANGEMENT)
    b, max_b = _render(frames, vc.SECOND_ARRANGEMENT)
    assert torch.equal(a, b) and torch.equal(max_a, max_b)


def test_argument_errors_launch_nothing():
    from hipops import abi, lib as L
    from hipops.lib import DynamoHipError
    H, W = 13, 37
    frames = vc.to_device(vc.scene(2, H, W, seed=8))
    r = _renderer(vc.GOLDEN_ARRANGEMENT, H, W, 1)
    r.add_frame(**frames[0])
    before, max_before = r.panel.clone(), r.maxima.clone()
    with pytest.raises(DynamoHipError, match="frame 2 of a renderer for 1 frames"):            # more frames than max_frames
        r.add_frame(**frames[1])
    r.reset()
    with pytest.raises(DynamoHipError, match="`disp` must be"):                                 # a CPU tensor
        r.add_frame(**dict(frames[1], disp=frames[1]["disp"].cpu()))
    with pytest.raises(DynamoHipError, match="needs `cam_T_cam`"):
        r.add_frame(**{k: v for k, v in frames[1].items() if k != "cam_T_cam"})
    with pytest.raises(DynamoHipError, match="no frame was added"):
        r.finish()
    with pytest.raises(DynamoHipError, match="at most 16 tiles"):                               # a seventeenth tile
        _renderer([["img"] * 17], H, W, 1)
    # the entry points themselves: hipErrorInvalidValue (1)
    lib = L.load()
    fr = frames[1]

    def frame_call(tiles, n_tiles, R=1, C=5, frame=0, panel=r.panel, h=H):
        arr = (abi.C.c_int * len(tiles))(*tiles)
        return lib.dd_vis_frame(abi.ptr(fr["color"]), None, abi.ptr(fr["disp"]), abi.ptr(fr["motion_mask"]), abi.ptr(fr["complete_flow"]), abi.ptr(fr["K"]),
                                abi.ptr(fr["inv_K"]), abi.ptr(fr["cam_T_cam"]), 0.1, 100.0, h, W, arr, n_tiles, R, C, abi.ptr(r._lut), 0.0, 1.0, 0.0, 1.0, frame, 1,
                                abi.ptr(panel), abi.ptr(r.side), abi.ptr(r._maxima), L.current_stream())

    good = [0, 0, 0, 2, 0, 1, 4, 0, 2, 5, 0, 3, 3, 0, 4]
    assert frame_call(good[:12] + [3, 0, 5], 5) == 1                    # a tile outside R x C (column 5 of 5)
    assert frame_call(good[:12] + [3, 1, 4], 5) == 1                    # (row 1 of 1)
    assert frame_call(good[:12] + [8, 0, 4], 5) == 1                    # no such kind
    assert frame_call([0, 0, 0] * 17, 17) == 1                          # a seventeenth tile
    assert frame_call(good, 5, frame=1) == 1                            # frame outside max_frames
    assert frame_call(good, 5, panel=None) == 1                         # a null pointer
    assert frame_call(good[:12] + [1, 0, 4], 5) == 1                    # ref_img without ref_color
    assert frame_call(good, 5, h=0) == 1                                # a non-positive size
    with pytest.raises(DynamoHipError, match="dd_vis_frame failed"):
        L.check(frame_call(good[:12] + [3, 0, 5], 5), "dd_vis_frame")
    arr = (abi.C.c_int * 15)(*good)
    for args in ((None, abi.ptr(r._maxima), arr, 5, 1, 5, H, W, 1), (abi.ptr(r.side), None, arr, 5, 1, 5, H, W, 1), (abi.ptr(r.side), abi.ptr(r._maxima), arr, 5, 1, 4, H, W, 1),
                 (abi.ptr(r.side), abi.ptr(r._maxima), arr, 5, 1, 5, H, W, 0), (abi.ptr(r.side), abi.ptr(r._maxima), arr, 17, 1, 5, H, W, 1)):
        assert lib.dd_vis_flow_tiles(*args, 1.0, 1, abi.ptr(r.panel), L.current_stream()) == 1
    torch.cuda.synchronize()
    assert torch.equal(r.panel, before) and float(r._maxima.abs().max()) == 0.0 and float(max_before[0]) > 0


def test_script_end_to_end(tmp_path, monkeypatch):
    """eval/visualize.py --synthetic: eight frames of (64, 5 * 96, 3), as PNG files where imageio is not installed; the torch backend
    (get_vis / combine_vis through the host) on the same seed within the caps."""
    from eval import visualize as ev
    from PIL import Image
    H, W = 64, 96
    args = ["-d", "kitti", "--synthetic", "--height", str(H), "--width", str(W), "--weights_init", "scratch", "--num_workers", "0",
            "--log_dir", str(tmp_path / "logs")]
    panels = {}
    for backend in ("hip", "torch"):
        if backend == "torch":
            pytest.importorskip("matplotlib")
        torch.manual_seed(0)
        written = ev.main(args + ["--eval_dir", str(tmp_path / backend), "--vis_backend", backend])
        assert len(written) == 1 and str(written[0]).startswith(str(tmp_path / backend)) and os.sep + "vis" + os.sep in str(written[0])
        try:
            import imageio  # noqa: F401
            assert written[0].endswith("segment-0.mp4") and os.path.getsize(written[0]) > 0
            continue
        except ImportError:
            pass
        files = sorted(glob.glob(os.path.join(written[0], "*.png")))
        assert [os.path.basename(f) for f in files] == ["{:06d}.png".format(i) for i in range(8)]
        panels[backend] = np.stack([np.asarray(Image.open(f)) for f in files])
        assert panels[backend].shape == (8, H, 5 * W, 3) and panels[backend].dtype == np.uint8
    if len(panels) == 2:
        _assert_within_caps(panels["hip"], panels["torch"], ev.ARRANGEMENT, H, W, "script, hip against torch backend")
        assert len(np.unique(panels["hip"])) > 32                        # a picture, not a constant
