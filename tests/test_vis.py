"""The visualisation panels on the host: tests/vis_case.py (the definition csrc/dd_vis.hip is held to on the GPU, tests/test_vis_gpu.py)
against a panel the unmodified reference produced (tests/golden/make_golden_vis.py), the premise of the GPU tolerance, and the
committed colour-map tables against matplotlib.

Measured on the golden inputs (three 24 x 40 frames, 17 280 flow-tile bytes): the fp32 definition reproduces the reference's panel
byte for byte, the fp32 and fp64 definitions differ in 0 bytes (on the other scenes of tests/test_vis_gpu.py: up to 0.05 % of the
bytes, never more than 1 level), their segment maxima lie 5.0e-8 apart (0.506201029 against 0.506200979)."""
import os

import numpy as np
import pytest
import torch

import vis_case as vc

N, H, W = 3, 24, 40


@pytest.fixture(scope="module")
def golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "vis_panel.npz"))
    keys = [k for k in g.files if k not in ("panel", "mags")]
    frames = [{k: torch.from_numpy(g[k][n]) for k in keys} for n in range(N)]
    return {"frames": frames, "panel": torch.from_numpy(g["panel"]), "mags": torch.from_numpy(g["mags"]),
            "fp32": vc.render(frames, vc.GOLDEN_ARRANGEMENT, dtype=torch.float32), "fp64": vc.render(frames, vc.GOLDEN_ARRANGEMENT, dtype=torch.float64)}


def test_golden_inputs_are_the_shared_scene(golden):
    assert tuple(golden["panel"].shape) == (N, H, 5 * W, 3) and golden["panel"].dtype == torch.uint8
    for got, want in zip(golden["frames"], vc.scene(N, H, W, seed=0)):
        for k in want:
            assert torch.equal(got[k], want[k]), k
    assert int(golden["mags"].max(1).values.argmax()) == 1              # the segment's largest flow is the middle frame's


def test_fp32_definition_reproduces_the_reference_panel(golden):
    panel, maxima = golden["fp32"]
    worst, share, rest_equal = vc.compare(panel, golden["panel"], vc.GOLDEN_ARRANGEMENT, H, W)
    print("fp32 definition against the reference: worst level {}, share of flow bytes off {:.5f}, other tiles equal {}".format(worst, share, rest_equal))
    assert worst <= 1 and share <= 1e-3 and rest_equal
    # the reference's per-frame `mag` is its largest magnitude + 1e-8
    want = golden["mags"].max(1).values
    assert float((maxima[1:].double() + 1e-8 - want).abs().max()) <= 1e-6
    assert abs(float(maxima[0]) + 1e-8 - float(want.max())) <= 1e-6


def test_fp32_against_fp64_definition(golden):
    """The premise of the GPU test's tolerance: fp32 arithmetic of the reference's own kind sits far inside the caps."""
    (p32, m32), (p64, m64) = golden["fp32"], golden["fp64"]
    worst, share, rest_equal = vc.compare(p32, p64, vc.GOLDEN_ARRANGEMENT, H, W)
    print("fp32 against fp64 definition: worst level {}, share of flow bytes off {:.5f}; maxima {:.9f} / {:.9f}".format(worst, share, float(m32[0]), float(m64[0])))
    assert worst <= 1 and share <= 1e-2 and rest_equal
    assert abs(float(m32[0]) - float(m64[0])) <= 1e-6
    assert m64.dtype == torch.float64 and int(m64[1:].argmax()) == 1


def _special_values():
    k = torch.arange(257, dtype=torch.float32) / 256
    vals = torch.cat([torch.tensor([0.0, 1.0, -0.1, 1.5, float("nan")]), k, torch.nextafter(k, torch.tensor(2.0)), torch.nextafter(k, torch.tensor(-2.0))])
    kk = torch.arange(257)
    want = torch.cat([torch.tensor([0, 255, 0, 255, -1]), kk.clamp(max=255), kk.clamp(max=255), (kk - 1).clamp(min=0)])
    return vals, want


def test_colour_map_special_values():
    """k / 256 is the first value of entry k, the float below it the last of entry k - 1; 1 and everything above it is entry 255,
    everything below 0 entry 0, NaN black."""
    vals, want = _special_values()
    assert torch.equal(vc.cmap_index(vals), want)
    table = np.arange(768, dtype=np.uint8).reshape(256, 3)
    got = vc.cmap_bytes(vals, table)
    assert torch.equal(got[4], torch.zeros(3, dtype=torch.uint8)) and torch.equal(got[1], torch.from_numpy(table[255]))
    # another range: the same entries for the same position in it
    assert torch.equal(vc.cmap_index(torch.tensor([0.5, 1.0, 2.0, 4.0, 0.25]), 0.5, 2.5), torch.tensor([0, 64, 192, 255, 0]))


def test_committed_tables_are_matplotlibs():
    matplotlib = pytest.importorskip("matplotlib")
    from hipops import vis
    import utils
    vals, _ = _special_values()
    for name in ("plasma", "hot"):
        cmap = matplotlib.colormaps[name]
        cmap._init()
        assert cmap.N == 256
        assert np.array_equal(vis.cmap_bytes(name), (cmap._lut[:256, :3] * 255).astype(np.uint8)), name
        # and the whole path of the reference (utils.score_map_vis, then (x * 255).astype(uint8)) on the special values
        with np.errstate(invalid="ignore"):
            want = (utils.score_map_vis(vals.reshape(1, 1, 8, 97), name, vminmax=(0, 1)) * 255).astype(np.uint8)
        got = vc.cmap_bytes(vals, vis.cmap_bytes(name)).reshape(8, 97, 3).numpy()
        assert np.array_equal(got, want), name


def test_arrangement_checks():
    from hipops import vis
    from hipops.lib import DynamoHipError
    tiles, R, C = vis.tile_list(vc.SECOND_ARRANGEMENT)
    assert (R, C) == (2, 3) and tiles[1] == (6, 0, 1) and tiles[5] == (5, 1, 2)
    with pytest.raises(DynamoHipError, match=r"Arrangement name \(=flow\) not recognized\."):
        vis.tile_list([["img", "flow"]])
    with pytest.raises(DynamoHipError, match="at most 16 tiles"):
        vis.tile_list([["img"] * 9, ["disp"] * 8])
    with pytest.raises(DynamoHipError):
        vis.tile_list("img")
    with pytest.raises(DynamoHipError, match="on the GPU"):
        vis.SegmentRenderer(vc.GOLDEN_ARRANGEMENT, H, W, 3, device="cpu")
    assert vis.lut_words().shape == (2, 256) and int(vis.lut_words()[1, 255]) == 0xffffff


def test_combine_vis_is_the_reference_arithmetic(golden):
    """eval/visualize.py's combine_vis (the --vis_backend torch path, what the demo notebook calls) on the golden inputs through this
    tree's vis_motion arithmetic: the reference's panel."""
    pytest.importorskip("matplotlib")
    import types
    from eval import visualize as ev
    import Trainer as T
    import oracle.ref_loss as orc
    me = types.SimpleNamespace(device=torch.device("cpu"), backproject_depth={0: orc.backproject},
                               project_3d={0: lambda pts, K, Tm: orc.project(pts, K, Tm, H, W)})
    vis_list = []
    for fr in golden["frames"]:
        color, disp, mask, cflow, K, inv_K, cam = (fr[k].unsqueeze(0) for k in ("color", "disp", "motion_mask", "complete_flow", "K", "inv_K", "cam_T_cam"))
        depth = 1 / (1 / vc.MAX_DEPTH + (1 / vc.MIN_DEPTH - 1 / vc.MAX_DEPTH) * disp)
        col = {"img": color, "disp": disp, "mask": mask}
        _, hsv, mag = T.Trainer.vis_motion(me, depth=depth, K=K, inv_K=inv_K, motion_map=None, camTcam=cam)
        col["ego_flow"] = {"hsv": hsv, "mag": mag}
        ego = me.project_3d[0](me.backproject_depth[0](depth, inv_K), K, cam)[1]
        _, hsv, mag = T.Trainer.vis_motion(me, depth=depth, K=K, inv_K=inv_K, motion_map=mask * (cflow - ego.reshape(-1, 3, H, W)), camTcam=None)
        col["ind_flow"] = {"hsv": hsv, "mag": mag}
        vis_list.append(col)
    out = ev.combine_vis(vis_list, vc.GOLDEN_ARRANGEMENT)
    assert len(out) == N and out[0].shape == (H, 5 * W, 3) and out[0].dtype == np.uint8
    worst, share, rest_equal = vc.compare(np.stack(out), golden["panel"], vc.GOLDEN_ARRANGEMENT, H, W)
    assert worst <= 1 and share <= 1e-3 and rest_equal
    with pytest.raises(Exception, match=r"Arrangement name \(=bogus\) not recognized\."):
        ev.combine_vis(vis_list, [["img", "bogus"]])
