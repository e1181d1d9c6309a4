"""The inputs of tests/test_ops_parity_gpu.py are what that file claims, asserted from the oracle alone (no GPU, no kernel): a quiet
drift in tests/golden/synth.py or tests/ops_case.py cannot turn the GPU tests vacuous or ill-conditioned."""
import pytest
import torch

import ops_case as OC

# the kernels' launch geometry, stated here and not imported from anywhere: 256 pixels per block, fold16_kernel folds 256 block
# partials per trip, dd_disp_to_depth launches at most 4096 blocks of 256
PIXELS_PER_BLOCK, PARTIALS_PER_TRIP, D2D_MAX_BLOCKS, D2D_BLOCK = 256, 256, 4096, 256


def rel(a, b):
    return float((a - b).norm()) / float(b.norm())


@pytest.mark.parametrize("invert", [False, True])
def test_pose_sweep_is_well_conditioned(invert):
    """every magnitude of the sweep: the fp32 oracle's g_axisangle sits within 5e-4 of float64 (relative L2), so 4 x that is a bar"""
    for s in OC.POSE_SWEEP:
        r = OC.pose_ref(OC.POSE_SWEEP_B, s, invert)
        if s == 0.0:
            assert float(r.g64[0].abs().max()) == 0.0 and float(r.g32[0].abs().max()) == 0.0      # exactly 0 at theta = 0
            continue
        assert rel(r.g32[0], r.g64[0]) <= 5e-4, (s, rel(r.g32[0], r.g64[0]))
        assert rel(r.g32[1], r.g64[1]) <= 1e-5, s
    for kind in ("mixed", "pi"):
        r = OC.pose_ref(OC.POSE_SWEEP_B, kind, invert)
        assert rel(r.g32[0], r.g64[0]) <= 5e-4, kind
    theta = OC.pose_ref(OC.POSE_SWEEP_B, "pi", invert).args[0].norm(dim=2)
    assert float((theta - torch.pi).abs().max()) <= 1.001e-3
    mixed = OC.pose_ref(OC.POSE_SWEEP_B, "mixed", invert).args[0].norm(dim=2).flatten()
    assert int((mixed == 0).sum()) == (OC.POSE_SWEEP_B + 2) // 3 and int((mixed > 0).sum()) > 0


@pytest.mark.parametrize("shape", OC.GEOM_SHAPES, ids=str)
def test_behind_camera_scenes(shape):
    s = OC.scene(*shape, "behind")
    for with_T in (True, False):
        z = OC.camera_z(s, with_T)
        assert float(z.abs().min()) >= 1e-2, float(z.abs().min())
        assert 0.2 <= float((z < 0).double().mean()) <= 0.4, float((z < 0).double().mean())
    z = OC.camera_z(OC.scene(*shape, "front"))
    assert float(z.min()) >= 5e-2
    for which in ("pix", "ego", "both"):
        for kind in ("front", "behind"):
            r = OC.project_ref(*shape, kind, True, which)
            assert rel(r.g32[0], r.g64[0]) <= 1e-5 and rel(r.g32[1], r.g64[1]) <= 1e-5, (kind, which)


def test_skewed_matrices_are_skewed():
    s = OC.scene(2, 24, 40, "front", True)
    assert float(s.K[:, :3, 3].abs().min()) > 0 and not torch.equal(s.T[0, 3], torch.tensor([0.0, 0.0, 0.0, 1.0]))
    assert float(OC.camera_z(s).min()) >= 5e-2
    assert float(OC.project_ref(2, 24, 40, "front", True, "both", True).g64[1][:, 3].abs().min()) > 0      # the last row of g_T is live


@pytest.mark.parametrize("shape", OC.SSIM_EDGE_SHAPES + OC.SSIM_SHAPES, ids=str)
def test_ssim_cases_are_well_conditioned(shape):
    kinds = OC.SSIM_KINDS if shape in OC.SSIM_SHAPES else ("random",)
    for kind in kinds:
        r = OC.ssim_ref(shape, kind)
        if kind in OC.SSIM_DEGENERATE:
            # the point of the two kinds: the gradient is (nearly) nothing but rounding next to the random case's
            assert float(r.g64[0].norm()) <= 1e-2 * r.scale[0] and float(r.g64[1].norm()) <= 1e-2 * r.scale[1], kind
            assert float((r.out32[0] - r.out64[0]).abs().max()) <= 5e-4
            if kind == "near":       # the value sits below the rounding of n/d in fp32: the clamp's decisions are rounding's
                assert float(r.out64[0].max()) <= 1e-5 and float(r.out64[0].median()) <= 2.0 ** -24
            continue
        assert float((r.out32[0] - r.out64[0]).abs().max()) <= 5e-4, kind
        assert rel(r.g32[0], r.g64[0]) <= 1e-3 and rel(r.g32[1], r.g64[1]) <= 1e-3, (kind, rel(r.g32[0], r.g64[0]))
        v = r.out64[0]
        # no pixel where a value error of 4 x the cap above could move the clamp's decision
        assert float(v.min()) > 2e-3 and float(v.max()) < 1 - 2e-3, (kind, float(v.min()), float(v.max()))
        if kind == "flat":       # the cancellation is there: the fp32 oracle loses 20 x what it loses on random images
            assert float((r.out32[0] - r.out64[0]).abs().max()) >= 5e-5


def test_sizes_reach_the_loop_trips():
    B, h, w = OC.GEOM_SHAPES[-1]
    assert (h * w + PIXELS_PER_BLOCK - 1) // PIXELS_PER_BLOCK > PARTIALS_PER_TRIP
    assert all((hh * ww + PIXELS_PER_BLOCK - 1) // PIXELS_PER_BLOCK <= PARTIALS_PER_TRIP for _, hh, ww in OC.GEOM_SHAPES[:-1])
    assert OC.DISP_SIZES[-1] > D2D_MAX_BLOCKS * D2D_BLOCK and all(n <= D2D_MAX_BLOCKS * D2D_BLOCK for n in OC.DISP_SIZES[:-1])
    assert OC.CHAIN_SHAPE == OC.GEOM_SHAPES[-1]
    for n in OC.DISP_SIZES:
        d = OC.disp_ref(n).args[0]
        assert float(d[0]) == 0.0 and (n < 3 or float(d[1]) == 1.0) and (n < 3 or float(d[2:].min()) >= 1e-3)


def test_chain_band_is_small():
    r = OC.chain_ref()
    assert float(r.band.double().mean()) <= 1e-2
    for g32, g64 in zip(r.g32, r.g64):
        assert rel(g32, g64) <= 1e-3, rel(g32, g64)
