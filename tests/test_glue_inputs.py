"""The inputs of tests/test_glue_parity_gpu.py are fair, asserted from the references alone (no GPU, no kernel): the fp32 CPU reference
meets the criterion of tests/glue_case.py by itself, the special values are where the cases say, the named shapes put their boundaries
where the cases say, and the channel-sum bound of the two capped shapes is small enough to mean something."""
import pytest
import torch

import glue_case as GC

DEC_NT = PAD_NT = 256          # workgroup sizes of up_cat_pad_kernel and reflect_pad1_nhwc_kernel, stated here and not imported


@pytest.mark.parametrize("dtype", GC.DTYPES, ids=GC.dtype_name)
@pytest.mark.parametrize("ci", range(len(GC.CASES)), ids=GC.CASE_IDS)
def test_fp32_reference_meets_the_criterion(ci, dtype):
    """with 4 x replaced by 1 x; and more: rho_32 <= F, so the bound in force on the GPU is F * scale_i, not the fp32 reference's error"""
    r = GC.glue_ref(ci, dtype)
    c = r.case
    rows = [("out", r.out64, r.out32, r.s_out, GC.out_kind(c)), ("g_x", r.gx64, r.gx32, r.s_gx, GC.gx_kind(c))]
    if c.C2:
        rows.append(("g_skip", r.gs64, r.gs32, r.s_gs, "g_skip"))
    for name, w64, w32, scale, kind in rows:
        assert bool(torch.isfinite(w64).all()) and bool(torch.isfinite(scale).all()), name
        assert bool((scale >= w64.abs() * (1 - 1e-12)).all()), name                  # the sum of absolute terms bounds the sum
        bound = GC.elem_bound(w64, w32, scale, kind, torch.float32, factor=1.0)
        assert bool(((w32 - w64).abs() <= bound).all()), name
        assert GC.rho32(w64, w32, scale) <= GC.floor_factor(kind), (name, GC.rho32(w64, w32, scale))
    if dtype != torch.float32:           # nothing a half type cannot hold: the half-type runs see finite inputs and finite references
        assert float(r.out64.abs().max()) < 6.0e4 and float(r.gx64.abs().max()) < 6.0e4


@pytest.mark.parametrize("shape", GC.PAD_CASES, ids=str)
def test_reflect_pad_reference_meets_the_criterion(shape):
    for dtype in GC.DTYPES:
        r = GC.pad_ref(*shape, dtype)
        assert GC.rho32(r.gx64, r.gx32, r.s_gx) <= GC.floor_factor("pad g_x")
        assert bool((r.s_gx >= r.gx64.abs() * (1 - 1e-12)).all())


def test_elu_edges_are_present():
    for ci, c in enumerate(GC.CASES):
        if c.xkind == "edges":
            x = GC.glue_ref(ci, torch.float32).x
            for v in GC.ELU_EDGES:
                hit = (x == v) & (torch.signbit(x) == torch.signbit(torch.tensor(v)))
                assert int(hit.sum()) >= 2, (c.name, v)
            small = (x > -0.05) & (x < 0) & (x.abs() > 1e-30)
            assert int(small.sum()) >= c.B * c.C1 * c.w - 2
            for dtype in (torch.float16, torch.bfloat16):             # the half types keep what they can represent
                xh = GC.glue_ref(ci, dtype).x.float()
                for v in (0.0, -20.0, -104.0, 50.0) + ((GC.FP32_MIN_NORMAL, -GC.FP32_MIN_NORMAL) if dtype == torch.bfloat16 else ()):
                    assert int((xh == v).sum()) >= 2, (c.name, dtype, v)
                assert int(((xh == 0) & torch.signbit(xh)).sum()) >= 2
        if c.xkind == "small_neg":
            for dtype in GC.DTYPES:
                x = GC.glue_ref(ci, dtype).x.float()
                assert float(x.min()) >= -0.05 and float(x.max()) <= 0.0
                assert float(GC.glue_ref(ci, dtype).s_out.max()) <= 0.05           # the scale is small everywhere
    assert sum(c.xkind == "edges" for c in GC.CASES) == 3 and sum(c.xkind == "small_neg" for c in GC.CASES) >= 1


def test_tiny_values_never_stand_alone():
    """every output of the ELU-edge cases has a tap of ordinary size: its scale is far above the subnormal range"""
    for ci, c in enumerate(GC.CASES):
        if c.xkind == "edges":
            for dtype in GC.DTYPES:
                r = GC.glue_ref(ci, dtype)
                if c.mode == 1:
                    assert float(r.s_out[:, :c.C1].min()) >= 1e-12, (c.name, dtype)


def test_ramp_taps_nearly_cancel():
    ci = GC.CASE_IDS.index("ramp")
    r = GC.glue_ref(ci, torch.float32)
    assert float((r.gx64.abs() / r.s_gx).median()) <= 0.05            # what an element gathers is a twentieth of its absolute terms
    assert float(r.x.min()) > 1.0                                      # ELU is the identity on it


def test_named_shapes_put_their_boundaries_where_they_say():
    by = {c.name: c for c in GC.CASES}
    c = by["row-258"]
    Wp, Cq = GC.dims(c)[1] + 2, (c.C1 + c.C2) // 4
    assert Wp * Cq == 258 and DEC_NT < Wp * Cq < 2 * DEC_NT
    assert (DEC_NT - 1) // Cq == DEC_NT // Cq == 85 and (DEC_NT - 1) % Cq == 0 and DEC_NT % Cq == 1         # threads 255 | 256 share pixel 85
    c = by["row-260"]
    Wp, Cq = GC.dims(c)[1] + 2, (c.C1 + c.C2) // 4
    assert Wp * Cq == 260 and (DEC_NT - 1) // Cq == DEC_NT // Cq == 51 and DEC_NT % Cq == 1
    assert sorted({(c.C1 + c.C2) // 4 for c in GC.CASES if c.name.startswith("channels-")}) == [1, 3, 5, 7]
    assert any(c.C2 > c.C1 for c in GC.CASES) and any(0 < c.C2 < c.C1 for c in GC.CASES) and any(c.C2 == 0 for c in GC.CASES)
    assert any(c.B == 3 for c in GC.CASES)
    H, W, C = GC.PAD_CASES[-1]
    assert (W + 2) * C == 257 == PAD_NT + 1


def test_channel_sum_shapes_reach_the_caps():
    C, rows = GC.CS_CAPPED_NARROW
    assert -(-rows * C // (GC.CS_NT * 8)) == 2110 and GC.channel_sum_launch(rows, C)[0] == GC.CS_MAX_BLOCKS
    stride = GC.channel_sum_launch(rows, C)[1]
    assert stride % C == 0 and stride <= GC.CS_MAX_BLOCKS * GC.CS_NT < stride + C
    C, rows = GC.CS_CAPPED_WIDE
    chunks, per = GC.channel_sum_launch(rows, C)
    assert (chunks, per) == (GC.CS_MAX_BLOCKS, 33) and 2000 * per < rows <= 2001 * per          # chunks 2001 .. 2047 start past the end
    for C, rows in (GC.CS_CAPPED_NARROW, GC.CS_CAPPED_WIDE):
        assert GC.channel_sum_depth(rows, C) < 128, GC.channel_sum_depth(rows, C)
    # no other shape reaches a cap, and every depth is at least the fold kernel's own
    for Cs, Rs in ((GC.CS_NARROW_C, GC.CS_NARROW_ROWS), (GC.CS_WIDE_C, GC.CS_WIDE_ROWS)):
        for C in Cs:
            for rows in Rs:
                assert GC.channel_sum_launch(rows, C)[0] < GC.CS_MAX_BLOCKS
                assert 10 <= GC.channel_sum_depth(rows, C) < 300


@pytest.mark.parametrize("C,rows", [(9, 4099), (256, 257), (300, 4097)])
def test_fp32_sum_meets_the_channel_sum_bound(C, rows):
    for mean in GC.CS_MEANS:
        for dtype in GC.DTYPES:
            want, ref32, bound = GC.channel_sum_bound(GC.channel_sum_input(rows, C, mean, dtype), rows, C)
            assert bool(((ref32.double() - want).abs() <= bound).all())
