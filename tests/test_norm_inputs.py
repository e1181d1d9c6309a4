"""The inputs of tests/test_norm_parity_gpu.py are fair and its bounds mean something, asserted from the references alone (no GPU, no
kernel): the fp32 CPU reference meets the criterion of tests/norm_case.py by itself with rho_32 <= F (the bound in force on the GPU is
F * scale_i), the named shapes reach the paths they name, and a plain-torch model of BatchNorm statistics from raw fp32 sums -- what
csrc/dd_bn.hip computed before its sums went to fp64 -- breaks the output bound and the running_var bound on every off-centre case."""
import pytest
import torch

import norm_case as NC

F32 = torch.float32


def _meets(name, w64, w32, scale, fl, band=None):
    assert bool(torch.isfinite(w64).all()) and bool(torch.isfinite(scale).all()), name
    assert bool((scale >= w64.abs() * (1 - 1e-9)).all()), name                          # the sum of absolute terms bounds the sum
    rho = NC.rho32(w64, w32, scale, band)
    assert rho <= fl, (name, rho, fl)


def _within(name, w64, w32, bound):
    e = (w32.double() - w64).abs()
    assert bool((e <= bound).all()), (name, float((e / bound.clamp_min(1e-300)).max()))


# ---- BatchNorm ---------------------------------------------------------------------------------------------------------------------
def _bn_dtypes(ci):
    return NC.DTYPES if ci in NC.BN_HALF_CASES else (F32,)


@pytest.mark.parametrize("ci", range(len(NC.BN_CASES)), ids=NC.BN_CASE_IDS)
def test_batch_norm_fp32_reference_meets_the_criterion(ci):
    c = NC.BN_CASES[ci]
    for dtype in _bn_dtypes(ci):
        for act, with_res in c.combos:
            for groups in c.groups:
                r = NC.bn_ref(ci, dtype, act, with_res, groups)
                tag = (c.name, NC.dtype_name(dtype), act, with_res, groups)
                _meets(tag + ("out",), r.out64, r.out32, r.s_out, r.fl_out)
                _meets(tag + ("g_x",), r.g64[0], r.g32[0], r.s_gx, r.fl_gx, r.band_gx)
                if with_res:
                    _meets(tag + ("g_res",), r.g64[3], r.g32[3], r.s_gp, r.fl_gp, r.band_gp)
                _within(tag + ("g_w",), r.g64[1], r.g32[1], r.b_gw)
                _within(tag + ("g_b",), r.g64[2], r.g32[2], r.b_gb)
                # (the running statistics are held to float64 relative to the variance itself, which the fp32 reference, whose mean is
                # an fp32 number, does not meet off-centre; exact statistics through the kernel's fp32 update do: the last test of this group)
                # the bands are the exception: under 2 % of the elements
                assert float((r.band_gp > 0).double().mean()) < 0.02, tag
                if dtype != F32:
                    assert float(r.x.float().abs().max()) < 400.0 and float(r.out64.abs().max()) < 6.0e4 and float(r.g64[0].abs().max()) < 6.0e4


@pytest.mark.parametrize("ci", range(len(NC.BN_CASES)), ids=NC.BN_CASE_IDS)
def test_batch_norm_channels_are_what_the_cases_say(ci):
    c = NC.BN_CASES[ci]
    B, C, H, W = c.shape
    r = NC.bn_ref(ci, F32, None, False, 1)
    mean, sd = r.mean[0], r.var[0].sqrt()
    kinds = NC.bn_channel_kinds(C, F32)
    assert any(NC.bn_ratio(k) >= 100 for k in kinds) and (C < 12 or set(kinds) == set(NC.BN_KINDS))
    for ch, k in enumerate(kinds):
        if k == "const":
            assert float(r.var[0][ch]) == 0.0 and float(mean[ch]) == 3.0
        elif not c.outlier and r.rows >= 100:
            want = 1000.0 if k == "small" else abs(k)
            assert 0.7 * want - 0.3 <= abs(float(mean[ch] / sd[ch])) <= 1.4 * want + 0.3, (ch, k, float(mean[ch] / sd[ch]))
        if c.outlier and k != "const":          # row 0 sits ~1000 sigma (of the other rows) from their mean
            rest = r.x.double()[:, ch].flatten()[1:]
            assert abs(float((r.x.double()[0, ch, 0, 0] - rest.mean()) / rest.std())) > 500.0


def test_batch_norm_shapes_reach_the_paths_they_name():
    plan = {c.name: NC.bn_plan(c.shape[0] * c.shape[2] * c.shape[3], c.shape[1]) for c in NC.BN_CASES}
    rows = {c.name: c.shape[0] * c.shape[2] * c.shape[3] for c in NC.BN_CASES}
    assert rows["1x8x1x2"] == 2
    assert plan["1x4x3x5"][0] == 1024 and plan["1x12x5x7"][0] * 3 == 1023 and plan["1x508x3x5"][0] * 127 == 1016
    assert rows["2x8x12x20"] < plan["2x8x12x20"][0] and plan["2x8x12x20"][1] == 1
    assert plan["2x48x9x11"][0] == 85 and plan["2x80x7x9"][0] == 51 and 1024 % 12 and 1024 % 20
    lanes, chunks, per, blocks, per_block = plan["3x64x24x40"]
    assert chunks == 6 and rows["3x64x24x40"] % per == 0 and per % lanes != 0          # every chunk ends on a partial trip of the lanes
    lanes, chunks, per, blocks, per_block = plan["2x512x96x96"]
    assert rows["2x512x96x96"] == 18432 and -(-18432 // (lanes * 8)) == 288 > NC.BN_MAX_CHUNKS == chunks and per == 72 and blocks == 288
    assert 2 * 512 * 96 * 96 * 4 < 40e6
    assert all(NC.bn_depth(rows[c.name], c.shape[1]) <= 12 for c in NC.BN_CASES)
    combos = {cb for c in NC.BN_CASES for cb in c.combos}
    assert combos == set(NC.BN_COMBOS) and any(2 in c.groups for c in NC.BN_CASES) and len(NC.BN_HALF_CASES) == 3


@pytest.mark.parametrize("ci", range(len(NC.BN_CASES)), ids=NC.BN_CASE_IDS)
def test_raw_fp32_sums_break_the_bounds_on_every_off_centre_case(ci):
    """fp32 sum x and sum x^2, var = s2 / n - mean^2: over the output bound and over the running_var bound wherever mean / sigma >= 100
    -- every case has such channels.  The same arithmetic with exact sums (float64 throughout) is inside both."""
    c = NC.BN_CASES[ci]
    B, C, H, W = c.shape
    r = NC.bn_ref(ci, F32, None, False, 1)
    off = torch.tensor([NC.bn_ratio(k) >= 100 for k in NC.bn_channel_kinds(C, F32)])
    assert bool(off.any())
    rows2d = r.x.permute(0, 2, 3, 1).reshape(r.rows, C)
    bound_out = NC.elem_bound(r.out64, r.out32, r.s_out, r.fl_out, F32)

    def over(model):
        out, rv = NC.bn_model_outputs(r, *model)
        return bool(((out - r.out64).abs() > bound_out)[:, off].any()), bool(((rv - r.rv64).abs() > r.b_rv)[off].any())
    assert over((r.mean[0], r.var[0])) == (False, False), c.name
    if c.outlier:
        # the outlier is part of the batch: it widens the true variance ((1000 sigma)^2 / rows on top of sigma^2) and the channels are no
        # longer 100 sigma off; what must not pass here is the shift taken from row 0: over the running_var bound
        assert over(NC.bn_first_row_shift_model(rows2d, r.rows, C))[1], c.name
    else:
        assert over(NC.bn_raw_sums_model(rows2d, r.rows, C)) == (True, True), c.name


def test_batch_norm_grid_case_puts_a_fifth_of_the_pre_activations_at_zero():
    x, w, b, g, offs = NC.bn_grid_case()
    assert torch.equal(x.mean((0, 2, 3)), offs) and bool((b == 0).all())
    at_mean = (x == offs.view(1, -1, 1, 1))
    assert int(at_mean.sum()) * 5 == x.numel() and bool(at_mean.flatten(2).any(2).all())


# ---- LayerNorm ---------------------------------------------------------------------------------------------------------------------
def _ln_check(rows, C, kind, dtype):
    r = NC.ln_ref(rows, C, kind, dtype)
    tag = (rows, C, kind, NC.dtype_name(dtype))
    _meets(tag + ("y",), r.y64, r.y32, r.s_y, NC.floor("ln y"))
    _meets(tag + ("g_x",), r.g64[0], r.g32[0], r.s_gx, NC.floor("ln g_x"))
    _within(tag + ("g_w",), r.g64[1], r.g32[1], r.b_gw)
    _within(tag + ("g_b",), r.g64[2], r.g32[2], r.b_gb)
    if dtype != F32:
        assert float(r.y64.abs().max()) < 6.0e4 and float(r.g64[0].abs().max()) < 6.0e4


@pytest.mark.parametrize("C", NC.LN_WIDTHS)
def test_layer_norm_fp32_reference_meets_the_criterion(C):
    for rows in NC.ln_row_counts(C):
        for kind in NC.LN_KINDS:
            for dtype in (NC.DTYPES if C in NC.LN_HALF_WIDTHS else (F32,)):
                _ln_check(rows, C, kind, dtype)


@pytest.mark.parametrize("C,rows", NC.LN_CAPPED)
def test_layer_norm_capped_reference_meets_the_criterion(C, rows):
    _ln_check(rows, C, "mixed", F32)
    assert -(-rows // (NC.ln_rpb(C) * NC.LN_ROWS_PER_THREAD)) > NC.LN_MAX_BLOCKS == NC.ln_blocks(rows, C)
    assert rows * C * 4 < 40e6


def test_layer_norm_shapes_and_rows_are_what_the_cases_say():
    assert [NC.ln_lp(C) for C in NC.LN_WIDTHS] == [16, 16, 16, 32, 32, 32, 64, 64, 64]          # both sides of the boundaries at 64 and 128
    assert [NC.ln_rpb(C) for C in (4, 68, 132)] == [16, 8, 4]
    for C in NC.LN_WIDTHS:
        assert NC.ln_row_counts(C)[1] + 2 == NC.ln_row_counts(C)[2] and NC.ln_blocks(1000, C) > 1
    x = NC.ln_ref(1000, 64, "mixed", F32).x.double()
    ratio = (x.mean(1).abs() / x.std(1)).view(-1, 4)
    assert bool((ratio[:, 0] < 1).all()) and bool((ratio[:, 1:3] > 500).all()) and bool((ratio[:, 3] > 5000).all())
    x = NC.ln_ref(1000, 64, "const", F32).x.double()
    assert bool((x.std(1) < 2e-4 * x.mean(1).abs()).all())
    assert bool((NC.ln_ref(1000, 64, "off", F32).x.double().mean(1).abs() > 400).all())


# ---- layer-scale residual ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,hw,C", NC.LS_CASES, ids=str)
def test_layer_scale_fp32_reference_meets_the_criterion(B, hw, C):
    for dtype in NC.DTYPES:
        r = NC.ls_ref(B, hw, C, dtype)
        _meets("out", r.out64, r.out32, r.s_out, NC.floor("ls out"))
        _meets("g_y", r.g64[1], r.g32[1], r.s_gy, NC.floor("ls g_y"))
        _within("g_scale", r.g64[2], r.g32[2], r.b_gs)
        assert torch.equal(r.g64[0], r.g.double())
        assert 5e-7 < float(r.scale.abs().max()) < 3e-6
        if r.dropped is not None:
            assert bool((r.scale[r.dropped] == 0).all()) and bool((r.g64[1][r.dropped] == 0).all()) and bool((r.g64[2][r.dropped] != 0).any())


def test_layer_scale_shapes_reach_the_chunk_cap():
    lanes, chunks, per = NC.ls_plan(23 * 23, 1024)          # 67 chunks of eight rows wanted, 64 allowed: nine rows each, 59 chunks
    assert lanes == 1 and -(-23 * 23 // 8) > NC.LS_MAX_CHUNKS >= chunks == 59 and per == 9
    assert NC.ls_plan(23 * 23, 4)[0] == 256 and NC.ls_plan(23 * 23, 252)[0] == 4 and NC.ls_plan(1, 252)[1] == 1


# ---- depth-wise convolution --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", range(len(NC.DW_CASES)), ids=NC.DW_CASE_IDS)
def test_depthwise_conv_fp32_reference_meets_the_criterion(ci):
    for dtype in (NC.DTYPES if ci in NC.DW_HALF_CASES else (F32,)):
        r = NC.dw_ref(ci, dtype)
        _meets("y", r.y64, r.y32, r.s_y, NC.floor("dw out"))
        _meets("g_x", r.g64[0], r.g32[0], r.s_gx, NC.floor("dw g_x"))
        _within("g_w", r.g64[1], r.g32[1], r.b_gw)
    c = NC.DW_CASES[ci]
    if c.dil >= c.H and c.dil >= c.W:          # only the centre tap is in the image: the other eight weight gradients are exactly 0
        gw = NC.dw_ref(ci, F32).g64[1].view(c.C, 9)
        assert bool((gw[:, [0, 1, 2, 3, 5, 6, 7, 8]] == 0).all()) and bool((gw[:, 4] != 0).all())


def test_depthwise_conv_cases_cover_what_is_asked():
    cs = NC.DW_CASES
    assert {c.H for c in cs} == {1, 2, 3, 5, 6, 7} and {c.C for c in cs} == {4, 12, 36, 508, 512} and {c.dil for c in cs} == {1, 2, 3, 5, 6}
    assert {c.W * c.C // 4 for c in cs} >= {255, 256, 257, 258} and {(c.C, c.W) for c in cs} >= {(4, 255), (4, 256), (4, 257), (12, 85), (12, 86)}
    assert {c.B for c in cs} == {1, 3} and any(c.B * c.H < 8 for c in cs) and any(c.B * c.H > 8 and c.B * c.H % 8 for c in cs)
    assert any(c.dil >= c.H and c.dil >= c.W for c in cs) and any(c.dil >= c.H and c.dil < c.W for c in cs) and any(c.dil >= c.W and c.dil < c.H for c in cs)
    assert all(cs[i].H % NC.DW_ROWS for i in NC.DW_GUARD_CASES) and len(NC.DW_HALF_CASES) == 3
