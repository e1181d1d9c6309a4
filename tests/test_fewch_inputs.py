"""The inputs of tests/test_fewch_parity_gpu.py are fair and its bounds mean something, asserted from the references alone (no GPU, no
kernel): the fp32 CPU reference meets the element-wise criterion of tests/fewch_case.py by itself with rho_32 <= F (the bound in force
on the GPU is between F * scale_i and 4 F * scale_i, F from nothing but the source's rounding count), the integer cases are exact in fp32 in any order,
every shape list reaches the tile, workgroup and partial counts it names, the supported set restated from DD_CS_PAIRS is the 18
triples, the depth helpers are monotone and equal a hand count, and the GPU module runs every case the case module generates."""
import pytest
import torch

import fewch_case as FC


def _meets(name, w64, w32, scale, fl):
    assert bool(torch.isfinite(w64).all()) and bool(torch.isfinite(scale).all()), name
    assert bool((scale >= w64.abs() * (1 - 1e-9)).all()), name                          # the sum of absolute terms bounds the sum
    rho = FC.rho32(w64, w32, scale)
    assert rho <= fl, (name, rho / FC.U, fl / FC.U)
    return rho


def _check_ref(name, r, with_y=True):
    """one reference of any family: off-centre / zero-centred -> rho_32 <= F; integers -> every sum of absolute terms below 2^24"""
    if r.exact:
        assert all(s < FC.EXACT_LIMIT for s in r.exact_sums), (name, r.exact_sums)
        for t in (r.y, r.g_x, r.g_w, r.g_b):
            assert bool((t == t.round()).all()) and float(t.abs().max()) < FC.EXACT_LIMIT, name
        return
    if with_y:
        _meets((name, "y"), r.y, r.y_32, r.s_y, r.fl_y)
        _meets((name, "y no bias"), r.y0, r.y0_32, r.s_y0, r.fl_y)
    _meets((name, "g_x"), r.g_x, r.g_x32, r.s_gx, r.fl_gx)
    assert bool((r.t_gw >= r.g_w.abs() * (1 - 1e-9)).all()) and bool((r.t_gb >= r.g_b.abs() * (1 - 1e-9)).all()), name
    if r.kind == "off":          # what "off-centre" means: the sum is most of its absolute terms (cancellation does not hide an order)
        assert float(r.x.min()) >= 1.0, name
        if r.g.numel() // r.g.shape[1] >= 100:
            assert float((r.g_w.abs() / r.t_gw).min()) > 0.5, name


# ---- every reference ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", range(len(FC.CS_CASES)), ids=FC.CS_CASE_IDS)
def test_small_conv_references(ci):
    c = FC.CS_CASES[ci]
    assert FC.cs_supported(c.ks, c.cin, c.cout) and "off" in c.kinds and "int" in c.kinds
    for kind in c.kinds:
        r = FC.cs_ref(ci, kind)
        _check_ref((FC.CS_CASE_IDS[ci], kind), r)
        assert r.fl_y == max(c.ks * c.ks * c.cin, 16) * FC.U and r.fl_gx == max(c.ks * c.ks * c.cout, 16) * FC.U


@pytest.mark.parametrize("ci", range(len(FC.CH_CASES)), ids=FC.CH_CASE_IDS)
def test_disparity_head_references(ci):
    c = FC.CH_CASES[ci]
    assert "off" in c.kinds and "int" in c.kinds
    for kind in c.kinds:
        r = FC.ch_ref(ci, kind)
        _check_ref((FC.CH_CASE_IDS[ci], kind), r)
        assert r.fl_y == {32: 17, 64: 18}[c.C] * FC.U and r.fl_gx == 16 * FC.U


@pytest.mark.parametrize("ci", range(len(FC.C1_CASES)), ids=FC.C1_CASE_IDS)
def test_one_channel_data_gradient_references(ci):
    c = FC.C1_CASES[ci]
    assert "off" in c.kinds and "int" in c.kinds
    for kind in c.kinds:
        _check_ref((FC.C1_CASE_IDS[ci], kind), FC.c1_ref(ci, kind), with_y=False)


@pytest.mark.parametrize("ci", range(len(FC.RD_CASES)), ids=FC.RD_CASE_IDS)
def test_reduction_references(ci):
    c = FC.RD_CASES[ci]
    assert "off" in c.kinds and "int" in c.kinds
    for kind in c.kinds:
        r = FC.rd_ref(ci, kind)
        _check_ref((FC.RD_CASE_IDS[ci], kind), r)
        assert r.fl_y == {64: 16, 128: 16, 256: 16, 512: 19}[c.C] * FC.U and r.fl_gx == 16 * FC.U


def test_one_zero_centred_control_per_family():
    for cases in (FC.CS_CASES, FC.CH_CASES, FC.C1_CASES, FC.RD_CASES):
        assert sum("zero" in c.kinds for c in cases) == 1


# ---- the shapes reach what they name -----------------------------------------------------------------------------------------------
def test_supported_set_is_the_eighteen_triples():
    got = {(ks, ci, co) for ks in range(0, 6) for ci in range(0, 19) for co in range(0, 19) if FC.cs_supported(ks, ci, co)}
    assert len(got) == 18 and got == set(FC.CS_PAIRS) == set(FC.CS_TRIPLES)
    never_a_forward_before = {(3, 9, 12), (3, 9, 10), (3, 12, 16), (3, 12, 13), (1, 3, 9), (1, 1, 9), (1, 3, 12), (1, 1, 12)}
    assert never_a_forward_before <= got
    assert {FC.cs_mt(ks, ci) for ks, ci, _ in got} == set(FC.CS_MTS)
    assert [FC.cs_mt(t[0], t[1]) for t in FC.CS_MT_TRIPLES] == list(FC.CS_MTS)
    # the bias row: (3,16,12) first row of an M-tile of its own, (3,10,9) inside the last tile
    assert (9 * 16) % 16 == 0 and FC.cs_mt(3, 16) == 9 * 16 // 16 + 1 and (9 * 10) % 16 == 10 and FC.cs_mt(3, 10) == 9 * 10 // 16 + 1


def test_small_conv_shapes_reach_the_paths_they_name():
    for t in FC.CS_TRIPLES:
        assert {c[3:6] for c in FC.CS_CASES if c[:3] == t} >= set(FC.CS_EDGE_SHAPES)
    assert FC.CS_EDGE_SHAPES == ((1, 1, 1), (1, 3, 5), (1, 8, 32), (2, 9, 33), (1, 7, 31))
    for n, s in FC.CS_TILE_SHAPES.items():
        ntiles, blocks, busiest, idlest = FC.cs_plan(*s)
        assert ntiles == n and blocks == min(n, FC.CS_WG_BLOCKS)
        assert s[1] % FC.CS_TH or s[2] % FC.CS_TW                                      # ragged
    assert set(FC.CS_TILE_SHAPES) == {31, 32, 33, 96, 97, 98, 1024, 1025}
    for t in FC.CS_MT_TRIPLES:
        assert {FC.cs_plan(c.B, c.H, c.W)[0] for c in FC.CS_CASES if c[:3] == t} >= set(FC.CS_TILE_SHAPES)
    # slice 0 of conv_small_wgrad_fold1_kernel: the 4x-unrolled body runs once there are more than 96 partials
    assert [(n - 1) // FC.CS_FOLD + 1 for n in (31, 32, 33, 96, 97, 98)] == [1, 1, 2, 3, 4, 4] and 0 + 3 * FC.CS_FOLD < 97 and not 0 + 3 * FC.CS_FOLD < 96
    assert FC.cs_plan(*FC.CS_TILE_SHAPES[1024])[2:] == (1, 1) and FC.cs_plan(*FC.CS_TILE_SHAPES[1025])[2:] == (2, 1)
    plans = [FC.cs_plan(*s) for s in FC.CS_WALK_SHAPES]
    assert plans[0] == (1050, 1024, 2, 1) and plans[1][0] == 2100 and 2 * 1024 < plans[1][0] < 3 * 1024 and plans[1][2:] == (3, 2)
    assert (3, 16, 12) in FC.CS_MT_TRIPLES and (3, 10, 9) in FC.CS_MT_TRIPLES


def test_disparity_head_shapes_reach_the_paths_they_name():
    for C in FC.CH_CHANNELS:
        px = FC.ch_px(C)
        assert px == {32: 32, 64: 16}[C]
        mine = [c for c in FC.CH_CASES if c.C == C]
        assert {(c.Ho, c.Wo) for c in mine} >= {(ho, wo) for ho in (1, 7, 8, 9) for wo in (1, px - 1, px, px + 1)}
        assert {FC.ch_blocks(c.B, c.Ho, c.Wo, C) for c in mine} >= {1, 32, 33, 64, 65}
        for n, s in FC.CH_BLOCK_SHAPES[C].items():
            assert FC.ch_blocks(s[0], s[1], s[2], C) == n
        assert {c.B for c in mine} >= {1, 2}
    # conv_head_fold1_kernel, slice 0: the unrolled body once there are more than 32 partials, its second trip above 96
    assert [n > FC.CH_FOLD for n in (32, 33, 64, 65)] == [False, True, True, True] and 64 + FC.CH_FOLD > 65 and 64 < 65


def test_one_channel_data_gradient_shapes_reach_the_paths_they_name():
    for pad in (0, 1):
        mine = [c for c in FC.C1_CASES if c.pad == pad]
        assert {c.C for c in mine} == {4, 32, 64, 512}
        assert {c.Wi * c.C // 4 for c in mine if c.C == 4} == {255, 256, 257}
        assert any(c.Hi == 3 and c.Wi == 3 for c in mine)
        assert {FC.c1_blocks_x(c.Wi, c.C) for c in mine} >= {1, 2, 3}
    assert FC.C1_CASES[FC.C1_FUNCTION_CASE].pad == 1


def test_reduction_shapes_reach_the_paths_they_name():
    for C, (lpp, quads) in FC.RD_SHAPES.items():
        px = FC.rd_px(C)
        assert px * lpp == FC.RD_NT and lpp * quads * 4 == C
        for cout in FC.RD_COUTS:
            assert {c.P for c in FC.RD_CASES if (c.C, c.cout) == (C, cout)} >= {1, px - 1, px, px + 1, 8 * px, 8 * px + 1}
        assert FC.rd_plan(8 * px, C)[1] == 1 and FC.rd_plan(8 * px + 1, C)[1] == 2
    assert {FC.rd_plan(c.P, c.C)[1] for c in FC.RD_CASES} >= {1, 2, 32, 33, 64, 65, FC.RD_MAX_BLOCKS}
    for n, combos in FC.RD_BLOCK_CASES.items():
        assert len(combos) == 2
        for C, cout in combos:
            assert any(FC.rd_plan(c.P, c.C)[1] == n for c in FC.RD_CASES if (c.C, c.cout) == (C, cout))
    capped = [c for c in FC.RD_CASES if FC._ceil(FC.rd_plan(c.P, c.C)[0], FC.RD_GROUPS_PER_BLOCK) > FC.RD_MAX_BLOCKS]
    assert [(c.C, c.cout) for c in capped] == [(256, 3)] and FC.rd_plan(capped[0].P, 256) == (8193, 1024, 9, 8)
    assert 0 < capped[0].P - 8 * 1024 * 4 <= 8


def test_workspace_sizes_restate_the_size_functions():
    """(the GPU launchers assert these against dd_*_workspace_bytes)"""
    assert FC.cs_workspace_bytes(3, 12, 9) == 4096 + (1024 + 32) * 7 * 256 * 4          # 3 * 3 * 12 * 9 * 4 = 3888 bytes of packed weights, rounded up to 256
    assert FC.ch_workspace_bytes(1, 3, 3, 32) == (1 + 32) * 289 * 4
    assert FC.rd_workspace_bytes(1, 64, 3) == (1 + 32) * (3 * 128 + 3) * 4


# ---- the depths --------------------------------------------------------------------------------------------------------------------
def test_depth_helpers_are_monotone_and_equal_a_hand_count():
    # one tile: 16 matrix steps of four products, the four waves (2), one partial in slice 0 (1) and the tree of four accumulators (2),
    # eight slices per accumulator and its tree (8 + 2)
    assert FC.cs_depth(1, 1, 1) == 64 + 2 + (1 + 2) + (8 + 2)
    # 2100 tiles on 1024 workgroups: three tiles; 1024 partials: 32 per slice, eight per accumulator, at most three more in the tail
    assert FC.cs_depth(3, 2, 22369) == 3 * 64 + 2 + (8 + 3 + 2) + (8 + 2)
    # one workgroup of a C = 32 head on one pixel: one row, 32 pixels, one partial (1) and the sum of the two accumulators (1)
    assert FC.ch_depth(1, 1, 1, 32) == 1 + 32 + (1 + 1) + (8 + 2)
    # 65 workgroups of a C = 64 head, 33 rows: eight rows, 16 pixels, three partials in slice 0: at most two in one accumulator
    assert FC.ch_depth(1, 33, 193, 64) == 8 + 16 + (2 + 1) + (8 + 2)
    # a C = 256 reduction of one pixel: one group, four pixel lanes, one partial
    assert FC.rd_depth(1, 256) == 1 + 4 + (1 + 1) + (8 + 2)
    # above the cap: nine groups, four lanes, 1024 partials: 32 per slice, 16 per accumulator and one more in the tail at most
    assert FC.rd_depth(FC.RD_CAP_P, 256) == 9 + 4 + (16 + 1 + 1) + (8 + 2)

    def monotone(values):
        return all(a <= b for a, b in zip(values, values[1:]))
    assert monotone([FC.cs_depth(1, 1, w) for w in range(1, 32 * 2200, 31)])
    assert monotone([FC.cs_depth(b, 9, 33) for b in range(1, 700)]) and monotone([FC.cs_depth(2, h, 33) for h in range(1, 3000, 7)])
    for C in FC.CH_CHANNELS:
        assert monotone([FC.ch_depth(1, 1, w, C) for w in range(1, 4000, 3)]) and monotone([FC.ch_depth(2, h, 33, C) for h in range(1, 400)])
        assert monotone([FC.ch_depth(b, 9, 33, C) for b in range(1, 200)])
    for C in FC.RD_SHAPES:
        assert monotone([FC.rd_depth(p, C) for p in list(range(1, 3000)) + list(range(3000, 300000, 37))])
    # a depth never under-counts the walk of the busiest workgroup
    for p in (1, 63, 64, 65, 1000, 32768, 32769, 100000):
        assert FC.rd_depth(p, 256) >= FC.rd_plan(p, 256)[2] + FC.rd_px(256)


# ---- nothing is skipped or filtered out --------------------------------------------------------------------------------------------
def test_the_gpu_module_runs_every_case():
    import test_fewch_parity_gpu as T
    for params, cases, ids in ((T.CS_PARAMS, FC.CS_CASES, FC.CS_CASE_IDS), (T.CH_PARAMS, FC.CH_CASES, FC.CH_CASE_IDS),
                               (T.C1_PARAMS, FC.C1_CASES, FC.C1_CASE_IDS), (T.RD_PARAMS, FC.RD_CASES, FC.RD_CASE_IDS)):
        assert params == list(range(len(cases))) and len(set(ids)) == len(cases)
    assert len(FC.CS_CASES) == 18 * 5 + 5 * 8 + 2 and len(FC.CH_CASES) == 2 * (16 + 4) and len(FC.C1_CASES) == 16
    assert len(FC.RD_CASES) == 4 * 2 * 6 + 8 + 1
    names = {m.args[0] for f in (T.test_small_conv, T.test_disparity_head, T.test_one_channel_data_gradient, T.test_reduction)
             for m in f.pytestmark if m.name == "parametrize"}
    assert names == {"ci"}
    for table, ids in ((T.CS_FN, FC.CS_CASE_IDS), (T.CH_FN, FC.CH_CASE_IDS), (T.RD_FN, FC.RD_CASE_IDS)):
        assert all(p[0] in ids for p in table)
    assert not any(m.name in ("skip", "skipif", "xfail") for f in vars(T).values() if callable(f) for m in getattr(f, "pytestmark", []))
