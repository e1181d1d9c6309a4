"""The inputs of tests/test_input_parity_gpu.py are what that file claims, asserted from the references alone (no GPU, no kernel): a
quiet drift in tests/input_case.py cannot turn the GPU tests vacuous or ill-conditioned.

JPEG: the numpy oracle equals PIL on EVERY file of the case lists (the whole set decodes in well under half a minute here, so
nothing is thinned out), the host parser agrees with the oracle's parse, and the lists hold the files the device decoder's paths
need.  Jitter: float64 is a fair judge of every case and the branches of the hue shift are all taken.  Pyramid: the float64 tap
restatement is torch's."""
import numpy as np
import pytest
import torch

import input_case as IC
import oracle.ref_jpeg as rj

# the kernels' geometry, stated here and not imported from anywhere: compressed bytes staged per trip of jpeg_huffman_kernel, bits of
# its look-ahead table, pixels per trip of jitter_mean_kernel (32 workgroups of 256), pixels per workgroup of the other two kernels
JPEG_CHUNK, JPEG_LOOK, MEAN_TRIP, PIXELS_PER_BLOCK = 8192, 9, 8192, 256


# ---- JPEG ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(IC.jpeg_lists()))
def test_oracle_equals_pil_on_every_file(name):
    for f in IC.jpeg_lists()[name]:
        want = IC.pil_decode(f.data)
        got = rj.decode(f.data)
        assert got.shape == want.shape and np.array_equal(got, want), f.label


def test_case_lists_are_the_stated_matrices():
    lists = IC.jpeg_lists()
    assert len(lists["main"]) == 4 * 7 * 3 * 4 * 2 and len(lists["restart"]) == 2 * 3 * 3 * 2 * 3
    assert all(len(v) > 0 for v in lists.values()) and set(lists) == {"main", "restart", "restart_rows", "qtables", "grey", "meta"}
    labels = [f.label for f in IC.jpeg_files()]
    assert len(set(labels)) == len(labels)
    for (w, h) in IC.JPEG_SIZES:                                      # PIL kept the sampling it was asked for, down to 1x1
        for ss, hv in zip(IC.JPEG_SAMPLINGS, ((1, 1), (2, 1), (2, 2))):
            assert (w, h, 3, (hv[0], 1, 1), (hv[1], 1, 1)) in IC.jpeg_batches()
    assert sum(len(v) for v in IC.jpeg_batches().values()) == len(labels)
    assert set(IC.JPEG_GEOMETRIES) == set(IC.jpeg_batches()) and len(set(IC.JPEG_GEOMETRIES)) == len(IC.JPEG_GEOMETRIES)


def test_host_parser_matches_the_oracles_parse():
    from hipops import abi, jpeg
    for f in IC.jpeg_files():
        rec, geom = jpeg.parse_header(f.data)
        want = rj.JpegHeader(f.data)
        hd = abi.DDJpegHeader.from_buffer_copy(rec.tobytes())
        assert (hd.data_offset, hd.data_end, hd.restart_interval) == (want.data_offset, len(f.data), want.restart), f.label
        assert geom == IC.geometry(f.data), f.label
        for k, (_, h, v, tq) in enumerate(want.components):
            assert (hd.h[k], hd.v[k], hd.tq[k]) == (h, v, tq), f.label
            assert np.array_equal(np.array(hd.qt[tq]), want.qt[tq]), f.label
        for (tc, th), (bits, vals) in want.huff.items():
            assert list(hd.bits[2 * tc + th]) == bits and list(hd.vals[2 * tc + th])[:len(vals)] == vals, f.label


def test_every_batch_starts_with_two_different_table_sets():
    """a kernel that read hdrs[0] for every image fails on every geometry: images 0 and 1 differ in their quantisation tables,
    and a batch with optimised files holds more than one Huffman table set (the metadata batch: two data offsets) as well"""
    for geom, files in IC.jpeg_batches().items():
        assert len(files) >= 2, geom
        a, b = rj.JpegHeader(files[0].data), rj.JpegHeader(files[1].data)
        assert any(not np.array_equal(a.qt[k], b.qt[k]) for k in a.qt), geom
        hdrs = [rj.JpegHeader(f.data) for f in files]
        if any("opt1" in f.label for f in files):              # (the 96x64 batches hold restart files only: standard tables)
            assert len({repr(sorted(h.huff.items())) for h in hdrs}) >= 2, geom
        if geom[:2] == IC.META_SIZE:
            assert len({h.data_offset for h in hdrs}) == 2, geom


def _scan(f):
    return f.data[rj.JpegHeader(f.data).data_offset:]


def _restart_markers(f):
    s = np.frombuffer(_scan(f), np.uint8)
    return int(((s[:-1] == 0xFF) & (s[1:] >= 0xD0) & (s[1:] <= 0xD7)).sum())


def test_the_files_the_decoder_paths_need_exist():
    files = IC.jpeg_files()
    hdrs = {f.label: rj.JpegHeader(f.data) for f in files}
    assert any(len(f.data) > 3 * JPEG_CHUNK for f in files)                                  # several staging trips ...
    assert any(len(f.data) > 4 * JPEG_CHUNK and hdrs[f.label].restart for f in files)       # ... with restart markers among them
    assert any(b"\xff\x00" in _scan(f) for f in files)
    for marker in ("opt0", "opt1"):                     # codes behind the look-ahead table, in the standard and in optimised tables
        assert any(marker in f.label and any(any(bits[JPEG_LOOK:]) for bits, _ in hdrs[f.label].huff.values()) for f in files), marker
    assert any(any(int(q.max()) == 255 for q in hdrs[f.label].qt.values()) for f in files)
    assert any(all(int(q.min()) == 1 and int(q.max()) == 1 for q in hdrs[f.label].qt.values()) for f in files)
    assert any(hdrs[f.label].data_offset > 65535 for f in files)
    assert any(_restart_markers(f) > 100 for f in files)
    assert any(hdrs[f.label].width < 8 and hdrs[f.label].height < 8 for f in files)
    both = [f for f in files if all(IC.pil_decode(f.data)[..., c].min() == 0 and IC.pil_decode(f.data)[..., c].max() == 255 for c in range(3))]
    assert both and any("ss2" in f.label for f in both) and any("ss0" in f.label for f in both)
    # every restart interval that was asked for is in the file
    for f in IC.jpeg_lists()["restart"]:
        assert hdrs[f.label].restart == int(f.label.split("rst")[1].split()[0]), f.label
    for f in IC.jpeg_lists()["restart_rows"]:
        assert hdrs[f.label].restart > 0 and _restart_markers(f) > 0, f.label


# ---- jitter -------------------------------------------------------------------------------------------------------------------
def test_jitter_parameter_rows():
    ranges = IC.jitter_ranges()
    assert tuple(ranges) == ((0.8, 1.2), (0.8, 1.2), (0.8, 1.2), (-0.1, 0.1))                # what the loader draws from
    pool = IC.jitter_pool()
    assert len(set(pool)) == 24 and IC.IDENTITY in pool
    assert all(all(lo <= v <= hi for v, (lo, hi) in zip(row, ranges)) for row in pool)
    seen_rows, idle_flipped, idle_upright = set(), False, False
    for shape in IC.JITTER_CASES:
        B, F, H, W = shape
        case = IC.jitter_case(shape)
        assert case.frames.shape == (B, F, H, W, 3) and case.frames.dtype == torch.uint8 and case.params.shape == (B, F, 9)
        rows = [tuple(r.tolist()) for r in case.params.reshape(-1, 9)]
        assert len(set(r[1:] for r in rows)) == B * F                                        # every (b, f) row is distinct
        assert all(sorted(r[1:5]) == [0.0, 1.0, 2.0, 3.0] for r in rows)
        seen_rows |= {r[5:] for r in rows}
        if B > 1:
            assert set(case.flip.tolist()) == {0, 1}
        if B * F > 3:
            assert {r[0] for r in rows} == {0.0, 1.0}
        assert rows[0][0] == 1.0
        for b in range(B):
            idle = bool((case.params[b, :, 0] < 0.5).any())
            idle_flipped |= idle and bool(case.flip[b])
            idle_upright |= idle and not bool(case.flip[b])
    assert idle_flipped and idle_upright
    f32 = lambda row: tuple(torch.tensor(row, dtype=torch.float32).tolist())
    assert all(f32(row) in seen_rows for row in pool)                                         # corners, identity and draws all used
    B, F, H, W = IC.JITTER_CASES[2]
    assert W % 2 == 1 and {tuple(int(x) for x in r[1:5]) for r in IC.jitter_case(IC.JITTER_CASES[2]).params.reshape(-1, 9).tolist()} == set(IC.ORDERS)
    sizes = [h * w for _, _, h, w in IC.JITTER_CASES]
    assert any(MEAN_TRIP < n < 2 * MEAN_TRIP and n % MEAN_TRIP % PIXELS_PER_BLOCK for n in sizes)      # a full trip and a ragged second one
    assert any(n % PIXELS_PER_BLOCK == 0 for n in sizes) and any(n < 64 for n in sizes)
    # every generator is in every case that has room for it
    for shape in IC.JITTER_CASES[1:]:
        frames = IC.jitter_case(shape).frames.reshape(-1, *shape[2:], 3)
        if len(frames) >= 16:                                                                          # a whole frame black, one white: grey mean 0 and 1
            assert any(int(f.max()) == 0 for f in frames) and any(int(f.min()) == 255 for f in frames)
        flat = frames.reshape(-1, 3).int()
        assert bool((flat == 0).all(1).any()) and bool((flat == 255).all(1).any())                    # black, white
        assert bool(((flat.max(1).values - flat.min(1).values) == 1).any())                            # near-grey
        assert bool(((flat == torch.tensor([255, 0, 0])).all(1)).any())                                # a primary


@pytest.mark.parametrize("shape", IC.JITTER_CASES, ids=str)
def test_jitter_cases_are_well_conditioned(shape):
    """the float32 oracle within 5e-6 of float64 (the bar of test_prepare_frames_matches_oracle): no case sits on a branch decision
    that rounding could move by more"""
    ref = IC.jitter_ref(shape)
    e = float((ref.aug32.double() - ref.aug64).abs().max())
    print("jitter %s: float32 oracle against float64 %.2e" % (shape, e))
    assert e <= 5e-6, e
    idle = ~ref.applied
    assert torch.equal(ref.aug32[idle], ref.color[idle]) and torch.equal(ref.aug64[idle], ref.color[idle].double())
    assert float(ref.aug64.min()) >= 0.0 and float(ref.aug64.max()) <= 1.0


def test_jitter_cases_take_every_branch():
    sectors, below, above, greys, clamps = set(), False, False, False, False
    for shape in IC.JITTER_CASES:
        for bright_in, factor, h, hue, hue_in in IC.jitter_trace(shape):
            moved = h + hue
            sectors |= set(torch.floor((moved % 1.0) * 6.0).long().remainder(6).unique().tolist())
            below |= bool((moved < 0).any())
            above |= bool((moved >= 1).any())
            greys |= bool((hue_in.max(0).values == hue_in.min(0).values).any())
            clamps |= bool((factor * bright_in > 1.0).any())
    assert sectors == {0, 1, 2, 3, 4, 5}
    assert below and above and greys and clamps


# ---- pyramid ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", IC.PYRAMID_SHAPES)
def test_pyramid_restatement_is_torchs(H, W):
    for planes in IC.PYRAMID_PLANES:
        for kind in IC.PYRAMID_KINDS:
            x = IC.pyramid_input(H, W, planes, kind).double()
            got = IC.pyramid_ref(H, W, planes, kind)
            assert got.shape == (1, planes, H // 2, W // 2)
            if W // 2 >= 2:
                want = torch.nn.functional.interpolate(x, (H // 2, W // 2), mode="bicubic", align_corners=False, antialias=True).numpy()
            else:
                # torch's CPU antialiased bicubic is wrong at output width 1 (arange(8).reshape(1,1,4,2) -> (2,1) gives 1.6736 for
                # both rows): these shapes are judged by the restatement alone.  The same image turned by 90 degrees has output
                # HEIGHT 1, where torch is right, and the two 1-D passes commute: that call stands in.
                want = torch.nn.functional.interpolate(x.transpose(-1, -2), (W // 2, H // 2), mode="bicubic", align_corners=False, antialias=True)
                want = want.transpose(-1, -2).numpy()
            assert np.abs(got - want).max() <= 1e-12, (planes, kind, np.abs(got - want).max())
            if kind == "zero":
                assert not got.any()


def test_pyramid_edges_overshoot():
    """0/1 content leaves [0,1] before the clamp, on both sides: the kernel's clamp is live"""
    lo = min(IC.pyramid_ref(H, W, p, k).min() for (H, W, p, k) in IC.PYRAMID_CASES if k == "edges")
    hi = max(IC.pyramid_ref(H, W, p, k).max() for (H, W, p, k) in IC.PYRAMID_CASES if k == "edges")
    assert lo < -1e-3 and hi > 1 + 1e-3, (lo, hi)
    assert set(IC.PYRAMID_CASES) == {(H, W, p, k) for (H, W) in IC.PYRAMID_SHAPES for p in (1, 6) for k in ("uniform", "edges", "zero")}
    assert {2, 4, 6} <= {H for H, _ in IC.PYRAMID_SHAPES} and {2, 4, 6} <= {W for _, W in IC.PYRAMID_SHAPES}      # both ends of the tap set clipped at once
    assert any((H // 2) * (W // 2) > PIXELS_PER_BLOCK for H, W in IC.PYRAMID_SHAPES)                    # more than one workgroup
