"""The inputs of tests/test_metrics_parity_gpu.py are what tests/metrics_case.py claims, asserted from the oracle alone (no GPU, no
kernel): ATen's fp32 F.interpolate lies within the per-point bound in every case, the CPU restatement tools.DepthMetrics._forward_torch
passes the same judge, the edge values sit where the cases say, both clamps of dm_tap are hit, the keep rule's hand-placed points are kept
or dropped as written down, the medians have the structure claimed, and at most one point per threshold and sample is undecided."""
import numpy as np
import pytest
import torch

import metrics_case as MC

CI = range(len(MC.CASES))
NAMES = ["de:abs_rel", "de:sq_rel", "de:rms", "de:log_rms", "da:a1", "da:a2", "da:a3"]


@pytest.mark.parametrize("ci", CI, ids=MC.CASE_IDS)
def test_aten_fp32_lies_within_the_point_bound(ci):
    """|ATen fp32 - float64| <= bv, the bound of the interpolated disparity, and 1 / it within the bound of the predicted depth; the
    dyadic cases: ATen's fp32 equals the float64 value exactly"""
    c = MC.CASES[ci]
    for o in MC.oracle(ci):
        if o.n == 0:
            continue
        e = np.abs(o.aten32.astype(np.float64) - o.v64)
        assert bool((e <= o.bv).all()), (c.name, float((e / o.bv).max()))
        assert bool((np.abs(o.p_aten32.astype(np.float64) - o.p64) <= o.ep).all())
        assert bool((o.bv >= 16 * MC.U * o.v64).all())
        if c.dyadic:
            assert bool((e == 0).all()), c.name
        if c.exact:
            assert o.exact_ok, c.name


@pytest.mark.parametrize("ci", CI, ids=MC.CASE_IDS)
def test_at_most_one_undecided_point(ci):
    c = MC.CASES[ci]
    for o in MC.oracle(ci):
        if o.n == 0:
            continue
        assert max(o.all.und) <= (0 if c.exact else 1), (c.name, o.all.und)
        assert sum(s.n for s in o.by_label.values()) == (o.n if o.labels is not None else 0)
        for s in o.by_label.values():
            assert max(s.und) <= 1
        assert bool(np.isfinite(o.all.bound).all()) and bool((o.all.bound > 0).all())
        assert float(o.eps.max()) < 1e-3            # the bounds mean something: no metric may move by more than a part in a thousand


@pytest.mark.parametrize("ci", CI, ids=MC.CASE_IDS)
def test_cpu_restatement_passes_the_judge(ci):
    """tools.DepthMetrics._forward_torch, sample by sample (its result is the batch mean; alone, a sample's own row): the metrics and
    the per-label rows through Judge.sample / Judge.labels.  A sample without a kept point is left out: the restatement raises there,
    as the reference does.  Criterion 7 (the fp32 chain) is the kernel's alone: the restatement sums in fp32."""
    from tools import DepthMetrics
    c = MC.CASES[ci]
    dm = DepthMetrics(list(c.bound), c.min_depth, c.max_depth)
    j = MC.Judge(c, "_forward_torch (CPU)", fp32_chain=False)
    for b, o in enumerate(MC.oracle(ci)):
        if o.n == 0:
            continue
        inputs = {"depth_gt": c.lidar[b:b + 1], "depth_valid": c.valid[b:b + 1], "gt_dim": c.gt_dim[b:b + 1]}
        mask = None
        if c.mask is not None:            # the restatement indexes the mask with ground-truth pixels: pad a smaller one with label 0
            gh, gw = int(c.gt_dim[b, 0]), int(c.gt_dim[b, 1])
            mask = torch.zeros((1, gh, gw), dtype=torch.uint8)
            mask[0, :c.mask.shape[1], :c.mask.shape[2]] = c.mask[b, :gh, :gw]
        out = dm._forward_torch(inputs, {("disp_scaled", 0, 0): c.disp[b:b + 1]}, mask)
        row = np.asarray([float(out[m]) for m in NAMES] + [o.n], dtype=np.float32)
        j.sample(b, o, row)
        if mask is not None:
            rows = np.zeros((256, 8), dtype=np.float32)
            for l, (_, cnt) in out["de:abs_rel_mask"].items():
                if cnt:
                    rows[l] = [out[m + "_mask"][l][0] / cnt for m in NAMES] + [cnt]
            j.labels(b, o, rows)
    fails = j.finish()
    assert not fails, fails


def test_keep_rule_points_are_kept_as_written_down():
    c = MC.by_name("keep-rule")
    o = MC.oracle(MC.CASE_IDS.index("keep-rule"))[0]
    assert o.bounds_int == (28, 56, 28, 57)
    b32 = [int(np.float32(f) * np.float32(100)) for f in MC.KEEP_BOUND]
    assert b32 == [29, 57, 29, 58]                                   # what a float product would give
    want = np.asarray(c.want_keep, dtype=bool)
    assert np.array_equal(o.keep[:want.size], want)
    assert bool(o.keep[want.size:].all()) and o.n == int(want.sum()) + 40
    pts, valid = c.lidar[0].numpy(), c.valid[0].numpy()
    lo, hi = np.float32(c.min_depth), np.float32(c.max_depth)
    for z in (lo, np.nextafter(lo, np.float32(0)), np.nextafter(lo, np.float32(1)), hi, np.nextafter(hi, np.float32(0)), np.nextafter(hi, np.float32(100))):
        assert int((pts[:, 2] == z).sum()) == 1
    assert int(((valid == 0) & np.signbit(valid)).sum()) == 1 and {0.5, 2.0, -1.0} <= set(valid.tolist())
    rows = set(pts[:, 0].tolist())
    assert {27.0, 28.0, 29.0, 55.0, 56.0, 57.0, 27.75, 28.75, 55.5} <= rows
    assert {27.0, 28.0, 29.0, 56.0, 57.0, 58.0, 27.75, 28.75, 56.5} <= set(pts[:, 1].tolist())
    assert bool((pts[want.size:, 0] % 1 == 0.5).all()) and bool((pts[want.size:, 1] % 1 == 0.75).all())


def test_both_clamps_of_the_source_tap_are_hit():
    """src < 0 before the clamp (first row / column when up-scaling) and i0 = in - 1, where i1 = i0 (last row / column)"""
    for name in ("kitti-like", "dyadic-x2", "dyadic-x4", "two-gt-dims", "white-noise", "masked-labels"):
        c = MC.by_name(name)
        for b, o in enumerate(MC.oracle(MC.CASE_IDS.index(name))):
            if o.n == 0 or (name == "masked-labels" and b != 1):        # its sample 0 holds the first 1025 pixels only
                continue
            assert float(o.raw_y.min()) < 0 and float(o.raw_x.min()) < 0, name
            assert int(o.y0.max()) == c.H - 1 and int(o.x0.max()) == c.W - 1, name
            gh, gw = int(c.gt_dim[b, 0]), int(c.gt_dim[b, 1])
            assert {0, gh - 1} <= set(o.rows.tolist()) and {0, gw - 1} <= set(o.cols.tolist()), name
    for name in ("identity-7x9", "down-scale"):                                   # down-scaling: neither clamp is reached
        c = MC.by_name(name)
        o = MC.oracle(MC.CASE_IDS.index(name))[0]
        last = (name == "identity-7x9")
        assert float(o.raw_y.min()) >= 0 and (int(o.y0.max()) == c.H - 1) == last and (int(o.x0.max()) == c.W - 1) == last
        assert o.n == c.M == int(c.gt_dim[0, 0]) * int(c.gt_dim[0, 1])            # every ground-truth pixel
    o = MC.oracle(MC.CASE_IDS.index("identity-7x9"))[0]
    assert np.array_equal(o.raw_y, o.rows.astype(np.float64)) and np.array_equal(o.v64, o.aten32.astype(np.float64))


def test_geometry_shapes_are_the_ones_named():
    shapes = {c.name: (c.H, c.W, [tuple(d) for d in c.gt_dim.tolist()], c.M) for c in MC.CASES}
    assert shapes["identity-7x9"] == (7, 9, [(7, 9)], 63)
    assert shapes["dyadic-x2"][2][0] == (12, 10) and shapes["dyadic-x4"][2][0] == (12, 16)
    assert shapes["kitti-like"] == (12, 40, [(37, 123)] * 2, 1025)
    assert shapes["down-scale"][:3] == (50, 70, [(17, 23)])
    assert shapes["disp-1x1"][:2] == (1, 1) and shapes["disp-1x13"][:2] == (1, 13) and shapes["disp-13x1"][:2] == (13, 1)
    assert len(set(shapes["two-gt-dims"][2])) == 2
    assert shapes["white-noise"][3] == 1024
    assert sorted({c.M for c in MC.CASES} & {1, 63, 1024, 1025, 2500}) == [1, 63, 1024, 1025, 2500]
    for c in MC.CASES:
        assert c.B <= 5 and c.M <= 2500 and c.H <= 50 and c.W <= 70, c.name
        for d in ("dyadic-x2", "dyadic-x4"):
            if c.name == d:
                assert bool(((c.disp * 64) % 1 == 0).all())
    # smooth cases: the blend term leads the bound; the white-noise case: the coordinate term does somewhere
    for name in ("kitti-like", "down-scale", "two-gt-dims"):
        for o in MC.oracle(MC.CASE_IDS.index(name)):
            assert bool((o.coord_part <= 0.5 * o.blend_part).all()) and bool((o.bv <= 32 * MC.U * o.v64).all()), name
    o = MC.oracle(MC.CASE_IDS.index("white-noise"))[0]
    assert float((o.coord_part / o.blend_part).max()) > 1.0


def test_medians_have_the_structure_claimed():
    os_ = MC.oracle(MC.CASE_IDS.index("median-small-n"))
    assert [o.n for o in os_] == [2, 3, 8, 63, 10]
    assert MC.oracle(MC.CASE_IDS.index("median-M1"))[0].n == 1
    for o in os_[:3]:                                     # the upper median is another value, of both lists
        k = (o.n - 1) // 2
        assert np.sort(o.z)[k] < np.sort(o.z)[o.n // 2 if o.n % 2 == 0 else k + 1]
        assert np.sort(o.p64)[k] < np.sort(o.p64)[o.n // 2 if o.n % 2 == 0 else k + 1]
    for o in os_[:3] + os_[4:]:                           # kept among dropped
        assert 0 < o.n < 63 and int(o.idx.max()) >= o.n
    assert len(set(os_[3].z.tolist())) == 1 and len(set(os_[3].p64.tolist())) == 1
    z = np.sort(os_[4].z)
    assert z[3] < z[4] == z[5] == z[6] < z[7]              # duplicates on both sides of the middle (k = 4)
    # one byte of the bit pattern differs, the other three are the same in every point; duplicates, but the two middle values distinct
    for name, n in (("median-bytes", 1024), ("median-bytes-pd", 800)):
        c = MC.by_name(name)
        for byte, o in enumerate(MC.oracle(MC.CASE_IDS.index(name))):
            src = c.lidar[byte, :, 2].numpy() if name == "median-bytes" else o.v64.astype(np.float32)
            bits = np.ascontiguousarray(src).view(np.uint32)
            other = bits & ~np.uint32(0xFF << (8 * byte))
            vals = ((bits >> np.uint32(8 * byte)) & np.uint32(0xFF)).tolist()
            assert len(set(other.tolist())) == 1 and len(set(vals)) >= 6 and len(vals) > len(set(vals)), (name, byte)
            assert o.n == n == c.M and o.chain_ok
            k = (o.n - 1) // 2
            mid = np.sort(o.z if name == "median-bytes" else (np.float32(1) / o.v64.astype(np.float32)))
            assert mid[k] < mid[k + 1], (name, byte)
            other_side = o.v64 if name == "median-bytes" else o.z64
            assert len(set(other_side.tolist())) == 1                      # the other list is constant
    for o in MC.oracle(MC.CASE_IDS.index("median-exponents")):
        assert float(np.log2(o.z.max() / o.z.min())) > 14 and float(np.log2(o.p64.max() / o.p64.min())) > 14
    a, b = MC.oracle(MC.CASE_IDS.index("median-M2500"))
    assert a.n == 451 and int(a.idx.min()) > 2048 and b.n == 2500


def test_clamp_and_tie_cases_are_exact_and_hit_what_they_say():
    c = MC.by_name("clamp")
    lo, hi = c.min_depth, c.max_depth
    for o in MC.oracle(MC.CASE_IDS.index("clamp")):
        assert o.exact_ok
        s = o.s64
        assert bool((s < lo).any()) and bool((s == lo).any()) and bool((s == hi).any()) and bool((s > hi).any())
    ratios = [float(o.med_gt) / o.med_pd64 for o in MC.oracle(MC.CASE_IDS.index("clamp"))]
    assert ratios == [1.0, 4.0]
    for o in MC.oracle(MC.CASE_IDS.index("threshold-ties")):
        assert o.exact_ok and float(o.med_gt) / o.med_pd64 == 1.0
        th = np.maximum(o.z64 / o.pc64, o.pc64 / o.z64)            # exact in float64 on the tie
        for T in MC.THRESHOLDS:
            assert int((th == T).sum()) >= 1
            assert int((o.th32 == np.float32(T)).sum()) >= 1 and int((o.th32 == np.nextafter(np.float32(T), np.float32(0))).sum()) >= 1
            assert int((o.th32 == np.nextafter(np.float32(T), np.float32(9))).sum()) >= 1
    o = MC.oracle(MC.CASE_IDS.index("threshold-ties"))[0]
    assert o.all.cnt == [2, 5, 8]                                      # by hand: g = p, and the floats below the ties


def test_masked_cases_hold_the_labels_claimed():
    c = MC.by_name("masked-labels")
    a, b, e = MC.oracle(MC.CASE_IDS.index("masked-labels"))
    assert sorted(a.by_label) == list(range(256))
    assert sorted(b.by_label) == [0, 7, 8, 255] and b.by_label[7].n == 1 and b.by_label[8].n == 1
    assert bool((c.mask[1] == 9).any()) and b.n == c.M - 1 and e.n == 0
    pts = c.lidar[0].numpy()
    assert bool((pts[:, 1] % 1 == 0.75).all())                          # fractional: the label is that of the truncated pixel
    m0 = c.mask[0].numpy()
    assert bool((m0[:, 1:] != m0[:, :-1]).all())                        # horizontal neighbours carry different labels
    c = MC.by_name("masked-small-mask")
    o = MC.oracle(MC.CASE_IDS.index("masked-small-mask"))[0]
    outside = (o.rows >= c.mask.shape[1]) | (o.cols >= c.mask.shape[2])
    assert int(outside.sum()) > 50 and bool((o.labels[outside] == 0).all()) and bool((o.labels[~outside] > 0).all())
    assert 0 not in set(c.mask.reshape(-1).tolist())


@pytest.mark.parametrize("name", ["median-bytes", "median-bytes-pd"])
def test_a_wrong_median_leaves_the_fp32_chains_ulp(name):
    """criterion 7 has teeth, shown from chain32 alone: in sample `byte` a median that is one unit of that byte off (2^(8 byte) ulps; one
    ulp in sample 0), either way, and the upper median each move abs_rel, sq_rel or rms by more than the one ulp the judge allows"""
    c = MC.by_name(name)
    for byte, o in enumerate(MC.oracle(MC.CASE_IDS.index(name))):
        base = o.all.m32

        def seen(**kw):
            m = MC.chain32(o, c, **kw)
            return bool((np.abs(m.astype(np.float64) - base.astype(np.float64)) > np.spacing(base)).any())
        which = "gt_ulps" if name == "median-bytes" else "pd_ulps"
        for sign in (1, -1):
            assert seen(**{which: sign * 2 ** (8 * byte)}), (name, byte, sign)
        assert seen(upper=True), (name, byte)


@pytest.mark.parametrize("ci", [i for i in CI if MC.CASES[i].chain], ids=[c.name for c in MC.CASES if c.chain])
def test_fp32_chain_agrees_with_the_float64_oracle(ci):
    """chain32 is the same computation as the oracle: inside the oracle's own bounds, and its inputs are exact (chain_ok)"""
    for o in MC.oracle(ci):
        if o.n:
            assert o.chain_ok
            assert bool((np.abs(o.all.m32.astype(np.float64) - o.all.m64[:3]) <= o.all.bound[:3]).all())
