"""Each regulariser of the loss path ALONE (coefficient 1, everything else 0) against the float64 oracle: dd_reg.hip's stage kernels,
the smoothness folded into the photometric tile kernel and the footprint pass (dd_fuse.h), and the term-set branches of
hipops/fused_loss.py -- values, per-scale values and the gradient on every leaf, through the five-launch pipeline, the ten-launch
one and the ten-launch one on the reference's per-frame tensors.  tests/reg_case.py holds the plumbing and says how the two
decisions (static set, RANSAC winner) are kept out of the comparison.

Shapes A-D (reg_case.SHAPES); every entry point accepted shape C (48x32, coarsest scale 6x4) as it stands.  c_consistency alone
(like p_photo alone) leaves the regulariser entry points nothing to do: PIPELINE="fused" then runs the photometric launches and
dd_assemble_losses, and that is what is asserted for it.  In the term sets that hold d_ground, the hinge's share of the reference
is the float64 restatement for the library's own plane, as in the single-term runs.

What this file found when it was written: the ten-launch smoothness formed a normalised difference as fma(a, 1/m, -round(b/m)), so
that two EQUAL disparities differed by a rounding error and took sign(+-1e-8) instead of abs'(0) = 0 (test_constructed_inputs,
d_smooth-ties: relative L2 1.3); and a thread of a tile that overhangs the image read warped colours nobody had stored, whose
weight-0 products were summed into the pose gradient (NaN now and then at shape A, disp_init).

Tolerances.  A gradient is held to relative L2 <= max(4 x the fp32 oracle's own distance from fp64, floor of the term's class);
the floors are 4 x the worst figure of profiles/reg_terms_parity.txt (the `worst:` line of every case of this file, run with -s on
an MI355X), the margin of 4 covering __expf in the edge weights and the summation order.  Caps that hold whatever is measured: no
gradient floor above 1e-4, no value tolerance above 3e-5 of the term's own value.
"""
import copy
import os

import numpy as np
import pytest
import torch

import oracle.ref_loss as orc
import reg_case as RC

gpu = pytest.mark.gpu

# class: 4 x the worst kernel-vs-fp64 figure of the class in profiles/reg_terms_parity.txt (the measured figure and its line beside it)
GRAD_FLOOR = {"smoothness": 1.8e-6,     # worst 4.451e-07: fine_tune A m_smooth (saturated), prob[0], five launches (line 154)
              "sparsity": 3.0e-7,       # worst 7.520e-08: mask_init D m_sparsity, prob[1], ten launches (line 58)
              "hinge": 2.1e-7,          # worst 5.215e-08: fine_tune B d_ground, disp[0] (line 85) -- the rounding of the one constant -w
              "consistency": 4.1e-5,    # worst 1.014e-05: mask_init B c_consistency, axisangle[+1] (line 41); the fp32 oracle: 1.016e-05
              "photo": 3e-4}            # not this file's subject: the bar Case.check_grads holds the photometric gradient to against fp64
VALUE_TOL = {"smoothness": 6.6e-7,      # worst 1.63e-07: disp_init A d_smooth, scale 1, five launches (line 5)
             "sparsity": 3.9e-7,        # worst 9.63e-08: mask_init B m_sparsity, scale 0 (line 52)
             "hinge": 2e-5,             # the bar of tests/test_ground_pin.py once the candidates are given; worst measured 2.47e-07 (line 85)
             "consistency": 4.6e-7,     # worst 1.14e-07: mask_init C c_consistency (line 44)
             "photo": 2e-5}             # Case.check's bar for p_photo
assert all(v <= 1e-4 for k, v in GRAD_FLOOR.items() if k != "photo") and all(v <= 3e-5 for v in VALUE_TOL.values())

PAIRS = [(p, t) for p, ts in RC.TERMS_OF_PHASE.items() for t in ts]
WAYS = {"fused-shared": ("fused", True), "split-shared": ("split", True), "split-perframe": ("split", False)}
SETS = [("d_ground", "m_sparsity"),       # no smoothness group at all
        ("d_smooth", "m_smooth"),         # no flow group
        ("c_smooth", "d_ground"),
        ("p_photo",)]                     # any_reg is false: dd_assemble_losses
CONSTRUCTED = [("d_smooth", "ties"), ("c_smooth", "ties"), ("m_smooth", "ties"), ("m_smooth", "saturated"), ("m_sparsity", "logits")]


def run(r, way, report):
    pipeline, shared = WAYS[way]
    vals, grads, ran, _ = RC.evaluate(r, pipeline, shared)
    B, H, W, scales = r.dims
    quads = all((W >> s) % 4 == 0 for s in scales if s > 0)
    # c_consistency is summed by the photometric kernel itself: alone (like p_photo alone) it leaves the regulariser entry points
    # nothing to do, any_reg is false and the photometric launches + dd_assemble_losses run whatever PIPELINE says
    reg_on = any(t not in ("p_photo", "c_consistency") for t in r.terms)
    assert ran == ("fused5" if (pipeline == "fused" and quads and reg_on) else "split"), ran
    h64 = h32 = None
    if "d_ground" in r.terms:
        planes = RC.planes_of(r, pipeline, shared)
        h64, h32 = RC.hinge(r, planes), RC.hinge(r, planes, torch.float32)
        for s in scales:
            assert int(h64[s][2].sum()) <= RC.BORDER_CAP * max(h64[s][3], 1), ("hinge border set", s)
    fails = RC.judge(r, vals, grads, GRAD_FLOOR, VALUE_TOL, report, h64, h32)
    print("\n".join("[%s] %s" % (way, line) for line in report))
    return fails, vals


# ---- 1: one term at a time ------------------------------------------------------------------------------------------------------
# shape D (rows of 26 at scale 2): the five launches do not apply, only the ten are asserted there
SHAPE_WAYS = [(sh, w) for sh in RC.SHAPES for w in WAYS if not (sh == "D" and w == "fused-shared")]


@gpu
@pytest.mark.parametrize("shape,way", SHAPE_WAYS, ids=["%s-%s" % x for x in SHAPE_WAYS])
@pytest.mark.parametrize("phase,term", PAIRS, ids=["%s-%s" % p for p in PAIRS])
def test_one_term_alone(phase, term, shape, way):
    fails, _ = run(RC.reference(phase, shape, (term,)), way, [])
    assert not fails, fails


# ---- 2: term sets no phase selects ----------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("way", ["fused-shared", "split-shared"])
@pytest.mark.parametrize("terms", SETS, ids=["+".join(t) for t in SETS])
def test_term_sets_no_phase_selects(terms, way):
    r = RC.reference("fine_tune", "A", terms)
    fails, vals = run(r, way, [])
    # the same per-term values as the single-term runs
    for t in terms:
        if t == "p_photo":
            continue
        alone, _, _, _ = RC.evaluate(RC.reference("fine_tune", "A", (t,)), WAYS[way][0], True)
        a, b = vals["loss_term/" + t], alone["loss_term/" + t]
        if abs(a - b) > 2 * VALUE_TOL[RC.CLASS_OF[t]] * abs(b):
            fails.append("%s in the set %.9g, alone %.9g" % (t, a, b))
    assert not fails, fails


# ---- 4: constructed inputs ------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("way", list(WAYS))
@pytest.mark.parametrize("term,variant", CONSTRUCTED, ids=["%s-%s" % c for c in CONSTRUCTED])
def test_constructed_inputs(term, variant, way):
    fails, _ = run(RC.reference("fine_tune", "A", (term,), variant), way, [])
    assert not fails, fails


# ---- 5: the hinge on disparities of trained networks ----------------------------------------------------------------------------
def ground_pin_case(golden_dir, name):
    z = np.load(os.path.join(golden_dir, "ground_pin.npz"))
    B, H, W, max_it, npi = [int(x) for x in z["meta"]]
    assert (max_it, npi) == (RC.GP["gp_max_it"], RC.GP["gp_np_per_it"]) and np.float32(z["tol"]) == np.float32(RC.GP["gp_tol"]) and np.float32(z["g_prior"]) == np.float32(RC.GP["gp_prior"])
    r = RC.reference("fine_tune", (B, H, W, (0,)), ("d_ground",))
    r = _with_disp(r, torch.from_numpy(z[name + "/disp"]), torch.from_numpy(z["inv_K"]), {0: z[name + "/rand_idx"].astype(np.int64)})
    return r, z[name + "/param"]


def _with_disp(r, disp, inv_K, ridx):
    """a copy of the reference whose scale-0 disparity, intrinsics and draws are the fixture's (the oracle part holds no active term:
    every value and gradient of it is 0, whatever the disparity)"""
    q = copy.copy(r)
    q.leaves = dict(r.leaves)
    q.leaves[("disp", 0)] = disp.clone()
    q.ridx = ridx
    q.case = copy.copy(r.case)
    q.case.inputs = dict(r.case.inputs)
    q.case.inputs[("inv_K", 0)] = inv_K
    q.case.inputs[("K", 0)] = torch.linalg.pinv(inv_K)
    return q


@gpu
@pytest.mark.parametrize("way", ["fused-shared", "split-shared"])
@pytest.mark.parametrize("name", ["trained", "smooth"])
def test_hinge_on_the_ground_pin_disparities(golden_dir, name, way):
    r, param = ground_pin_case(golden_dir, name)
    pipeline, shared = WAYS[way]
    planes = RC.planes_of(r, pipeline, shared)
    got = planes[0].numpy()
    assert np.allclose(got, param.reshape(got.shape), rtol=2e-3, atol=1e-5), (got, param)      # tests/test_ground_pin.py::test_kernel_end_to_end
    vals, grads, ran, _ = RC.evaluate(r, pipeline, shared)
    h64, h32 = RC.hinge(r, planes), RC.hinge(r, planes, torch.float32)
    assert int(h64[0][2].sum()) <= RC.BORDER_CAP * max(h64[0][3], 1)
    report = []
    fails = RC.judge(r, vals, grads, GRAD_FLOOR, VALUE_TOL, report, h64, h32)
    print("\n".join("[%s %s] %s" % (name, way, line) for line in report))
    assert h64[0][0] > 0 and float(h64[0][1].abs().sum()) > 0, "the case decides nothing"
    assert not fails, fails


# ---- 7: the validation pass, the stand-alone smoothness, the conditioning of the inputs ----------------------------------------
@gpu
@pytest.mark.parametrize("phase", list(RC.TERMS_OF_PHASE))
def test_values_without_gradients(phase):
    """torch.no_grad(): the validation pass (always the ten launches), all of the phase's terms on at coefficient 1."""
    terms = RC.TERMS_OF_PHASE[phase]
    r = RC.reference(phase, "A", terms)
    vals, _, ran, _ = RC.evaluate(r, "fused", True, grad=False)
    assert ran == "split"
    h64 = h32 = None
    if "d_ground" in terms:
        planes = RC.planes_of(r, "fused", True)
        h64, h32 = RC.hinge(r, planes), RC.hinge(r, planes, torch.float32)
    report = []
    fails = RC.judge(r, vals, {}, GRAD_FLOOR, VALUE_TOL, report, h64, h32, values_only=True)
    print("\n".join("[no_grad] %s" % line for line in report))
    assert not fails, fails


@gpu
@pytest.mark.parametrize("with_img", [True, False], ids=["img", "noimg"])
@pytest.mark.parametrize("dims", [(2, 3, 5, 7), (1, 1, 9, 33)], ids=lambda d: "x".join(map(str, d)))
def test_standalone_smooth_loss(dims, with_img):
    import tools
    g = torch.Generator().manual_seed(17)
    x = torch.randn(*dims, generator=g)
    img = torch.rand(dims[0], 3, dims[2], dims[3], generator=g) if with_img else None
    x64 = x.double().requires_grad_()
    want = orc.smooth_loss(x64, None if img is None else img.double())
    want.backward()
    x32 = x.clone().requires_grad_()
    w32 = orc.smooth_loss(x32, img)
    w32.backward()
    xg = x.cuda().requires_grad_()
    got = tools.compute_smooth_loss(xg, None if img is None else img.cuda())
    got.backward()
    e_v, e_v32 = abs(float(got) - float(want)) / float(want), abs(float(w32) - float(want)) / float(want)
    den = float(x64.grad.norm())
    e_g, e_g32 = float((xg.grad.double().cpu() - x64.grad).norm()) / den, float((x32.grad.double() - x64.grad).norm()) / den
    print("standalone smooth %s img=%s value rel %.2e (fp32 oracle %.2e) grad rel_l2 %.2e (fp32 oracle %.2e)" % (dims, with_img, e_v, e_v32, e_g, e_g32))
    assert bool(torch.isfinite(xg.grad).all())
    assert e_v <= VALUE_TOL["smoothness"] and e_g <= max(4 * e_g32, GRAD_FLOOR["smoothness"])


def _all_cases():
    for phase, term in PAIRS:
        for shape in RC.SHAPES:
            yield phase, shape, (term,), None
    for terms in SETS:
        yield "fine_tune", "A", terms, None
    for term, variant in CONSTRUCTED:
        yield "fine_tune", "A", (term,), variant
    for phase, terms in RC.TERMS_OF_PHASE.items():
        yield phase, "A", terms, None


def test_inputs_are_well_conditioned():
    """CPU only: for every case the GPU tests use, the fp32 oracle is within 2e-5 of fp64 (values and gradients), at most 0.5 % of any
    (scale, frame) is within 1e-3 of the static threshold, and at most 1 % of a scale's unclamped pixels sit on the hinge's border
    (with the oracle's own plane)."""
    bad, worst = [], {}
    for phase, shape, terms, variant in _all_cases():
        if terms == ("p_photo",):
            continue                     # the photometric term's conditioning is tests/test_photo_gpu.py's subject
        r = RC.reference(phase, shape, terms, variant)
        tag = "%s %s %s %s" % (phase, shape, "+".join(terms), variant or "")
        for t in terms:
            if t == "d_ground":
                continue
            a, b = r.v32["loss_term/" + t], r.v64["loss_term/" + t]
            e = abs(a - b) / abs(b)
            worst[("value", RC.CLASS_OF[t])] = max(worst.get(("value", RC.CLASS_OF[t]), 0.0), e)
            if not e <= 2e-5:
                bad.append("%s: value of %s %.2e" % (tag, t, e))
        for key, g64 in r.g64.items():
            if g64 is None or float(g64.norm()) == 0:
                continue
            keep = ~r.marked[key[1]] if (key[0] == "prob" and r.marked) else torch.ones_like(g64, dtype=torch.bool)
            e = float(((r.g32[key] - g64) * keep).norm() / (g64 * keep).norm())
            k = RC.leaf_class(r, key)
            worst[("grad", k)] = max(worst.get(("grad", k), 0.0), e)
            if not e <= 2e-5:
                bad.append("%s: gradient on %s %.2e" % (tag, key, e))
        if r.marked_share > RC.MARK_CAP:
            bad.append("%s: %.4f of a (scale, frame) within %.0e of the static threshold" % (tag, r.marked_share, RC.MARK_TAU))
        worst["marked"] = max(worst.get("marked", 0.0), r.marked_share)
        if "d_ground" in terms:
            planes = {}
            for s in r.dims[3]:
                planes[s] = orc.ground_terms(r.leaves[("disp", s)], r.case.inputs[("inv_K", s)], r.case.cfg, r.ridx[s])[3].reshape(-1, 3)
            h64, h32 = RC.hinge(r, planes), RC.hinge(r, planes, torch.float32)
            for s in r.dims[3]:
                share = int(h64[s][2].sum()) / max(h64[s][3], 1)
                worst["border"] = max(worst.get("border", 0.0), share)
                if share > RC.BORDER_CAP:
                    bad.append("%s: %.4f of scale %d's unclamped pixels on the hinge's border" % (tag, share, s))
                keep = ~h64[s][2]
                if float((h64[s][1] * keep).norm()) > 0:
                    e = float(((h32[s][1] - h64[s][1]) * keep).norm() / (h64[s][1] * keep).norm())
                    worst[("grad", "hinge")] = max(worst.get(("grad", "hinge"), 0.0), e)
                    if not e <= 2e-5:
                        bad.append("%s: hinge gradient at scale %d %.2e" % (tag, s, e))
                if h64[s][0] > 0:
                    e = abs(h32[s][0] - h64[s][0]) / h64[s][0]
                    worst[("value", "hinge")] = max(worst.get(("value", "hinge"), 0.0), e)
                    if not e <= 2e-5:
                        bad.append("%s: hinge value at scale %d %.2e" % (tag, s, e))
    print("worst fp32-oracle distance from fp64 / worst shares:", {str(k): "%.2e" % v for k, v in worst.items()})
    assert not bad, bad
