"""The one-by-one operators of csrc/dd_ops.hip (dd_backproject, dd_project3d, dd_ssim, dd_disp_to_depth, dd_pose_matrix and their
_bwd) against the float64 oracle at the edges the golden of tests/test_ops_gpu.py (B=3, 24x40, one draw of angles) never reaches:
one partial wave, exactly one block, 258 blocks (fold16_kernel's second trip), the grid-stride loop's second trip, H or W of 2 and
3 (both reflections on the same rows), one of two gradients requested, the NULL arguments of the C ABI that autograd never passes,
points behind the camera, and pose vectors from 3 down to 1e-8 and exactly 0.

tests/ops_case.py holds the inputs, the oracle in both precisions and the one criterion (e_k <= max(4 e_32, F S), every quantity in
its own tensor, nothing in a bound from the kernel's output); tests/test_ops_inputs.py asserts on the CPU that the inputs are what is
claimed here.

Every case prints one `worst:` line (run with -s); profiles/ops_parity.txt keeps those of one MI355X run as a record.
"""
import pytest
import torch

import ops_case as OC
from ops_case import Judge

gpu = pytest.mark.gpu
NAN = float("nan")


def cu(t):
    return None if t is None else t.detach().cuda().contiguous()


# ---- BackprojectDepth / Project3D --------------------------------------------------------------------------------------------------
def backproject_case(shape, kind):
    import tools
    B, h, w = shape
    s, r = OC.scene(B, h, w, kind), OC.backproject_ref(B, h, w, kind)
    bp, inv_K = tools.BackprojectDepth(B, h, w), cu(s.inv_K)
    outs, grads = OC.run(lambda d: bp(d, inv_K), [s.depth], [True], [s.w_points], device="cuda")
    j = Judge("backproject", "%s %s" % (shape, kind))
    j.check("points", outs[0], r.out64[0], r.out32[0], "max")
    j.equal("points[:, 3] == 1", outs[0][:, 3], torch.ones(B, h * w, dtype=torch.float64))
    j.check("g_depth", grads[0], r.g64[0], r.g32[0], "l2")
    return j.finish()


def project_case(shape, kind, with_T, which, skew=False):
    import tools
    B, h, w = shape
    r = OC.project_ref(B, h, w, kind, with_T, which, skew)
    s = r.scene
    pj, K = tools.Project3D(B, h, w), cu(s.K)
    if with_T:
        outs, grads = OC.run(lambda p, T: pj(p, K, T), [s.points, s.T], [True, True], [r.w_pix, r.w_ego], device="cuda")
    else:
        outs, grads = OC.run(lambda p: pj(p, K, None), [s.moved], [True], [r.w_pix, r.w_ego], device="cuda")
    j = Judge("project3d", "%s %s %s%s downstream: %s" % (shape, kind, "T" if with_T else "T=None", " skewed K and T" if skew else "", which))
    j.check("pix", outs[0], r.out64[0], r.out32[0], "max")
    j.check("ego", outs[1], r.out64[1], r.out32[1], "max")             # T=None: the oracle is exactly 0, so is the bound
    j.check("g_points", grads[0], r.g64[0], r.g32[0], "l2")
    if with_T:
        j.check("g_T", grads[1], r.g64[1], r.g32[1], "l2", floor=r.gT_floor)
    return j.finish()


def project_null_case(shape, kind, with_T, which):
    """dd_project3d_bwd with g_ego = NULL (which = 'pix') or g_pix = NULL ('ego'): autograd materialises both, the ABI documents NULL.
    Without T also g_T and the workspace are NULL.  Judged against the oracle with that output unused."""
    from hipops import lib as L
    from hipops.functions import _p, _ws
    B, h, w = shape
    r = OC.project_ref(B, h, w, kind, with_T, which)
    s, lib = r.scene, L.load()
    pts, K, T = cu(s.points if with_T else s.moved), cu(s.K), cu(s.T) if with_T else None
    g_pix, g_ego = cu(r.w_pix), cu(r.w_ego)
    assert (g_pix is None) != (g_ego is None)
    g_points = torch.full_like(pts, NAN)
    g_T = torch.full((B, 4, 4), NAN, device="cuda") if with_T else None
    ws = _ws(lib.dd_project3d_workspace_bytes(B, h, w), pts.device) if with_T else None
    L.check(lib.dd_project3d_bwd(_p(pts), _p(K), _p(T), _p(g_pix), _p(g_ego), B, h, w, 1e-7, _p(g_points), _p(g_T), _p(ws), L.current_stream()),
            "dd_project3d_bwd")
    torch.cuda.synchronize()
    j = Judge("project3d_bwd ABI", "%s %s %s %s = NULL" % (shape, kind, "T" if with_T else "T=None", "g_ego" if which == "pix" else "g_pix"))
    j.check("g_points", g_points, r.g64[0], r.g32[0], "l2")
    if with_T:
        j.check("g_T", g_T, r.g64[1], r.g32[1], "l2", floor=r.gT_floor)
    return j.finish()


@gpu
@pytest.mark.parametrize("kind", ["front", "behind"])
@pytest.mark.parametrize("shape", OC.GEOM_SHAPES, ids=str)
def test_backproject_project(shape, kind):
    fails = backproject_case(shape, kind)
    for with_T in (True, False):
        for which in ("pix", "ego", "both"):
            fails += project_case(shape, kind, with_T, which)
        for which in ("pix", "ego"):
            fails += project_null_case(shape, kind, with_T, which)
    assert not fails, fails


@gpu
def test_project_multiplies_all_four_components():
    """a K with a fourth column, a T whose last row is not (0, 0, 0, 1)"""
    fails = []
    for which in ("pix", "both"):
        fails += project_case((2, 24, 40), "front", True, which, skew=True)
    assert not fails, fails


# ---- SSIM --------------------------------------------------------------------------------------------------------------------------
SSIM_CASES = [(s, "random") for s in OC.SSIM_EDGE_SHAPES] + [(s, k) for s in OC.SSIM_SHAPES for k in OC.SSIM_KINDS]


@gpu
@pytest.mark.parametrize("shape,kind", SSIM_CASES, ids=["%s-%s" % c for c in SSIM_CASES])
def test_ssim(shape, kind):
    import tools
    r = OC.ssim_ref(shape, kind)
    ssim, fails = tools.SSIM(), []
    for needs in ((True, True), (True, False), (False, True)):          # the last two: the kernel's NULL g_y / g_x
        outs, grads = OC.run(ssim, r.args, needs, r.weights, device="cuda")
        j = Judge("ssim", "%s %s gradient of %s" % (shape, kind, "+".join(n for n, need in zip("xy", needs) if need)))
        j.check("ssim", outs[0], r.out64[0], r.out32[0], "max")
        for i, name in enumerate(("g_x", "g_y")):
            if needs[i] and kind in OC.SSIM_GRADIENT_NOT_JUDGED:
                assert bool(torch.isfinite(grads[i]).all()), name
            elif needs[i]:
                j.check(name, grads[i], r.g64[i], r.g32[i], "l2", kind="g_ssim", scale=r.scale[i])
            else:
                assert grads[i] is None
        fails += j.finish()
    assert not fails, fails


# ---- disp_to_depth -----------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n", OC.DISP_SIZES)
def test_disp_to_depth(n):
    import tools
    from hipops import lib as L
    from hipops.functions import _p
    r = OC.disp_ref(n)
    outs, grads = OC.run(lambda d: tools.disp_to_depth(d, OC.MIN_DEPTH, OC.MAX_DEPTH), r.args, [True], r.weights, device="cuda")
    j = Judge("disp_to_depth", "n = %d" % n)
    j.check("scaled", outs[0], r.out64[0], r.out32[0], "max")
    j.check("depth", outs[1], r.out64[1], r.out32[1], "max")
    j.check("g_disp", grads[0], r.g64[0], r.g32[0], "l2")
    # the ABI's NULL outputs: the other output is what the both-outputs call writes, bit for bit
    lib, disp = L.load(), cu(r.args[0])
    both, only = [torch.full_like(disp, NAN) for _ in range(2)], [torch.full_like(disp, NAN) for _ in range(2)]
    for scaled, depth in ((both[0], both[1]), (only[0], None), (None, only[1])):
        L.check(lib.dd_disp_to_depth(_p(disp), n, OC.MIN_DEPTH, OC.MAX_DEPTH, _p(scaled), _p(depth), L.current_stream()), "dd_disp_to_depth")
    torch.cuda.synchronize()
    j.equal("both outputs == autograd's", torch.stack(both).double().cpu(), torch.stack(outs))
    j.equal("scaled with depth = NULL", only[0], both[0])
    j.equal("depth with scaled = NULL", only[1], both[1])
    fails = j.finish()
    assert not fails, fails


# ---- pose matrix -------------------------------------------------------------------------------------------------------------------
def pose_case(B, kind, invert, flat_layout):
    from networks.layers import transformation_from_parameters
    r = OC.pose_ref(B, kind, invert)
    aa, tr = r.args
    args = [aa.reshape(B, 3), tr.reshape(B, 3)] if flat_layout else [aa, tr]
    outs, grads = OC.run(lambda a, t: transformation_from_parameters(a, t, invert=invert), args, [True, True], r.weights, device="cuda")
    assert grads[0].shape == args[0].shape and grads[1].shape == args[1].shape
    j = Judge("pose_matrix", "B = %d |aa| ~ %s invert = %d layout %s" % (B, kind, invert, "(B,3)" if flat_layout else "(B,1,3)"))
    j.check("T", outs[0], r.out64[0], r.out32[0], "max")
    j.check("g_axisangle", grads[0], r.g64[0], r.g32[0], "l2")
    j.check("g_translation", grads[1], r.g64[1], r.g32[1], "l2")
    zero = (aa.reshape(B, 3).abs().sum(1) == 0)
    if bool(zero.any()):        # theta = 0: the oracle's gradient is exactly 0 (torch.norm's backward at the origin); bound 0
        assert float(r.g64[0].reshape(B, 3)[zero].abs().max()) == 0.0
        j.check("g_axisangle[theta == 0]", grads[0].reshape(B, 3)[zero], r.g64[0].reshape(B, 3)[zero], r.g32[0].reshape(B, 3)[zero], "l2",
                kind="g_axisangle")
    return j.finish()


@gpu
@pytest.mark.parametrize("invert", [False, True])
@pytest.mark.parametrize("B", OC.POSE_BATCHES)
def test_pose_batch_sizes(B, invert):
    """the magnitude of training (0.01 x the head's output), every batch size around the 64-thread block, both layouts"""
    fails = pose_case(B, 1e-2, invert, False) + pose_case(B, 1e-2, invert, True)
    assert not fails, fails


@gpu
@pytest.mark.parametrize("invert", [False, True])
@pytest.mark.parametrize("kind", OC.POSE_SWEEP + ["mixed", "pi"], ids=str)
def test_pose_magnitudes(kind, invert):
    fails = pose_case(OC.POSE_SWEEP_B, kind, invert, kind == "mixed")
    assert not fails, fails


# ---- the chain ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_chain():
    """the five operators composed: a layout that two of them disagree on passes each alone and fails here"""
    import tools
    from networks.layers import transformation_from_parameters
    r = OC.chain_ref()
    s = r.scene
    B, h, w = OC.CHAIN_SHAPE
    bp, pj, ssim = tools.BackprojectDepth(B, h, w), tools.Project3D(B, h, w), tools.SSIM()
    ops = (tools.disp_to_depth, bp, lambda p, K, T, hh, ww: pj(p, K, T), lambda a, t, inv: transformation_from_parameters(a, t, invert=inv), ssim)
    fn = OC.chain_fn(ops, cu(s.K), cu(s.inv_K), cu(r.frames[1]), cu(r.frames[0]), h, w, r.band)
    outs, grads = OC.run(fn, r.args, r.needs, r.weights, device="cuda")
    j = Judge("chain", "%s disp_to_depth > backproject > project(pose) > grid_sample > ssim > mean" % (OC.CHAIN_SHAPE,))
    j.check("loss", outs[0], r.out64[0], r.out32[0], "max", kind="chain")
    for name, got, g64, g32 in zip(("g_disp", "g_axisangle", "g_translation"), grads, r.g64, r.g32):
        j.check(name + " (chain)", got, g64, g32, "l2", kind="chain")
    fails = j.finish()
    assert not fails, fails
