"""Shared plumbing of tests/test_reg_terms_gpu.py: ONE loss term (or a hand-picked set of terms) of the loss path at coefficient 1
and everything else at 0, the float64 oracle of exactly that, and hipops.fused_loss.fused_loss on the same leaves.

Why: at their training weights the regularisers are 1e-4 .. 3e-1 of the whole gradient, so a test of the summed gradient sees
the photometric term and little else.  Alone, each regulariser's fp32 oracle gradient sits 1e-7 from fp64 -- a tight bar exists, it
is only hidden under the photometric gradient.

Two terms carry a discrete decision that rounding may take either way; both are judged outside a band around the decision that is
computed from the float64 oracle alone (never from the kernel's output):
  * m_sparsity: the static set `mag < mean(mag)` (Trainer.py:385-391).  Pixels with |mag - mean| / mean < 1e-3 are `marked`.
  * d_ground: the RANSAC winner is not judged here (tests/test_ground_pin.py pins it; on the stand-in disparities the best two
    inlier fractions are usually equal).  The hinge is restated in float64 for the plane the library itself reports, and judged
    outside the pixels with |diff| < 1e-5 or a ground depth within 1e-3 of a clamp.
"""
import functools

import numpy as np
import torch

import synth
import oracle.ref_loss as orc
from photo_case import Case

# (B, H, W, scales): the smallest shapes that still reach each edge
SHAPES = {"A": (2, 80, 144, (0, 1, 2)),        # partial 16x32 tiles on both axes
          "B": (1, 96, 160, (0, 1, 2, 3)),     # four scales, rows of 20 at the coarsest
          "C": (1, 48, 32, (0, 1, 2, 3)),      # one tile column; coarsest scale 6x4: one quad per row, ground prior of 2 rows
          "D": (2, 64, 104, (0, 1, 2))}        # rows of 26 at scale 2: no quads, dd_fused_loss_supported says no
# seeds 3 and 4 keep the marked static pixels at or below 0.15 % on all four shapes; seed 3's plane at scale 1 of shape D has
# w3 + tol = -3e-5 (ground depth ~ 0 on 3/4 of the pixels: all border), seed 4 has an empty border set everywhere
# (test_inputs_are_well_conditioned asserts both caps)
SEED = 4
TERMS_OF_PHASE = {"disp_init": ("d_smooth",),
                  "motion_init": ("c_smooth",),
                  "mask_init": ("c_smooth", "c_consistency", "m_sparsity", "m_smooth"),
                  "fine_tune": ("d_smooth", "d_ground", "c_smooth", "c_consistency", "m_sparsity", "m_smooth")}
CLASS_OF = {"d_smooth": "smoothness", "c_smooth": "smoothness", "m_smooth": "smoothness", "m_sparsity": "sparsity",
            "d_ground": "hinge", "c_consistency": "consistency", "p_photo": "photo"}
GP = dict(gp_prior=0.4, gp_tol=0.005, gp_max_it=100, gp_np_per_it=5)
MARK_TAU = 1e-3          # |mag - mean| / mean below this: the static decision may go either way (the tolerance Case.check gives disp_mag)
MARK_CAP = 5e-3          # at most this share of any (scale, frame) may be marked
BORDER_CAP = 1e-2        # at most this share of a scale's unclamped pixels may sit on the hinge's border


def draws(B, H, W, scales):
    rs = np.random.RandomState(5)
    return {s: rs.randint(0, int(GP["gp_prior"] * (H >> s)) * (W >> s), (B, GP["gp_max_it"] * GP["gp_np_per_it"])).astype(np.int64) for s in scales}


def _blocks(t):
    """piecewise constant in 3x4 blocks: most neighbour differences are exactly 0"""
    h, w = t.shape[-2:]
    return t[:, :, ::3, ::4].repeat_interleave(3, 2).repeat_interleave(4, 3)[:, :, :h, :w].contiguous()


def _vary(leaves, variant, scales):
    for s in scales:
        d, f, p = (leaves[(k, s)].detach().clone() for k in ("disp", "flow", "prob"))
        h, w = p.shape[-2:]
        if variant == "ties":
            d, f, p = _blocks(d), _blocks(f), _blocks(p)
        elif variant == "saturated":          # sigmoid is exactly 0 or 1 in places
            p = p * 12
        elif variant == "logits":             # the logit form of the reference gives 100 and 0 per pixel, gradients 1 and 0
            p[:, :, : h // 2, : w // 3] = 100.0
            p[:, :, h // 2:, 2 * w // 3:] = -100.0
        elif variant is not None:
            raise ValueError(variant)
        for k, v in (("disp", d), ("flow", f), ("prob", p)):
            leaves[(k, s)] = v.requires_grad_()


class Ref:
    """The oracle's answer for one (phase, shape, term set, variant): values and gradients in fp32 and fp64 (CPU, float64 tensors)."""


@functools.lru_cache(maxsize=None)
def reference(phase, shape, terms, variant=None, seed=SEED, with_ground=False):
    """with_ground=False: d_ground is left out of the ORACLE (its winner is not judged; hinge() restates the term for the library's
    own plane and judge() adds it).  with_ground=True: the oracle's own RANSAC, for the CPU conditioning test."""
    B, H, W, scales = SHAPES[shape] if isinstance(shape, str) else shape
    scales = list(scales)
    r = Ref()
    r.phase, r.shape, r.terms, r.dims, r.variant = phase, shape, tuple(terms), (B, H, W, scales), variant
    r.coefs = {k: (1.0 if k in terms else 0.0) for k in orc.LOSS_TERMS}
    c = Case(phase, B, H, W, scales, seed=seed, active=())
    c.coefs = dict(r.coefs)
    if not with_ground:
        c.coefs["d_ground"] = 0.0
    c.cfg = orc.LossConfig(H, W, scales, coefs=c.coefs)
    _vary(c.leaves, variant, scales)
    r.ridx = draws(B, H, W, scales)
    c.run_oracle(rand_idx=r.ridx, fp64=True)
    r.case = c
    r.leaves = {k: v.detach().clone() for k, v in c.leaves.items()}
    r.g32 = {k: (None if v.grad is None else v.grad.detach().double()) for k, v in c.leaves.items()}
    r.g64 = {k: (None if c.grad64.get(k) is None else c.grad64[k].detach()) for k in c.leaves}
    r.v32 = {k: float(v.detach() if torch.is_tensor(v) else v) for k, v in c.losses.items()}
    r.v64 = {k: float(v.detach() if torch.is_tensor(v) else v) for k, v in c.losses64.items()}
    # m_sparsity: the pixels whose static decision is within rounding, per scale (either frame), and the allowance they buy
    r.marked, r.allowance, r.marked_share = {}, {}, 0.0
    if "m_sparsity" in terms:
        o = c.outputs64
        for s in scales:
            h, w = H >> s, W >> s
            m_any, allow = torch.zeros(B, 1, h, w, dtype=torch.bool), 0.0
            for f in (-1, 1):
                e = orc.resize_bilinear(o[("sample_ego", f, s)].permute(0, 3, 1, 2), (h, w))
                k = orc.resize_bilinear(o[("sample_complete", f, s)].permute(0, 3, 1, 2), (h, w))
                mag = ((e - k) ** 2).sum(1, keepdim=True)
                mean = mag.mean()
                m = ((mag - mean).abs() / mean) < MARK_TAU
                static = int((mag < mean).sum())
                r.marked_share = max(r.marked_share, float(m.double().mean()))
                allow = max(allow, float(m.sum()) / max(static, 1))
                m_any |= m
            r.marked[s], r.allowance[s] = m_any, allow
    return r


def hinge(r, planes, dtype=torch.float64):
    """oracle.ref_loss.ground_terms lines 238-249 + the hinge of compute_losses, restated for given planes {s: (B,3)}.
    Returns {s: (value of the term at the scale, d loss / d disp, border set, unclamped pixels)}; border set in fp64 only."""
    B, H, W, scales = r.dims
    cfg, out = r.case.cfg, {}
    for s in scales:
        disp = r.leaves[("disp", s)].to(dtype)
        h, w = disp.shape[-2:]
        inv_K = r.case.inputs[("inv_K", s)].to(dtype)
        p4 = torch.as_tensor(planes[s]).detach().cpu().to(dtype).reshape(B, 3, 1).clone()
        p4[:, 2] += cfg.gp_tol
        rays = torch.matmul(inv_K[:, :3, :3], orc.pixel_grid(B, h, w).to(dtype))
        w1, w2, w3 = p4[:, 0:1], p4[:, 1:2], p4[:, 2:3]
        vx, vy, vz = rays[:, 0:1], rays[:, 1:2], rays[:, 2:3]
        raw = (w3 / (vy - vx * w1 - vz * w2)).reshape(B, 1, h, w)
        clamped = (raw < 0) | (raw > cfg.max_depth)
        gdepth = torch.where(clamped, torch.full_like(raw, cfg.max_depth), raw)
        diff = disp - orc.depth_to_disp(gdepth, cfg.min_depth, cfg.max_depth)
        diff = torch.where(gdepth == cfg.max_depth, torch.zeros_like(diff), diff)
        value = float(-torch.clamp(diff, max=0).mean() / (2 ** s))
        active = (diff < 0) & ~clamped
        grad = -(r.coefs["d_ground"] / len(scales) / (2 ** s) / (B * h * w)) * active.to(dtype)
        border = (diff.abs() < 1e-5) & ~clamped
        # the two clamp decisions: gdepth < 0 (the sign can only turn at |gdepth| -> 0; through a vanishing denominator both sides
        # are clamped) and gdepth > max_depth
        border |= (raw.abs() < 1e-3) | ((raw - cfg.max_depth).abs() < 1e-3 * cfg.max_depth)
        out[s] = (value, grad.double(), border, int((~clamped).sum()))
    return out


# ------------------------------------------------------------------------------------------------------------------------------
def evaluate(r, pipeline, shared=True, materialise=False, grad=True):
    """fused_loss on the reference's leaves and inputs with its coefficients.  shared: publish the shared flow field and the shared
    mask as networks.Model does; otherwise the reference's per-frame tensors.  Returns (values, gradients, pipeline run, outputs)."""
    from hipops import fused_loss as FL
    from hipops.functions import PoseMatrixFn
    B, H, W, scales = r.dims
    c = r.case
    inputs = {k: v.cuda() for k, v in c.inputs.items()}
    leaves = {k: v.detach().cuda().requires_grad_() for k, v in r.leaves.items()}
    outputs = synth.leaves_to_outputs(leaves, scales, lambda a, t, invert: PoseMatrixFn.apply(a, t, invert), c.cmpflow, c.motmask)
    if c.cmpflow and shared:
        for s in scales:
            outputs[("complete_flow_field", 1, s)] = leaves[("flow", s)]
            if c.motmask:
                outputs[("motion_mask", -1, s)] = outputs[("motion_mask", 1, s)]
    if not grad:
        outputs = {k: v.detach() for k, v in outputs.items()}
    plan = FL.LossPlan(height=H, width=W, scales=scales, min_depth=c.cfg.min_depth, max_depth=c.cfg.max_depth, ssim_weight=c.cfg.ssim_weight,
                       mask_disp_thrd=c.cfg.mask_disp_thrd, cmpflow=c.cmpflow, motmask=c.motmask, automask=c.automask, optimised=c.optimised,
                       coefs=dict(r.coefs), **GP)
    noise = {s: c.noise[s].cuda() for s in scales} if c.automask else None
    old = FL.PIPELINE
    FL.PIPELINE = pipeline
    # the five-launch pipeline does not zero its gradient buffers: leave NaNs in the caching allocator's free blocks, so that an
    # element nobody writes shows up in the comparison
    poison = torch.full((64 << 20,), float("nan"), device="cuda")
    del poison
    try:
        if grad:
            losses = FL.fused_loss(plan, inputs, outputs, noise=noise, rand_idx=r.ridx, materialise=materialise)
        else:
            with torch.no_grad():
                losses = FL.fused_loss(plan, inputs, outputs, noise=noise, rand_idx=r.ridx, materialise=materialise)
        ran = FL.LAST_PIPELINE[0]
    finally:
        FL.PIPELINE = old
    if grad:
        losses["loss"].backward()
    torch.cuda.synchronize()
    vals = {k: float(v.detach() if torch.is_tensor(v) else v) for k, v in losses.items()}
    grads = {k: (torch.zeros_like(v) if v.grad is None else v.grad).double().cpu() for k, v in leaves.items()}
    return vals, grads, ran, outputs


def planes_of(r, pipeline, shared=True):
    """The planes the library reports (a second call with materialise=True; the draws are injected, so they are the first call's)."""
    _, _, _, outputs = evaluate(r, pipeline, shared, materialise=True)
    return {s: outputs[("ground_plane", s)].detach().cpu() for s in r.dims[3]}


def leaf_class(r, key):
    """which term reaches this leaf alone -- its class sets the floor (the hand-picked sets put one term on each leaf)"""
    kind = key[0]
    reach = {"disp": ("d_smooth", "d_ground", "c_consistency", "p_photo"), "flow": ("c_smooth", "c_consistency", "p_photo"),
             "prob": ("m_sparsity", "m_smooth", "p_photo"), "axisangle": ("c_consistency", "p_photo"), "translation": ("c_consistency", "p_photo")}[kind]
    classes = {CLASS_OF[t] for t in r.terms if t in reach}
    for k in ("photo", "consistency", "hinge", "sparsity", "smoothness"):      # the loosest class present decides
        if k in classes:
            return k
    return None


def judge(r, vals, grads, floors, value_tol, report, hinge64=None, hinge32=None, values_only=False):
    """Every value and every gradient against the fp64 oracle.  floors / value_tol: {class: number}.  Returns the failures; `report`
    receives one line per comparison with the kernel's distance from fp64 next to the fp32 oracle's own, and a last line `worst:`
    with the case's largest value and gradient distances (profiles/reg_terms_parity.txt keeps those lines)."""
    B, H, W, scales = r.dims
    fails = []
    tag = "%s %s %s%s" % (r.phase, r.shape, "+".join(r.terms), " (%s)" % r.variant if r.variant else "")
    worst_v, worst_g, zeros = (-1.0, 0.0, ""), {}, 0

    def summary():
        line = "%s worst: value %s rel %.2e (fp32 oracle %.2e)" % (tag, worst_v[2], worst_v[0], worst_v[1])
        for k in sorted(worst_g):
            line += " | grad [%s] %s kernel %.3e, fp32 oracle %.3e, bar %.2e" % ((k,) + worst_g[k][3:] + worst_g[k][:3])
        report.append(line + (" | %d leaves exactly 0 like the oracle" % zeros if not values_only else ""))

    def value(name, got, want, want32, tol, extra=0.0):
        rel = abs(got - want) / max(abs(want), 1e-30)
        rel32 = abs(want32 - want) / max(abs(want), 1e-30)
        nonlocal worst_v
        if rel > worst_v[0]:
            worst_v = (rel, rel32, name)
        report.append("%s value %-24s kernel %.9g fp64 %.9g: rel %.2e (fp32 oracle %.2e) bar %.1e" % (tag, name, got, want, rel, rel32, tol + extra))
        if not np.isfinite(got) or rel > tol + extra:
            fails.append("value %s: %.9g vs %.9g (rel %.2e > %.1e)" % (name, got, want, rel, tol + extra))

    allow = max(r.allowance.values()) if r.allowance else 0.0
    for t in orc.LOSS_TERMS:
        got = vals["loss_term/" + t]
        if t not in r.terms:
            if t != "p_photo" and got != 0.0:
                fails.append("inactive term %s = %g" % (t, got))
            continue
        want, want32 = r.v64["loss_term/" + t], r.v32["loss_term/" + t]
        if t == "d_ground":
            want, want32 = sum(v[0] for v in hinge64.values()), sum(v[0] for v in hinge32.values())
        value(t, got, want, want32, value_tol[CLASS_OF[t]], allow if t == "m_sparsity" else 0.0)
    for s in scales:
        want, want32 = r.v64["loss_term/%d" % s], r.v32["loss_term/%d" % s]
        if "d_ground" in r.terms:
            want, want32 = want + hinge64[s][0], want32 + hinge32[s][0]
        tol = max(value_tol[CLASS_OF[t]] for t in r.terms)
        value("scale %d" % s, vals["loss_term/%d" % s], want, want32, tol, r.allowance.get(s, 0.0))
    if values_only:
        summary()
        return fails

    for key in sorted(grads, key=str):
        got = grads[key]
        if not bool(torch.isfinite(got).all()):
            fails.append("grad %s: non-finite elements" % (key,))
            continue
        g64, g32 = r.g64.get(key), r.g32.get(key)
        g64 = torch.zeros_like(got) if g64 is None else g64.reshape(got.shape).clone()
        g32 = torch.zeros_like(got) if g32 is None else g32.reshape(got.shape).clone()
        keep = torch.ones_like(got, dtype=torch.bool)
        extra = 0.0
        if key[0] == "disp" and "d_ground" in r.terms:
            g64 += hinge64[key[1]][1]
            g32 += hinge32[key[1]][1]
            keep &= ~hinge64[key[1]][2]
        if key[0] == "prob" and "m_sparsity" in r.terms:
            keep &= ~r.marked[key[1]].expand_as(keep)
            extra = r.allowance[key[1]]
            # outside the marked pixels the static set is the oracle's: same zero pattern (a gradient below 1e-30 is a sigmoid that
            # fp32 may flush: compare values there, not patterns)
            wrong = keep & (((g64 == 0) & (got != 0)) | ((g64.abs() > 1e-30) & (got == 0)))
            if bool(wrong.any()):
                fails.append("grad %s: %d elements on the wrong side of the static decision" % (key, int(wrong.sum())))
        if float(g64.norm()) == 0.0:
            nz = int((got != 0).sum())
            report.append("%s grad %-20s oracle is exactly 0; kernel has %d nonzero elements" % (tag, key, nz))
            if nz:
                fails.append("grad %s must be exactly 0, %d elements are not (max %.3e)" % (key, nz, float(got.abs().max())))
            zeros += not nz
            continue
        den = float((g64 * keep).norm())
        e_k = float(((got - g64) * keep).norm()) / den
        e_32 = float(((g32 - g64) * keep).norm()) / den
        klass = leaf_class(r, key)
        bar = max(4.0 * e_32, floors[klass]) + extra
        report.append("%s grad %-20s [%s] vs fp64: kernel %.3e, fp32 oracle %.3e, bar %.2e" % (tag, key, klass, e_k, e_32, bar))
        if klass not in worst_g or e_k > worst_g[klass][0]:
            worst_g[klass] = (e_k, e_32, bar, "%s[%s]" % key)
        if e_k > bar:
            fails.append("grad %s: %.3e > %.2e (fp32 oracle %.3e)" % (key, e_k, bar, e_32))
    summary()
    return fails
