"""Size-independent properties of the fused photometric kernel at the FULL benchmark shapes of BASELINE.json
(KITTI 192x640 B=12 S=3, Waymo 320x480 B=8 S=3, nuScenes 288x512 B=16 S=4), where the CPU oracle would take minutes:
identity warp reproduces the source frames and the identity loss, gradients are linear in the loss weight (bit-exact),
every output is run-to-run deterministic, and batch items are independent.  GPU only."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import photo_case as pc

pytestmark = pytest.mark.gpu

SHAPES = [("fine_tune", 12, 192, 640, [0, 1, 2]), ("mask_init", 8, 320, 480, [0, 1, 2]), ("disp_init", 16, 288, 512, [0, 1, 2, 3])]


def make_case(phase, B, H, W, scales, seed=4):
    case = pc.Case(phase, B, H, W, scales, seed=seed)
    case.outputs = pc.synth.leaves_to_outputs(case.leaves, case.scales, pc.orc.pose_matrix, case.cmpflow, case.motmask)
    return case


def launch(case, args):
    from hipops import lib as L
    L.check(L.load().dd_photo_loss(C.byref(args), L.current_stream()), "dd_photo_loss")
    torch.cuda.synchronize()


def grads_of(t):
    out = [g.clone() for g in t["g_T"]]
    for d in t["scales"]:
        out.append(d["g_disp"].clone())
        for key in ("g_flow", "g_mask"):
            out += [g.clone() for g in d.get(key, [])]
    return out


def torch_ssim_l1(x, y, alpha=0.85):
    xp, yp = F.pad(x, (1, 1, 1, 1), mode="reflect"), F.pad(y, (1, 1, 1, 1), mode="reflect")
    mx, my = F.avg_pool2d(xp, 3, 1), F.avg_pool2d(yp, 3, 1)
    sx, sy = F.avg_pool2d(xp * xp, 3, 1) - mx * mx, F.avg_pool2d(yp * yp, 3, 1) - my * my
    sxy = F.avg_pool2d(xp * yp, 3, 1) - mx * my
    ssim = torch.clamp((1 - (2 * mx * my + 1e-4) * (2 * sxy + 9e-4) / ((mx * mx + my * my + 1e-4) * (sx + sy + 9e-4))) / 2, 0, 1)
    return alpha * ssim.mean(1, True) + (1 - alpha) * (y - x).abs().mean(1, True)


@pytest.mark.parametrize("phase,B,H,W,scales", SHAPES)
def test_identity_warp_reproduces_sources_and_identity_loss(phase, B, H, W, scales):
    case = make_case(phase, B, H, W, scales)
    eye = torch.eye(4).repeat(B, 1, 1)
    for f in (-1, 1):
        case.outputs[("cam_T_cam", 0, f)] = eye.clone()
        for s in scales:
            if ("complete_flow", f, s) in case.outputs:
                case.outputs[("complete_flow", f, s)] = torch.zeros_like(case.outputs[("complete_flow", f, s)])
    if case.automask:
        case.noise = {s: torch.zeros(B, 2, H, W) for s in scales}
    args, t = case.photo_buffers("cuda", materialise=True, want_grad=True)
    launch(case, args)
    tgt = t["target"]
    for si, s in enumerate(scales):
        d = t["scales"][si]
        for fi in range(2):
            # K @ inv_K is the identity only to fp32 rounding: samples land within ~1e-4 px of the pixel centres
            assert (d["out_color"][fi] - t["source"][fi]).abs().max().item() < 2e-3
        rho = torch.cat([torch_ssim_l1(t["source"][fi], tgt) for fi in range(2)], 1).min(1)[0]
        want = rho.mean().item()           # automask adds identity candidates that equal the warped ones here
        got = t["sums"][si, 0].item() / (B * H * W)
        assert abs(got - want) < 2e-4 * max(want, 1e-3), (s, got, want)


@pytest.mark.parametrize("phase,B,H,W,scales", SHAPES)
def test_gradients_are_linear_in_the_weight_and_deterministic(phase, B, H, W, scales):
    case = make_case(phase, B, H, W, scales)
    args, t = case.photo_buffers("cuda", materialise=False, want_grad=True)
    launch(case, args)
    ref, sums = grads_of(t), t["sums"].clone()
    assert all(torch.isfinite(g).all() for g in ref) and sum(float(g.abs().sum()) for g in ref) > 0
    # run-to-run determinism: fixed-order reductions, no float atomics anywhere in the photometric path
    for g in t["g_T"]:
        g.zero_()
    for d in t["scales"]:
        for key in ("g_disp",):
            d[key].zero_()
        for key in ("g_flow", "g_mask"):
            for g in d.get(key, []):
                g.zero_()
    launch(case, args)
    again = grads_of(t)
    assert torch.equal(sums, t["sums"])
    for a, b in zip(ref, again):
        assert torch.equal(a, b)
    # doubling every weight doubles every gradient bit-exactly (the weights enter as one final factor of two)
    for si in range(len(scales)):
        args.scale[si].w_photo *= 2
        args.scale[si].w_cons *= 2
    launch(case, args)
    for a, b in zip(ref, grads_of(t)):
        assert torch.equal(2 * a, b)


def test_batch_items_are_independent():
    phase, B, H, W, scales = "fine_tune", 6, 192, 640, [0, 1, 2]
    case = make_case(phase, B, H, W, scales)
    args, t = case.photo_buffers("cuda", materialise=False, want_grad=True)
    launch(case, args)
    full = [g.clone() for g in grads_of(t)]
    perm = torch.tensor([3, 0, 5, 1, 4, 2])
    case2 = make_case(phase, B, H, W, scales)
    for k, v in case2.inputs.items():
        if torch.is_tensor(v) and v.shape[:1] == (B,):
            case2.inputs[k] = v[perm].contiguous()
    for k, v in case2.outputs.items():
        if torch.is_tensor(v) and v.shape[:1] == (B,):
            case2.outputs[k] = v.detach()[perm].contiguous()
    args2, t2 = case2.photo_buffers("cuda", materialise=False, want_grad=True)
    launch(case2, args2)
    for a, b in zip(full, grads_of(t2)):
        assert torch.equal(a[perm.to(a.device)], b)


@pytest.mark.parametrize("phase", ["disp_init", "fine_tune"])
def test_part_calls_equal_the_whole_call(phase):
    """dd_photo_loss_part 1 then 2 (the tile kernel, then combine + finalize: the TILE_CUT branch of the split pipeline) issues the
    launches of dd_photo_loss in the same order: sums and gradients are equal bit for bit.  4 x 3 tiles, every scale shift; the rigid
    case with automask and the flow-plus-mask case.  part = 3 is refused before anything is launched."""
    from hipops import lib as L
    case = make_case(phase, 2, 64, 96, [0, 1, 2, 3], seed=7)                 # = pc.Case(phase, 2, 64, 96, [0, 1, 2, 3]) with its outputs
    args, t = case.photo_buffers("cuda", materialise=False, want_grad=True)
    launch(case, args)
    ref, sums = grads_of(t), t["sums"].clone()
    assert all(torch.isfinite(g).all() for g in ref) and sum(float(g.abs().sum()) for g in ref) > 0
    for g in t["g_T"]:
        g.zero_()
    for d in t["scales"]:
        d["g_disp"].zero_()
        for key in ("g_flow", "g_mask"):
            for g in d.get(key, []):
                g.zero_()
    t["sums"].zero_()
    lib = L.load()
    for part in (1, 2):
        L.check(lib.dd_photo_loss_part(C.byref(args), L.current_stream(), part), "dd_photo_loss_part %d" % part)
    torch.cuda.synchronize()
    assert lib.dd_photo_loss_part(C.byref(args), L.current_stream(), 3) != 0
    torch.cuda.synchronize()
    assert torch.equal(sums, t["sums"])
    for a, b in zip(ref, grads_of(t)):
        assert torch.equal(a, b)
