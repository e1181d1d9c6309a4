"""dd_export_cloud at 12 x (192x640 -> 375x1242), stride 1, beside the torch-operator restatement of the same cloud (F.interpolate of
the scaled disparity, the colours and the mask, reciprocal, back-projection, the three masks, nonzero, gathers, stack) on the same
tensors: both warmed, timed with device events in alternating windows.  Also runs the wrapper once under
torch.cuda.set_sync_debug_mode("error"): a host synchronisation inside it would raise.  Needs a GPU; prints one text block
(-> profiles/cloud_timing.txt).

    python scripts/time_cloud.py [--B 12] [--h 192 --w 640] [--H 375 --W 1242] [--stride 1] [--iters 100] [--rounds 5]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dynamo-depth_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from hipops import cloud as C  # noqa: E402
from hipops.export import depth_params  # noqa: E402


def taps(out_size, in_size, device):
    """The upper-left tap index of every destination index (dm_tap's i0)."""
    src = ((torch.arange(out_size, device=device, dtype=torch.float32) + 0.5) * (in_size / out_size) - 0.5).clamp_(min=0)
    return src.to(torch.int64).clamp_(max=in_size - 1)


def torch_chain(disp, color, mask, pose, H, W, cam, lo, span, max_range, edge, thresh, y0, x0, X, Y):
    """The same cloud from torch operators: (records (n,16) uint8, counts (B,))."""
    s = lo + span * disp
    depth = 1.0 / F.interpolate(s, (H, W), mode="bilinear", align_corners=False)[:, 0]
    rgb = (F.interpolate(color, (H, W), mode="bilinear", align_corners=False).clamp(0, 1) * 255).to(torch.uint8)
    m = F.interpolate(mask, (H, W), mode="bilinear", align_corners=False)[:, 0]
    sp = F.pad(s, (0, 1, 0, 1), mode="replicate")
    smax, smin = F.max_pool2d(sp, 2, 1)[:, 0], -F.max_pool2d(-sp, 2, 1)[:, 0]
    spread = (smax - smin <= edge * smin)[:, y0][:, :, x0]
    keep = (depth > 0) & (depth <= max_range) & spread & (m < thresh)
    b, yy, xx = torch.nonzero(keep, as_tuple=True)                  # the host waits here
    z = depth[b, yy, xx]
    x, y = (X[xx] - cam[2]) / cam[0] * z, (Y[yy] - cam[3]) / cam[1] * z
    T = pose[b]
    p = torch.stack([T[:, k, 0] * x + T[:, k, 1] * y + T[:, k, 2] * z + T[:, k, 3] for k in range(3)], dim=1)
    rgba = torch.cat([rgb[b, :, yy, xx], torch.full_like(b, 255, dtype=torch.uint8)[:, None]], dim=1)
    return torch.cat([p.contiguous().view(torch.uint8), rgba], dim=1), torch.bincount(b, minlength=disp.shape[0])


def window(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / iters            # us per call


def main(argv=None):
    ap = argparse.ArgumentParser()
    for name, default in (("B", 12), ("h", 192), ("w", 640), ("H", 375), ("W", 1242), ("stride", 1), ("iters", 100), ("rounds", 5)):
        ap.add_argument("--" + name, type=int, default=default)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("time_cloud.py measures on a GPU; none is visible")
    torch.manual_seed(0)
    dev = "cuda"
    # a smooth disparity with a few steps, so that the edge rule keeps most pixels and drops some, as on a real frame
    ramp = torch.linspace(0.02, 0.4, a.h, device=dev)[None, None, :, None] + 0.002 * torch.rand(a.B, 1, a.h, a.w, device=dev)
    disp = ramp + 0.2 * (torch.rand(a.B, 1, a.h // 16, a.w // 16, device=dev) > 0.8).float().repeat_interleave(16, 2).repeat_interleave(16, 3)
    flipped = torch.flip(disp, [3]) + 0.002 * torch.rand_like(disp)
    color = torch.rand(a.B, 3, a.h, a.w, device=dev)
    mask = (torch.rand(a.B, 1, a.h // 8, a.w // 8, device=dev) > 0.9).float().repeat_interleave(8, 2).repeat_interleave(8, 3)
    pose = torch.eye(4, device=dev)[None, :3].repeat(a.B, 1, 1).contiguous()
    pose[:, :, 3] = torch.randn(a.B, 3, device=dev)
    cam = (0.58 * a.W, 1.92 * a.H, 0.5 * a.W, 0.5 * a.H)
    lo, span = (float(v) for v in depth_params(0.1, 100.0))
    kw = dict(min_depth=0.1, max_depth=100.0, max_range=80.0, edge=0.05, motion_thresh=0.5, stride=a.stride)
    y0, x0 = taps(a.H, a.h, dev), taps(a.W, a.w, dev)
    X, Y = torch.arange(a.W, device=dev, dtype=torch.float32), torch.arange(a.H, device=dev, dtype=torch.float32)
    paths = {
        "dd_export_cloud": lambda: C.export_cloud(disp, color, a.H, a.W, cam, **kw),
        "dd_export_cloud, mask and pose": lambda: C.export_cloud(disp, color, a.H, a.W, cam, motion_mask=mask, pose=pose, **kw),
        "dd_export_cloud, mask, pose, post-processing": lambda: C.export_cloud(disp, color, a.H, a.W, cam, motion_mask=mask, pose=pose, disp_flipped=flipped, **kw),
    }
    if a.stride == 1:
        paths["torch operators, mask and pose"] = lambda: torch_chain(disp, color, mask, pose, a.H, a.W, cam, lo, span, 80.0, 0.05, 0.5, y0, x0, X, Y)
    for fn in paths.values():                               # warm-up: code objects, the caching allocator's blocks
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in paths}
    for _ in range(a.rounds):                               # alternating windows
        for name, fn in paths.items():
            times[name].append(window(fn, a.iters))
    torch.cuda.set_sync_debug_mode("error")
    try:
        records, offsets = paths["dd_export_cloud, mask and pose"]()
        sync = "no host synchronisation in the wrapper (torch.cuda.set_sync_debug_mode('error') stayed silent)"
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    n = int(offsets[-1])
    cand = C.candidates(a.B, a.H, a.W, a.stride)
    print("point clouds, B = {} {}x{} -> {}x{}, stride {}: {} candidates, {} kept with mask and pose ({:.1%}); {} calls per window, {} alternating "
          "windows (median; min .. max), device events".format(a.B, a.h, a.w, a.H, a.W, a.stride, cand, n, n / cand, a.iters, a.rounds))
    for name, t in times.items():
        t = sorted(t)
        print("  {:46s} {:8.1f} us  ({:.1f} .. {:.1f})".format(name, t[len(t) // 2], t[0], t[-1]))
    print("  " + sync)
    if a.stride == 1:
        ref, counts = paths["torch operators, mask and pose"]()
        got_counts = (offsets[1:] - offsets[:-1]).cpu().numpy()
        print("  kernel against the operator chain: {} against {} points ({} frames of {} with another count: ATen's GPU bilinear rounds "
              "differently at the rules' bounds)".format(n, ref.shape[0], int((got_counts != counts.cpu().numpy()).sum()), a.B))
        if ref.shape[0] == n:
            gx, rx = C.unpack_records(records[:n].cpu().numpy())[0], C.unpack_records(ref.cpu().numpy())[0]
            print("  same count: coordinates within {:.2e} of each other".format(float(np.abs(gx - rx).max())))


if __name__ == "__main__":
    main()
