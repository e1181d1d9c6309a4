"""dd_export_depth at 192x640 -> 1280x1920, B = 4, all three outputs, beside the torch-operator restatement of the same outputs
(F.interpolate of the scaled and of the raw disparity, reciprocal, scale, round, clamp, cast, colour-table lookup) on the same
tensors: both warmed, timed with device events in alternating windows, with the kernel's store bytes (13 B per output pixel) over
its time.  Needs a GPU; prints one text block (-> profiles/export_depth_timing.txt) and the largest difference between the paths.

    python scripts/time_export.py [--B 4] [--h 192 --w 640] [--H 1280 --W 1920] [--iters 200] [--rounds 5]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dynamo-depth_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from hipops import export as E  # noqa: E402


def torch_chain(disp, lut_rgb, H, W, lo, span, depth_scale):
    """The same three outputs from torch operators."""
    d_up = F.interpolate(disp, (H, W), mode="bilinear", align_corners=False)
    u = F.interpolate(lo + span * disp, (H, W), mode="bilinear", align_corners=False)
    depth = 1.0 / u
    depth16 = torch.round(depth * depth_scale).clamp(0, 65535).to(torch.int32)          # (no uint16 arithmetic in torch: the cast to 16 bits is one pass more)
    idx = (d_up * 256.0).clamp(0, 255).to(torch.int64)
    rgb = lut_rgb[idx[:, 0]]
    return depth[:, 0], depth16[:, 0].to(torch.int16), rgb          # the 16 bits of the unsigned value


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
    for name, default in (("B", 4), ("h", 192), ("w", 640), ("H", 1280), ("W", 1920), ("iters", 200), ("rounds", 5)):
        ap.add_argument("--" + name, type=int, default=default)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("time_export.py measures on a GPU; none is visible")
    torch.manual_seed(0)
    disp = torch.rand(a.B, 1, a.h, a.w, device="cuda")
    flipped = torch.rand(a.B, 1, a.h, a.w, device="cuda")
    lut_rgb = torch.from_numpy(E.cmap_bytes("plasma")).cuda()
    lo, span = (float(v) for v in E.depth_params(0.1, 100.0))
    want = ("depth", "depth16", "rgb")
    paths = {
        "dd_export_depth": lambda: E.export_depth(disp, a.H, a.W, min_depth=0.1, max_depth=100.0, want=want),
        "dd_export_depth, post-processing": lambda: E.export_depth(disp, a.H, a.W, disp_flipped=flipped, min_depth=0.1, max_depth=100.0, want=want),
        "dd_export_depth, depth16 only": lambda: E.export_depth(disp, a.H, a.W, min_depth=0.1, max_depth=100.0, want=("depth16",)),
        "torch operators": lambda: torch_chain(disp, lut_rgb, a.H, a.W, lo, span, 256.0),
    }
    for fn in paths.values():                               # warm-up: code objects, the caching allocator's blocks
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in paths}
    for _ in range(a.rounds):                               # alternating windows
        for name, fn in paths.items():
            times[name].append(window(fn, a.iters))
    got, ref = paths["dd_export_depth"](), paths["torch operators"]()
    torch.cuda.synchronize()
    pixels = a.B * a.H * a.W
    print("depth export, B = {} {}x{} -> {}x{}, {} calls per window, {} alternating windows (median; min .. max), device events".format(
        a.B, a.h, a.w, a.H, a.W, a.iters, a.rounds))
    for name, t in times.items():
        t = sorted(t)
        med = t[len(t) // 2]
        line = "  {:34s} {:8.1f} us  ({:.1f} .. {:.1f})".format(name, med, t[0], t[-1])
        if name.startswith("dd_export_depth"):
            per = 2 if "only" in name else 13
            line += "   {} B/pixel stored = {:.1f} MB -> {:.2f} TB/s".format(per, per * pixels / 1e6, per * pixels / med / 1e6)
        print(line)
    rel = ((got["depth"] - ref[0]).abs() / ref[0]).max().item()
    d16 = int(np.abs(got["depth16"].cpu().numpy().astype(np.int64) - ref[1].cpu().numpy().view(np.uint16).astype(np.int64)).max())
    rgb = (got["rgb"] != ref[2]).any(-1).float().mean().item()
    print("  kernel against the operator chain: depth within {:.2e} relative, depth16 within {} levels, {:.4%} of the colour pixels differ".format(rel, d16, rgb))


if __name__ == "__main__":
    main()
