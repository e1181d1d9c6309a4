"""dd_motion_pr vs the reference-structured torch scan (eval/motion_segmentation.py:52-95 of the reference: interpolate, `> thrds`
broadcast to (B, 150, H, W), three sums per sample) on the same device tensors, at the nuScenes and Waymo evaluation shapes.
Device-event times; the kernel's byte floor is its label bytes plus the low-resolution mask over the HBM peak.

    python scripts/time_motion_pr.py [--out profiles/motion_pr_timing.txt]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dynamo-depth_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from tools import MotionSegMetrics  # noqa: E402

HBM_PEAK = 8e12                     # bytes/s
SHAPES = (("nuScenes", 16, 288, 512, 900, 1600, 0), ("Waymo", 12, 320, 480, 1280, 1920, 29))


def torch_scan(pred, mot, thrds, record, whole):
    """The reference's loop body for one batch; `whole` = the (B, T, H, W) broadcast in one go as the reference does, else per sample."""
    H, W = mot.shape[1:]
    th = thrds.reshape(1, -1, 1, 1)
    gt = mot.unsqueeze(1)
    gm_all, vm_all = gt == 1, (gt != 3).int()
    up = F.interpolate(pred, (H, W), mode="bilinear", align_corners=False)
    pm_all = (up > th) if whole else None
    for b in range(pred.shape[0]):
        vm, gm = vm_all[b], gm_all[b]
        pm = pm_all[b] if whole else (up[b:b + 1] > th)[0]
        tp = torch.logical_and(gm, pm).sum((1, 2))
        record["tp"] += tp
        record["fp"] += (pm * vm).sum((1, 2)) - tp
        record["fn"] += gm.sum((1, 2)) - tp


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3          # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_motion_pr.py measures on the GPU"
    lines = ["dd_motion_pr vs the reference-structured torch scan, same device tensors, device-event times ({})".format(torch.cuda.get_device_name(0))]
    for name, B, h, w, H, W, num_sem in SHAPES:
        g = torch.Generator().manual_seed(0)
        blobs = torch.sigmoid(6 * F.interpolate(torch.randn(B, 1, h // 16, w // 16, generator=g), (h, w), mode="bilinear", align_corners=False) - 7)
        masks = {"trained-like mask (near 0, a few moving blobs)": blobs, "uniform noise (every wave spread over the bins)": torch.rand(B, 1, h, w, generator=g)}
        mot = torch.randint(0, 4, (B, H, W), generator=g, dtype=torch.uint8).cuda()
        sem = torch.randint(0, 29, (B, H, W), generator=g, dtype=torch.uint8).cuda() if num_sem else None
        floor_us = (B * H * W * (2 if num_sem else 1) + B * h * w * 4) / HBM_PEAK * 1e6
        lines.append("")
        lines.append("{}: {}x{} -> {}x{}, B = {}, num_sem = {}; byte floor {:.1f} us (labels {:.1f} MB + mask {:.1f} MB at 8 TB/s)".format(
            name, h, w, H, W, B, num_sem, floor_us, B * H * W * (2 if num_sem else 1) / 1e6, B * h * w * 4 / 1e6))
        for what, pred in masks.items():
            pred = pred.cuda()
            m = MotionSegMetrics(num_thrd=150, num_sem=num_sem)
            m.update(pred, mot, sem)
            thrds = m.thrds
            record = {k: torch.zeros(150, device="cuda") for k in ("tp", "fp", "fn")}
            whole = True
            try:
                torch_scan(pred, mot, thrds, record, True)
                torch.cuda.synchronize()
            except torch.OutOfMemoryError:
                whole = False
                torch.cuda.empty_cache()
            for k in record:
                record[k].zero_()
            t_scan = timed(lambda: torch_scan(pred, mot, thrds, record, whole), 2, 5)
            t_kernel = timed(lambda: m.update(pred, mot, sem), 5, 50)
            lines.append("  {}".format(what))
            lines.append("    torch scan ({}; tp/fp/fn only, no false-positive tally)  {:10.1f} us per batch".format(
                "one (B,150,H,W) broadcast" if whole else "per sample", t_scan))
            lines.append("    dd_motion_pr ({} histogram rows)                          {:10.1f} us per batch = {:.1f} x its byte floor ({:.0f} % of it), {:.0f} x faster".format(
                2 + num_sem, t_kernel, t_kernel / floor_us, 100 * floor_us / t_kernel, t_scan / t_kernel))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
