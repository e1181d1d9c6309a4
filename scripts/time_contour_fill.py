"""dd_fill_contours at the Waymo evaluation shape (B = 12 masks of 1280x1920) on the tiny_waymo frame's contours, replicated: the
kernel's time per batch (device events) against its byte floor -- the mask bytes it writes plus the record bytes it reads, over the
HBM peak -- and beside what it replaces on the same machine: the numpy fill per sample in a loader worker and the host-to-device copy
of the filled (B, 1280, 1920) uint8 masks.

    python scripts/time_contour_fill.py [--out profiles/contour_fill_timing.txt]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dynamo-depth_amd"))
import torch  # noqa: E402
import datasets  # noqa: E402
from hipops import contours  # noqa: E402

HBM_PEAK = 8e12                     # bytes/s, as scripts/time_motion_pr.py
B, H, W = 12, 1280, 1920
DATA, FOLDER = os.path.join(ROOT, "tests", "golden", "tiny_waymo"), "val/segment-1024360143612057520_3580_000_3600_000"


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
    assert torch.cuda.is_available(), "time_contour_fill.py measures on the GPU"
    reader = datasets.WaymoDataset(data_path=DATA, filenames=[FOLDER + " 1"], height=320, width=480, cam_name="FRONT", img_type="downsample",
                                   frame_idxs=[0], num_scales=4)
    _, objects, _ = reader.get_mask_objects(FOLDER, 1, "l")
    vertices, records = contours.pack(objects, H, W)
    n_contours, n_vertices = int((records[:, 1] > 0).sum()), int(records[:, 1].sum())
    host_mask = contours.fill_host(objects, H, W)
    t0 = time.perf_counter()
    for _ in range(5):
        contours.fill_host(objects, H, W)
    t_host = (time.perf_counter() - t0) / 5 * 1e6

    dv = torch.from_numpy(vertices).cuda().unsqueeze(0).repeat(B, 1, 1).contiguous()
    dr = torch.from_numpy(records).cuda().unsqueeze(0).repeat(B, 1, 1).contiguous()
    out = torch.empty((B, H, W), dtype=torch.uint8, device="cuda")
    t_kernel = timed(lambda: contours.fill_contours(dv, dr, H, W, out=out), 10, 200)
    assert bool((out.cpu() == torch.from_numpy(host_mask)).all())
    empty = torch.zeros_like(dr)
    t_empty = timed(lambda: contours.fill_contours(dv, empty, H, W, out=out), 10, 200)
    assert not bool(out.any())

    masks = torch.from_numpy(host_mask).unsqueeze(0).repeat(B, 1, 1).contiguous()
    pinned = masks.pin_memory()
    t_copy_pinned = timed(lambda: out.copy_(pinned, non_blocking=True), 5, 50)
    t_copy_pageable = timed(lambda: out.copy_(masks), 3, 20)
    rec_host = (torch.from_numpy(vertices).unsqueeze(0).repeat(B, 1, 1).contiguous().pin_memory(), torch.from_numpy(records).unsqueeze(0).repeat(B, 1, 1).contiguous().pin_memory())
    t_copy_records = timed(lambda: (dv.copy_(rec_host[0], non_blocking=True), dr.copy_(rec_host[1], non_blocking=True)), 5, 50)

    used = n_vertices * 4 + n_contours * contours.REC_WORDS * 4
    floor_us = B * (H * W + used) / HBM_PEAK * 1e6
    lines = [
        "dd_fill_contours at the Waymo evaluation shape, device-event times ({})".format(torch.cuda.get_device_name(0)),
        "B = {} masks of {}x{}; per sample {} contours, {} vertices (the tiny_waymo frame); records as shipped {:.0f} KB per sample, {:.1f} KB of them used".format(
            B, H, W, n_contours, n_vertices, (vertices.nbytes + records.nbytes) / 1024, used / 1024),
        "",
        "  dd_fill_contours                                   {:10.1f} us per batch = {:.1f} x its byte floor of {:.1f} us ({:.1f} MB written + {:.2f} MB read at 8 TB/s; {:.0f} % of it)".format(
            t_kernel, t_kernel / floor_us, floor_us, B * H * W / 1e6, B * used / 1e6, 100 * floor_us / t_kernel),
        "  dd_fill_contours, samples without objects          {:10.1f} us per batch (the store path alone)".format(t_empty),
        "what it replaces:",
        "  numpy fill on the host (hipops.contours.fill_host) {:10.1f} us per SAMPLE = {:.1f} ms per batch of worker time".format(t_host, t_host * B / 1e3),
        "  host-to-device copy of the (B,{},{}) uint8 masks   {:10.1f} us per batch from pinned memory, {:.1f} us from pageable memory".format(H, W, t_copy_pinned, t_copy_pageable),
        "what it adds:",
        "  host-to-device copy of the records                 {:10.1f} us per batch from pinned memory".format(t_copy_records),
    ]
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
