"""dd_lidar_depth_points at the KITTI preparation shape (16 scans x 2 cameras, 375x1242, tiny_kitti's calibration) on seeded 64-beam
scans of 121 600 points: the call's time per batch (device events) against its byte floor -- the words it initialises and reads back,
the values it writes and reads, the points and the rows, over the HBM peak -- and beside the wall time of the numpy definition
(hipops.lidar.depth_points_host) for the same batch on this machine's CPU, plus what the device path adds: the copies in and out.

    python scripts/time_lidar_depth.py [--out profiles/lidar_depth_timing.txt]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dynamo-depth_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from hipops import lidar  # noqa: E402

HBM_PEAK = 8e12                     # bytes/s, as scripts/time_motion_pr.py
S, C = 16, 2
BEAMS, STEPS = 64, 1900             # one revolution: 121 600 returns before the range cut


def scan(seed):
    """A full revolution over a ground plane with walls ahead, behind and to both sides, 2 cm of range noise."""
    rng = np.random.default_rng(seed)
    el = np.deg2rad(np.linspace(2.0, -24.8, BEAMS))[:, None]
    az = np.deg2rad(np.linspace(-180.0, 180.0, STEPS, endpoint=False))[None, :] + rng.uniform(0, 1e-3)
    ray = np.stack(np.broadcast_arrays(np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el) + 0 * az), axis=-1).reshape(-1, 3)
    with np.errstate(divide="ignore"):
        ground = np.where(ray[:, 2] < 0, -1.73 / ray[:, 2], np.inf)
        walls = np.minimum(rng.uniform(15, 40) / np.abs(ray[:, 0]), rng.uniform(8, 20) / np.abs(ray[:, 1]))
    rng_m = np.minimum(np.minimum(ground, walls), 120.0) + rng.normal(0.0, 0.02, ray.shape[0])
    return np.concatenate([ray * rng_m[:, None], rng.uniform(0, 1, (ray.shape[0], 1))], axis=1).astype(np.float32)


def windows(fn, warmup, iters, repeats):
    """us per call: the median and the extremes over `repeats` device-event windows of `iters` calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    got = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        got.append(a.elapsed_time(b) / iters * 1e3)
    return statistics.median(got), min(got), max(got)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_lidar_depth.py measures on the GPU"
    with np.load(os.path.join(ROOT, "tests", "golden", "kitti_prepare.npz")) as z:
        P, (H, W) = np.array(z["real_calib/P"]), (int(v) for v in z["real_calib/HW"])
    scans = [scan(1000 + s) for s in range(S)]
    offsets = np.concatenate([[0], np.cumsum([s.shape[0] for s in scans])]).astype(np.int64)
    n_total = int(offsets[-1])

    t0 = time.perf_counter()
    host = [[lidar.depth_points_host(s, P[c], H, W)[0] for c in range(C)] for s in scans]
    t_host = time.perf_counter() - t0
    n_rows = sum(r.shape[0] for job in host for r in job)

    stacked = torch.from_numpy(np.concatenate(scans))
    points, dP = stacked.cuda(), torch.from_numpy(P).cuda()
    rows, counts = lidar.depth_points(points, offsets, dP, H, W)
    jobs = lidar.split_rows(rows, counts, offsets)
    assert all(np.array_equal(jobs[s][c], host[s][c]) for s in range(S) for c in range(C)), "the device rows differ from the host definition"
    t_call = windows(lambda: lidar.depth_points(points, offsets, dP, H, W), 10, 50, 7)
    t_maps = windows(lambda: lidar.depth_points(points, offsets, dP, H, W, return_maps=True), 10, 50, 7)
    pinned = stacked.pin_memory()
    t_in = windows(lambda: points.copy_(pinned, non_blocking=True), 5, 50, 5)
    back = torch.empty(rows.shape, dtype=rows.dtype).pin_memory()
    t_out = windows(lambda: back.copy_(rows, non_blocking=True), 5, 20, 5)

    hw, nb = H * W, H * (W - 1) + 1
    words = S * C * (hw + 3 * nb) * 4
    values = S * C * hw * 4
    floor_bytes = 2 * words + 2 * values + n_total * 16 + n_rows * 24
    floor_us = floor_bytes / HBM_PEAK * 1e6
    lines = [
        "dd_lidar_depth_points at the KITTI preparation shape, device-event times ({})".format(torch.cuda.get_device_name(0)),
        "{} scans x {} cameras at {}x{}; {} points per scan ({} with x >= 0 on average), {} rows per job on average".format(
            S, C, H, W, scans[0].shape[0], int(np.mean([(s[:, 0] >= 0).sum() for s in scans])), n_rows // (S * C)),
        "median (min .. max) over 7 windows of 50 calls after 10 warm-up calls; workspace allocation through the caching allocator included",
        "",
        "  hipops.lidar.depth_points                  {:10.1f} us per batch ({:.1f} .. {:.1f}) = {:.1f} x its byte floor of {:.1f} us".format(
            t_call[0], t_call[1], t_call[2], t_call[0] / floor_us, floor_us),
        "      floor: {:.1f} MB of pixel and bucket words set and read back, {:.1f} MB of values written and read, {:.1f} MB of points, {:.1f} MB of rows, at 8 TB/s".format(
            2 * words / 1e6, 2 * values / 1e6, n_total * 16 / 1e6, n_rows * 24 / 1e6),
        "  ... with the dense (S, C, H, W) maps       {:10.1f} us per batch ({:.1f} .. {:.1f})".format(*t_maps),
        "what it replaces:",
        "  numpy definition on the host (depth_points_host), {} jobs   {:10.1f} ms per batch of one core's wall time = {:.1f} ms per job".format(
            S * C, t_host * 1e3, t_host * 1e3 / (S * C)),
        "what it adds:",
        "  host-to-device copy of the points ({:.1f} MB, pinned)        {:10.1f} us per batch ({:.1f} .. {:.1f})".format(n_total * 16 / 1e6, *t_in),
        "  device-to-host copy of the whole rows buffer ({:.1f} MB)    {:10.1f} us per batch ({:.1f} .. {:.1f})".format(rows.numel() * 8 / 1e6, *t_out),
    ]
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
