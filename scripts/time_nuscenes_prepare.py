"""The two batch kernels of the nuScenes preparation at its shapes, device-event times against their byte floors:
dd_resize_area at 16 frames 1600x900 -> 512x288 and dd_lidar_pose_points at 16 scans of 34 720 points.  Each call is
checked against its numpy definition on the timed inputs first.

    python scripts/time_nuscenes_prepare.py [--out profiles/nuscenes_prepare_timing.txt]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dynamo-depth_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from hipops import lidar, resize  # noqa: E402

HBM_PEAK = 8e12                     # bytes/s, as scripts/time_lidar_depth.py
N, HS, WS, HD, WD = 16, 900, 1600, 288, 512
S, POINTS = 16, 34720
CAM_CS = {"translation": [1.70079118954, 0.0159456324149, 1.51095763913], "rotation": [0.4998015430569128, -0.5030316162024876, 0.4997798114386805, -0.49737083824542755]}
LIDAR_CS = {"translation": [0.943713, 0.0, 1.84023], "rotation": [0.7077955119163518, -0.006492242056004365, 0.010646214713995808, -0.7063073142877817]}
K = [[1266.417203046554, 0.0, 816.2670197447984], [0.0, 1266.417203046554, 491.50706579294757], [0.0, 0.0, 1.0]]


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


def scan(seed):
    """A 32-beam revolution over a ground plane between walls, in the sensor frame."""
    rng = np.random.default_rng(seed)
    el = np.deg2rad(np.linspace(10.0, -30.0, 32))[:, None]
    az = np.deg2rad(np.linspace(-180.0, 180.0, POINTS // 32, endpoint=False))[None, :]
    ray = np.stack(np.broadcast_arrays(np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el) + 0 * az), axis=-1).reshape(-1, 3)
    with np.errstate(divide="ignore"):
        ground = np.where(ray[:, 2] < 0, -1.84 / ray[:, 2], np.inf)
        walls = np.minimum(rng.uniform(15, 40) / np.abs(ray[:, 0]), rng.uniform(8, 20) / np.abs(ray[:, 1]))
    r = np.minimum(np.minimum(ground, walls), 100.0) + rng.normal(0.0, 0.02, ray.shape[0])
    return np.concatenate([ray * r[:, None], rng.uniform(0, 255, (ray.shape[0], 1))], axis=1).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_nuscenes_prepare.py measures on the GPU"

    frames = np.random.default_rng(1).integers(0, 256, size=(N, HS, WS, 3), dtype=np.uint8)
    d_frames = torch.from_numpy(frames).cuda()
    small = resize.resize_area_batch(d_frames, HD, WD).cpu().numpy()
    sums = resize.resize_area_sums(frames[:2], HD, WD)
    off = (small[:2] != np.clip(np.rint(sums), 0, 255).astype(np.uint8)) & (np.abs(sums - np.floor(sums) - 0.5) >= 1e-4)
    assert not off.any(), "the device down-sample differs from the definition"
    t_resize = windows(lambda: resize.resize_area_batch(d_frames, HD, WD), 10, 50, 7)
    resize_bytes = frames.size + small.size

    scans = [scan(100 + s) for s in range(S)]
    assert scans[0].shape[0] == POINTS
    params = []
    for s in range(S):
        yaw = 0.3 + 0.01 * s
        lidar_pose = {"translation": [1010.0 + 0.9 * s, 610.0 + 0.3 * s, 0.0], "rotation": [np.cos(yaw / 2), 0.0, 0.0, np.sin(yaw / 2)]}
        cam_pose = {"translation": [1010.0 + 0.9 * s + 0.04, 610.0 + 0.3 * s + 0.01, 0.0], "rotation": [np.cos(yaw / 2 + 1e-4), 0.0, 0.0, np.sin(yaw / 2 + 1e-4)]}
        params.append(lidar.pose_params(LIDAR_CS, lidar_pose, cam_pose, CAM_CS, K, WS, HS))
    offsets = np.concatenate([[0], np.cumsum([s.shape[0] for s in scans])]).astype(np.int64)
    points, d_params = torch.from_numpy(np.concatenate(scans)).cuda(), torch.from_numpy(np.stack(params)).cuda()
    rows, counts = lidar.pose_points(points, offsets, d_params)
    jobs = lidar.split_rows(rows, counts, offsets)
    host = [lidar.pose_points_host(scans[s], params[s])[0] for s in range(S)]
    assert all(np.array_equal(jobs[s][0], host[s]) for s in range(S)), "the device rows differ from the host definition"
    n_rows = sum(h.shape[0] for h in host)
    t_pose = windows(lambda: lidar.pose_points(points, offsets, d_params), 10, 50, 7)
    pose_bytes = 2 * points.numel() * 4 + n_rows * 48        # the points are read by both passes, the kept rows written once

    def line(name, t, nbytes, what):
        return "  {:34s} {:9.1f} us per batch ({:.1f} .. {:.1f}); {:.1f} MB moved ({}) = {:.2f} TB/s = {:.1f} % of the 8 TB/s HBM peak".format(
            name, t[0], t[1], t[2], nbytes / 1e6, what, nbytes / t[0] / 1e6, 100 * nbytes / (t[0] * 1e-6) / HBM_PEAK)
    lines = [
        "The batch kernels of the nuScenes preparation, device-event times ({})".format(torch.cuda.get_device_name(0)),
        "median (min .. max) over 7 windows of 50 calls after 10 warm-up calls; output and workspace allocation through the caching allocator included",
        "first measurements: there is no earlier value of either kernel to compare with",
        "",
        line("hipops.resize.resize_area_batch", t_resize, resize_bytes, "{} frames {}x{} read once, {}x{} written".format(N, WS, HS, WD, HD)),
        line("hipops.lidar.pose_points", t_pose, pose_bytes, "{} scans of {} points read twice, {} rows of 48 bytes written".format(S, POINTS, n_rows)),
        "  both inputs fit the 256 MiB Infinity Cache and are re-read from it by every timed call: the share of HBM peak is the byte floor over the time, not a measured HBM rate",
    ]
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
