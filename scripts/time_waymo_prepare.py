"""The batch kernels of the Waymo preparation at its shapes, device-event times against their byte floors: dd_undistort and
dd_resize_area at 16 frames of 1920x1280 (-> 480x320) and dd_range_image_points at 16 frames' range images (one 64x2650 with a
per-pixel pose and four 200x600 each: 80 images, 10.4 M pixels), DESIGN 4.23.  Each call is checked against its numpy definition on
(a part of) the timed inputs first.  Beside them the host work the script does per frame (zlib inflate of the range images, Pillow's
two JPEG encodes), timed on one thread, to say what share of a batch the kernels take.

    python scripts/time_waymo_prepare.py [--out profiles/waymo_prepare_timing.txt]"""
import argparse
import io
import os
import statistics
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dynamo-depth_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402
from hipops import lidar, resize, undistort  # noqa: E402

HBM_PEAK = 8e12                     # bytes/s, as scripts/time_lidar_depth.py
N, H, W = 16, 1280, 1920
SHAPES = [(64, 2650)] + [(200, 600)] * 4
INTRINSIC = [2044.5083584358413, 2044.5083584358413, 949.5746451352071, 633.2422462156501, 0.040358363932006036, -0.33001662226602974,
             0.0010402702690110032, -0.0015669020781401406, 0.0]
CAM_EXTRINSIC = [0.9999943159291765, -0.0027625635198727494, 0.001932964597970193, 1.5386347086190375, 0.0027454768460688306, 0.9999576234529306,
                 0.008787130092066883, -0.024394341231793928, -0.0019571576906416434, -0.008781773235849106, 0.9999595241771579, 2.1150940771840068,
                 0.0, 0.0, 0.0, 1.0]
WORKERS = 8                         # the script's default --num_workers


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


def yaw_matrix(yaw, t):
    M = np.eye(4)
    M[:2, :2] = [[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]]
    M[:3, 3] = t
    return M


def frame_images(seed):
    """The five range images of one frame: a ground plane between walls seen from each laser, a third of the returns missing."""
    rng = np.random.default_rng(seed)
    frame_pose = yaw_matrix(0.3 + 0.01 * seed, [5.0e4 + 0.9 * seed, -3.0e4, 30.0])
    K = np.array([[INTRINSIC[0], 0, INTRINSIC[2]], [0, INTRINSIC[1], INTRINSIC[3]], [0, 0, 1.0]])
    e2c = lidar.vehicle_to_camera(CAM_EXTRINSIC)
    out = []
    for name, (h, w) in enumerate(SHAPES):
        extrinsic = yaw_matrix([-2.6, 0.0, 1.57, -1.57, 3.13][name], [1.43 - 0.4 * name, 0.0, 2.18 - 0.4 * name])
        incl = lidar.inclination_table(h, [], -0.31 if name == 0 else -1.5, 0.04 if name == 0 else 0.5)
        trig = lidar.range_image_trig(incl, w, extrinsic)
        with np.errstate(divide="ignore"):
            ground = np.where(trig[h:2 * h] < 0, -extrinsic[2, 3] / trig[h:2 * h], np.inf)[:, None]
        rho = (np.minimum(ground, rng.uniform(20.0, 75.0, size=(1, w))) + rng.normal(0.0, 0.02, size=(h, w))).astype(np.float32)
        rho[rng.uniform(size=(h, w)) < 0.33] = -1.0
        pose = None
        if name == 0:
            pose = np.zeros((h, w, 6), dtype=np.float32)
            pose[:, :, 2] = 0.3 + 0.01 * seed + rng.uniform(-1e-3, 1e-3, size=(h, w))
            pose[:, :, 3:] = frame_pose[:3, 3] + rng.uniform(-0.05, 0.05, size=(h, w, 3))
        cp = rng.integers(0, 1280, size=(h, w, 3)).astype(np.int32)
        out.append((rho, cp, pose, trig, lidar.range_image_params(extrinsic, frame_pose if name == 0 else None, e2c, K, W, H)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_waymo_prepare.py measures on the GPU"

    frames = np.random.default_rng(1).integers(0, 256, size=(N, H, W, 3), dtype=np.uint8)
    frames[:, ::2] //= 2                                              # not white noise throughout: rows of two brightnesses
    d_frames = torch.from_numpy(frames).cuda()
    flat = undistort.undistort_batch(d_frames, INTRINSIC)
    assert np.array_equal(flat[:1].cpu().numpy(), undistort.undistort_host(frames[:1], INTRINSIC)), "the device undistortion differs from the definition"
    t_undistort = windows(lambda: undistort.undistort_batch(d_frames, INTRINSIC), 5, 20, 7)
    t_resize = windows(lambda: resize.resize_area_batch(flat, H // 4, W // 4), 5, 20, 7)
    undistort_bytes, resize_bytes = 2 * frames.size, frames.size + frames.size // 16

    images = [im for seed in range(N) for im in frame_images(seed)]
    ranges, cps, poses, trigs, params = (list(c) for c in zip(*images))
    rng, cp, pose, trig, desc = lidar.range_image_pack(ranges, cps, poses, trigs)
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (rng, cp, pose, trig, np.stack(params))]
    points, cp_out, rows, counts = lidar.range_image_points_device(dev[0], dev[1], dev[2], dev[3], desc, dev[4])
    counts = counts.cpu().numpy()
    host, host_counts = lidar.range_image_points_host(ranges[:5], cps[:5], poses[:5], trigs[:5], np.stack(params[:5]))
    assert np.array_equal(counts[:5], host_counts), "the device counts differ from the host definition"
    bound = 64 * 2.0 ** -52 * (5.0e4 + 75.0)
    for s in range(5):
        a, n = int(desc[s, 0]), int(counts[s, 0])
        assert np.abs(points[a:a + n].cpu().numpy() - host[s][0]).max() <= bound, "the device points differ from the host definition"
        assert np.array_equal(cp_out[a:a + n].cpu().numpy(), host[s][1])
    t_points = windows(lambda: lidar.range_image_points_device(dev[0], dev[1], dev[2], dev[3], desc, dev[4]), 5, 20, 7)
    n_valid, n_kept = int(counts[:, 0].sum()), int(counts[:, 1].sum())
    points_bytes = rng.size * 4 + cp.size * 4 + pose.size * 4 + n_valid * (24 + 12) + n_kept * 24

    # the host's share of a frame, one thread: inflate of the three compressed matrices per laser, the two JPEG encodes
    packed = [zlib.compress(np.concatenate([im[0][:, :, None]] * 4, axis=2).tobytes()) for im in images[:5]]
    packed += [zlib.compress(np.concatenate([im[1]] * 2, axis=2).tobytes()) for im in images[:5]] + [zlib.compress(images[0][2].tobytes())]
    t0 = time.perf_counter()
    for blob in packed:
        zlib.decompress(blob)
    t_inflate = time.perf_counter() - t0
    photo = np.kron(np.random.default_rng(2).integers(0, 256, size=(H // 8, W // 8, 3), dtype=np.uint8), np.ones((8, 8, 1), dtype=np.uint8))
    photo = (photo.astype(np.int16) + np.random.default_rng(3).integers(-6, 7, size=photo.shape)).clip(0, 255).astype(np.uint8)
    t0 = time.perf_counter()
    for img in (photo, photo[::4, ::4]):
        Image.fromarray(np.ascontiguousarray(img)).save(io.BytesIO(), format="JPEG", quality=95)
    t_encode = time.perf_counter() - t0
    host_batch = N * (t_inflate + t_encode) / WORKERS * 1e6
    kernel_batch = t_undistort[0] + t_resize[0] + t_points[0]

    def line(name, t, nbytes, what):
        return "  {:40s} {:9.1f} us per batch ({:.1f} .. {:.1f}); {:.1f} MB must move ({}) = {:.2f} TB/s = {:.1f} % of the 8 TB/s HBM peak".format(
            name, t[0], t[1], t[2], nbytes / 1e6, what, nbytes / t[0] / 1e6, 100 * nbytes / (t[0] * 1e-6) / HBM_PEAK)
    lines = [
        "The batch kernels of the Waymo preparation, device-event times ({})".format(torch.cuda.get_device_name(0)),
        "median (min .. max) over 7 windows of 20 calls after 5 warm-up calls; output and workspace allocation through the caching allocator included",
        "first measurements: there is no earlier value of the two new kernels to compare with, and no time threshold is set",
        "",
        line("hipops.undistort.undistort_batch", t_undistort, undistort_bytes, "{} frames {}x{} read and written once".format(N, W, H)),
        line("hipops.resize.resize_area_batch", t_resize, resize_bytes, "the same frames read once, {}x{} written".format(W // 4, H // 4)),
        line("hipops.lidar.range_image_points_device", t_points, points_bytes,
             "{} images, {} pixels: range, projection triple and pose read once, {} points and triples, {} rows written".format(len(images), rng.size, n_valid, n_kept)),
        "  the range images are read by three of the five launches and the points again by the last; the floor counts every array once",
        "",
        "The host's part of one frame, one thread on this machine: inflating its 11 compressed matrices {:.1f} ms, Pillow's two JPEG encodes at quality 95 {:.1f} ms".format(
            t_inflate * 1e3, t_encode * 1e3),
        "  (protobuf parsing, JPEG decode of files the device refuses, contours and file writes not counted).  For a batch of {} frames on {} threads that is".format(N, WORKERS),
        "  {:.0f} us of host work against {:.0f} us in the three kernels: the kernels take {:.1f} % of a batch; the script's wall time is the host's".format(
            host_batch, kernel_batch, 100 * kernel_batch / (kernel_batch + host_batch)),
    ]
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
