"""KITTI preparation, launch-line compatible with the reference's prepare_data/kitti.py:

    python prepare_data/kitti.py <raw_dataset> <out_dataset> [--skip_rgb] [--skip_depth] [--height 192] [--width 640] [--batch 16] [--num_workers 8]

From a raw KITTI download (<raw>/<date>/{calib_*.txt, <drive>/{image_02,image_03}/data/*.png, <drive>/velodyne_points/data/*.bin}) to the
layout datasets/kitti_dataset.py reads, for every date that starts with 2011 and every drive of it:

    <out>/<date>/<drive>/calib_*.txt                                  links to the date's calibration files
    <out>/<date>/<drive>/image_0{2,3}/rgb/original/<frame>.png        links to the raw frames
    <out>/<date>/<drive>/image_0{2,3}/rgb/downsample/<frame>.jpg      height x width bicubic down-samples, skipped when they exist
    <out>/<date>/<drive>/image_0{2,3}/depth/<frame>.npy               float64 (n, 3) [row, column, depth] LiDAR lists, always rewritten

The down-samples go through hipops.resize.resize_batch in batches of equal source size (Pillow's bytes, bit for bit) and are saved by
Pillow; the depth lists go through hipops.lidar.depth_points, `--batch` scans and both cameras per launch.  One process:
a pool of at most 16 threads reads and writes files, the main thread launches.  `prepare` takes the two device steps as callables, so
the walk, the naming and the writing can be driven on the host (tests/test_kitti_prepare.py)."""
import argparse
import os
import os.path as osp
import sys
from concurrent.futures import ThreadPoolExecutor

proj_dir = osp.dirname(osp.dirname(osp.abspath(__file__)))      # prepare_data/ -> the package root
if proj_dir not in sys.path:
    sys.path.insert(0, proj_dir)

import numpy as np  # noqa: E402
from PIL import Image  # noqa: E402

from hipops import lidar  # noqa: E402

CAM_NAMES = ("image_02", "image_03")
MAX_THREADS = 16


def device_depth_rows(scans, mats, H, W):
    """out[s][c] = float64 (n, 3) rows of scan s through mats[c]: one dd_lidar_depth_points call for the whole batch."""
    import torch
    offsets = np.concatenate([[0], np.cumsum([s.shape[0] for s in scans])]).astype(np.int64)
    points = torch.from_numpy(np.ascontiguousarray(np.concatenate(scans, axis=0), dtype=np.float32)).cuda()
    rows, counts = lidar.depth_points(points, offsets, torch.from_numpy(np.ascontiguousarray(mats, dtype=np.float64)).cuda(), H, W)
    return lidar.split_rows(rows, counts, offsets)


def host_depth_rows(scans, mats, H, W):
    """The same from the numpy definition (tests; no GPU)."""
    return [[lidar.depth_points_host(s, P, H, W)[0] for P in mats] for s in scans]


def device_resize(frames, height, width):
    """frames (n, Hs, Ws, 3) uint8 -> (n, height, width, 3) uint8: Image.resize((width, height)) of every frame, on the device."""
    import torch

    from hipops import resize
    return resize.resize_batch(torch.from_numpy(frames).cuda(), height, width).cpu().numpy()


def link(src, dst):
    if not osp.lexists(dst):
        os.symlink(osp.realpath(src), dst)


def read_scan(path):
    return np.fromfile(path, dtype=np.float32).reshape(-1, 4)


def decode_png(path):
    """The frame as (H, W, 3) uint8, or None for a file that is not plain 8-bit RGB (it takes Pillow's own resize on the host)."""
    with Image.open(path) as img:
        if img.mode != "RGB" or "comment" in img.info:
            return None
        return np.asarray(img)


def host_downsample(src, dst, height, width):
    """The reference's line (prepare_data/kitti.py:101-102)."""
    Image.open(src).resize((width, height)).save(dst)


def frame_names(drive_dir, cam):
    return sorted(f.split(".")[0] for f in os.listdir(osp.join(drive_dir, cam, "data")) if f.endswith(".png"))


def chunks(items, size):
    return [items[i:i + size] for i in range(0, len(items), size)]


def prepare_rgb(pool, drive_dir, out_dir, height, width, batch, resize):
    """Links to the raw frames and the down-samples that do not exist yet, both cameras of one drive."""
    todo = []
    for cam in CAM_NAMES:
        for name in frame_names(drive_dir, cam):
            src = osp.join(drive_dir, cam, "data", name + ".png")
            link(src, osp.join(out_dir, cam, "rgb", "original", name + ".png"))
            dst = osp.join(out_dir, cam, "rgb", "downsample", name + ".jpg")
            if not osp.exists(dst):
                todo.append((src, dst))
    for part in chunks(todo, max(batch, 1) * len(CAM_NAMES)):
        frames = list(pool.map(decode_png, [src for src, _ in part]))
        by_size = {}
        for (src, dst), frame in zip(part, frames):
            if frame is None:
                host_downsample(src, dst, height, width)
            else:
                by_size.setdefault(frame.shape, []).append((dst, frame))
        for group in by_size.values():
            small = resize(np.stack([frame for _, frame in group]), height, width)
            list(pool.map(lambda job: Image.fromarray(job[1]).save(job[0]), [(dst, small[k]) for k, (dst, _) in enumerate(group)]))


def prepare_depth(pool, date_dir, drive_dir, out_dir, batch, depth_rows, log):
    """The LiDAR lists of one drive: every scan once, through both cameras' matrices."""
    mats, H, W = [], 0, 0
    for cam in CAM_NAMES:
        P, H, W = lidar.projection(date_dir, int(cam[-1]))
        mats.append(P)
    mats = np.stack(mats)
    wanted = {}                                                          # frame -> the cameras that have it
    for c, cam in enumerate(CAM_NAMES):
        for name in frame_names(drive_dir, cam):
            src = osp.join(drive_dir, "velodyne_points", "data", name + ".bin")
            if not osp.exists(src):
                log("Depth Data {} Not Found - Skipped".format(src))
                continue
            wanted.setdefault(name, []).append(c)
    for part in chunks(sorted(wanted), max(batch, 1)):
        scans = list(pool.map(read_scan, [osp.join(drive_dir, "velodyne_points", "data", name + ".bin") for name in part]))
        rows = depth_rows(scans, mats, H, W)
        jobs = [(osp.join(out_dir, CAM_NAMES[c], "depth", name + ".npy"), rows[s][c]) for s, name in enumerate(part) for c in wanted[name]]
        list(pool.map(lambda job: np.save(job[0], job[1]), jobs))


def prepare_drive(pool, date_dir, drive, out_date_dir, height, width, batch, skip_rgb, skip_depth, depth_rows, resize, log):
    drive_dir, out_dir = osp.join(date_dir, drive), osp.join(out_date_dir, drive)
    os.makedirs(out_dir, exist_ok=True)
    for txt in sorted(f for f in os.listdir(date_dir) if f.endswith(".txt")):
        link(osp.join(date_dir, txt), osp.join(out_dir, txt))
    for cam in CAM_NAMES:
        for sub in (("rgb", "original"), ("rgb", "downsample"), ("depth",)):
            os.makedirs(osp.join(out_dir, cam, *sub), exist_ok=True)
    if not skip_rgb:
        prepare_rgb(pool, drive_dir, out_dir, height, width, batch, resize)
    if not skip_depth:
        prepare_depth(pool, date_dir, drive_dir, out_dir, batch, depth_rows, log)


def prepare(raw_dataset, out_dataset, height=192, width=640, batch=16, num_workers=8, skip_rgb=False, skip_depth=False,
            depth_rows=device_depth_rows, resize=device_resize, log=print):
    """The whole tree.  depth_rows(scans, mats, H, W) -> out[s][c] rows and resize(frames, height, width) -> frames are the device
    steps by default."""
    os.makedirs(out_dataset, exist_ok=True)
    with ThreadPoolExecutor(max_workers=min(max(int(num_workers), 1), MAX_THREADS)) as pool:
        for date in sorted(f for f in os.listdir(raw_dataset) if f.startswith("2011")):
            date_dir = osp.join(raw_dataset, date)
            os.makedirs(osp.join(out_dataset, date), exist_ok=True)
            for drive in sorted(f for f in os.listdir(date_dir) if f.startswith(date)):
                log("Processing {} {}".format(date, drive))
                prepare_drive(pool, date_dir, drive, osp.join(out_dataset, date), height, width, batch, skip_rgb, skip_depth, depth_rows, resize, log)


def main(argv=None):
    ap = argparse.ArgumentParser(description="raw KITTI -> the processed layout of datasets/kitti_dataset.py")
    ap.add_argument("raw_dataset")
    ap.add_argument("out_dataset")
    ap.add_argument("--skip_rgb", action="store_true", help="no links to the raw frames, no down-samples")
    ap.add_argument("--skip_depth", action="store_true", help="no LiDAR lists")
    ap.add_argument("--height", type=int, default=192)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--batch", type=int, default=16, help="scans (and twice as many frames) per launch")
    ap.add_argument("--num_workers", type=int, default=8, help="file threads, at most {}".format(MAX_THREADS))
    args = ap.parse_args(argv)
    prepare(args.raw_dataset, args.out_dataset, height=args.height, width=args.width, batch=args.batch, num_workers=args.num_workers,
            skip_rgb=args.skip_rgb, skip_depth=args.skip_depth)


if __name__ == "__main__":
    main()
