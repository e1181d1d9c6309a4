"""Waymo preparation, launch-line compatible with the reference's prepare_data/waymo.py:

    python prepare_data/waymo.py <records dir> <dataset dir> [split_idx split_num] [--skip_rgb] [--skip_depth] [--skip_mask]
                                 [--segments segment-... ...] [--cams FRONT ...] [--batch 16] [--num_workers 8]

From the Waymo Open Dataset segments (<records dir>/{train,val}/segment-*_with_camera_labels.tfrecord) to the layout
datasets/waymo_dataset.py and the evaluation scripts read, for every split, segment and camera:

    <dataset dir>/<split>/<segment>/<cam>/rgb/original/%06d.jpg     the undistorted frame, quality 95
    <dataset dir>/<split>/<segment>/<cam>/rgb/downsample/%06d.jpg   its H/4 x W/4 area down-sample, quality 95
    <dataset dir>/<split>/<segment>/<cam>/rgb/cam.json              intrinsic, dim, extrinsic, intrinsic_mat
    <dataset dir>/<split>/<segment>/<cam>/depth/%06d.npy            float64 (n, 3) [u, v, depth] of the five lasers' first returns
    <dataset dir>/<split>/<segment>/<cam>/mask/%06d.{npz,pickle}    frames with a panoptic label: semantic, instance; the per-object dicts
    <dataset dir>/<split>/<segment>/<cam>/odometry.txt

No TensorFlow, no OpenCV, none of the Waymo utilities: the records are read by prepare_data/waymo_records.py (which needs the Waymo
package's dataset_pb2 and protobuf only), the frames are decoded by hipops.jpeg (Pillow for files its geometry check refuses),
undistorted by hipops.undistort and down-sampled by hipops.resize.resize_area_batch, the range images of `--batch` frames go through
hipops.lidar.range_image_points in one call and the labelled frames' boxes through hipops.lidar.box_fit; the objects' contours are
traced by hipops.contours.trace.  One process: a pool of at most 16 threads reads, inflates, encodes and writes, the
main thread launches.  `prepare` takes the device steps as callables, so the walk can be driven on the host
(tests/test_waymo_prepare.py)."""
import argparse
import json
import os
import os.path as osp
import pickle
import sys
from concurrent.futures import ThreadPoolExecutor

proj_dir = osp.dirname(osp.dirname(osp.abspath(__file__)))      # prepare_data/ -> the package root
if proj_dir not in sys.path:
    sys.path.insert(0, proj_dir)

import numpy as np  # noqa: E402

from hipops import contours, lidar  # noqa: E402
from prepare_data import waymo_records as wr  # noqa: E402
from prepare_data.common import MAX_THREADS, chunks, device_decode, device_resize, host_decode, host_resize, save_jpeg  # noqa: E402,F401

SPLITS = ("train", "val")
SEGMENTS_EXPECTED = {"train": 798, "val": 202}
DOWNSAMPLE_FACTOR = 4
MOVEABLE_CATEGORIES = {2: "car", 3: "truck", 4: "bus", 5: "other_vehicle", 6: "bicycle", 7: "motorcycle", 8: "trailer", 9: "pedestrian",
                       10: "bicyclist", 11: "motorcyclist", 12: "bird", 13: "ground_animal", 16: "pedestrian_object", 27: "dynamic"}


def host_undistort(frames, intrinsic):
    from hipops import undistort
    return undistort.undistort_host(np.stack([np.asarray(f) for f in frames]), intrinsic)


def device_undistort(frames, intrinsic):
    """Equal-sized frames (GPU tensors or host arrays) of one calibration -> (n, H, W, 3) uint8 on the GPU, one launch."""
    import torch

    from hipops import undistort
    stack = torch.stack([f if torch.is_tensor(f) else torch.from_numpy(np.ascontiguousarray(f)).cuda() for f in frames])
    return undistort.undistort_batch(stack, intrinsic)


def to_host(stack):
    return stack if isinstance(stack, np.ndarray) else stack.cpu().numpy()


def intrinsic_matrix(intrinsic):
    f_u, f_v, c_u, c_v = intrinsic[:4]
    K = np.eye(3)
    K[0, 0], K[0, 2], K[1, 1], K[1, 2] = f_u, c_u, f_v, c_v
    return K


def write_cam(path, intrinsic, extrinsic, dim):
    """cam.json of reference waymo.py:199-207: the intrinsic matrix with row 0 divided by the width and row 1 by the height."""
    K = intrinsic_matrix(intrinsic)
    K[0] /= dim[1]
    K[1] /= dim[0]
    with open(path, "w") as fh:
        json.dump({"intrinsic": list(intrinsic), "dim": list(dim), "extrinsic": list(extrinsic), "intrinsic_mat": K.tolist()}, fh)


def object_image(semantic, instance, labels=tuple(MOVEABLE_CATEGORIES)):
    """get_instance_masks of the reference as one image: (object index per pixel int32 (H, W), -1 where none; the objects' class
    labels).  Classes in `labels`' order; in class c the ids are (instance + 1) * (semantic == c), the + 1 in the stored dtype, and
    there is one object per i = 1 .. ids.max(), those without a pixel included."""
    sem, ins = np.asarray(semantic)[:, :, 0], np.asarray(instance)[:, :, 0]
    ids_all = (ins + 1).astype(np.int64)
    objects = np.full(sem.shape, -1, dtype=np.int32)
    obj_labels = []
    for c in labels:
        of_class = sem == c
        if of_class.any():
            ids = ids_all * of_class
            hit = ids > 0
            objects[hit] = len(obj_labels) + ids[hit] - 1
            obj_labels.extend([c] * int(ids.max()))
    return objects, obj_labels


def object_contours(objects, n_objects):
    """Per object the tuple of its contours (hipops.contours.trace on its bounding box)."""
    H, W = objects.shape
    pix = np.flatnonzero(objects.reshape(-1) >= 0)
    k, y, x = objects.reshape(-1)[pix], pix // W, pix % W
    lo_y, lo_x, hi_y, hi_x = np.full(n_objects, H), np.full(n_objects, W), np.full(n_objects, -1), np.full(n_objects, -1)
    np.minimum.at(lo_y, k, y), np.minimum.at(lo_x, k, x), np.maximum.at(hi_y, k, y), np.maximum.at(hi_x, k, x)
    out = []
    for o in range(n_objects):
        if hi_y[o] < 0:
            out.append(())
            continue
        found = contours.trace(objects[lo_y[o]:hi_y[o] + 1, lo_x[o]:hi_x[o] + 1] == o)
        out.append(tuple(c + np.array([lo_x[o], lo_y[o]], dtype=np.int32) for c in found))
    return out


def object_labels(semantic, instance, points, cp, cam_code, labels, fit):
    """Reference waymo.py:256-301 for one labelled frame: the list of per-object dicts.  points (n, 3) and cp (n, 3) [camera, x, y]
    of the frame's valid range pixels, labels the laser labels of `FrameArrays`."""
    objects, obj_labels = object_image(semantic, instance)
    H, W = objects.shape
    n_objects = len(obj_labels)
    seen = cp[:, 0] == cam_code
    visible, xy = points[seen], cp[seen][:, 1:3]
    point_of = np.full((H, W), -1, dtype=np.int64)                  # the last point that projects onto a pixel keeps it
    np.maximum.at(point_of, (xy[:, 1], xy[:, 0]), np.arange(xy.shape[0]))
    both = (point_of >= 0) & (objects >= 0)
    owner, index = objects[both], point_of[both]                    # row-major over the pixels
    order = np.argsort(owner, kind="stable")
    seg = np.concatenate([[0], np.cumsum(np.bincount(owner, minlength=n_objects))]).astype(np.int32)
    corners = np.array([lidar.upright_box_corners(l["box"]) for l in labels], dtype=np.float64).reshape(-1, 8, 3)
    best = np.full((n_objects, 2), -1)
    if n_objects:
        _, best = fit(visible[index[order]], seg, [0] * n_objects, lidar.box_params(corners), [0] * len(labels))
    outlines = object_contours(objects, n_objects)
    out = []
    for o in range(n_objects):
        b, count, size = int(best[o][0]), int(best[o][1]), int(seg[o + 1] - seg[o])
        entry = {"mask": outlines[o], "mask_label": obj_labels[o], "speed": [None] * 3, "accel": [None] * 3, "center": [None] * 3,
                 "dim": [None] * 3, "heading": None, "box_label": None, "match": 0}
        if b >= 0 and count > 0 and size > 0:
            l = labels[b]
            entry.update(speed=list(l["speed"]), accel=list(l["accel"]), center=list(l["box"][0:3]), dim=list(l["box"][3:6]), heading=l["box"][6],
                         box_label=l["type"], match=np.float64(count) / np.float64(size))
        out.append(entry)
    return out


def save_npy(job):
    np.save(job[0], job[1])


def save_mask(job):
    stem, semantic, instance, entries = job
    np.savez_compressed(stem + ".npz", semantic=semantic, instance=instance)
    with open(stem + ".pickle", "wb") as fh:
        pickle.dump(entries, fh)


def prepare_frames(pool, part, first, cam_dirs, cams, skip_rgb, skip_depth, skip_mask, steps):
    """One batch of FrameArrays, numbered from `first`."""
    for cam in cams:
        base = cam_dirs[cam]
        infos = [fa.cameras[cam] for fa in part]
        if first == 0 and not skip_rgb:
            write_cam(osp.join(base, "rgb", "cam.json"), infos[0]["intrinsic"], infos[0]["extrinsic"], [infos[0]["height"], infos[0]["width"]])
        if not skip_rgb:
            frames = steps["decode"]([info["image"] for info in infos])
            groups = {}
            for k, (info, frame) in enumerate(zip(infos, frames)):
                groups.setdefault((tuple(frame.shape), tuple(info["intrinsic"])), []).append(k)
            for (shape, intrinsic), members in groups.items():
                flat = steps["undistort"]([frames[k] for k in members], list(intrinsic))
                small = steps["resize"](list(flat), shape[0] // DOWNSAMPLE_FACTOR, shape[1] // DOWNSAMPLE_FACTOR)
                flat = to_host(flat)
                list(pool.map(save_jpeg, [(osp.join(base, "rgb", kind, "{:06}.jpg".format(first + k)), imgs[j]) for j, k in enumerate(members)
                                          for kind, imgs in (("original", flat), ("downsample", small))]))
        want_mask = [not skip_mask and info["panoptic"] is not None for info in infos]
        if skip_depth and not any(want_mask):
            continue
        ranges, cps, poses, trigs, params = [], [], [], [], []
        for fa, info in zip(part, infos):
            e2c, K = lidar.vehicle_to_camera(info["extrinsic"]), intrinsic_matrix(info["intrinsic"])
            for laser in fa.lasers:
                ranges.append(laser["range"]), cps.append(laser["cp"]), poses.append(laser["pose"])
                trigs.append(lidar.range_image_trig(laser["inclinations"], laser["range"].shape[1], laser["extrinsic"]))
                params.append(lidar.range_image_params(laser["extrinsic"], fa.pose if laser["pose"] is not None else None, e2c, K,
                                                       info["width"], info["height"]))
        found, _ = steps["points"](ranges, cps, poses, trigs, np.stack(params)) if ranges else ([], None)
        at, jobs_npy, jobs_mask = 0, [], []
        for k, (fa, info) in enumerate(zip(part, infos)):
            mine = found[at:at + len(fa.lasers)]
            at += len(fa.lasers)
            if not skip_depth:
                jobs_npy.append((osp.join(base, "depth", "{:06}.npy".format(first + k)),
                                 np.concatenate([m[2] for m in mine]) if mine else np.zeros((0, 3), dtype=np.float64)))
            if want_mask[k]:
                semantic, instance = wr.decode_panoptic(info["panoptic"], info["divisor"])
                points = np.concatenate([m[0] for m in mine]) if mine else np.zeros((0, 3), dtype=np.float64)
                cp = np.concatenate([m[1] for m in mine]) if mine else np.zeros((0, 3), dtype=np.int32)
                entries = object_labels(semantic, instance, points, cp, info["code"], fa.labels, steps["fit"])
                jobs_mask.append((osp.join(base, "mask", "{:06}".format(first + k)), semantic, instance, entries))
        list(pool.map(save_npy, jobs_npy))
        list(pool.map(save_mask, jobs_mask))


def prepare_segment(pool, path, segment_dir, cams, batch, skip_rgb, skip_depth, skip_mask, steps, messages, check_data=False):
    Frame, MatrixFloat, MatrixInt32 = messages
    cam_dirs = {cam: osp.join(segment_dir, cam) for cam in cams}
    for base in cam_dirs.values():
        for d in (osp.join(base, "rgb", "original"), osp.join(base, "rgb", "downsample"), osp.join(base, "depth"), osp.join(base, "mask")):
            os.makedirs(d, exist_ok=True)

    def load(payload):
        frame = Frame()
        frame.ParseFromString(payload)
        return wr.frame_to_arrays(frame, cams, MatrixFloat, MatrixInt32)

    poses = {cam: [] for cam in cams}
    num_frames, pending = 0, []

    def flush():
        nonlocal num_frames, pending
        part = list(pool.map(load, pending))
        prepare_frames(pool, part, num_frames, cam_dirs, cams, skip_rgb, skip_depth, skip_mask, steps)
        for fa in part:
            for cam in cams:
                poses[cam].append(" ".join(str(x) for x in fa.cameras[cam]["pose"]))
        num_frames, pending = num_frames + len(part), []

    for payload in wr.read_records(path, check_data=check_data):
        pending.append(payload)
        if len(pending) >= max(batch, 1):
            flush()
    if pending:
        flush()
    for cam in cams:
        with open(osp.join(cam_dirs[cam], "odometry.txt"), "w") as fh:
            for line in poses[cam]:
                fh.write(line + "\n")
    return num_frames


def prepare(record_dir, dataset_dir, split_idx=0, split_num=1, batch=16, num_workers=8, skip_rgb=False, skip_depth=False, skip_mask=False,
            segments=None, cams=("FRONT",), splits=SPLITS, decode=device_decode, undistort=device_undistort, resize=device_resize,
            points=lidar.range_image_points, fit=lidar.box_fit, messages=None, check_data=False, log=print):
    """The whole tree.  decode(files' bytes) -> frames, undistort(frames, intrinsic) -> (n, H, W, 3), resize(frames, height, width) ->
    (n, height, width, 3) on the host, points (hipops.lidar.range_image_points' signature) and fit (hipops.lidar.box_fit's) are the
    device steps by default; host_decode, host_undistort, host_resize, hipops.lidar.range_image_points_host and box_fit_host are the
    same on the host.  messages: the (Frame, MatrixFloat, MatrixInt32) classes, the Waymo package's by default."""
    steps = {"decode": decode, "undistort": undistort, "resize": resize, "points": points, "fit": fit}
    wanted = None if not segments else set(segments)
    found, warned = set(), set()
    os.makedirs(dataset_dir, exist_ok=True)
    with ThreadPoolExecutor(max_workers=min(max(int(num_workers), 1), MAX_THREADS)) as pool:
        for split in splits:
            split_dir = osp.join(record_dir, split)
            if not osp.isdir(split_dir):
                raise FileNotFoundError("Directory not found: {}".format(split_dir))
            traversals = sorted(((osp.join(split_dir, f), f[:f.index("_with")] if "_with" in f else f[:-len(".tfrecord")])
                                 for f in os.listdir(split_dir) if f.endswith(".tfrecord")), key=lambda t: t[1])
            if split in SEGMENTS_EXPECTED and len(traversals) != SEGMENTS_EXPECTED[split] and split not in warned:
                warned.add(split)
                log("Warning: number of .tfrecord files in {} is {} (!= {}).".format(split_dir, len(traversals), SEGMENTS_EXPECTED[split]))
            log("Processing {} | # Traversals = {}".format(split_dir, len(traversals)))
            traversals = traversals[len(traversals) * split_idx // split_num:len(traversals) * (split_idx + 1) // split_num]
            for path, name in traversals:
                if wanted is not None and name not in wanted:
                    continue
                found.add(name)
                if messages is None:
                    messages = wr.message_classes()
                n = prepare_segment(pool, path, osp.join(dataset_dir, split, name), tuple(cams), batch, skip_rgb, skip_depth, skip_mask, steps,
                                    messages, check_data)
                log("{}: {} frames".format(name, n))
    if wanted is not None and wanted - found and split_num == 1:
        raise ValueError("no such segments: {}".format(sorted(wanted - found)))


def main(argv=None):
    ap = argparse.ArgumentParser(description="Waymo Open Dataset segments -> the processed layout of datasets/waymo_dataset.py")
    ap.add_argument("record_dir")
    ap.add_argument("dataset_dir")
    ap.add_argument("split", nargs="*", type=int, default=[], help="split_idx split_num: this process takes its share of every split's segments")
    ap.add_argument("--skip_rgb", action="store_true", help="no frames, no down-samples, no cam.json")
    ap.add_argument("--skip_depth", action="store_true", help="no LiDAR lists")
    ap.add_argument("--skip_mask", action="store_true", help="no semantic / instance labels and no objects")
    ap.add_argument("--segments", nargs="*", default=None, help="segment names, all by default")
    ap.add_argument("--cams", nargs="*", default=["FRONT"], choices=sorted(wr.CAMERA_NAMES.values()))
    ap.add_argument("--batch", type=int, default=16, help="frames per launch")
    ap.add_argument("--num_workers", type=int, default=8, help="file threads, at most {}".format(MAX_THREADS))
    ap.add_argument("--check_data", action="store_true", help="verify every record's payload checksum (slow)")
    args = ap.parse_args(argv)
    if len(args.split) not in (0, 2) or (args.split and not 0 <= args.split[0] < args.split[1]):
        ap.error("split_idx split_num: two integers with 0 <= split_idx < split_num")
    split_idx, split_num = args.split or (0, 1)
    prepare(args.record_dir, args.dataset_dir, split_idx, split_num, batch=args.batch, num_workers=args.num_workers, skip_rgb=args.skip_rgb,
            skip_depth=args.skip_depth, skip_mask=args.skip_mask, segments=args.segments, cams=args.cams, check_data=args.check_data)


if __name__ == "__main__":
    main()
