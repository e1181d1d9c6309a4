"""nuScenes preparation, launch-line compatible with the reference's prepare_data/nuScenes.py:

    python prepare_data/nuScenes.py <data_root> [--skip_rgb] [--skip_depth] [--skip_mask] [--scenes scene-0001 ...] [--batch 16] [--num_workers 8]

From a nuScenes download with the panoptic package (<data_root>/{v1.0-trainval, samples, sweeps, panoptic}) to the layout
datasets/nuscenes_dataset.py and the evaluation scripts read, for every scene and CAM_FRONT:

    <data_root>/scenes/<scene>/FRONT/rgb/original/%06d.jpg      links to the camera frames
    <data_root>/scenes/<scene>/FRONT/rgb/downsample/%06d.jpg    int(H / 3.125) x int(W / 3.125) area-weighted down-samples, quality 95
    <data_root>/scenes/<scene>/FRONT/depth/%06d.npy             float64 (n, 3) [u, v, depth] of the associated LIDAR_TOP scan
    <data_root>/scenes/<scene>/FRONT/mask/%06d.npz              key frames: panoptic_label, panoptic2ann, motion_label
    <data_root>/scenes/<scene>/FRONT/rgb/{cam.json, ts.json}, <data_root>/scenes/<scene>/FRONT/odometry.txt

No devkit, pyquaternion or cv2: the tables come from prepare_data/nuscenes_tables.py, the frames are decoded by hipops.jpeg (Pillow
for files its geometry check refuses) and down-sampled by hipops.resize.resize_area_batch, the scans go through
hipops.lidar.pose_points `--batch` at a time and the key frames' labels through hipops.lidar.box_fit.  Files that
exist are kept, as in the reference; an existing depth list is compared with the new one.  One process: a pool of at most 16
threads reads and writes files, the main thread launches.  `prepare` takes the device steps as callables, so the walk can be driven
on the host (tests/test_nuscenes_prepare.py)."""
import argparse
import json
import os
import os.path as osp
import sys
from concurrent.futures import ThreadPoolExecutor

proj_dir = osp.dirname(osp.dirname(osp.abspath(__file__)))      # prepare_data/ -> the package root
if proj_dir not in sys.path:
    sys.path.insert(0, proj_dir)

import numpy as np  # noqa: E402

from hipops import lidar  # noqa: E402
from prepare_data import nuscenes_tables as nt  # noqa: E402
from prepare_data.common import (JPEG_QUALITY, MAX_THREADS, chunks, device_decode, device_resize, host_decode, host_resize,  # noqa: E402,F401
                                 pil_decode, read_bytes, save_jpeg)

CAM_CHANNEL, LIDAR_CHANNEL = "CAM_FRONT", "LIDAR_TOP"
CAM_NAME = CAM_CHANNEL[4:]
DOWNSAMPLE_FACTOR = 3.125
EGO_CATEGORY = 31               # vehicle.ego: the camera is mounted on it


def host_pose_rows(scans, params):
    """out[s] = float64 (m, 6) rows [u, v, depth, gx, gy, gz] of scan s through params[s], from the numpy definition."""
    return [lidar.pose_points_host(s, p)[0] for s, p in zip(scans, params)]


def device_pose_rows(scans, params):
    """The same from one dd_lidar_pose_points call for the whole batch."""
    import torch
    offsets = np.concatenate([[0], np.cumsum([s.shape[0] for s in scans])]).astype(np.int64)
    points = torch.from_numpy(np.ascontiguousarray(np.concatenate(scans, axis=0)[:, :4], dtype=np.float32)).cuda()
    rows, counts = lidar.pose_points(points, offsets, torch.from_numpy(np.ascontiguousarray(np.stack(params), dtype=np.float64)).cuda())
    return [r[0] for r in lidar.split_rows(rows, counts, offsets)]


def link(src, dst):
    if not osp.lexists(dst):
        os.symlink(osp.realpath(src), dst)


def associate(nusc, sc):
    """(cams, lidars) of one scene as reference nuScenes.py:107-125: every CAM_FRONT record in order, the LIDAR_TOP record nearest
    in time, the sample's own for key frames; with the reference's consistency asserts."""
    first_sample = nusc.get("sample", sc["first_sample_token"])
    samples = nusc.linked_list(first_sample, "sample")
    cams = nusc.linked_list(nusc.get("sample_data", first_sample["data"][CAM_CHANNEL]), "sample_data")
    sample_cams = [c for c in cams if c["is_key_frame"]]
    unmapped = nusc.linked_list(nusc.get("sample_data", first_sample["data"][LIDAR_CHANNEL]), "sample_data")
    stamps = np.array([l["timestamp"] for l in unmapped], dtype=np.int64)
    lidars = [unmapped[int(np.abs(stamps - cam["timestamp"]).argmin())] for cam in cams]
    for ii, cam in enumerate(cams):
        if cam["is_key_frame"]:
            lidars[ii] = nusc.get("sample_data", nusc.get("sample", cam["sample_token"])["data"][LIDAR_CHANNEL])
    assert len(samples) == len(sample_cams) == sc["nbr_samples"], "Number of samples should be consistent."
    assert all(s["token"] == c["sample_token"] for s, c in zip(samples, sample_cams)), "Order of samples and sample_cams should be consistent"
    assert samples[-1]["token"] == sc["last_sample_token"], "last_sample_token should be consistent."
    return cams, lidars


def prepare_rgb(pool, data_root, cams, org_d, dwn_d, batch, decode, resize):
    todo = []
    for ii, cam in enumerate(cams):
        src = osp.join(data_root, cam["filename"])
        link(src, osp.join(org_d, "{:06}.jpg".format(ii)))
        dst = osp.join(dwn_d, "{:06}.jpg".format(ii))
        if not osp.exists(dst):
            todo.append((src, dst, int(cam["height"] / DOWNSAMPLE_FACTOR), int(cam["width"] / DOWNSAMPLE_FACTOR)))
    for part in chunks(todo, max(batch, 1)):
        frames = decode(list(pool.map(read_bytes, [job[0] for job in part])))
        groups = {}
        for job, frame in zip(part, frames):
            groups.setdefault((tuple(frame.shape), job[2], job[3]), []).append((job[1], frame))
        for (_, height, width), members in groups.items():
            small = resize([frame for _, frame in members], height, width)
            list(pool.map(save_jpeg, [(dst, small[k]) for k, (dst, _) in enumerate(members)]))


def frame_boxes(nusc, sample, cat2idx, moving_attr_tokens):
    """[(token, category index, corners (8, 3), moving)] of a sample's annotations, in their order."""
    out = []
    for token in sample["anns"]:
        ann = nusc.get("sample_annotation", token)
        out.append((token, cat2idx[ann["category_name"]], lidar.box_corners(ann["translation"], ann["size"], ann["rotation"]),
                    any(at in moving_attr_tokens for at in ann["attribute_tokens"])))
    return out


def prepare_lidar(pool, nusc, data_root, cams, lidars, depth_d, mask_d, batch, skip_depth, skip_mask, pose_rows, fit, labels):
    cat2idx, moving_attr_tokens, movable = labels
    jobs = []
    for ii, (cam, lid) in enumerate(zip(cams, lidars)):
        depth_path, mask_path = osp.join(depth_d, "{:06}.npy".format(ii)), osp.join(mask_d, "{:06}.npz".format(ii))
        want_mask = not skip_mask and cam["is_key_frame"] and not osp.exists(mask_path)
        if not skip_depth or want_mask:
            jobs.append((ii, cam, lid, depth_path, mask_path, want_mask))
    for part in chunks(jobs, max(batch, 1)):
        scans = list(pool.map(nt.read_scan, [osp.join(data_root, job[2]["filename"]) for job in part]))
        params = []
        for _, cam, lid, _, _, _ in part:
            cam_cs = nusc.get("calibrated_sensor", cam["calibrated_sensor_token"])
            params.append(lidar.pose_params(nusc.get("calibrated_sensor", lid["calibrated_sensor_token"]), nusc.get("ego_pose", lid["ego_pose_token"]),
                                            nusc.get("ego_pose", cam["ego_pose_token"]), cam_cs, cam_cs["camera_intrinsic"], cam["width"], cam["height"]))
        rows = pose_rows(scans, params)
        for (ii, cam, lid, depth_path, mask_path, want_mask), scan, p, r in zip(part, scans, params, rows):
            depth_points = np.ascontiguousarray(r[:, :3])
            if not skip_depth:
                if not osp.exists(depth_path):
                    if cam["is_key_frame"]:
                        assert lid["token"] == nusc.get("sample", cam["sample_token"])["data"][LIDAR_CHANNEL]
                    np.save(depth_path, depth_points)
                else:
                    assert np.linalg.norm(np.load(depth_path) - depth_points) == 0
            if want_mask:
                kept = lidar.pose_points_host(scan, p)[2] if r.shape[0] != scan.shape[0] else np.ones(scan.shape[0], dtype=bool)
                assert int(kept.sum()) == r.shape[0], "the host and the device keep different points"
                panoptic = nt.read_panoptic(osp.join(data_root, nusc.get("panoptic", lid["token"])["filename"]))[kept]
                boxes = frame_boxes(nusc, nusc.get("sample", cam["sample_token"]), cat2idx, moving_attr_tokens)
                motion, panoptic2ann = lidar.motion_labels(panoptic, r[:, 3:6], boxes, movable, fit=fit)
                np.savez_compressed(mask_path, panoptic_label=panoptic, panoptic2ann=panoptic2ann, motion_label=motion.astype(np.uint8))


def write_cam(cam_path, cs, height, width):
    intrinsic = np.array(cs["camera_intrinsic"], dtype=np.float64)
    intrinsic[0] /= width
    intrinsic[1] /= height
    with open(cam_path, "w") as fh:
        json.dump({"camera_intrinsic": cs["camera_intrinsic"], "translation": cs["translation"], "rotation": cs["rotation"],
                   "dim": [height, width], "intrinsic_mat": intrinsic.tolist()}, fh)


def prepare_scene(pool, nusc, sc, data_root, batch, skip_rgb, skip_depth, skip_mask, steps, labels):
    cams, lidars = associate(nusc, sc)
    base = osp.join(data_root, "scenes", sc["name"], CAM_NAME)
    org_d, dwn_d = osp.join(base, "rgb", "original"), osp.join(base, "rgb", "downsample")
    depth_d, mask_d = osp.join(base, "depth"), osp.join(base, "mask")
    for d in (org_d, dwn_d, depth_d, mask_d):
        os.makedirs(d, exist_ok=True)
    if not skip_rgb:
        prepare_rgb(pool, data_root, cams, org_d, dwn_d, batch, steps["decode"], steps["resize"])
    if not (skip_depth and skip_mask):
        prepare_lidar(pool, nusc, data_root, cams, lidars, depth_d, mask_d, batch, skip_depth, skip_mask, steps["pose_rows"], steps["fit"], labels)
    cam_path = osp.join(base, "rgb", "cam.json")
    if not osp.exists(cam_path):
        write_cam(cam_path, nusc.get("calibrated_sensor", cams[0]["calibrated_sensor_token"]), cams[0]["height"], cams[0]["width"])
    poses = []
    for cam in cams:
        ego = nusc.get("ego_pose", cam["ego_pose_token"])
        poses.append(" ".join(str(x) for x in lidar.transform_matrix(ego["translation"], ego["rotation"]).flatten()))
    if not skip_rgb:
        assert len(os.listdir(org_d)) == len(poses)
    with open(osp.join(base, "odometry.txt"), "w") as fh:
        for line in poses:
            fh.write(line + "\n")
    steps_ms = np.array([np.rint((c2["timestamp"] - c1["timestamp"]) / 1000) for c1, c2 in zip(cams[:-1], cams[1:])]).astype(np.uint8).tolist()
    with open(osp.join(base, "rgb", "ts.json"), "w") as fh:
        json.dump(steps_ms, fh)


def prepare(data_root, batch=16, num_workers=8, skip_rgb=False, skip_depth=False, skip_mask=False, scenes=None, version="v1.0-trainval",
            decode=device_decode, resize=device_resize, pose_rows=device_pose_rows, fit=lidar.box_fit, log=print):
    """The whole tree.  decode(files' bytes) -> frames, resize(frames, height, width) -> (n, height, width, 3), pose_rows(scans,
    params) -> rows per scan and fit (hipops.lidar.box_fit's signature) are the device steps by default; host_decode, host_resize,
    host_pose_rows and hipops.lidar.box_fit_host are the same on the host."""
    nusc = nt.Tables(data_root, version)
    cat2idx = {c["name"]: c["index"] for c in nusc.category}
    moving_attr_tokens = {a["token"] for a in nusc.attribute if "moving" in a["name"]}
    movable = {c["index"] for c in nusc.category if "animal" in c["name"] or "human" in c["name"] or "vehicle" in c["name"]}
    movable.discard(EGO_CATEGORY)
    steps = {"decode": decode, "resize": resize, "pose_rows": pose_rows, "fit": fit}
    wanted = None if not scenes else set(scenes)
    unknown = (wanted or set()) - {sc["name"] for sc in nusc.scene}
    if unknown:
        raise ValueError("no such scenes: {}".format(sorted(unknown)))
    with ThreadPoolExecutor(max_workers=min(max(int(num_workers), 1), MAX_THREADS)) as pool:
        for sc in nusc.scene:
            if wanted is not None and sc["name"] not in wanted:
                continue
            log("Processing {}".format(sc["name"]))
            prepare_scene(pool, nusc, sc, data_root, batch, skip_rgb, skip_depth, skip_mask, steps, (cat2idx, moving_attr_tokens, movable))


def main(argv=None):
    ap = argparse.ArgumentParser(description="raw nuScenes -> the processed layout of datasets/nuscenes_dataset.py")
    ap.add_argument("data_root")
    ap.add_argument("--skip_rgb", action="store_true", help="no links to the camera frames, no down-samples")
    ap.add_argument("--skip_depth", action="store_true", help="no LiDAR lists")
    ap.add_argument("--skip_mask", action="store_true", help="no motion labels of key frames")
    ap.add_argument("--scenes", nargs="*", default=None, help="scene names, all by default")
    ap.add_argument("--batch", type=int, default=16, help="frames and scans per launch")
    ap.add_argument("--num_workers", type=int, default=8, help="file threads, at most {}".format(MAX_THREADS))
    args = ap.parse_args(argv)
    prepare(args.data_root, batch=args.batch, num_workers=args.num_workers, skip_rgb=args.skip_rgb, skip_depth=args.skip_depth,
            skip_mask=args.skip_mask, scenes=args.scenes)


if __name__ == "__main__":
    main()
