"""Depth for a folder of frames, at the frames' own resolution:

    python predict.py <frames dir> -l <checkpoint folder> [--depth_model ...] [--height H --width W] [-b B] [--out <dir>]
                      [--save depth16 npy color cloud objects tracks] [--depth_scale 256] [--post_process] [--motion] [--scene]
                      [--intrinsics fx fy cx cy] [--cloud_stride 1] [--cloud_max_range R] [--cloud_edge 0.05] [--cloud_motion_thresh 0.5]
                      [--object_motion_thresh 0.5] [--object_connectivity 8] [--object_min_pixels 16] [--object_max 256]
                      [--track_min_iou 0.25] [--write_threads 8]

The counterpart of the reference's quick demo on a few frames (its README's first offer; the demo notebook goes through
eval/visualize.py get_vis and shows the network-resolution disparity): no dataset layout, no split list.  The frames are read by
datasets.FolderDataset (baseline JPEGs decoded and resized on the device), `-d` only selects the default network resolution.

Per frame, named by the source file's stem:
    <out>/depth/<stem>.png        16-bit PNG (Pillow mode I;16): depth * depth_scale, rounded half to even, 65535 at and beyond the top
    <out>/depth_npy/<stem>.npy    float32 depth                                                                  (--save npy)
    <out>/color/<stem>.png        the disparity through matplotlib's plasma map                                  (--save color)
    <out>/cloud/<stem>.ply        the frame as a coloured point cloud in its own camera coordinates (binary PLY)   (--save cloud)
    <out>/objects/<stem>.png      16-bit label image of the moving objects at the source size, 0 = none       (--motion --save objects)
    <out>/objects/<stem>.json     the frame's objects: id, pixels, box, centroid, motion, speed, confidence, z_min, z_max
    <out>/tracks/<stem>.png       the label image of the objects with every object number replaced by its track id (--motion --save tracks)
    <out>/tracks.json             per track its id, first and last frame, length, path length and its object in every frame
    <out>/predict.json            min_depth, max_depth, depth_scale, the network resolution; depth is up to scale
depth = 1 / bilinear(disp_to_depth(disp)) at the source size: the depth metrics' definition of a prediction (tools.py:42, 291-298),
written by one kernel per batch (hipops.export, csrc/dd_export.hip); only the bytes that go to disk cross to the host.
--post_process runs the network on the mirrored image too and fuses the two disparities (the literature's "PP").
--motion reads the triplets (i-1, i, i+1) of the interior frames and also writes <out>/motion_mask/<stem>.png (the motion mask,
bytes) and <out>/poses.txt: per interior frame its stem and the 16 numbers of the 4x4 transform from the frame to its predecessor.
--save cloud back-projects the depth at every --cloud_stride-th pixel of the source frame (x right, y down, z forward; --intrinsics
or KITTI's), drops what lies beyond --cloud_max_range and the "flying pixels" at depth edges (--cloud_edge, 0 turns it off), and
writes the rest with the colours of the network-resolution frame: hipops.cloud, csrc/dd_cloud.hip, three launches per batch.
--scene (with --motion, frames of one size) writes <out>/scene.ply: the points of every interior frame that the motion mask calls
static (mask < --cloud_motion_thresh), moved by the chained poses into the coordinates of the first interior frame -- the static
scene of the drive, the moving objects removed by the network's own mask.  Depth, and with it every cloud, is up to scale.
--save objects (with --motion) describes what --scene removes: the connected components (--object_connectivity) of the motion mask at
--object_motion_thresh and above, at the network's resolution, those of at least --object_min_pixels pixels numbered in row-major
order of their first pixel, at most --object_max per frame.  Per object its size, its box in source pixels, the mean of its points in
the frame's camera coordinates (centroid), its own mean 3-D motion to the neighbouring frame with the ego-motion removed (motion,
speed), its mean mask value (confidence) and its depth range: hipops.objects, csrc/dd_objects.hip, labelled and reduced on the device.
--save tracks (with --motion, frames of one size, frame_ids[1] == -1) gives the same object one identity through the drive: every pixel
of an object of frame i is carried by the network's own complete flow into the camera of frame i-1 and votes for the object it lands
on there (hipops.tracks, csrc/dd_tracks.hip, on the device); an object continues the track of the predecessor's object it shares most
pixels with when their intersection over union reaches --track_min_iou, otherwise it opens a new track.  A track's positions are its
centroids in the coordinates of the first interior frame, through the pose chain of --scene.  No re-identification after a gap.
"""
import contextlib
import json
import os
import os.path as osp
from concurrent.futures import ThreadPoolExecutor

import miopen_env  # noqa: E402

miopen_env.setup()      # before torch, as train.py does

import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402
from torch.utils.data import DataLoader  # noqa: E402

from datasets.folder_dataset import FolderDataset, sample_lines  # noqa: E402
from hipops.cloud import chain_poses  # noqa: E402  (the scene's pose chain: numpy alone, tested without a GPU)
from networks.layers import transformation_from_parameters  # noqa: E402
from options import DynamoOptions  # noqa: E402
from Trainer import Trainer  # noqa: E402

MAX_THREADS = 16
CLOUD = "cloud"         # --save cloud: not an output of export_depth
OBJECTS = "objects"     # --save objects: neither
TRACKS = "tracks"       # --save tracks: neither
SAVE = {"depth16": ("depth16", "depth", ".png"), "npy": ("depth", "depth_npy", ".npy"), "color": ("rgb", "color", ".png")}   # --save name -> (export output, folder, extension)
SCALE_NOTE = "depth is up to scale: a self-supervised monocular network predicts it up to one unknown factor per model"


def parse(argv=None):
    options = DynamoOptions()
    p = options.p
    p.add_argument("frames_dir", type=str, help="a directory of .jpg / .jpeg / .png frames")
    p.add_argument("--out", type=str, default=None, help="output directory (default: <eval_dir>/predict/<frames dir's name>)")
    p.add_argument("--save", nargs="+", type=str, default=["depth16"], choices=sorted(SAVE) + [CLOUD, OBJECTS, TRACKS], help="what to write per frame")
    p.add_argument("--depth_scale", type=float, default=256.0, help="the 16-bit image holds depth * depth_scale")
    p.add_argument("--post_process", action="store_true", help="fuse the disparities of the image and of its mirror image")
    p.add_argument("--motion", action="store_true", help="triplets of frames: also the motion mask and the pose of every interior frame")
    p.add_argument("--write_threads", type=int, default=8, help="threads that encode and write the files (at most {})".format(MAX_THREADS))
    p.add_argument("--intrinsics", nargs=4, type=float, default=None, metavar=("fx", "fy", "cx", "cy"), help="in pixels of the frames (default: KITTI's)")
    p.add_argument("--scene", action="store_true", help="with --motion: <out>/scene.ply, the static points of all interior frames in the first one's coordinates")
    p.add_argument("--cloud_stride", type=int, default=1, help="clouds take every n-th pixel of the source frame in both directions")
    p.add_argument("--cloud_max_range", type=float, default=None, help="clouds drop points beyond this depth (default: max_depth)")
    p.add_argument("--cloud_edge", type=float, default=0.05, help="clouds drop pixels whose disparity taps differ by more than this fraction (0: keep them)")
    p.add_argument("--cloud_motion_thresh", type=float, default=0.5, help="--scene keeps the pixels whose motion mask is below this")
    p.add_argument("--object_motion_thresh", type=float, default=0.5, help="--save objects: a pixel is foreground where its motion mask is at or above this")
    p.add_argument("--object_connectivity", type=int, default=8, choices=[4, 8], help="--save objects: the neighbourhood that connects foreground pixels")
    p.add_argument("--object_min_pixels", type=int, default=16, help="--save objects: smaller components (network pixels) are not objects")
    p.add_argument("--object_max", type=int, default=256, help="--save objects: at most this many objects per frame (up to 65535)")
    p.add_argument("--track_min_iou", type=float, default=0.25, help="--save tracks: an object continues a track when its link's intersection over union is at least this")
    opt = options.parse(args=argv)
    opt.print_opt = False
    if TRACKS in opt.save and not opt.motion:
        p.error("--save tracks needs --motion: the tracks link the objects of the motion mask through the motion networks' flow")
    if TRACKS in opt.save and (len(opt.frame_ids) < 2 or opt.frame_ids[1] != -1):
        p.error("--save tracks needs frame_ids[1] == -1: the flow has to point at the frame in front")
    if TRACKS in opt.save and opt.object_max > 1024:
        p.error("--save tracks takes an --object_max of at most 1024")
    if OBJECTS in opt.save and not opt.motion:
        p.error("--save objects needs --motion: the objects are the components of the motion mask, their motion comes from the motion networks")
    if opt.object_min_pixels < 1 or not 1 <= opt.object_max <= 65535:
        p.error("--object_min_pixels is at least 1 and --object_max between 1 and 65535")
    if opt.scene and not opt.motion:
        p.error("--scene needs --motion: the static scene is built from the motion masks and the poses of the interior frames")
    if opt.cloud_stride < 1:
        p.error("--cloud_stride is at least 1")
    if opt.load_ckpt == "" and opt.weights_init != "scratch":
        p.error("a checkpoint folder is needed: -l <folder> (--weights_init scratch runs untrained networks)")
    if opt.out is None:
        opt.out = osp.join(opt.eval_dir, "predict", osp.basename(osp.normpath(opt.frames_dir)))
    return opt


def build_trainer(opt):
    """The Trainer as the evaluation scripts build it: one frame and no motion networks, or (--motion) the triplet and every network."""
    motion = getattr(opt, "motion", False)
    if not motion:
        opt.frame_ids = [0]
    trainer = Trainer(opt)
    if motion:
        trainer.set_eval()
        trainer.setup_phase("fine_tune")        # as eval/visualize.py: every module is assumed trained
    else:
        trainer.base_model.bool_CmpFlow = trainer.base_model.bool_MotMask = False
        trainer.set_eval()
    return trainer


def folder_dataset(opt, trainer, frames_dir, indices=None, intrinsics=None):
    """The FolderDataset over `frames_dir` with the switches Trainer.get_dataset gives the other readers; `indices`: the frames to visit."""
    kwargs = {}
    if trainer.device.type == "cuda" and getattr(opt, "device_preprocess", True):
        kwargs = dict(device_preprocess=True, device_decode=getattr(opt, "device_decode", True), device_resize=getattr(opt, "device_resize", True))
    filenames = None if indices is None else sample_lines(frames_dir, indices)
    return FolderDataset(frames_dir, filenames, height=opt.height, width=opt.width, cam_name=opt.cam_name, img_type=None, frame_idxs=opt.frame_ids,
                         num_scales=len(opt.scales), is_train=False, path=True, intrinsics=intrinsics, **kwargs)


def predict_batch(opt, trainer, inputs, post_process=False, motion=False, cloud=False, objects=False):
    """Uploads the batch and runs the networks: {"disp": (B,1,h,w)} on the device, with post_process "disp_flipped" (the disparity of the
    mirrored image, not mirrored back), with motion "motion_mask" (B,1,h,w) and "cam_T_cam" (B,4,4) for frame 0 -> frame_ids[1], with
    cloud "color" (B,3,h,w), the network-resolution frame, with objects (and motion) "complete_flow" (B,3,h,w) for frame_ids[1] and
    "ts" (B,), that gap's time step where the dataset gives one, else 1."""
    with torch.no_grad():
        trainer.process_inputs(inputs)
        outputs = trainer.model(inputs)
        res = {"disp": outputs[("disp", 0, 0)]}
        if post_process:
            mirrored, flipped = {("color_aug", 0, 0): torch.flip(inputs[("color_aug", 0, 0)], [3])}, {}
            trainer.base_model.predict_depths(mirrored, flipped, frames=[0])
            res["disp_flipped"] = flipped[("disp", 0, 0)]
        if motion:
            f = opt.frame_ids[1]
            res["motion_mask"] = outputs[("motion_mask", f, 0)]
            res["cam_T_cam"] = transformation_from_parameters(outputs[("axisangle", 0, f)], outputs[("translation", 0, f)], invert=True)
        if motion and objects:
            res["complete_flow"] = outputs[("complete_flow", f, 0)]
            B = res["disp"].shape[0]
            ts = inputs.get(("ts", f))
            res["ts"] = torch.ones(B, device=res["disp"].device) if ts is None else torch.as_tensor(ts, dtype=torch.float32, device=res["disp"].device).reshape(B)
        if cloud:
            res["color"] = inputs[("color", 0, 0)]
    return res


def export_batch(opt, res, H, W, save=("depth16",), depth_scale=256.0):
    """The batch's files as device tensors, keyed by the output folder: one launch for the depth outputs, one for the motion mask."""
    from hipops.export import export_depth, export_plane_u8
    want = tuple(dict.fromkeys(SAVE[name][0] for name in save))
    files = {}
    if want:            # --save cloud alone asks for none of them
        out = export_depth(res["disp"], H, W, disp_flipped=res.get("disp_flipped"), min_depth=opt.min_depth, max_depth=opt.max_depth,
                           depth_scale=depth_scale, want=want)
        files = {SAVE[name][1]: out[SAVE[name][0]] for name in save}
    if "motion_mask" in res:
        files["motion_mask"] = export_plane_u8(res["motion_mask"], H, W)
    return files


def cloud_parameters(opt):
    """The clouds' filters from the options: what predict.json records."""
    max_range = getattr(opt, "cloud_max_range", None)
    return {"stride": int(getattr(opt, "cloud_stride", 1)), "max_range": float(opt.max_depth if max_range is None else max_range),
            "edge": float(getattr(opt, "cloud_edge", 0.05)), "motion_thresh": float(getattr(opt, "cloud_motion_thresh", 0.5))}


def cloud_intrinsics(K, H, W):
    """(fx, fy, cx, cy) in pixels of an H x W frame from the dataset's normalised intrinsics."""
    return (float(K[0, 0]) * W, float(K[1, 1]) * H, float(K[0, 2]) * W, float(K[1, 2]) * H)


def object_parameters(opt):
    """The objects' parameters from the options: what predict.json records."""
    return {"motion_thresh": float(getattr(opt, "object_motion_thresh", 0.5)), "connectivity": int(getattr(opt, "object_connectivity", 8)),
            "min_pixels": int(getattr(opt, "object_min_pixels", 16)), "max_objects": int(getattr(opt, "object_max", 256))}


def track_parameters(opt):
    """The tracks' parameter from the options: what predict.json and tracks.json record."""
    return {"min_iou": float(getattr(opt, "track_min_iou", 0.25))}


def export_objects(opt, res, H, W, intrinsics, params, with_labels=False):
    """The batch's objects on the device: (label images (B,H,W) uint16, table, counts), with_labels: and the labels (B,h,w) int32 at the
    network's resolution.  `intrinsics`: in pixels of the network's frame."""
    from hipops.objects import find_objects, labels_u16
    labels, table, counts = find_objects(res["motion_mask"], res["disp"], res["complete_flow"].float(), res["ts"], res["cam_T_cam"].float(), intrinsics,
                                         disp_flipped=res.get("disp_flipped"), min_depth=opt.min_depth, max_depth=opt.max_depth, thresh=params["motion_thresh"],
                                         connectivity=params["connectivity"], min_pixels=params["min_pixels"], max_objects=params["max_objects"])
    return (labels_u16(labels, H, W), table, counts) + ((labels,) if with_labels else ())


def link_batch(opt, res, labels, carry, intrinsics, params):
    """The links of the batch's frames to their predecessors on the device: links (B, M, 6) int32.  `labels`: the batch's object labels;
    `carry`: the label map of the frame in front of the batch (1,h,w), None at the drive's first interior frame, whose row links to an
    empty map and is not used."""
    from hipops.tracks import link_objects
    before = torch.zeros_like(labels[:1]) if carry is None else carry
    labels_dst = torch.cat([before, labels[:-1]], dim=0)            # the one device copy: every frame's predecessor beside it
    _, links = link_objects(labels, labels_dst, res["disp"], res["complete_flow"].float(), res["ts"], intrinsics, disp_flipped=res.get("disp_flipped"),
                            min_depth=opt.min_depth, max_depth=opt.max_depth, max_objects=params["max_objects"])
    return links


def _write_json(path, value):
    with open(path, "w") as fh:
        json.dump(value, fh, indent=1)
    return path


def export_clouds(opt, res, H, W, intrinsics, params, pose=None, static=False):
    """The batch's clouds as (records, offsets) on the device; `static`: the motion filter on (the scene), else never (a snapshot)."""
    from hipops.cloud import export_cloud
    return export_cloud(res["disp"], res["color"], H, W, intrinsics, disp_flipped=res.get("disp_flipped"), motion_mask=res["motion_mask"] if static else None,
                        pose=pose, min_depth=opt.min_depth, max_depth=opt.max_depth, max_range=params["max_range"], edge=params["edge"],
                        motion_thresh=params["motion_thresh"], stride=params["stride"])


def _fetch_clouds(records, offsets):
    """One small copy for the counts, then the used prefix of the records: (bytes of the batch's records, offsets on the host)."""
    off = offsets.cpu().numpy()
    return records[:int(off[-1])].cpu().numpy().reshape(-1), off


def _write(path, array):
    if path.endswith(".npy"):
        np.save(path, array)
    else:
        Image.fromarray(array).save(path)       # uint16 (H,W) -> I;16, uint8 (H,W) -> L, uint8 (H,W,3) -> RGB
    return path


def predict_folder(opt, trainer, frames_dir, out_dir, save=("depth16",), depth_scale=256.0, post_process=False, motion=False, intrinsics=None,
                   write_threads=8, scene=False, cloud=None, objects=None, tracks=None):
    """Every frame of `frames_dir` (with motion: every interior frame) -> the files described above; returns the written paths.
    The main thread launches and makes one copy to the host per batch and requested output; a thread pool encodes and writes.
    `cloud`: cloud_parameters(opt), for --save cloud and `scene`; `objects`: object_parameters(opt), for --save objects
    and --save tracks; `tracks`: track_parameters(opt), for --save tracks."""
    from hipops.cloud import RECORD, ScenePly, write_ply
    save = tuple(dict.fromkeys(save))
    want_cloud, want_objects, want_tracks = CLOUD in save, OBJECTS in save, TRACKS in save
    save = tuple(name for name in save if name not in (CLOUD, OBJECTS, TRACKS))
    if want_objects and not motion:
        raise ValueError("the objects need the motion networks (--motion)")
    object_params = dict(objects) if objects is not None else object_parameters(opt)
    track_params = dict(tracks) if tracks is not None else track_parameters(opt)
    if want_tracks and not motion:
        raise ValueError("the tracks need the motion networks (--motion)")
    if want_tracks and (len(opt.frame_ids) < 2 or opt.frame_ids[1] != -1):
        raise ValueError("the tracks need frame_ids[1] == -1, not frame_ids = {}: the flow has to point at the frame in front".format(list(opt.frame_ids)))
    if want_tracks and object_params["max_objects"] > 1024:
        raise ValueError("the tracks take at most 1024 objects per frame, not {}".format(object_params["max_objects"]))
    if scene and not motion:
        raise ValueError("the scene cloud needs the motion networks (--motion)")
    params = dict(cloud) if cloud is not None else cloud_parameters(opt)
    whole = folder_dataset(opt, trainer, frames_dir, None, intrinsics)
    n = len(whole.frames)
    indices = list(range(1, n - 1)) if motion else list(range(n))
    if not indices:
        raise ValueError("--motion needs at least three frames, {} holds {}".format(frames_dir, n))
    by_size = {}            # frames of one source size share a batch: one export call serves it
    for i in indices:
        by_size.setdefault(whole.get_gt_dim(None, i, None), []).append(i)
    if scene and len(by_size) != 1:
        raise ValueError("--scene needs frames of one size, {} holds {}".format(frames_dir, sorted(by_size)))
    if want_tracks and len(by_size) != 1:
        raise ValueError("--save tracks needs frames of one size, so that a batch holds consecutive frames; {} holds {}".format(frames_dir, sorted(by_size)))
    folders = [SAVE[name][1] for name in save] + (["motion_mask"] if motion else []) + ([CLOUD] if want_cloud else []) + ([OBJECTS] if want_objects else []) + ([TRACKS] if want_tracks else [])
    ext = {SAVE[name][1]: SAVE[name][2] for name in save}
    for folder in folders:
        os.makedirs(osp.join(out_dir, folder), exist_ok=True)
    pending, poses, counts, scene_counts, used_intrinsics, object_counts = [], {}, {}, {}, {}, {}
    scene_file, chain = (ScenePly(osp.join(out_dir, "scene.ply")) if scene else None), None
    builder, carry = None, None             # --save tracks: the tracks so far, the label map of the last frame of the batch before
    if want_tracks:
        from hipops.tracks import TrackBuilder, track_image, tracks_json
        builder = TrackBuilder(track_params["min_iou"])
    with ThreadPoolExecutor(max_workers=min(max(int(write_threads), 1), MAX_THREADS)) as pool, (scene_file or contextlib.nullcontext()):
        for (H, W), idx in sorted(by_size.items()):
            dataset = folder_dataset(opt, trainer, frames_dir, idx, intrinsics)
            loader = DataLoader(dataset, opt.batch_size, False, num_workers=opt.num_workers, pin_memory=trainer.device.type == "cuda", drop_last=False,
                                collate_fn=dataset.collate, **trainer._worker_start())
            for inputs in loader:
                stems = list(inputs["paths"])
                extra = dict(objects=True) if want_objects or want_tracks else {}           # only then: the call is what it was without
                if want_cloud or scene:
                    res = predict_batch(opt, trainer, inputs, post_process=post_process, motion=motion, cloud=True, **extra)
                    camera = used_intrinsics.setdefault("{}x{}".format(H, W), cloud_intrinsics(dataset.K, H, W))
                else:
                    res = predict_batch(opt, trainer, inputs, post_process=post_process, motion=motion, **extra)
                files = export_batch(opt, res, H, W, save, depth_scale)
                clouds = export_clouds(opt, res, H, W, camera, params) if want_cloud else None
                pose = res["cam_T_cam"].reshape(-1, 16).cpu().numpy() if motion else None
                if scene or want_tracks:
                    G = chain_poses(pose, chain)
                    chain = G[-1]
                if scene:
                    world = torch.from_numpy(np.ascontiguousarray(G[:, :3].astype(np.float32))).to(res["disp"].device)
                    data, off = _fetch_clouds(*export_clouds(opt, res, H, W, camera, params, pose=world, static=True))
                    scene_file.append(data)
                    scene_counts.update({stem: int(off[b + 1] - off[b]) for b, stem in enumerate(stems)})
                if clouds is not None:
                    data, off = _fetch_clouds(*clouds)
                    for b, stem in enumerate(stems):
                        counts[stem] = int(off[b + 1] - off[b])
                        pending.append(pool.submit(write_ply, osp.join(out_dir, CLOUD, stem + ".ply"), data[off[b] * RECORD:off[b + 1] * RECORD]))
                if want_tracks:
                    from hipops.objects import unpack_table
                    h, w = res["disp"].shape[-2:]
                    images, table, found, labels = export_objects(opt, res, H, W, cloud_intrinsics(dataset.K, h, w), object_params, with_labels=True)
                    links = link_batch(opt, res, labels, carry, cloud_intrinsics(dataset.K, h, w), object_params)
                    first, carry = carry is None, labels[-1:]
                elif want_objects:
                    from hipops.objects import unpack_table
                    h, w = res["disp"].shape[-2:]
                    images, table, found = export_objects(opt, res, H, W, cloud_intrinsics(dataset.K, h, w), object_params)
                if want_objects or want_tracks:
                    if want_objects:
                        files[OBJECTS] = images             # the label images go to the host with the other images below
                    packed = torch.cat([table.reshape(len(stems), -1), found], dim=1).cpu().numpy()      # the batch's one copy of the tables
                    frames = unpack_table(packed[:, :-3].reshape(tuple(table.shape)), packed[:, -3:], size=(h, w, H, W))
                    for stem, frame in zip(stems, frames):
                        object_counts[stem] = {"kept": len(frame["objects"]), "found": frame["found"], "truncated": frame["truncated"]}
                        if want_objects:
                            pending.append(pool.submit(_write_json, osp.join(out_dir, OBJECTS, stem + ".json"), frame))
                if want_tracks:
                    rows, label_images = links.cpu().numpy(), images.cpu().numpy()
                    for b, stem in enumerate(stems):
                        ids = builder.add(stem, frames[b]["objects"], None if first and b == 0 else rows[b], G[b])
                        pending.append(pool.submit(_write, osp.join(out_dir, TRACKS, stem + ".png"), track_image(label_images[b], ids)))
                for folder, tensor in files.items():
                    host = tensor.cpu().numpy()             # the batch's one copy of this output
                    for b, stem in enumerate(stems):
                        pending.append(pool.submit(_write, osp.join(out_dir, folder, stem + ext.get(folder, ".png")), host[b]))
                for b, stem in enumerate(stems):
                    if motion:
                        poses[stem] = pose[b]
        written = [f.result() for f in pending]
    if scene:
        written.append(scene_file.close())
    if want_tracks:
        from hipops.objects import MOTION_NOTE as motion_note
        record = tracks_json(builder, dict(object_params, **track_params), notes=(SCALE_NOTE, motion_note))
        written.append(_write_json(osp.join(out_dir, "tracks.json"), record))
    if motion:
        path = osp.join(out_dir, "poses.txt")
        with open(path, "w") as fh:
            for i in indices:           # in frame order, whatever the grouping by size did
                stem = whole.stem(i)
                fh.write(" ".join([stem] + ["{:.9g}".format(float(v)) for v in poses[stem]]) + "\n")
        written.append(path)
    path = osp.join(out_dir, "predict.json")
    meta = {"min_depth": opt.min_depth, "max_depth": opt.max_depth, "depth_scale": depth_scale, "height": opt.height, "width": opt.width,
            "depth_model": opt.depth_model, "post_process": bool(post_process), "frames": len(indices), "note": SCALE_NOTE}
    if want_cloud or scene:
        order = [whole.stem(i) for i in indices]
        meta["cloud"] = dict(params, intrinsics={size: list(k) for size, k in used_intrinsics.items()}, note=SCALE_NOTE,
                             convention="x right, y down, z forward; pixel centres at integer coordinates")
        if want_cloud:
            meta["cloud"]["points"] = {stem: counts[stem] for stem in order}
        if scene:
            meta["cloud"]["scene_points"] = {stem: scene_counts[stem] for stem in order}
            meta["cloud"]["scene_total"] = int(sum(scene_counts.values()))
    if want_objects:
        from hipops.objects import MOTION_NOTE
        meta["objects"] = dict(object_params, note=SCALE_NOTE, motion_note=MOTION_NOTE,
                               convention="x right, y down, z forward; pixel centres at integer coordinates; boxes in source pixels, inclusive",
                               frames={whole.stem(i): object_counts[whole.stem(i)] for i in indices})
    if want_tracks:
        meta["tracks"] = {k: record[k] for k in ("parameters", "count", "longest", "links_accepted", "links_refused", "notes")}
    with open(path, "w") as fh:
        json.dump(meta, fh, indent=2)
    written.append(path)
    return written


def main(argv=None):
    opt = parse(argv)
    trainer = build_trainer(opt)
    written = predict_folder(opt, trainer, opt.frames_dir, opt.out, save=opt.save, depth_scale=opt.depth_scale, post_process=opt.post_process,
                             motion=opt.motion, intrinsics=opt.intrinsics, write_threads=opt.write_threads, scene=opt.scene, cloud=cloud_parameters(opt), objects=object_parameters(opt),
                             tracks=track_parameters(opt))
    print("{} files written to `{}`".format(len(written), opt.out))
    return written


if __name__ == "__main__":
    main()
