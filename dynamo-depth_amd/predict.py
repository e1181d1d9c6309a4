"""Depth for a folder of frames, at the frames' own resolution:

    python predict.py <frames dir> -l <checkpoint folder> [--depth_model ...] [--height H --width W] [-b B] [--out <dir>]
                      [--save depth16 npy color] [--depth_scale 256] [--post_process] [--motion] [--intrinsics fx fy cx cy]
                      [--write_threads 8]

The counterpart of the reference's quick demo on a few frames (its README's first offer; the demo notebook goes through
eval/visualize.py get_vis and shows the network-resolution disparity): no dataset layout, no split list.  The frames are read by
datasets.FolderDataset (baseline JPEGs decoded and resized on the device), `-d` only selects the default network resolution.

Per frame, named by the source file's stem:
    <out>/depth/<stem>.png        16-bit PNG (Pillow mode I;16): depth * depth_scale, rounded half to even, 65535 at and beyond the top
    <out>/depth_npy/<stem>.npy    float32 depth                                                                  (--save npy)
    <out>/color/<stem>.png        the disparity through matplotlib's plasma map                                  (--save color)
    <out>/predict.json            min_depth, max_depth, depth_scale, the network resolution; depth is up to scale
depth = 1 / bilinear(disp_to_depth(disp)) at the source size: the depth metrics' definition of a prediction (tools.py:42, 291-298),
written by one kernel per batch (hipops.export, csrc/dd_export.hip); only the bytes that go to disk cross to the host.
--post_process runs the network on the mirrored image too and fuses the two disparities (the literature's "PP").
--motion reads the triplets (i-1, i, i+1) of the interior frames and also writes <out>/motion_mask/<stem>.png (the motion mask,
bytes) and <out>/poses.txt: per interior frame its stem and the 16 numbers of the 4x4 transform from the frame to its predecessor.
"""
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
from networks.layers import transformation_from_parameters  # noqa: E402
from options import DynamoOptions  # noqa: E402
from Trainer import Trainer  # noqa: E402

MAX_THREADS = 16
SAVE = {"depth16": ("depth16", "depth", ".png"), "npy": ("depth", "depth_npy", ".npy"), "color": ("rgb", "color", ".png")}   # --save name -> (export output, folder, extension)
SCALE_NOTE = "depth is up to scale: a self-supervised monocular network predicts it up to one unknown factor per model"


def parse(argv=None):
    options = DynamoOptions()
    p = options.p
    p.add_argument("frames_dir", type=str, help="a directory of .jpg / .jpeg / .png frames")
    p.add_argument("--out", type=str, default=None, help="output directory (default: <eval_dir>/predict/<frames dir's name>)")
    p.add_argument("--save", nargs="+", type=str, default=["depth16"], choices=sorted(SAVE), help="what to write per frame")
    p.add_argument("--depth_scale", type=float, default=256.0, help="the 16-bit image holds depth * depth_scale")
    p.add_argument("--post_process", action="store_true", help="fuse the disparities of the image and of its mirror image")
    p.add_argument("--motion", action="store_true", help="triplets of frames: also the motion mask and the pose of every interior frame")
    p.add_argument("--write_threads", type=int, default=8, help="threads that encode and write the files (at most {})".format(MAX_THREADS))
    p.add_argument("--intrinsics", nargs=4, type=float, default=None, metavar=("fx", "fy", "cx", "cy"), help="in pixels of the frames (default: KITTI's)")
    opt = options.parse(args=argv)
    opt.print_opt = False
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


def predict_batch(opt, trainer, inputs, post_process=False, motion=False):
    """Uploads the batch and runs the networks: {"disp": (B,1,h,w)} on the device, with post_process "disp_flipped" (the disparity of the
    mirrored image, not mirrored back), with motion "motion_mask" (B,1,h,w) and "cam_T_cam" (B,4,4) for frame 0 -> frame_ids[1]."""
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
    return res


def export_batch(opt, res, H, W, save=("depth16",), depth_scale=256.0):
    """The batch's files as device tensors, keyed by the output folder: one launch for the depth outputs, one for the motion mask."""
    from hipops.export import export_depth, export_plane_u8
    want = tuple(dict.fromkeys(SAVE[name][0] for name in save))
    out = export_depth(res["disp"], H, W, disp_flipped=res.get("disp_flipped"), min_depth=opt.min_depth, max_depth=opt.max_depth,
                       depth_scale=depth_scale, want=want)
    files = {SAVE[name][1]: out[SAVE[name][0]] for name in save}
    if "motion_mask" in res:
        files["motion_mask"] = export_plane_u8(res["motion_mask"], H, W)
    return files


def _write(path, array):
    if path.endswith(".npy"):
        np.save(path, array)
    else:
        Image.fromarray(array).save(path)       # uint16 (H,W) -> I;16, uint8 (H,W) -> L, uint8 (H,W,3) -> RGB
    return path


def predict_folder(opt, trainer, frames_dir, out_dir, save=("depth16",), depth_scale=256.0, post_process=False, motion=False, intrinsics=None,
                   write_threads=8):
    """Every frame of `frames_dir` (with motion: every interior frame) -> the files described above; returns the written paths.
    The main thread launches and makes one copy to the host per batch and requested output; a thread pool encodes and writes."""
    save = tuple(dict.fromkeys(save))
    whole = folder_dataset(opt, trainer, frames_dir, None, intrinsics)
    n = len(whole.frames)
    indices = list(range(1, n - 1)) if motion else list(range(n))
    if not indices:
        raise ValueError("--motion needs at least three frames, {} holds {}".format(frames_dir, n))
    by_size = {}            # frames of one source size share a batch: one export call serves it
    for i in indices:
        by_size.setdefault(whole.get_gt_dim(None, i, None), []).append(i)
    folders = [SAVE[name][1] for name in save] + (["motion_mask"] if motion else [])
    ext = {SAVE[name][1]: SAVE[name][2] for name in save}
    for folder in folders:
        os.makedirs(osp.join(out_dir, folder), exist_ok=True)
    pending, poses = [], {}
    with ThreadPoolExecutor(max_workers=min(max(int(write_threads), 1), MAX_THREADS)) as pool:
        for (H, W), idx in sorted(by_size.items()):
            dataset = folder_dataset(opt, trainer, frames_dir, idx, intrinsics)
            loader = DataLoader(dataset, opt.batch_size, False, num_workers=opt.num_workers, pin_memory=trainer.device.type == "cuda", drop_last=False,
                                collate_fn=dataset.collate, **trainer._worker_start())
            for inputs in loader:
                stems = list(inputs["paths"])
                res = predict_batch(opt, trainer, inputs, post_process=post_process, motion=motion)
                files = export_batch(opt, res, H, W, save, depth_scale)
                pose = res["cam_T_cam"].reshape(-1, 16).cpu().numpy() if motion else None
                for folder, tensor in files.items():
                    host = tensor.cpu().numpy()             # the batch's one copy of this output
                    for b, stem in enumerate(stems):
                        pending.append(pool.submit(_write, osp.join(out_dir, folder, stem + ext.get(folder, ".png")), host[b]))
                for b, stem in enumerate(stems):
                    if motion:
                        poses[stem] = pose[b]
        written = [f.result() for f in pending]
    if motion:
        path = osp.join(out_dir, "poses.txt")
        with open(path, "w") as fh:
            for i in indices:           # in frame order, whatever the grouping by size did
                stem = whole.stem(i)
                fh.write(" ".join([stem] + ["{:.9g}".format(float(v)) for v in poses[stem]]) + "\n")
        written.append(path)
    path = osp.join(out_dir, "predict.json")
    with open(path, "w") as fh:
        json.dump({"min_depth": opt.min_depth, "max_depth": opt.max_depth, "depth_scale": depth_scale, "height": opt.height, "width": opt.width,
                   "depth_model": opt.depth_model, "post_process": bool(post_process), "frames": len(indices), "note": SCALE_NOTE}, fh, indent=2)
    written.append(path)
    return written


def main(argv=None):
    opt = parse(argv)
    trainer = build_trainer(opt)
    written = predict_folder(opt, trainer, opt.frames_dir, opt.out, save=opt.save, depth_scale=opt.depth_scale, post_process=opt.post_process,
                             motion=opt.motion, intrinsics=opt.intrinsics, write_threads=opt.write_threads)
    print("{} files written to `{}`".format(len(written), opt.out))
    return written


if __name__ == "__main__":
    main()
