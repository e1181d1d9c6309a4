"""Per-segment visualisation videos, launch-line and output compatible with the reference's eval/visualize.py:

    python eval/visualize.py -d nuscenes --split <split> -l <checkpoint folder> [--eval_dir ./outputs]
    python eval/visualize.py -d kitti --synthetic ...                          # one generated segment of eight frames, no dataset on disk

writes <eval_dir>/<model>_<dataset>/vis/<ckpt>/<segment>.mp4: image | disparity | ego flow | independent flow | motion mask per
frame.  Where `imageio` is not installed the frames are written as <segment>/NNNNNN.png instead.

--vis_backend hip (the default): every frame's tiles are rendered where the network left its outputs (hipops.vis.SegmentRenderer,
csrc/dd_vis.hip: one launch per frame, one per segment; the flow brightness is normalised by the segment's largest flow magnitude,
which never leaves the device) and the finished segment is copied to the host once.  --vis_backend torch: the reference's path --
`get_vis` per frame, every frame's float tensors kept until the segment ends, `combine_vis` on the host through matplotlib.
`get_vis` / `combine_vis` have the reference's signatures and return shapes (its demo notebook calls them)."""
import os.path as osp
import sys

proj_dir = osp.dirname(osp.dirname(osp.abspath(__file__)))      # eval/ -> the package root
if proj_dir not in sys.path:
    sys.path.insert(0, proj_dir)

import miopen_env  # noqa: E402

miopen_env.setup()      # before torch, as train.py does

import numpy as np  # noqa: E402
import torch  # noqa: E402
from torch.utils.data import DataLoader  # noqa: E402

from networks.layers import transformation_from_parameters  # noqa: E402
from options import DynamoOptions  # noqa: E402
from tools import disp_to_depth  # noqa: E402
from Trainer import Trainer  # noqa: E402
from utils import get_filenames, get_model_ckpt_name, hsv_to_rgb, is_edge, join_dir, make_mp4, readlines, score_map_vis  # noqa: E402

ARRANGEMENT = [["img", "disp", "ego_flow", "ind_flow", "mask"]]     # what is visualised and how it is arranged
SYNTHETIC_FRAMES = 8


def get_rgb_np(img):
    """Convert given img tensor (1,3,H,W) into numpy"""
    return img[0].permute(1, 2, 0).cpu().numpy()


def _cam_T_cam(inputs, outputs, f_id):
    """The pose from frame 0 to f_id at the loader's time step (never close to 0)."""
    time_step = inputs[("ts", f_id)].reshape(-1, 1, 1).float()
    return transformation_from_parameters(outputs[("axisangle", 0, f_id)] / time_step, outputs[("translation", 0, f_id)] / time_step, invert=True)


def predict(trainer, inputs):
    """Uploads the batch, finishes it on the device and runs the networks."""
    with torch.no_grad():
        trainer.process_inputs(inputs)
        return trainer.model(inputs)


def get_vis(opt, trainer, inputs, ref_frame_id, scale=0, items=("img", "disp", "ego_flow", "ind_flow", "mask")):
    """Process a given batch and produce raw visualizations given by items"""
    return collect_vis(opt, trainer, inputs, predict(trainer, inputs), ref_frame_id, scale, items)


def collect_vis(opt, trainer, inputs, outputs, ref_frame_id, scale=0, items=("img", "disp", "ego_flow", "ind_flow", "mask")):
    """get_vis behind the network forward: the raw visualizations of one processed batch and its outputs"""
    s, f_id = scale, ref_frame_id
    collection = dict()
    if "img" in items:
        collection["img"] = inputs[("color", 0, s)]                         # (B, 3, H, W)
    if "ref_img" in items:
        collection["ref_img"] = inputs[("color", f_id, s)]                  # (B, 3, H, W)
    if "disp" in items:
        collection["disp"] = outputs[("disp", 0, s)]                        # (B, 1, H, W)
    if "mask" in items:
        collection["mask"] = outputs[("motion_mask", f_id, s)]              # (B, 1, H, W)
    if any("flow" in it for it in items):
        with torch.no_grad():
            _, depth = disp_to_depth(outputs[("disp", 0, s)], opt.min_depth, opt.max_depth)
            K, inv_K = inputs[("K", s)], inputs[("inv_K", s)]
            camTcam = _cam_T_cam(inputs, outputs, f_id)
            if "ego_flow" in items:
                _, hsv, mag = trainer.vis_motion(depth=depth, K=K, inv_K=inv_K, motion_map=None, camTcam=camTcam, scale=s)
                collection["ego_flow"] = {"hsv": hsv, "mag": mag}
            if "ind_flow" in items or "samp_flow" in items:
                cam_points = trainer.backproject_depth[s](depth, inv_K)
                _, ego_flow = trainer.project_3d[s](cam_points, K, camTcam)
                independ_flow = outputs[("motion_mask", f_id, s)] * (outputs[("complete_flow", f_id, s)] - ego_flow.reshape(-1, 3, opt.height, opt.width))
                _, hsv, mag = trainer.vis_motion(depth=depth, K=K, inv_K=inv_K, motion_map=independ_flow, camTcam=None, scale=s)
                collection["ind_flow"] = {"hsv": hsv, "mag": mag}
            if "comp_flow" in items:
                _, hsv, mag = trainer.vis_motion(depth=depth, K=K, inv_K=inv_K, motion_map=outputs[("complete_flow", f_id, s)], camTcam=None, scale=s)
                collection["comp_flow"] = {"hsv": hsv, "mag": mag}
            if "samp_flow" in items:
                _, hsv, mag = trainer.vis_motion(depth=depth, K=K, inv_K=inv_K, motion_map=independ_flow, camTcam=camTcam, scale=s)
                collection["samp_flow"] = {"hsv": hsv, "mag": mag}
    return collection


def combine_vis(vis_list, arrangement, consistent_flow=True, flow_mag_factor=1.0, mask_max_mag=1.0):
    """aggregate visualizations into an image according to the arrangement"""
    vis_frames = list()
    flow_names = [a for arr in arrangement for a in arr if "flow" in a]
    if consistent_flow and flow_names:
        max_flow_mag = max(max(vis[a]["mag"] for a in flow_names) for vis in vis_list)
    for vis in vis_list:
        to_vstack = list()
        for arr in arrangement:
            to_hstack = list()
            for a in arr:
                if a not in vis:
                    raise Exception("Arrangement name (={}) not recognized.".format(a))
                out = vis[a]
                if "img" in a:
                    out = get_rgb_np(out)
                elif a == "mask":
                    out = score_map_vis(out, "hot", vminmax=(0, mask_max_mag))
                elif a == "disp":
                    out = score_map_vis(out, "plasma", vminmax=(0, 1))
                elif "flow" in a:
                    # makes small motion vectors more visible if max_flow_mag < 1
                    max_mag = flow_mag_factor * (max_flow_mag if consistent_flow else max(vis[b]["mag"] for b in flow_names))
                    hsv = vis[a]["hsv"]
                    hsv[:, 2] = torch.clamp(hsv[:, 2] * vis[a]["mag"] / max_mag, 0, 1)
                    out = get_rgb_np(1 - hsv_to_rgb(hsv))
                else:
                    raise Exception("Arrangement name (={}) not recognized.".format(a))
                to_hstack.append((out * 255).astype(np.uint8))
            to_vstack.append(np.hstack(to_hstack))
        vis_frames.append(np.vstack(to_vstack))
    return vis_frames


def add_frame(renderer, opt, inputs, outputs, ref_frame_id, scale=0):
    """One frame's network outputs into the renderer: one launch, nothing copied to the host."""
    s, f_id = scale, ref_frame_id
    names = set(renderer.names)
    flow = renderer.n_flow > 0
    motion = bool(names & {"ind_flow", "comp_flow", "samp_flow"})
    renderer.add_frame(color=inputs[("color", 0, s)] if "img" in names else None,
                       ref_color=inputs[("color", f_id, s)] if "ref_img" in names else None,
                       disp=outputs[("disp", 0, s)] if flow or "disp" in names else None,
                       motion_mask=outputs[("motion_mask", f_id, s)] if motion or "mask" in names else None,
                       complete_flow=outputs[("complete_flow", f_id, s)] if motion else None,
                       K=inputs[("K", s)] if flow else None, inv_K=inputs[("inv_K", s)] if flow else None,
                       cam_T_cam=_cam_T_cam(inputs, outputs, f_id) if flow else None, min_depth=opt.min_depth, max_depth=opt.max_depth)


def segment_loader(opt, trainer, val_segment):
    if opt.synthetic:
        filenames = ["{} {}".format(val_segment, i) for i in range(SYNTHETIC_FRAMES)]
    else:
        filenames = [f for f in get_filenames(val_segment, opt) if not is_edge(f, opt)]
    dataset = trainer.get_dataset(filenames, is_train=False, load_depth=False, load_mask=False, path=True)
    dataset.img_type = opt.eval_img_type
    return DataLoader(dataset, 1, False, num_workers=opt.num_workers, pin_memory=trainer.device.type == "cuda", drop_last=False,
                      collate_fn=getattr(dataset, "collate", None), **trainer._worker_start())


def frame_index(opt, inputs, batch_idx):
    """Where the frame goes in the video: real datasets number their frames from 1 in the path; generated frames come in loader order."""
    return batch_idx if opt.synthetic or "paths" not in inputs else int(inputs["paths"][1][0]) - 1


def render_segment(opt, trainer, loader, backend="hip", renderer=None):
    """-> (N, H, 5W, 3) uint8 on the host.  hip: `renderer` (made here when None) is reset and filled; torch: get_vis / combine_vis."""
    f_id = opt.frame_ids[1]
    if backend == "torch":
        vis_list = [dict() for _ in range(len(loader))]
        for batch_idx, inputs in enumerate(loader):
            frame_vis = get_vis(opt, trainer, inputs, ref_frame_id=f_id, scale=0, items=ARRANGEMENT[0])
            vis_list[frame_index(opt, inputs, batch_idx)].update(frame_vis)
        return np.stack(combine_vis(vis_list, ARRANGEMENT))
    from hipops.vis import SegmentRenderer
    if renderer is None:
        renderer = SegmentRenderer(ARRANGEMENT, opt.height, opt.width, len(loader), device=trainer.device)
    renderer.reset()
    order = []
    for batch_idx, inputs in enumerate(loader):
        outputs = predict(trainer, inputs)
        add_frame(renderer, opt, inputs, outputs, f_id)
        order.append(frame_index(opt, inputs, batch_idx))
    frames = renderer.finish().cpu().numpy()            # the segment's one copy to the host
    if order != list(range(len(order))):
        out = np.empty_like(frames)
        out[order] = frames
        frames = out
    return frames


def write_video(frames, outdir, name, fps):
    """<outdir>/<name>.mp4 through utils.make_mp4, or -- without imageio -- <outdir>/<name>/NNNNNN.png."""
    try:
        import imageio  # noqa: F401
    except ImportError:
        from PIL import Image
        folder = join_dir(outdir, name)
        for i, frame in enumerate(frames):
            Image.fromarray(np.ascontiguousarray(frame)).save(osp.join(folder, "{:06d}.png".format(i)))
        print("imageio is not installed: {} frames saved as PNG files to `{}` (for {} fps)\n".format(len(frames), folder, fps))
        return folder
    path = osp.join(outdir, "{}.mp4".format(name))
    make_mp4(list(frames), path, fps=fps, bgr=False)
    print("Saved to `{}`\n".format(path))
    return path


def vis_segment(opt, trainer, val_segment, outdir, renderers=None):
    """Predict for every frame of a segment and write its video.  `renderers`: a dict that keeps the device buffers from segment to
    segment (a longer segment than any before it gets larger ones)."""
    loader = segment_loader(opt, trainer, val_segment)
    backend = getattr(opt, "vis_backend", "hip")
    renderer = None
    if backend == "hip" and renderers is not None:
        renderer = renderers.get("hip")
        if renderer is None or renderer.max_frames < len(loader):
            from hipops.vis import SegmentRenderer
            renderer = renderers["hip"] = SegmentRenderer(ARRANGEMENT, opt.height, opt.width, len(loader), device=trainer.device)
    frames = render_segment(opt, trainer, loader, backend=backend, renderer=renderer)
    fps = 13 if opt.dataset == "nuscenes" else 10       # dataset info
    return write_video(frames, outdir, val_segment.split("/")[-1], fps)


def main(argv=None):
    options = DynamoOptions()
    options.p.add_argument("--vis_backend", type=str, default="hip", choices=["hip", "torch"],
                           help="hip: tiles rendered on the device; torch: the reference's path through the host and matplotlib")
    opt = options.parse(args=argv)
    opt.num_workers = min(opt.num_workers, 1)
    opt.batch_size = 1
    opt.print_opt = False       # suppress command line print out of opt

    model_name, ckpt_name = get_model_ckpt_name(opt.load_ckpt)
    outdir = join_dir(opt.eval_dir, "{}_{}".format(model_name, opt.dataset), "vis", ckpt_name)

    trainer = Trainer(opt)
    trainer.set_eval()
    trainer.setup_phase("fine_tune")    # assuming all modules are trained / no model is just initialized that needs to be turned off

    if opt.synthetic:
        segments = ["synthetic/segment-0"]
    else:
        files = readlines(trainer._split_file("test_files.txt"))
        segments = sorted(set(f.split()[0] for f in files))
    written, renderers = [], {}
    for ii, segment in enumerate(segments):
        print("{}/{} segments - {}".format(ii + 1, len(segments), segment))
        written.append(vis_segment(opt, trainer, segment, outdir, renderers))
    return written


if __name__ == "__main__":
    main()
