"""Odometry evaluation, launch-line and output compatible with the reference's eval/odometry.py:

    python eval/odometry.py -d waymo --split <split> -l <checkpoint folder> [--eval_dir ./outputs]
    python eval/odometry.py -d kitti --synthetic ...                           # two generated segments, no dataset on disk

writes <eval_dir>/<model>_<dataset>/odometry/record_<ckpt>-5.txt (per segment `ATE: mean ± std, Speed: mean ± std, Len:`, then the
Mean / std / Min / Median / Max of both over all 5-frame snippets) and record_<ckpt>-5.npy, (len, 2) = (ate, speed) per snippet.

Per segment the frame-pair transforms of the pose network are written into one device buffer, batch by batch (-b is honoured: the
reference forces a batch of 1, the predictions do not depend on the batch size beyond rounding), and tools.OdometryMetrics turns them
and the segment's odometry.txt into snippet errors with one float64 launch.  Nothing returns to the host before the last segment;
the reference copies one pose per frame."""
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
from tools import OdometryMetrics  # noqa: E402
from Trainer import Trainer  # noqa: E402
from utils import get_filenames, get_model_ckpt_name, is_edge, join_dir, readlines, write_to_file  # noqa: E402

TRACK_LENGTH = 5
STOP_SEGMENT = 100
SYNTHETIC_FRAMES = (9, 4)       # evaluated frames of the two generated segments
SYNTHETIC_SEED = 20


def read_odometry(path, num_frames):
    """(num_frames + 1, 3 or 4, 4) float64 global poses of a segment's odometry.txt: one row of 12 or 16 numbers per frame file, the
    first row dropped as the reference drops it.  num_frames: the segment's evaluated (non-edge) frames."""
    rows = np.loadtxt(path)[1:]     # ignore the first frame
    assert num_frames == rows.shape[0] - 1, "{}: {} pose rows after the first, expected {} (one per evaluated frame plus one)".format(
        path, rows.shape[0], num_frames + 1)
    return rows.reshape(num_frames + 1, -1, 4)


def synthetic_trajectory(num_poses, seed, magnitude=1e4):
    """(num_poses, 4, 4) float64 global poses ~`magnitude` metres from the origin: an arbitrary heading, then about a metre per frame
    along the camera axis with small random turns."""
    rng = np.random.RandomState(seed)

    def rot(axis, angle):
        axis = axis / np.linalg.norm(axis)
        K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)

    pose = np.eye(4)
    pose[:3, :3] = rot(rng.randn(3), rng.uniform(0, np.pi))
    start = rng.randn(3)
    pose[:3, 3] = magnitude * start / np.linalg.norm(start)
    poses = [pose.copy()]
    for _ in range(num_poses - 1):
        move = np.eye(4)
        move[:3, :3] = rot(np.array([0.05 * rng.randn(), 1.0, 0.05 * rng.randn()]), 0.03 * rng.randn())
        move[:3, 3] = [0.02 * rng.randn(), 0.02 * rng.randn(), 1 + 0.2 * rng.randn()]
        pose = pose @ move
        poses.append(pose.copy())
    return np.stack(poses)


def _loader(trainer, dataset):
    opt = trainer.opt
    dataset.img_type = opt.eval_img_type
    return DataLoader(dataset, opt.batch_size, False, num_workers=opt.num_workers, pin_memory=trainer.device.type == "cuda", drop_last=False,
                      collate_fn=getattr(dataset, "collate", None), **trainer._worker_start())


def synthetic_segments(trainer):
    """[(name, loader, gt_global)]: generated frames and generated ground-truth tracks."""
    out = []
    for k, n in enumerate(SYNTHETIC_FRAMES):
        dataset = trainer.get_dataset(["synthetic {}".format(i) for i in range(n)], is_train=False, load_depth=False, load_mask=False, seed=k + 1)
        out.append(("synthetic-segment-{}".format(k), _loader(trainer, dataset), synthetic_trajectory(n + 1, SYNTHETIC_SEED + k)))
    return out


def dataset_segments(trainer, stop_segment=STOP_SEGMENT):
    """[(name, loader, gt_global)] over the first `stop_segment` segments named in the split's test_files.txt: a segment's non-edge frames
    in order, and its odometry.txt."""
    opt = trainer.opt
    files = readlines(trainer._split_file("test_files.txt"))
    out = []
    for segment in sorted(set(f.split()[0] for f in files))[:stop_segment]:
        filenames = [f for f in get_filenames(segment, opt) if not is_edge(f, opt)]
        gt_global = read_odometry(osp.join(opt.data_path, segment, opt.cam_name, "odometry.txt"), len(filenames))
        dataset = trainer.get_dataset(filenames, is_train=False, load_depth=False, load_mask=False)
        out.append((segment, _loader(trainer, dataset), gt_global))
    return out


def segment_poses(trainer, loader):
    """(N,4,4) fp32 on the device: transformation_from_parameters of the pose network's (0 -> +1) output for every frame of the loader."""
    N = len(loader.dataset)
    pred = torch.empty((N, 4, 4), dtype=torch.float32, device=trainer.device)
    at = 0
    with torch.no_grad():
        for inputs in loader:
            trainer.process_inputs(inputs)
            outputs = trainer.model(inputs)
            T = transformation_from_parameters(outputs[("axisangle", 0, 1)], outputs[("translation", 0, 1)])
            pred[at:at + T.shape[0]] = T
            at += T.shape[0]
    assert at == N, (at, N)
    return pred


def evaluate(trainer, segments, track_length=TRACK_LENGTH):
    """Runs the pose network over every segment and returns the OdometryMetrics (one slice per segment, nothing copied to the host)."""
    metrics = OdometryMetrics(track_length)
    for _, loader, gt_global in segments:
        metrics.add_segment(segment_poses(trainer, loader), gt_global)
    return metrics


def _mean_std(values):
    return (float(np.mean(values)), float(np.std(values))) if len(values) else (float("nan"), float("nan"))


def segment_line(name, track_length, ates, speeds, total):
    (am, asd), (sm, ssd) = _mean_std(ates), _mean_std(speeds)
    return "{:50s} Track={} ATE: {:0.3f} ± {:0.3f},  Speed: {:0.3f} ± {:0.3f},  Len: {}".format(name, track_length, am, asd, sm, ssd, total)


def summary_lines(ates, speeds, track_length):
    def block(values):
        stats = [f(values) if len(values) else float("nan") for f in (np.mean, np.std, np.min, np.median, np.max)]
        return ["Mean:   {}".format(stats[0]), "std:    {}".format(stats[1]), "--", "Min:    {}".format(stats[2]),
                "Median: {}".format(stats[3]), "Max:    {}".format(stats[4])]

    return (["\nATE Trajectory error (Track={}):  ".format(track_length)] + block(ates) + ["==", "\nSpeed:  "] + block(speeds)
            + ["--", "len:    {}".format(len(speeds))])


def output_paths(opt, track_length=TRACK_LENGTH):
    model_name, ckpt_name = get_model_ckpt_name(opt.load_ckpt)
    outdir = join_dir(opt.eval_dir, "{}_{}".format(model_name, opt.dataset), "odometry")
    stem = osp.join(outdir, "record_{}-{}".format(ckpt_name, track_length))
    return stem + ".txt", stem + ".npy"


def main(argv=None):
    opt = DynamoOptions().parse(args=argv)
    opt.print_opt = False
    opt.frame_ids = [0, -1, 1]
    assert opt.dataset in ("waymo", "nuscenes") or opt.synthetic, \
        "Only implemented for waymo and nuscenes, {} is not supported (it is accepted with --synthetic).".format(opt.dataset)
    txt_path, npy_path = output_paths(opt, TRACK_LENGTH)

    trainer = Trainer(opt)
    trainer.base_model.bool_CmpFlow = False     # the pose network is all that is needed
    trainer.base_model.bool_MotMask = False
    trainer.set_eval()

    segments = synthetic_segments(trainer) if opt.synthetic else dataset_segments(trainer)
    res = evaluate(trainer, segments, TRACK_LENGTH).compute()

    out = ["=== track_length: {}".format(TRACK_LENGTH)]
    total = 0
    for (name, _, _), (ates, speeds) in zip(segments, res["segments"]):
        total += len(ates)
        out.append(segment_line(name, TRACK_LENGTH, ates, speeds, total))
    out += summary_lines(res["ates"], res["speeds"], TRACK_LENGTH)
    for s in out:
        print(s)
    write_to_file(out, txt_path)
    np.save(npy_path, np.stack((res["ates"], res["speeds"])).transpose((1, 0)))
    return res


if __name__ == "__main__":
    main()
