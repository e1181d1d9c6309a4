"""Depth evaluation, launch-line and output compatible with the reference's eval/depth.py:

    python eval/depth.py -d nuscenes --split <split> -l <checkpoint folder> [--eval_dir ./outputs]
    python eval/depth.py -d nuscenes --synthetic ...                           # generated frames, LiDAR points and masks, no dataset on disk

writes <eval_dir>/<model>_<dataset>/depth/<ckpt>.txt and prints it: part 1, the seven sparse-LiDAR metrics (per-image median scaling)
over the split's test_files.txt; part 2, the same over test_mask_files.txt conditioned on the motion mask -- background, static
objects, moving objects -- for the datasets that carry one.

Every batch goes through tools.DepthMetricsAccumulator: the metrics kernel, then one launch that adds the batch to running totals on
the device.  Nothing returns to the host before the end of a part; the reference pulls seven scalars per batch, and the totals here
do not depend on the batch size."""
import os.path as osp
import sys

proj_dir = osp.dirname(osp.dirname(osp.abspath(__file__)))      # eval/ -> the package root
if proj_dir not in sys.path:
    sys.path.insert(0, proj_dir)

import miopen_env  # noqa: E402

miopen_env.setup()      # before torch, as train.py does

import torch  # noqa: E402
from torch.utils.data import DataLoader  # noqa: E402

from options import DynamoOptions  # noqa: E402
from tools import DepthMetricsAccumulator, disp_to_depth  # noqa: E402
from Trainer import Trainer  # noqa: E402
from utils import get_model_ckpt_name, join_dir, readlines, write_to_file  # noqa: E402

SPLIT_LABELS = (("bg", 0), ("static", 2), ("mot", 1))      # the rows of part 2 and their motion-mask labels, in the reference's order


def display_str(cells):
    return "".join("{:^15s}".format(c) for c in cells)


def metric_row(name, values):
    """One table row: `values` the seven metrics in order, or None for a split without a LiDAR point (the reference divides by zero there)."""
    values = [float("nan")] * 7 if values is None else values
    return display_str([name] + ["& {:.3f}".format(v) for v in values])


def overall_row(res, names):
    return metric_row("OVERALL", [res["overall"][m] for m in names])


def split_rows(res, names):
    by_label = res.get("by_label", {})
    return [metric_row(split.upper(), [by_label[label][m] for m in names] if label in by_label else None) for split, label in SPLIT_LABELS]


def skipped_line(res):
    return "=== {} of {} samples had no LiDAR point inside the evaluation bounds and are not part of the averages ===".format(
        res["skipped"], res["num"] + res["skipped"])


def output_path(opt):
    model_name, ckpt_name = get_model_ckpt_name(opt.load_ckpt)
    return osp.join(join_dir(opt.eval_dir, "{}_{}".format(model_name, opt.dataset), "depth"), "{}.txt".format(ckpt_name))


def evaluate(trainer, loader, masked=False):
    """Runs the model over `loader` and returns the DepthMetricsAccumulator; masked: conditioned on inputs['mot_mask']."""
    opt = trainer.opt
    acc = DepthMetricsAccumulator(opt.eval_img_bound, opt.eval_min_depth, opt.eval_max_depth)
    with torch.no_grad():
        for inputs in loader:
            trainer.process_inputs(inputs)
            outputs = trainer.model(inputs)
            disp_scaled, _ = disp_to_depth(outputs[("disp", 0, 0)], opt.min_depth, opt.max_depth)
            acc.update(inputs, disp_scaled, inputs["mot_mask"] if masked else None)
    return acc


def eval_loader(trainer, split_file, load_mask):
    """The loader over the split's `split_file`, or over generated samples with --synthetic; the last batch may be short."""
    opt = trainer.opt
    if opt.synthetic:
        filenames = ["synthetic {}".format(i) for i in range(2 * max(opt.batch_size, 4) + 1)]
    else:
        filenames = readlines(trainer._split_file(split_file))
    assert len(filenames) > 0, "Number of items for eval must be > 0."
    dataset = trainer.get_dataset(filenames, is_train=False, load_depth=True, load_mask=load_mask)
    dataset.img_type = opt.eval_img_type
    return DataLoader(dataset, opt.batch_size, False, num_workers=opt.num_workers, pin_memory=trainer.device.type == "cuda", drop_last=False,
                      collate_fn=getattr(dataset, "collate", None), **trainer._worker_start())


def main(argv=None):
    opt = DynamoOptions().parse(args=argv)
    opt.print_opt = False
    opt.frame_ids = [0]                 # one frame per sample
    opt.img_ext = opt.eval_img_ext
    out_path = output_path(opt)

    trainer = Trainer(opt)
    trainer.base_model.bool_CmpFlow = False     # the motion networks are not needed
    trainer.base_model.bool_MotMask = False
    trainer.set_eval()
    names = trainer.depth_metrics.depth_metric_names
    header = display_str(["Split"] + names)
    out = ["====== Model Path - {} ======\n".format(opt.load_ckpt)]

    out.append("====== Depth Eval on Overall Test Set ======\n")
    loader = eval_loader(trainer, "test_files.txt", load_mask=False)
    out += ["=== len={} ===".format(len(loader.dataset)), header]
    overall = evaluate(trainer, loader, masked=False).compute()
    out.append(overall_row(overall, names))
    if overall["skipped"] > 0:
        out.append(skipped_line(overall))
    out.append("\n")

    out.append("====== Depth Eval on Test Set with Segmentation Annotations ======\n")
    by_mask = None
    if opt.dataset == "kitti":
        out.append("Mask Split Evaluation Skipped for KITTI.")
    else:
        loader = eval_loader(trainer, "test_mask_files.txt", load_mask=True)
        out += ["=== len={} ===".format(len(loader.dataset)), header]
        by_mask = evaluate(trainer, loader, masked=True).compute()
        out += split_rows(by_mask, names)
        if by_mask["skipped"] > 0:
            out.append(skipped_line(by_mask))
        out.append("\n")

    for s in out:
        print(s)
    write_to_file(out, out_path)
    return {"overall": overall, "by_mask": by_mask, "path": out_path}


if __name__ == "__main__":
    main()
