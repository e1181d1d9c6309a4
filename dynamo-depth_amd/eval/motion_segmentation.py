"""Motion-segmentation evaluation, launch-line and output compatible with the reference's eval/motion_segmentation.py:

    python eval/motion_segmentation.py -d nuscenes --split <split> -l <checkpoint folder> [--eval_dir ./outputs]
    python eval/motion_segmentation.py -d kitti --synthetic ...                # generated frames and masks, no dataset on disk

writes <eval_dir>/<model>_<dataset>/mot_seg/pr_record_<ckpt>.npz (precision, recall, f1, thrds over 150 thresholds at
ground-truth resolution), pr_curve_<ckpt>.pdf and -- where the loader carries semantic labels -- fp_tally_<ckpt>.pdf.

One pass: every batch goes through tools.MotionSegMetrics (dd_motion_pr on the GPU), which keeps integer histograms from which
every threshold's tp / fp / fn and every class's false positives follow.  The reference scans a (B, 150, H, W) boolean tensor per
batch, stores every full-resolution prediction on the host and walks the dataset a second time for the tally."""
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

from options import DynamoOptions  # noqa: E402
from tools import MotionSegMetrics  # noqa: E402
from Trainer import Trainer  # noqa: E402
from utils import get_model_ckpt_name, is_edge, join_dir, readlines  # noqa: E402

NUM_THRD = 150


def evaluate(trainer, loader, num_thrd=NUM_THRD, num_sem=0):
    """Runs the model over `loader` and returns the accumulated MotionSegMetrics (nothing is copied to the host per image)."""
    metrics = MotionSegMetrics(num_thrd=num_thrd, num_sem=num_sem)
    with torch.no_grad():
        for inputs in loader:
            trainer.process_inputs(inputs)
            outputs = trainer.model(inputs)
            metrics.update(outputs[("motion_mask", -1, 0)], inputs["mot_mask"], inputs.get("sem_mask") if num_sem > 0 else None)
    return metrics


def eval_loader(trainer):
    """The loader over the split's test_mask_files.txt (edge frames pruned), or over generated samples with --synthetic."""
    opt = trainer.opt
    if opt.synthetic:
        filenames = ["synthetic {}".format(i) for i in range(4 * max(opt.batch_size, 8))]       # as Trainer.setup_val_loader
    else:
        filenames = readlines(trainer._split_file("test_mask_files.txt"))
        # evaluated frames must not be the first or last frame of their sequence
        filenames = [f for f in filenames if not is_edge(f, opt)]
    assert len(filenames) > 0, "Number of items for eval must be > 0."
    dataset = trainer.get_dataset(filenames, is_train=False, load_depth=False, load_mask=True)
    dataset.img_type = opt.eval_img_type
    return DataLoader(dataset, opt.batch_size, False, num_workers=opt.num_workers, pin_memory=trainer.device.type == "cuda", drop_last=False,
                      collate_fn=getattr(dataset, "collate", None), **trainer._worker_start())


def plot_pr_curve(plt, res, path):
    precision, recall = res["precision"].numpy(), res["recall"].numpy()
    fig = plt.figure()
    plt.axhline(y=precision[0], linestyle=":", color="C0")      # baseline: everything predicted moving
    plt.plot(recall[recall > 0], precision[recall > 0], color="C0")
    plt.xlim(0, 1)
    plt.ylim(0, 1)
    plt.xlabel("Recall")
    plt.ylabel("Precision")
    plt.title("Motion Segmentation PR Curve")
    fig.savefig(path)
    plt.close(fig)


def plot_fp_tally(plt, res, categories, path):
    tally = res["fp_tally"]
    total = max(tally["total"], 1)
    names = [str(categories.get(l, l)) for l in tally if l != "total"]
    share = [c / total for l, c in tally.items() if l != "total"]
    order = np.argsort(share)[::-1]
    fig = plt.figure()
    fig.set_size_inches(20, 10)
    plt.bar(np.array(names)[order], np.array(share)[order])
    plt.tick_params(axis="x", labelrotation=60)
    plt.ylim([0, 1])
    plt.ylabel("False Positive Rate")
    best = res["best_thrd_idx"]
    plt.title("Motion Segmentation False Positive Tally - Thrd {:.2f} - Macro F1 {:.3f}".format(float(res["thrds"][best]), float(res["f1"][best])))
    fig.savefig(path)
    plt.close(fig)


def main(argv=None):
    opt = DynamoOptions().parse(args=argv)
    opt.frame_ids = [0, -1, 1]
    opt.print_opt = False

    model_name, ckpt_name = get_model_ckpt_name(opt.load_ckpt)
    outdir = join_dir(opt.eval_dir, "{}_{}".format(model_name, opt.dataset), "mot_seg")
    pr_curve_path = osp.join(outdir, "pr_curve_{}.pdf".format(ckpt_name))
    pr_record_path = osp.join(outdir, "pr_record_{}.npz".format(ckpt_name))
    fp_tally_path = osp.join(outdir, "fp_tally_{}.pdf".format(ckpt_name))

    trainer = Trainer(opt)
    trainer.set_eval()
    loader = eval_loader(trainer)
    dataset = loader.dataset
    print("=== len={} ===".format(len(dataset)))
    # semantic labels (Waymo-like loaders name them in `categories`): the false-positive tally comes out of the same pass
    categories = getattr(dataset, "categories", None) or {}
    num_sem = max(categories) + 1 if categories else 0

    res = evaluate(trainer, loader, NUM_THRD, num_sem).compute()
    np.savez(pr_record_path, precision=res["precision"].numpy(), recall=res["recall"].numpy(), f1=res["f1"].numpy(), thrds=res["thrds"].numpy())
    print("PR record saved to `{}`.".format(pr_record_path))
    best = res["best_thrd_idx"]
    print("best F1 {:.4f} at threshold {:.3f}".format(float(res["f1"][best]), float(res["thrds"][best])))
    try:
        import matplotlib
        matplotlib.use("Agg")
        from matplotlib import pyplot as plt
    except ImportError:
        print("matplotlib is not installed: no plots")
        return res
    plot_pr_curve(plt, res, pr_curve_path)
    print("PR curve saved to `{}`.".format(pr_curve_path))
    if num_sem > 0:
        plot_fp_tally(plt, res, categories, fp_tally_path)
        print("FP tally saved to `{}`.".format(fp_tally_path))
    return res


if __name__ == "__main__":
    main()
