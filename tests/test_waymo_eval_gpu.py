"""The Waymo path end to end on the tiny_waymo fixture: loader with device_preprocess -> Trainer.process_inputs (dd_fill_contours)
-> tools.MotionSegMetrics, and eval/motion_segmentation.py on a two-line split.  A file of its own that sorts behind the kernel
parity files: it builds Trainers in this process (recorded GEMM solutions, the multi-stream set-up), as the end-to-end test of
tests/test_motion_pr_gpu.py does, and the kernel-against-library comparisons before it should see the process as they always have."""
import glob
import os

import numpy as np
import pytest
import torch

import test_waymo_reader as wr

pytestmark = pytest.mark.gpu


def test_end_to_end_loader_trainer_evaluation(tmp_path, monkeypatch):
    from eval import motion_segmentation as ms
    from options import DynamoOptions
    from tools import MotionSegMetrics
    from Trainer import Trainer
    from torch.utils.data import DataLoader
    args = ["-d", "waymo", "--data_path", wr.WAYMO, "--depth_model", "litemono", "-b", "2", "--weights_init", "scratch", "--num_workers", "0",
            "--log_dir", str(tmp_path / "logs"), "--eval_dir", str(tmp_path / "out")]
    torch.manual_seed(0)
    opt = DynamoOptions().parse(args=args)
    opt.print_opt = False
    opt.frame_ids = [0, -1, 1]
    trainer = Trainer(opt)
    trainer.set_eval()
    dataset = trainer.get_dataset([wr.FOLDER + " 1", wr.FOLDER + " 1"], is_train=False, load_depth=False, load_mask=True)
    assert dataset.device_preprocess and dataset.device_masks and (opt.height, opt.width) == (320, 480)
    loader = DataLoader(dataset, 2, False, num_workers=0, collate_fn=dataset.collate)
    inputs = next(iter(loader))
    assert "mot_mask" not in inputs and tuple(inputs["mask_contours"].shape[:1]) == (2,)
    trainer.process_inputs(inputs)
    assert "mask_contours" not in inputs and "mask_vertices" not in inputs
    mot = inputs["mot_mask"]
    assert mot.is_cuda and mot.dtype == torch.uint8 and tuple(mot.shape) == (2, 1280, 1920)
    want = torch.from_numpy(dataset.get_mask(wr.FOLDER, 1, "l", False)[1])          # the host reader's mask
    assert torch.equal(mot[0].cpu(), want) and torch.equal(mot[1].cpu(), want)
    assert tuple(inputs[("color", 0, 0)].shape) == (2, 3, 320, 480)
    metrics = MotionSegMetrics(num_thrd=150, num_sem=29)
    metrics.update(torch.rand(2, 1, 320, 480, device="cuda"), mot, inputs["sem_mask"])
    assert int(metrics.counts[0].sum()) == 2 * wr.LABEL_COUNTS[1] and int(metrics.counts[1].sum()) == 2 * (1280 * 1920 - wr.LABEL_COUNTS[3])

    # the evaluation script on a two-line split over the fixture frame
    split = tmp_path / "splits" / "waymo"
    split.mkdir(parents=True)
    (split / "test_mask_files.txt").write_text("{0} 1\n{0} 1\n".format(wr.FOLDER))
    monkeypatch.setenv("DYNAMO_SPLITS", str(tmp_path / "splits"))
    res = ms.main(args)
    files = glob.glob(str(tmp_path / "out" / "*_waymo" / "mot_seg" / "pr_record_*.npz"))
    assert len(files) == 1 and all(np.load(files[0])[k].shape == (150,) for k in ("precision", "recall", "f1", "thrds"))
    tally = res["fp_tally"]
    assert tally["total"] == int(res["fp"][res["best_thrd_idx"]]) and all(l in dataset.categories for l in tally if l != "total")
    assert int(res["tp"][0] + res["fn"][0]) == 2 * wr.LABEL_COUNTS[1]
    assert os.path.dirname(files[0]).endswith("mot_seg")
