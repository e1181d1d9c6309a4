"""dd_odom_snippets on the device (through tools.OdometryMetrics) against the reference's recorded results
(tests/golden/odometry.npz, within the bound of tests/odometry_case.py), the slices of several segments appended in a row, and
eval/odometry.py end to end on generated segments."""
import glob
import os

import numpy as np
import pytest
import torch

import odometry_case as oc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden(golden_dir):
    z = np.load(os.path.join(golden_dir, "odometry.npz"))
    names = sorted(set(k.split("/")[0] for k in z.files))
    return {n: {k: z["{}/{}".format(n, k)] for k in ("pred", "gt", "ates", "speeds", "track_length")} for n in names}


def _run(case, metrics=None):
    from tools import OdometryMetrics
    m = OdometryMetrics(int(case["track_length"])) if metrics is None else metrics
    m.add_segment(torch.from_numpy(case["pred"]).cuda(), case["gt"])
    return m


NAMES = ["n2", "n3", "n4", "n5", "n9", "n9_track2", "n9_track3", "n9_cols12", "n70_waymo", "n40_nuscenes", "n9_zero_pred"]


def test_every_golden_case_is_run(golden):
    assert sorted(golden) == sorted(NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_kernel_against_the_reference(golden, name):
    case = golden[name]
    m = _run(case)
    res = m.compute()
    N, track = case["pred"].shape[0], int(case["track_length"])
    assert m.segments == [(0, len(case["ates"]))] and len(case["ates"]) == oc.snippet_count(N, track)
    assert res["ates"].dtype == np.float64 and res["ates"].shape == case["ates"].shape and res["speeds"].shape == case["speeds"].shape
    if name == "n2":
        assert len(res["ates"]) == 0                          # S = 0: no launch, nothing written
        return
    if name == "n3":
        assert len(res["ates"]) == 1                          # one snippet of four points
    if name == "n70_waymo":
        assert len(res["ates"]) > 64                          # more than one workgroup
    _, _, ext = oc.snippets(case["pred"], case["gt"], track)
    ua, us = oc.units(res["ates"], case["ates"], case["gt"], ext), oc.units(res["speeds"], case["speeds"], case["gt"], ext)
    print("{:14s} kernel vs reference: ate {:.3f} speed {:.3f} units (bound {:.3f})".format(name, ua.max(), us.max(), oc.BOUND_UNITS))
    assert np.array_equal(np.isnan(res["ates"]), np.isnan(case["ates"])) and not np.isnan(res["speeds"]).any()
    if name == "n9_zero_pred":
        assert np.isnan(res["ates"]).all()
    assert ua.max() <= oc.BOUND_UNITS and us.max() <= oc.BOUND_UNITS, (ua.max(), us.max())


def test_bad_arguments_launch_nothing():
    from hipops import abi, lib as L
    lib = L.load()
    pred = torch.eye(4, device="cuda").repeat(6, 1, 1).contiguous()
    gt = torch.eye(4, dtype=torch.float64, device="cuda").repeat(7, 1, 1).contiguous()
    ate = torch.full((8,), 7.0, dtype=torch.float64, device="cuda")
    speed = torch.full((8,), 7.0, dtype=torch.float64, device="cuda")
    s = L.current_stream()
    assert lib.dd_odom_snippets(abi.ptr(pred), abi.ptr(gt), 6, 1, abi.ptr(ate), abi.ptr(speed), s) == 1
    assert lib.dd_odom_snippets(abi.ptr(pred), abi.ptr(gt), 6, 17, abi.ptr(ate), abi.ptr(speed), s) == 1
    assert lib.dd_odom_snippets(abi.ptr(pred), abi.ptr(gt), 0, 5, abi.ptr(ate), abi.ptr(speed), s) == 1
    assert lib.dd_odom_snippets(None, abi.ptr(gt), 6, 5, abi.ptr(ate), abi.ptr(speed), s) == 1
    assert lib.dd_odom_snippets(abi.ptr(pred), None, 6, 5, abi.ptr(ate), abi.ptr(speed), s) == 1
    assert lib.dd_odom_snippets(abi.ptr(pred), abi.ptr(gt), 6, 5, None, abi.ptr(speed), s) == 1
    assert lib.dd_odom_snippets(abi.ptr(pred), abi.ptr(gt), 6, 5, abi.ptr(ate), None, s) == 1
    assert lib.dd_odom_snippets(None, None, 2, 5, None, None, s) == 0            # S = 0: success, nothing to touch
    assert lib.dd_odom_snippet_count(6, 5) == 4 and lib.dd_odom_snippet_count(2, 5) == 0 and lib.dd_odom_snippet_count(6, 17) == -1
    torch.cuda.synchronize()
    assert bool((ate == 7).all()) and bool((speed == 7).all())
    assert lib.dd_odom_snippets(abi.ptr(pred), abi.ptr(gt), 6, 5, abi.ptr(ate), abi.ptr(speed), s) == 0
    torch.cuda.synchronize()
    assert bool((ate[4:] == 7).all()) and bool((speed[4:] == 7).all())           # S = 4 values written, nothing behind them
    assert bool(torch.isnan(ate[:4]).all()) and bool((speed[:4] == 0).all())     # identity everywhere: 0/0, and no movement


def test_segments_appended_in_a_row_keep_their_slices(golden):
    from tools import OdometryMetrics
    names = ["n9", "n2", "n70_waymo", "n5"]                   # an empty slice in the middle
    m = OdometryMetrics(5)
    for n in names:
        _run(golden[n], m)
    assert m.values.is_cuda and m.segments == [(0, 7), (7, 0), (7, 68), (75, 3)]
    res = m.compute()
    assert len(res["ates"]) == 78 and len(res["segments"]) == 4
    for n, (ates, speeds) in zip(names, res["segments"]):
        alone = _run(golden[n]).compute()
        assert np.array_equal(ates, alone["ates"]) and np.array_equal(speeds, alone["speeds"]), n
    assert np.array_equal(np.concatenate([a for a, _ in res["segments"]]), res["ates"])


def test_buffer_grows_and_keeps_what_it_holds(golden):
    from tools import OdometryMetrics
    m = OdometryMetrics(5)
    for _ in range(16):                                       # 16 x 68 snippets: past the first allocation
        _run(golden["n70_waymo"], m)
    res = m.compute()
    assert m.used == 16 * 68 and m.values.shape[1] >= m.used
    for ates, speeds in res["segments"]:
        assert np.array_equal(ates, res["segments"][0][0]) and np.array_equal(speeds, res["segments"][0][1])


def _args(tmp_path, b, out):
    return ["-d", "kitti", "--synthetic", "--depth_model", "litemono", "--height", "64", "--width", "96", "-b", str(b), "--weights_init", "scratch",
            "--num_workers", "0", "--log_dir", str(tmp_path / "logs"), "--eval_dir", str(tmp_path / out)]


def _run_script(tmp_path, b):
    """eval/odometry.py's main on the generated segments with seed-0 weights at batch size b -> (record (len, 2), lines of the text file)."""
    from eval import odometry as od
    torch.manual_seed(0)
    od.main(_args(tmp_path, b, "out{}".format(b)))
    stem = str(tmp_path / "out{}".format(b) / "*_kitti" / "odometry" / "record_*-5")
    txt, npy = glob.glob(stem + ".txt"), glob.glob(stem + ".npy")
    assert len(txt) == 1 and len(npy) == 1
    return np.load(npy[0]), open(txt[0]).read().splitlines()


def test_end_to_end_evaluation(tmp_path):
    from eval import odometry as od
    from options import DynamoOptions
    from Trainer import Trainer
    torch.manual_seed(0)
    opt = DynamoOptions().parse(args=_args(tmp_path, 4, "tap"))
    opt.print_opt = False
    opt.frame_ids = [0, -1, 1]
    trainer = Trainer(opt)
    trainer.base_model.bool_CmpFlow = trainer.base_model.bool_MotMask = False
    trainer.set_eval()
    segments = od.synthetic_segments(trainer)
    assert [len(loader.dataset) for _, loader, _ in segments] == [9, 4] and all(np.abs(gt[:, :3, 3]).max() > 3e3 for _, _, gt in segments)
    seen, model = [], trainer.model

    def tapped(inputs):                                       # the same outputs; the pose matrices copied to the host for the restatement
        outputs = model(inputs)
        seen.append(od.transformation_from_parameters(outputs[("axisangle", 0, 1)], outputs[("translation", 0, 1)]).cpu().numpy())
        return outputs

    trainer.model = tapped
    metrics = od.evaluate(trainer, segments)
    trainer.model = model
    assert metrics.values.is_cuda and metrics.segments == [(0, 7), (7, 2)] and [len(s) for s in seen] == [4, 4, 1, 4]
    res = metrics.compute()
    preds = [np.concatenate(seen[:3]), seen[3]]
    for pred, (_, _, gt), (ates, speeds) in zip(preds, segments, res["segments"]):
        want_a, want_s, ext = oc.snippets(pred, gt, 5)
        ua, us = oc.units(ates, want_a, gt, ext), oc.units(speeds, want_s, gt, ext)
        print("evaluate vs restatement: ate {:.3f} speed {:.3f} units".format(ua.max(), us.max()))
        assert ua.max() <= oc.BOUND_UNITS and us.max() <= oc.BOUND_UNITS

    record, lines = _run_script(tmp_path, 4)
    assert record.shape == (9, 2) and record.dtype == np.float64                      # the sum of the segments' S: 7 + 2
    assert lines[0] == "=== track_length: 5" and lines[1].endswith("Len: 7") and lines[2].endswith("Len: 9") and lines[-1] == "len:    9"
    assert "Mean:   {}".format(np.mean(record[:, 0])) in lines and "Median: {}".format(np.median(record[:, 1])) in lines
    assert np.array_equal(record[:, 1], res["speeds"])        # the speeds are the ground truth's alone


def test_batch_of_4_and_batch_of_1_give_the_same_record(tmp_path):
    """eval/odometry.py with -b 4 and again with -b 1 (the reference's batch) on the same weights: the two records within the odometry
    bound, the same one the kernel is held to.  That bound is float64 rounding (6.3 units = 1.4e-11 m at these magnitudes): it holds where
    the fp32 pose network gives every frame the same bits at both batch sizes, and that is a property of the process the script sets up --
    eval/odometry.py puts MIOpen into its FAST find mode (miopen_env.setup()) before torch is imported.  In a process whose MIOpen was
    initialised before that (any earlier test of a suite that runs a convolution first) the library's default mode picks the solver of the
    pose encoder's 7x7 stem by timing, per batch size: the stem's output then differs by 1.4e-6 between the batch sizes and the ATE
    column by up to 1.4e-7 m = 68 789 units (measured; the first differing layer found by comparing every layer of the pose path at
    batch 4 and batch 1).  So both runs are started the way the script is started, each as a process of its own, side by side."""
    import subprocess
    import sys
    from eval import odometry as od
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "odometry_worker.py")
    procs = {b: subprocess.Popen([sys.executable, worker, "0"] + _args(tmp_path, b, "out{}".format(b)), stdout=subprocess.PIPE,
                                 stderr=subprocess.STDOUT, text=True) for b in (4, 1)}
    records = {}
    try:
        for b, proc in procs.items():
            out, _ = proc.communicate(timeout=240)
            assert proc.returncode == 0, out[-4000:]
            npy = glob.glob(str(tmp_path / "out{}".format(b) / "*_kitti" / "odometry" / "record_*-5.npy"))
            assert len(npy) == 1
            records[b] = np.load(npy[0])
    finally:
        for proc in procs.values():
            if proc.poll() is None:
                proc.kill()
                proc.wait()
    assert records[4].shape == records[1].shape == (9, 2) and not np.isnan(records[4]).any()
    gts = [od.synthetic_trajectory(n + 1, od.SYNTHETIC_SEED + k) for k, n in enumerate(od.SYNTHETIC_FRAMES)]
    # the snippets' extents are the ground truth's: any prediction of the right length serves
    ext = np.concatenate([oc.snippets(np.tile(np.eye(4, dtype=np.float32), (len(gt) - 1, 1, 1)), gt, 5)[2] for gt in gts])
    for col in (0, 1):
        u = oc.units(records[4][:, col], records[1][:, col], np.concatenate(gts), ext)
        print("-b 4 against -b 1, column {}: {:.3f} units (bound {:.3f}); largest difference {:.3e}".format(
            col, u.max(), oc.BOUND_UNITS, np.abs(records[4][:, col] - records[1][:, col]).max()))
        assert u.max() <= oc.BOUND_UNITS
