"""Times the metrics side of one depth-evaluation pass at the nuScenes shape (288 x 512 disparity, B = 16, 25 000 padded LiDAR slots
of which ~3 000 are valid, 900 x 1600 ground truth) two ways on the same device tensors: tools.DepthMetricsAccumulator (no host sync
until compute()) and the reference's loop over tools.DepthMetrics.forward with `.item()` per metric and batch.  The network is not
part of either loop.  Wall-clock per pass (the loops differ in host syncs, which device events do not see), median of `--repeats`.

    python scripts/time_eval_accumulators.py [--batches 40] [--repeats 5]      -> the rows of profiles/eval_accumulators.txt"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dynamo-depth_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tools import DepthMetrics, DepthMetricsAccumulator  # noqa: E402

H, W, GH, GW, B, M, VALID = 288, 512, 900, 1600, 16, 25000, 3000
BOUND, MIN_DEPTH, MAX_DEPTH = [0, 1, 0, 1], 1e-3, 75.0


def make_batches(n):
    g = torch.Generator().manual_seed(0)
    out = []
    for _ in range(n):
        rows = torch.randint(0, GH, (B, M), generator=g).float()
        cols = torch.randint(0, GW, (B, M), generator=g).float()
        z = 1 + 70 * torch.rand(B, M, generator=g)
        valid = torch.zeros(B, M)
        valid[:, :VALID] = 1
        inputs = {"depth_gt": torch.stack([rows, cols, z], 2).cuda(), "depth_valid": valid.cuda(),
                  "gt_dim": torch.tensor([[GH, GW]] * B, dtype=torch.int32).cuda()}
        disp = (0.01 + 0.3 * torch.rand(B, 1, H, W, generator=g)).cuda()
        mask = torch.randint(0, 4, (B, GH // 20, GW // 20), generator=g, dtype=torch.uint8).repeat_interleave(20, 1).repeat_interleave(20, 2).cuda()
        out.append((inputs, disp, mask))
    return out


def with_accumulator(batches, masked):
    acc = DepthMetricsAccumulator(BOUND, MIN_DEPTH, MAX_DEPTH)
    for inputs, disp, mask in batches:
        acc.update(inputs, disp, mask if masked else None)
    return acc.compute()["overall"]["de:abs_rel"]


def with_items(batches, masked):
    dm = DepthMetrics(BOUND, MIN_DEPTH, MAX_DEPTH)
    names = dm.depth_metric_names
    sums, total = {m: 0.0 for m in names}, 0
    tally = {l: {m: [0.0, 0] for m in names} for l in (0, 1, 2)}
    for inputs, disp, mask in batches:
        met = dm(inputs, {("disp_scaled", 0, 0): disp}, mask=mask if masked else None)
        for m in names:
            sums[m] += met[m].item() * disp.shape[0]
            if masked:
                for l in tally:
                    if l in met[m + "_mask"]:
                        tally[l][m][0] += met[m + "_mask"][l][0]
                        tally[l][m][1] += met[m + "_mask"][l][1]
        total += disp.shape[0]
    return sums["de:abs_rel"] / total


def wall(fn, *args, repeats=5):
    fn(*args)                               # warm-up: allocations, the library's first load
    times = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        value = fn(*args)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return float(np.median(times)), float(np.min(times)), float(np.max(times)), value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    batches = make_batches(a.batches)
    print("metrics side of one depth-evaluation pass, nuScenes shape: {}x{} -> {}x{}, B = {}, {} batches, {} of {} LiDAR slots valid ({})".format(
        H, W, GH, GW, B, a.batches, VALID, M, torch.cuda.get_device_name(0)))
    print("wall-clock per pass, median of {} (min .. max); the network is in neither loop".format(a.repeats))
    for masked in (False, True):
        print("  {}".format("conditioned on the motion mask (part 2)" if masked else "overall (part 1)"))
        for name, fn in (("DepthMetricsAccumulator, one transfer at the end", with_accumulator),
                         ("DepthMetrics.forward + .item() per metric and batch", with_items)):
            med, lo, hi, value = wall(fn, batches, masked, repeats=a.repeats)
            print("    {:55s} {:9.2f} ms  ({:.2f} .. {:.2f})   {:7.1f} us per batch   abs_rel {:.6f}".format(
                name, med * 1e3, lo * 1e3, hi * 1e3, med * 1e6 / a.batches, value))


if __name__ == "__main__":
    main()
