"""find_objects (csrc/dd_objects.hip) at the headline shape, B = 12 at 192 x 640, on two masks -- a smooth-blob field and a Bernoulli
field of density 0.6, whose ragged percolation-scale components are the hard case for the merge across tiles -- warmed, timed with
device events in alternating windows; the per-launch split from torch.profiler's kernel records; and beside them the --motion
network forward of the same batch (LiteMono, untrained weights: the time does not depend on them).  Needs a GPU; prints one text
block (-> profiles/objects_timing.txt).

    python scripts/time_objects.py [--B 12] [--h 192 --w 640] [--iters 50] [--rounds 5] [--no_network]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "dynamo-depth_amd"), os.path.join(ROOT, "tests")]

import miopen_env  # noqa: E402

miopen_env.setup()

import numpy as np  # noqa: E402
import torch  # noqa: E402

from hipops import objects as O  # noqa: E402
import objects_case as OC  # noqa: E402


def window(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / iters            # us per call


def stage_split(fn, calls):
    """{kernel name: us per call} from the profiler's kernel records."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
    out = {}
    for evt in prof.key_averages():
        total = getattr(evt, "device_time_total", None)
        total = getattr(evt, "cuda_time_total", 0.0) if total is None else total
        if "objects_" in evt.key and total > 0:
            out[evt.key.split("(")[0].replace("void ", "").replace("dd::", "")] = total / calls
    return out


def network_forward(a):
    from options import DynamoOptions
    from torch.utils.data import DataLoader
    from Trainer import Trainer
    opt = DynamoOptions().parse(args=["-d", "kitti", "--depth_model", "litemono", "-b", str(a.B), "--height", str(a.h), "--width", str(a.w), "--weights_init",
                                      "scratch", "--synthetic", "--num_workers", "0", "--log_dir", "/tmp/dd_time_objects_logs"])
    opt.print_opt = False
    trainer = Trainer(opt)
    trainer.set_eval()
    trainer.setup_phase("fine_tune")
    inputs = next(iter(DataLoader(trainer.get_dataset(["s {}".format(i) for i in range(a.B)]), batch_size=a.B)))
    with torch.no_grad():
        trainer.process_inputs(inputs)
        fn = lambda: trainer.model(inputs)           # noqa: E731
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        return sorted(window(fn, 10) for _ in range(a.rounds))


def main(argv=None):
    ap = argparse.ArgumentParser()
    for name, default in (("B", 12), ("h", 192), ("w", 640), ("iters", 50), ("rounds", 5)):
        ap.add_argument("--" + name, type=int, default=default)
    ap.add_argument("--no_network", action="store_true")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("time_objects.py measures on a GPU; none is visible")
    dev = "cuda"
    rng = np.random.default_rng(0)
    fields = {"blob field": np.stack([OC.blob_field(a.h, a.w, seed=b) for b in range(a.B)]),
              "Bernoulli 0.6": rng.random((a.B, a.h, a.w)) < 0.6}
    disp = torch.from_numpy((0.02 + 0.96 * rng.random((a.B, 1, a.h, a.w))).astype(np.float32)).to(dev)
    flow = torch.from_numpy((0.3 * rng.standard_normal((a.B, 3, a.h, a.w))).astype(np.float32)).to(dev)
    ts = torch.ones(a.B, device=dev)
    pose = torch.eye(4, device=dev)[None, :3].repeat(a.B, 1, 1).contiguous()
    pose[:, :, 3] = 0.1 * torch.randn(a.B, 3, device=dev)
    cam = OC.intrinsics(a.h, a.w)
    kw = dict(min_depth=0.1, max_depth=100.0)
    paths, found = {}, {}
    for name, fg in fields.items():
        mask = torch.from_numpy(np.stack([OC.mask_values(fg[b], b) for b in range(a.B)])[:, None]).to(dev)
        paths[name] = lambda mask=mask: O.find_objects(mask, disp, flow, ts, pose, cam, **kw)
    for name, fn in paths.items():
        for _ in range(5):
            counts = fn()[2]
        found[name] = counts.cpu().numpy()
    torch.cuda.synchronize()
    times = {name: [] for name in paths}
    for _ in range(a.rounds):
        for name, fn in paths.items():
            times[name].append(window(fn, a.iters))
    print("find_objects, B = {} at {}x{}, 8-connectivity, min_pixels 16, max_objects 256: {} calls per window, {} alternating windows "
          "(median; min .. max), device events".format(a.B, a.h, a.w, a.iters, a.rounds))
    for name, t in times.items():
        t = sorted(t)
        c = found[name]
        print("  {:16s} {:8.1f} us  ({:.1f} .. {:.1f})   objects kept per frame {} .. {}, found {} .. {}".format(
            name, t[len(t) // 2], t[0], t[-1], c[:, 0].min(), c[:, 0].max(), c[:, 1].min(), c[:, 1].max()))
    for name, fn in paths.items():
        split = stage_split(fn, 20)
        print("  per launch, {} (profiler's kernel records, us per call; the rest of a call is launch gaps):".format(name))
        for kernel, us in split.items():
            print("    {:44s} {:8.1f}".format(kernel, us))
        print("    {:44s} {:8.1f}".format("sum", sum(split.values())))
    if not a.no_network:
        t = network_forward(a)
        print("  the --motion network forward of the same batch (LiteMono, all networks, no grad): {:.0f} us  ({:.0f} .. {:.0f})".format(t[len(t) // 2], t[0], t[-1]))


if __name__ == "__main__":
    main()
