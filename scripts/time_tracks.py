"""link_objects (csrc/dd_tracks.hip) at the headline shape, B = 12 at 192 x 640, M = 256, on the label maps of two masks -- the smooth-blob
field and the Bernoulli field of scripts/time_objects.py -- under a smooth flow of a few pixels: warmed, timed with device events in
alternating windows against a restatement of the same votes in torch operators on the same device (index arithmetic and one
torch.bincount over row * (M + 2) + col), with the find_objects call of the same batch beside it; the per-launch split from
torch.profiler's kernel records; and the --motion network forward of the same batch.  Needs a GPU; prints one text block
(-> profiles/tracks_timing.txt).

    python scripts/time_tracks.py [--B 12] [--h 192 --w 640] [--M 256] [--iters 50] [--rounds 5] [--no_network]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "dynamo-depth_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")]

import time_objects as TO  # noqa: E402  (first: it prepares the environment before torch is imported)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from hipops import objects as O  # noqa: E402
from hipops import tracks as T  # noqa: E402
from hipops.cloud import inverse_focal  # noqa: E402
from hipops.export import depth_params  # noqa: E402
import objects_case as OC  # noqa: E402


def torch_votes(src, dst, disp, flow, ts, cam, lo, span, M):
    """The definition's votes in torch operators (no flip fuse): (B, M, M+2) int64."""
    B, h, w = src.shape
    fx, fy, cx, cy = (float(np.float32(v)) for v in cam)
    z = 1.0 / (lo + span * disp[:, 0])
    xc = (torch.arange(w, device=src.device, dtype=torch.float32)[None, None, :] - cx) * float(inverse_focal(fx))
    yc = (torch.arange(h, device=src.device, dtype=torch.float32)[None, :, None] - cy) * float(inverse_focal(fy))
    c = flow * ts[:, None, None, None]
    m0, m1, m2 = xc * z + c[:, 0], yc * z + c[:, 1], z + c[:, 2]
    uf, vf = torch.floor(fx * (m0 / m2) + cx + 0.5), torch.floor(fy * (m1 / m2) + cy + 0.5)
    inside = (m2 > 0) & (uf >= 0) & (uf <= w - 1) & (vf >= 0) & (vf <= h - 1)
    ui, vi = torch.where(inside, uf, torch.zeros_like(uf)).long(), torch.where(inside, vf, torch.zeros_like(vf)).long()
    t = dst.reshape(B, -1).gather(1, (vi * w + ui).reshape(B, -1)).reshape(B, h, w).long()
    col = torch.where(inside, torch.where((t >= 1) & (t <= M), t, torch.zeros_like(t)), torch.full_like(t, M + 1))
    act = (src >= 1) & (src <= M)
    row = torch.arange(B, device=src.device)[:, None, None] * M + (src.long() - 1)
    return torch.bincount((row * (M + 2) + col)[act], minlength=B * M * (M + 2)).reshape(B, M, M + 2)


def stage_split(fn, calls):
    """{kernel name: us per call} from the profiler's kernel records: the call's two kernels and its memset."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
    out = {}
    for evt in prof.key_averages():
        total = getattr(evt, "device_time_total", None)
        total = getattr(evt, "cuda_time_total", 0.0) if total is None else total
        if ("tracks_" in evt.key or "emset" in evt.key) and total > 0:
            out[evt.key.split("(")[0].replace("void ", "").replace("dd::", "")] = total / calls
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    for name, default in (("B", 12), ("h", 192), ("w", 640), ("M", 256), ("iters", 50), ("rounds", 5)):
        ap.add_argument("--" + name, type=int, default=default)
    ap.add_argument("--no_network", action="store_true")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("time_tracks.py measures on a GPU; none is visible")
    dev = "cuda"
    rng = np.random.default_rng(0)
    fields = {"blob field": np.stack([OC.blob_field(a.h, a.w, seed=b) for b in range(a.B)]),
              "Bernoulli 0.6": rng.random((a.B, a.h, a.w)) < 0.6}
    disp = torch.from_numpy((0.02 + 0.96 * rng.random((a.B, 1, a.h, a.w))).astype(np.float32)).to(dev)
    cam = OC.intrinsics(a.h, a.w)
    lo, span = (float(v) for v in depth_params(0.1, 100.0))
    yy, xx = np.mgrid[0:a.h, 0:a.w]
    z = 1.0 / (lo + span * disp[:, 0].cpu().numpy().astype(np.float64))
    c = np.stack([3.0 * np.sin(yy / 40.0 + xx / 90.0)[None] * z / cam[0], 2.0 * np.cos(yy / 55.0 - xx / 70.0)[None] * z / cam[1], 0.05 * z], axis=1)
    flow = torch.from_numpy(c.astype(np.float32)).to(dev)           # a smooth field of up to three pixels
    ts = torch.ones(a.B, device=dev)
    pose = torch.eye(4, device=dev)[None, :3].repeat(a.B, 1, 1).contiguous()
    kw = dict(min_depth=0.1, max_depth=100.0)
    paths, note = {}, {}
    for name, fg in fields.items():
        mask = torch.from_numpy(np.stack([OC.mask_values(fg[b], b) for b in range(a.B)])[:, None]).to(dev)
        find = lambda mask=mask: O.find_objects(mask, disp, flow, ts, pose, cam, max_objects=a.M, **kw)         # noqa: E731
        src = find()[0]
        dst = torch.roll(src, 1, 0).contiguous()            # the label map of another image of the same field
        link = lambda src=src, dst=dst: T.link_objects(src, dst, disp, flow, ts, cam, max_objects=a.M, **kw)      # noqa: E731
        restated = lambda src=src, dst=dst: torch_votes(src, dst, disp, flow, ts, cam, lo, span, a.M)            # noqa: E731
        votes = link()[0]
        same = bool((votes.long() == restated()).all())
        per_row = (votes[:, :, 1:a.M + 1] > 0).sum(2)[votes.sum(2) > 0].float()
        note[name] = "votes {}, rows with votes {}, destinations per such row {:.1f}; torch restatement equal: {}".format(
            int(votes.sum()), int((votes.sum(2) > 0).sum()), float(per_row.mean()) if per_row.numel() else 0.0, same)
        paths[name] = {"link_objects": link, "torch operators": restated, "find_objects": find}
    for fns in paths.values():
        for fn in fns.values():
            for _ in range(5):
                fn()
    torch.cuda.synchronize()
    times = {name: {k: [] for k in fns} for name, fns in paths.items()}
    for _ in range(a.rounds):
        for name, fns in paths.items():
            for k, fn in fns.items():
                times[name][k].append(TO.window(fn, a.iters))
    print("link_objects, B = {} at {}x{}, M = {}: {} calls per window, {} alternating windows (median; min .. max), device events".format(
        a.B, a.h, a.w, a.M, a.iters, a.rounds))
    for name, per in times.items():
        print("  {}: {}".format(name, note[name]))
        for k, t in per.items():
            t = sorted(t)
            print("    {:16s} {:8.1f} us  ({:.1f} .. {:.1f})".format(k, t[len(t) // 2], t[0], t[-1]))
    for name, fns in paths.items():
        split = stage_split(fns["link_objects"], 20)
        print("  per launch, {} (profiler's kernel records, us per call; the rest of a call is launch gaps):".format(name))
        for kernel, us in split.items():
            print("    {:44s} {:8.1f}".format(kernel, us))
        print("    {:44s} {:8.1f}".format("sum", sum(split.values())))
    if not a.no_network:
        t = TO.network_forward(a)
        print("  the --motion network forward of the same batch (LiteMono, all networks, no grad): {:.0f} us  ({:.0f} .. {:.0f})".format(t[len(t) // 2], t[0], t[-1]))


if __name__ == "__main__":
    main()
