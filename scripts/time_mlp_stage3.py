"""Device timing of LiteMono's stage-3 MLP block (C = 224, hidden 1344) without a tape: the library path (two BLAS GEMMs with ATen's
GELU between them, what the block runs with DD_STOCK_MLP_FUSED=1) against dd_mlp_fwd_n (hipops.functions.mlp_fused: pack, kernel, fold --
every launch the path needs is inside the timed graph).  As scripts/time_mlp.py: each variant is captured into a hipGraph (ten
repetitions) and the replays are timed, so the figures are device time.  The two paths ALTERNATE, five rounds, in one process; a path is
ahead when its worst round beats the other's best.  Rows: the side batch of the 192x640 workload (24 x 12 x 40 = 11 520), the training
batch's rows (5 760) and smaller batches down to one image, for the row count from which the fused path is ahead."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dynamo-depth_amd")):
    sys.path.insert(0, p)
from hipops import lib as L  # noqa: E402
from hipops.functions import mlp_fused  # noqa: E402


class Block(torch.nn.Module):
    def __init__(self, C):
        super().__init__()
        self.pwconv1 = torch.nn.Linear(C, 6 * C)
        self.act = torch.nn.GELU()
        self.pwconv2 = torch.nn.Linear(6 * C, C)


def timed(fn, reps=10, n=20):
    """scripts/time_mlp.py's: ten repetitions captured into one graph, twenty timed replays -> microseconds per repetition"""
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            for _ in range(reps):
                fn()
    torch.cuda.synchronize()
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000 / (n * reps)


ROUNDS = 5


def main():
    lib = L.load()
    print("%-18s %6s %3s %5s | %-44s | %-44s | %s" % ("B,H,W,C", "rows", "S", "wgs", "library us (rounds)", "dd_mlp_fwd_n us (rounds)", "verdict"))
    for B in (24, 12, 8, 4, 2, 1):
        shape = (B, 12, 40, 224)
        M = B * 12 * 40
        torch.manual_seed(B)
        blk = Block(224).cuda()
        y = torch.randn(*shape, device="cuda")

        def stock():
            with torch.no_grad():
                return blk.pwconv2(blk.act(blk.pwconv1(y)))

        def fused():
            with torch.no_grad():
                return mlp_fused(y, blk)
        t_lib, t_own = [], []
        for _ in range(ROUNDS):
            t_lib.append(timed(stock))
            t_own.append(timed(fused))
        S = int(lib.dd_mlp_fwd_splits(M, 224))
        verdict = "fused ahead" if max(t_own) < min(t_lib) else ("library ahead" if max(t_lib) < min(t_own) else "within the spread")
        print("%-18s %6d %3d %5d | %-44s | %-44s | %s" % (shape, M, S, (M + 127) // 128 * S, " ".join("%7.1f" % v for v in t_lib),
                                                          " ".join("%7.1f" % v for v in t_own), verdict))


if __name__ == "__main__":
    main()
