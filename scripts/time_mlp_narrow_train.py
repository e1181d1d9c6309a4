"""Device timing of LiteMono's stage-1 and stage-2 MLP blocks (C = 64 / 128, hidden 6C) in a TRAINING pass, forward + backward: the
library path (what the block runs with DD_STOCK_MLP=1 or below the gate: two BLAS GEMMs and ATen's GELU forward, two BLAS GEMMs and
ATen's GELU backward for the data gradient) against hipops.functions.mlp_train_narrow (dd_mlp_train_pack_narrow, dd_mlp_train_fwd,
dd_mlp_train_bwd).  Both paths compute the weight and bias gradients with the same dd_linear_wgrad launches, which are inside both
figures.  The method is scripts/time_mlp_stage3_train.py's: captured graphs, device time, the two paths ALTERNATE, five rounds, one
process; a path is ahead when its worst round beats the other's best.  Rows: the training batch of the 192x640 workload (12 x 48 x 160 at
C = 64, 12 x 24 x 80 at C = 128) and smaller batches (6, 2, 1) for the row count from which the new path is ahead."""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dynamo-depth_amd")):
    sys.path.insert(0, p)
from hipops.functions import mlp_train_narrow, pointwise_linear  # noqa: E402
from time_mlp_stage3 import Block, timed  # noqa: E402

ROUNDS = 5


def main():
    fmt = "%-18s %6s | %-5s | %-44s | %-44s | %s"
    print(fmt % ("B,H,W,C", "rows", "what", "library us (rounds)", "mlp_train_narrow us (rounds)", "verdict"))
    for C, H, W in ((64, 48, 160), (128, 24, 80)):
        for B in (12, 6, 2, 1):
            shape = (B, H, W, C)
            M = B * H * W
            torch.manual_seed(B)
            blk = Block(C).cuda()
            y = torch.randn(*shape, device="cuda", requires_grad=True)
            gout = torch.randn(*shape, device="cuda")
            wrt = [y] + list(blk.parameters())

            def stock_fwd():
                return pointwise_linear(blk.act(pointwise_linear(y, blk.pwconv1)), blk.pwconv2)

            def own_fwd():
                return mlp_train_narrow(y, blk)

            def both(fwd):
                return lambda: torch.autograd.grad(fwd(), wrt, gout)
            t = {k: [] for k in ("lib", "own", "lib_f", "own_f")}
            for _ in range(ROUNDS):
                t["lib"].append(timed(both(stock_fwd)))
                t["own"].append(timed(both(own_fwd)))
                t["lib_f"].append(timed(stock_fwd))
                t["own_f"].append(timed(own_fwd))

            def row(what, a, b):
                verdict = "mlp_train_narrow ahead" if max(b) < min(a) else ("library ahead" if max(a) < min(b) else "within the spread")
                print(fmt % (shape, M, what, " ".join("%7.1f" % v for v in a), " ".join("%7.1f" % v for v in b), verdict), flush=True)
            row("f + b", t["lib"], t["own"])
            row("fwd", t["lib_f"], t["own_f"])
            med = {k: statistics.median(v) for k, v in t.items()}
            print("%-18s %6d | bwd   | median %.1f (f + b) - %.1f (fwd) = %.1f | median %.1f - %.1f = %.1f" % (
                shape, M, med["lib"], med["lib_f"], med["lib"] - med["lib_f"], med["own"], med["own_f"], med["own"] - med["own_f"]), flush=True)


if __name__ == "__main__":
    main()
