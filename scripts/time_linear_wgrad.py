"""Weight + bias gradient of LiteMono's point-wise Linears per shape: the library path (MIOpen 1x1 weight gradient + dd_channel_sum_nhwc_t)
against dd_linear_wgrad (csrc/dd_linear_wgrad.hip).  One path per process, so that a kernel trace holds every launch of that path:

   rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python scripts/time_linear_wgrad.py lib|own [reps]
   python scripts/time_linear_wgrad.py table <lib kernel_trace.csv> <own kernel_trace.csv> [reps]     # -> the table of profiles/linear_wgrad.txt

Between two shapes the process idles for 50 ms: `table` cuts the trace at those gaps (warm-up and timed segment of every shape, in SHAPES
order) and sums ALL kernels of a timed segment -- the library's zeroing and the two bias launches included -- per call.  The run itself
also prints event times per call, which include the launch gaps."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dynamo-depth_amd"))

B, H, W = 12, 192, 640
# (M, cout, cin, calls per headline step, what): LiteMono-8m's pwconv1 / pwconv2 per stage, then XCA's qkv / proj
SHAPES = []
for s, (C, n) in enumerate(((64, 4), (128, 4), (224, 10))):
    hw = (H >> (s + 2), W >> (s + 2))
    M = B * hw[0] * hw[1]
    SHAPES += [(M, 6 * C, C, n, "stage %d pwconv1" % (s + 1), hw), (M, C, 6 * C, n, "stage %d pwconv2" % (s + 1), hw),
               (M, 3 * C, C, 1, "stage %d xca qkv" % (s + 1), hw), (M, C, C, 1, "stage %d xca proj" % (s + 1), hw)]
# below the workload's sizes: the shapes of tests/test_linear_wgrad_gpu.py's autograd cases and of a batch-2 step (none of them in the step)
SHAPES += [(2 * 12 * 40, 1344, 224, 0, "batch 2 stage 3", (12, 80)), (480, 672, 224, 0, "480 rows", (12, 40)), (30, 96, 32, 0, "30 rows", (3, 10)),
           (15, 300, 8, 0, "15 rows, cin 8", (3, 5))]
GAP_NS = 20e6


def run(path, reps):
    import miopen_env
    miopen_env.setup()          # the step's find-db records: the library picks the solvers it picks in the step
    import torch
    from hipops import lib as L
    from hipops import functions as F
    lib = L.load()
    if path == "own" and not hasattr(lib, "dd_linear_wgrad_n"):
        sys.exit("this tree has no dd_linear_wgrad")
    st = L.current_stream()
    for M, cout, cin, _, what, hw in SHAPES:
        g = torch.randn(M, cout, device="cuda")
        x = torch.randn(M, cin, device="cuda")
        w = torch.empty(cout, cin, device="cuda")
        if path == "lib":
            Bv, Hv, Wv = M // (hw[0] * hw[1]), hw[0], hw[1]

            def call():
                gw = F._wgrad_1x1(g, x, w, Bv, Hv, Wv)
                return gw, F._channel_sum(g, M, cout, 0, st)
        else:
            nbytes = int(lib.dd_linear_wgrad_workspace_bytes(M, cout, cin))
            ws = torch.empty(max(nbytes // 4, 1), device="cuda")
            gw, gb = torch.empty(cout, cin, device="cuda"), torch.empty(cout, device="cuda")

            def call():
                L.check(lib.dd_linear_wgrad_n(F._p(g), F._p(x), M, cout, cin, 6, F._p(gw), F._p(gb), F._p(ws), nbytes, st), "dd_linear_wgrad_n")
                return gw, gb
        for _ in range(3):
            call()
        torch.cuda.synchronize(); time.sleep(0.05)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            call()
        e1.record(); torch.cuda.synchronize()
        print("%-4s %-18s M %6d  %4d x %-4d  %8.1f us per call (events, launch gaps included)" % (path, what, M, cout, cin, e0.elapsed_time(e1) * 1e3 / reps), flush=True)
        time.sleep(0.05)


def segments(csv_path, reps):
    import csv
    rows = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(csv_path))))
    segs, cur = [], []
    for r in rows:
        if cur and r[0] - cur[-1][1] > GAP_NS:
            segs.append(cur); cur = []
        cur.append(r)
    segs.append(cur)
    # the timed segment of a shape is the one with `reps` fold launches -- the column sum's or dd_linear_wgrad's, one per call (the warm-up
    # has three, and the library's first call of a shape can idle long enough on the host to be cut off from the rest of its warm-up)
    timed = [s for s in segs if sum(1 for _, _, k in s if "channel_sum_fold" in k or "linear_wgrad_fold" in k) >= reps]
    assert len(timed) == len(SHAPES), len(timed)
    return timed


def table(lib_csv, own_csv, reps):
    lib, own = segments(lib_csv, reps), segments(own_csv, reps)
    print("%-18s %6s %11s | %9s %8s %8s %8s | %9s %8s %7s %7s %8s | %s" % ("layer", "M", "cout x cin", "lib us", "wrw", "zero", "bias", "own us", "kernel", "fold", "GB/s", "TFLOP/s", "floor us: the larger of HBM at 6.4 TB/s and six bf16 MFMA products at 2.5 PFLOP/s"))
    tot = [0.0, 0.0]
    for (M, cout, cin, n, what, _), ls, os_ in zip(SHAPES, lib, own):
        def us(seg, key=None):
            return sum(e - s for s, e, k in seg if key is None or key(k)) / 1e3 / reps
        l_all, o_all = us(ls), us(os_)
        l_bias = us(ls, lambda k: "channel_sum" in k)
        l_zero = us(ls, lambda k: "SubTensorOp" in k)
        o_fold = us(os_, lambda k: "fold" in k)
        byts, flop = 4.0 * M * (cout + cin), 2.0 * M * cout * cin
        floor = max(byts / 6.4e12, 6 * flop / 2.5e15) * 1e6
        print("%-18s %6d %4d x %-4d | %9.1f %8.1f %8.1f %8.1f | %9.1f %8.1f %7.1f %7.0f %8.1f | %5.1f   x%d per step  %s" % (
            what, M, cout, cin, l_all, l_all - l_bias - l_zero, l_zero, l_bias, o_all, o_all - o_fold, o_fold, byts / o_all * 1e-3, flop / o_all * 1e-6, floor, n,
            "own" if o_all < l_all else "LIBRARY"))
        tot[0] += n * l_all; tot[1] += n * min(o_all, l_all)
    print("per step over these layers: library %.0f us, with the gate %.0f us" % (tot[0], tot[1]))


if __name__ == "__main__":
    if sys.argv[1] == "table":
        table(sys.argv[2], sys.argv[3], int(sys.argv[4]) if len(sys.argv) > 4 else 20)
    else:
        run(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 20)
