"""The kernels that share csrc/dd_store_tile.h, timed alone with HIP events through the C ABI: dd_conv3x3_mfma at the roofline shape
(12 x 64 -> 64 x 96 x 320) and three more levels, dd_conv3x3_mfma_flat (+ fold) at the two deep levels, dd_mlp_fwd at the side batch's
stage-1 and stage-2 shapes.  Prints one JSON line: per entry the five repeat averages (us per launch), sorted.  A/B against another build:
DYNAMO_HIP_LIB=<other libdynamo_hip.so> python scripts/time_store_tail.py, alternating (profiles/mfma_store_tail.txt)."""
import os, sys, json
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "dynamo-depth_amd"))
import torch
from hipops import lib as L
from hipops.functions import _p
lib = L.load()
st = L.current_stream()
def timeit(fn, reps=50):
    for _ in range(5): fn()
    torch.cuda.synchronize()
    best = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps): fn()
        e1.record(); torch.cuda.synchronize()
        best.append(e0.elapsed_time(e1) / reps * 1e3)
    return [round(b, 2) for b in sorted(best)]
res = {"lib": os.path.basename(L.LIB_PATH)}
def conv(B, cin, cout, H, W, flat=False):
    x = torch.randn(B, H, W, cin, device="cuda"); w = torch.randn(cout, cin, 3, 3, device="cuda") / 24; b = torch.randn(cout, device="cuda")
    pf = torch.empty(int(lib.dd_conv3x3_mfma_pack_bytes(cout, cin)) // 4, device="cuda"); sw = w.stride()
    L.check(lib.dd_conv3x3_mfma_pack(_p(w), sw[0], sw[1], sw[2], sw[3], cout, cin, _p(pf), None, st), "pack")
    y = torch.empty(B, H, W, cout, device="cuda")
    if flat:
        nb = int(lib.dd_conv3x3_mfma_flat_workspace_bytes(B, H, W, cin, cout)); ws = torch.empty(max(nb // 4, 4), device="cuda")
        return timeit(lambda: lib.dd_conv3x3_mfma_flat(_p(x), _p(pf), _p(b), B, H, W, cin, cout, _p(y), _p(ws), nb, st))
    return timeit(lambda: lib.dd_conv3x3_mfma(_p(x), _p(pf), _p(b), B, H, W, cin, cout, 1, _p(y), st))
res["conv 12x64->64x96x320"] = conv(12, 64, 64, 96, 320)
res["conv 12x128->128x24x80"] = conv(12, 128, 128, 24, 80)
res["conv 24x64->64x48x160"] = conv(24, 64, 64, 48, 160)
res["conv 12x32->32x96x320"] = conv(12, 32, 32, 96, 320)
res["flat+fold 12x256->256x12x40"] = conv(12, 256, 256, 12, 40, flat=True)
res["flat+fold 12x512->512x6x20"] = conv(12, 512, 512, 6, 20, flat=True)
def mlp(M, C):
    hid = 6 * C
    y = torch.randn(M, C, device="cuda"); w1 = torch.randn(hid, C, device="cuda") / C ** .5; w2 = torch.randn(C, hid, device="cuda") / hid ** .5
    b1 = torch.randn(hid, device="cuda"); b2 = torch.randn(C, device="cuda")
    nb1, nb2 = int(lib.dd_pw_gemm_pack_bytes(hid, C)), int(lib.dd_pw_gemm_pack_bytes(C, hid))
    packs = torch.empty((nb1 + nb2) // 4, device="cuda"); p0 = packs.data_ptr()
    L.check(lib.dd_mlp_pack(_p(w1), w1.stride(0), w1.stride(1), _p(w2), w2.stride(0), w2.stride(1), C, hid, p0, None, None, None, p0 + nb1, st), "mlp_pack")
    out = torch.empty(M, C, device="cuda")
    return timeit(lambda: lib.dd_mlp_fwd(_p(y), p0, p0 + nb1, _p(b1), _p(b2), M, C, _p(out), st), reps=20)
res["mlp_fwd 24x48x160 C64"] = mlp(24 * 48 * 160, 64)
res["mlp_fwd 24x24x80 C128"] = mlp(24 * 24 * 80, 128)
print(json.dumps(res))
