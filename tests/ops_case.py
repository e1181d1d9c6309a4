"""Shared plumbing of tests/test_ops_parity_gpu.py and tests/test_ops_inputs.py: the one-by-one operators of csrc/dd_ops.hip
(BackprojectDepth, Project3D, SSIM, disp_to_depth, the pose matrix) at the shapes, values and gradient requests where one thread per
pixel, a block fold or a cancelling formula can go wrong, each against the float64 oracle (oracle/ref_loss.py, unchanged; its fp32
pixel grid handed over in double as photo_case.Case._oracle_fp64 does).

ONE criterion, values and gradients alike, every quantity in its own tensor (Judge.check):

    e_k = |kernel - fp64|      e_32 = |fp32 oracle - fp64|      same norm, same inputs
    e_k <= max(4 * e_32, F * S)

  * norm: max-abs for element-wise outputs, L2 for gradients and reduced quantities.
  * 4: two correct fp32 implementations that order their operations differently stay within a small multiple of each other.
  * F * S is there only because e_32 can be 0 by luck (integer-valued data, theta = 0).  S = max|fp64| or ||fp64|| of the tensor;
    F = 2^-24 x the number of roundings on the longest path from a leaf to the output in the kernel, at least 16 (ROUNDINGS below
    counts them, every multiply and add as one, contraction to fma ignored).  A sum over n pixels (g_T of Project3D) has the floor
    2^-24 (log2 n + 4) sum|term_i| with the terms of the float64 oracle: the bound of any summation tree (sum_floor_gT).
  * y == x has a true SSIM gradient of 0; its S is ||g64|| of the random-image case at the same shape under the same upstream
    gradient.  y = x + 1e-4 N: the gradient is not judged (ssim_ref says why), the value is.
Nothing in a bound comes from the kernel's output.  An oracle that is exactly 0 (theta = 0, ego without T) gives bound 0: the kernel
must be exactly 0 too.
"""
import contextlib
import functools
import math

import torch
import torch.nn.functional as F

import synth
import oracle.ref_loss as orc

U = 2.0 ** -24
FACTOR = 4.0
MIN_ROUNDINGS = 16
SEED = 11
MIN_DEPTH, MAX_DEPTH = 0.1, 100.0

# longest leaf-to-output path in the kernel, one per multiply / add / divide / sqrt / sin / cos (dd_ops.hip, dd_math.h)
ROUNDINGS = {
    "points": 5,           # A0*x, A1*y, +, +A2, *d
    "g_depth": 8,          # ray (4), *g, three terms added
    "pix": 20,             # Q (7), c (7), +eps, 1/x, *inv, 1/(w-1), *, -0.5
    "ego": 8,              # Q (7), -P
    "g_points": 34,        # Q (7), c2 (7), +eps, 1/x, u, gu*u, +gv*v, *inv, gQ (5), +ge, gP (7), -ge
    "ssim": 18,            # sx (8), /9 (2), mx*mx, sxx/9 - ., +vy, +C2, b1*b2, 1/d, n*inv_d, 1 - q
    "g_ssim": 36,          # 1/d as above (16), dmu (6), the three products (3), g*mult/9 (2), nine centres added (9)
    "scaled": 2, "depth": 3, "g_disp": 6,
    "T": 17,               # theta (6), +1e-7, 1/x, n, cos, 1-ca, x*x, *C, +ca; invert: *t and three terms added
    "g_axisangle": 31,     # n (9), gR (2), acc (5), C*acc, sa*(.) (3), dot (5), *inv*inv*dth (3), -, gth*dth, +
    "g_translation": 17,   # R (13), *g, three terms added
    "chain": 88,           # disp_to_depth (3) + backproject (5) + project (34) + grid_sample (10) + SSIM (36)
}


def floor_factor(qty):
    return max(ROUNDINGS[qty], MIN_ROUNDINGS) * U


# ---- the oracle in either precision ----------------------------------------------------------------------------------------------
@contextlib.contextmanager
def grid_as(dtype):
    """oracle.ref_loss.pixel_grid is fp32 by construction; the integers it holds are exact in both types."""
    grid32 = orc.pixel_grid
    orc.pixel_grid = lambda *a, **k: grid32(*a, **k).to(dtype)
    try:
        yield
    finally:
        orc.pixel_grid = grid32


def run(fn, args, needs, weights, dtype=torch.float32, device="cpu"):
    """fn(*args) -> outputs; sum(output * weight) (weight None: the output is not used downstream) differentiated with respect to
    the args flagged in `needs`.  Returns ([outputs], [gradient or None per arg]) as float64 CPU tensors."""
    leaves = []
    for a, need in zip(args, needs):
        if torch.is_tensor(a) and a.is_floating_point():
            a = a.detach().to(device=device, dtype=dtype).requires_grad_(bool(need))
        leaves.append(a)
    with grid_as(dtype):
        outs = fn(*leaves)
        outs = list(outs) if isinstance(outs, (tuple, list)) else [outs]
        total = None
        for o, w in zip(outs, weights):
            if w is not None:
                t = (o * w.to(device=device, dtype=dtype).reshape(o.shape)).sum()
                total = t if total is None else total + t
        wanted = [a for a, need in zip(leaves, needs) if need]
        got = torch.autograd.grad(total, wanted, allow_unused=True) if wanted and total is not None else []
    if device != "cpu":
        torch.cuda.synchronize()
    grads, it = [], iter(got)
    for a, need in zip(leaves, needs):
        g = next(it) if need else None
        grads.append(None if g is None else g.detach().double().cpu())
    return [o.detach().double().cpu() for o in outs], grads


class Ref:
    pass


def reference(fn, args, needs, weights):
    r = Ref()
    r.args, r.needs, r.weights = args, needs, weights
    r.out64, r.g64 = run(fn, args, needs, weights, torch.float64)
    r.out32, r.g32 = run(fn, args, needs, weights, torch.float32)
    return r


# ---- the judge ---------------------------------------------------------------------------------------------------------------------
def _dist(t, norm):
    return float(t.abs().max()) if norm == "max" else float(t.norm())


class Judge:
    """Collects the comparisons of one case; finish() prints the case's `worst:` line (profiles/ops_parity.txt keeps them) and
    returns the failures."""

    def __init__(self, op, case):
        self.op, self.case, self.rows, self.fails = op, case, [], []

    def check(self, qty, got, want64, want32, norm, kind=None, scale=None, floor=None):
        """kind: the key of ROUNDINGS (default: qty).  scale: S when it is not the tensor's own.  floor: replaces F * S (sums)."""
        want64 = torch.zeros_like(got, dtype=torch.float64, device="cpu") if want64 is None else want64
        want32 = torch.zeros_like(want64) if want32 is None else want32
        got = got.detach().double().cpu().reshape(want64.shape)
        want32 = want32.reshape(want64.shape)
        if not bool(torch.isfinite(got).all()):
            self.rows.append((qty, float("inf"), 0.0, 0.0))
            self.fails.append("%s: non-finite elements" % qty)
            return
        e_k, e_32 = _dist(got - want64, norm), _dist(want32 - want64, norm)
        s = _dist(want64, norm) if scale is None else scale
        fl = floor_factor(kind or qty) * s if floor is None else floor
        bound = max(FACTOR * e_32, fl)
        self.rows.append((qty, e_k, e_32, bound))
        if not e_k <= bound:
            self.fails.append("%s: e_k %.3e > bound %.3e (e_32 %.3e, floor %.3e)" % (qty, e_k, bound, e_32, fl))

    def equal(self, qty, got, want):
        """bit-identical tensors"""
        same = torch.equal(got.detach().cpu(), want.detach().cpu())
        self.rows.append((qty, 0.0 if same else float("inf"), 0.0, 0.0))
        if not same:
            self.fails.append("%s: not bit-identical" % qty)

    def finish(self):
        def ratio(row):
            return 0.0 if row[1] == 0.0 else (float("inf") if row[3] == 0.0 else row[1] / row[3])
        q, e_k, e_32, bound = max(self.rows, key=ratio)
        print("worst: %s | %s | %s | e_k %.3e | e_32 %.3e | bound %.3e | %d quantities" % (self.op, self.case, q, e_k, e_32, bound, len(self.rows)))
        return self.fails


# ---- BackprojectDepth / Project3D --------------------------------------------------------------------------------------------------
GEOM_SHAPES = [(2, 2, 2),          # one partial wave; w-1 = h-1 = 1
               (1, 3, 50),         # less than one block
               (3, 16, 16),        # exactly one full block
               (2, 24, 40),        # the golden's shape
               (1, 129, 512)]      # 258 blocks: fold16's second trip for threads 0 and 1
GAP = 0.1                          # behind-camera scenes: no transformed depth within GAP/2 (less the rotation's share) of 0


def _gen(*key):
    return torch.Generator().manual_seed(SEED + sum((i + 1) * int(k) for i, k in enumerate(key)))


@functools.lru_cache(maxsize=None)
def scene(B, h, w, kind, skew=False):
    """Intrinsics, depth and a pose from tests/golden/synth.py.  kind 'behind': the depths above their 30 % quantile move GAP further
    out and the pose's z translation is set to -(quantile + GAP/2): about 30 % of the points land behind the camera and none near its
    plane.  skew: a K with a fourth column and a T with a last row that is not (0,0,0,1) -- the kernels multiply all four components."""
    s = Ref()
    k = synth.make_intrinsics(B, h, w, 1)
    s.K, s.inv_K = k[("K", 0)].clone(), k[("inv_K", 0)].clone()
    leaves = synth.make_leaves(SEED, B, h, w, [0])
    s.disp = leaves[("disp", 0)].detach()
    s.depth = orc.disp_to_depth(s.disp, MIN_DEPTH, MAX_DEPTH)[1].contiguous()
    s.T = orc.pose_matrix(leaves[("axisangle", 1)].detach(), leaves[("translation", 1)].detach(), invert=True).contiguous()
    if kind == "behind":
        q = float(torch.quantile(s.depth.flatten(), 0.3))
        s.depth = s.depth + GAP * (s.depth > q)
        s.T[:, 2, 3] = -(q + GAP / 2)
    elif kind != "front":
        raise ValueError(kind)
    if skew:
        s.K[:, :3, 3] = torch.tensor([0.3, -0.2, 0.05])
        s.T[:, 3, :] = torch.tensor([0.01, -0.02, 0.03, 1.1])
    s.points = orc.backproject(s.depth, s.inv_K).contiguous()           # fp32: the operator's input
    s.moved = torch.matmul(s.T, s.points).contiguous()                  # the same scene for the runs without T
    g = _gen(B, h, w)
    s.w_points = torch.randn(B, 4, h * w, generator=g)
    s.w_pix = torch.randn(B, h, w, 2, generator=g)
    s.w_ego = torch.randn(B, 3, h * w, generator=g)
    s.dims = (B, h, w)
    return s


def camera_z(s, with_T=True):
    """c2 + eps of Project3D in float64 for the scene's points"""
    pts = s.points.double() if with_T else s.moved.double()
    moved = torch.matmul(s.T.double(), pts) if with_T else pts
    return torch.matmul(s.K.double()[:, :3, :], moved)[:, 2, :] + 1e-7


@functools.lru_cache(maxsize=None)
def backproject_ref(B, h, w, kind):
    s = scene(B, h, w, kind)
    return reference(lambda d: orc.backproject(d, s.inv_K.to(d.dtype)), [s.depth], [True], [s.w_points])


@functools.lru_cache(maxsize=None)
def project_ref(B, h, w, kind, with_T, which, skew=False):
    """which: 'pix', 'ego' or 'both' -- the outputs used downstream"""
    s = scene(B, h, w, kind, skew)
    wp = s.w_pix if which in ("pix", "both") else None
    we = s.w_ego if which in ("ego", "both") else None
    if with_T:
        r = reference(lambda p, T: orc.project(p, s.K.to(p.dtype), T, h, w), [s.points, s.T], [True, True], [wp, we])
    else:
        r = reference(lambda p: orc.project(p, s.K.to(p.dtype), None, h, w), [s.moved], [True], [wp, we])
    r.scene, r.w_pix, r.w_ego = s, wp, we
    r.gT_floor = sum_floor_gT(s, wp, we) if with_T else None
    return r


def sum_floor_gT(s, w_pix, w_ego):
    """g_T[b,i,k] = sum over the pixels of gQ[b,i,n] * P[b,k,n]: 2^-24 (log2 n + 4) sum|term| per element, terms in float64, as the L2
    norm over the tensor's elements.  gQ is the oracle's own gradient at the transformed points."""
    B, h, w = s.dims
    P = s.points.double()
    moved = torch.matmul(s.T.double(), P).detach().requires_grad_()
    gQ = torch.zeros_like(moved)
    if w_pix is not None:
        pix, _ = orc.project(moved, s.K.double(), None, h, w)
        gQ = gQ + torch.autograd.grad((pix * w_pix.double()).sum(), moved)[0]
    if w_ego is not None:
        gQ[:, :3] += w_ego.double()
    terms = torch.einsum("bin,bkn->bik", gQ.abs(), P.abs())
    return float((U * (math.log2(h * w) + 4) * terms).norm())


# ---- SSIM --------------------------------------------------------------------------------------------------------------------------
SSIM_EDGE_SHAPES = [(2, 3, 2, 2), (2, 3, 3, 3), (1, 3, 2, 7), (1, 1, 4, 3)]      # H or W of 2, 3 or 4
SSIM_SHAPES = [(2, 3, 5, 67),      # blocks straddle rows and end mid-row
               (1, 3, 19, 45)]     # general small image
SSIM_KINDS = ("random", "flat", "same", "near")
SSIM_DEGENERATE = ("same", "near")
SSIM_GRADIENT_NOT_JUDGED = ("near",)


@functools.lru_cache(maxsize=None)
def ssim_ref(shape, kind):
    g = _gen(*shape)
    up = torch.randn(shape, generator=g)                    # the same upstream gradient for every kind at a shape
    x = torch.rand(shape, generator=g)
    if kind == "random":
        y = torch.rand(shape, generator=g)
    elif kind == "flat":
        # bright and flat: the cancellation in sxx/9 - mx^2 (variance 1e-6 under a square of 0.8), in both images.  y sits at 0.7:
        # with both at 0.9 the value is ~1e-3, within 4 x the fp32 oracle's own value error (2e-4) of the clamp at 0, the clamp's
        # pass decision is then rounding's and the oracle's e_32 on the gradient jumps between 2e-4 and 2e-2 from seed to seed; at
        # 0.7 the value is 1.5e-2 and the cancellation is the same (test_ops_inputs asserts both)
        x = 0.9 + 1e-3 * torch.randn(shape, generator=g)
        y = 0.7 + 1e-3 * torch.randn(shape, generator=g)
    elif kind == "same":
        y = x.clone()
    elif kind == "near":
        # the true value is ~3e-8 here, below the rounding of n/d in fp32: which windows fall under the clamp at 0 and lose their
        # gradient is rounding's choice in every fp32 implementation, the oracle's included (its g32 sits 0.2 .. 0.9 of ||g64|| from
        # g64 depending on the draw), so 4 x e_32 is no bar for another implementation's decisions.  The value is judged; the
        # gradient of this kind is only required to be finite (test_ops_inputs asserts the value's size, the reason).
        y = x + 1e-4 * torch.randn(shape, generator=g)
    else:
        raise ValueError(kind)
    r = reference(orc.ssim_map, [x, y], [True, True], [up])
    r.scale = [None, None]
    if kind in SSIM_DEGENERATE:
        r.scale = [float(t.norm()) for t in ssim_ref(shape, "random").g64]
    return r


# ---- disp_to_depth -----------------------------------------------------------------------------------------------------------------
BLOCK, MAX_BLOCKS = 256, 4096                               # stated here, not imported: the launch of dd_disp_to_depth
DISP_SIZES = [1, 255, 257, MAX_BLOCKS * BLOCK + 257]        # the last: the grid-stride loop's second trip (4 MB)


@functools.lru_cache(maxsize=None)
def disp_ref(n):
    g = _gen(n)
    disp = 1e-3 + (1 - 1e-3) * torch.rand(n, generator=g)
    disp[0] = 0.0
    if n > 2:
        disp[1] = 1.0
    return reference(lambda d: orc.disp_to_depth(d, MIN_DEPTH, MAX_DEPTH), [disp], [True],
                     [torch.randn(n, generator=g), torch.randn(n, generator=g)])


# ---- pose matrix -------------------------------------------------------------------------------------------------------------------
POSE_BATCHES = [1, 63, 64, 65, 130]                         # 64-thread blocks
POSE_SWEEP = [3.0, 1.0, 1e-2, 1e-3, 1e-4, 1e-5, 1e-6, 1e-8, 0.0]
POSE_SWEEP_B = 65


@functools.lru_cache(maxsize=None)
def pose_ref(B, kind, invert):
    """kind: a float s (|aa| ~ s N(0,1)), 'mixed' (every third row exactly 0, the rest 1e-2 N) or 'pi' (theta within 1e-3 of pi)."""
    g = _gen(B, 7)
    aa = torch.randn(B, 1, 3, generator=g)
    if kind == "mixed":
        aa = 1e-2 * aa
        aa[::3] = 0.0
    elif kind == "pi":
        aa = aa / aa.norm(dim=2, keepdim=True) * (math.pi + 1e-3 * (2 * torch.rand(B, 1, 1, generator=g) - 1))
    else:
        aa = float(kind) * aa
    tr = 0.1 * torch.randn(B, 1, 3, generator=g)
    return reference(lambda a, t: orc.pose_matrix(a, t, invert=invert), [aa, tr], [True, True], [torch.randn(B, 4, 4, generator=g)])


# ---- the chain ---------------------------------------------------------------------------------------------------------------------
CHAIN_SHAPE = (1, 129, 512)
TAP_BAND = 1e-3       # pixels: a sample this close to an integer coordinate may take the other pair of taps in fp32


def chain_fn(ops, K, inv_K, img_src, img_tgt, h, w, band):
    """disp_to_depth -> BackprojectDepth -> Project3D(T from the pose) -> grid_sample -> SSIM -> mean.  ops: the five operators.
    band (B,1,h,w) bool: pixels whose bilinear taps are decided by rounding; their sample is taken as a constant on both sides."""
    d2d, backproject, project, pose, ssim = ops

    def fn(disp, aa, tr):
        _, depth = d2d(disp, MIN_DEPTH, MAX_DEPTH)
        pix, _ = project(backproject(depth, inv_K.to(disp)), K.to(disp), pose(aa, tr, True), h, w)
        warped = F.grid_sample(img_src.to(disp), pix, padding_mode="border", align_corners=False)
        if band is not None:
            warped = torch.where(band.to(warped.device), warped.detach(), warped)
        return ssim(warped, img_tgt.to(disp)).mean()
    return fn


ORACLE_OPS = (orc.disp_to_depth, orc.backproject, orc.project, lambda a, t, inv: orc.pose_matrix(a, t, invert=inv), orc.ssim_map)


@functools.lru_cache(maxsize=None)
def chain_ref():
    B, h, w = CHAIN_SHAPE
    s = scene(B, h, w, "front")
    leaves = synth.make_leaves(SEED, B, h, w, [0])
    aa, tr = leaves[("axisangle", -1)].detach(), leaves[("translation", -1)].detach()
    frames = synth.make_frames(_gen(B, h, w, 3), B, h, w)
    # the tap band, from the float64 oracle alone
    with grid_as(torch.float64):
        depth = orc.disp_to_depth(s.disp.double(), MIN_DEPTH, MAX_DEPTH)[1]
        pix, _ = orc.project(orc.backproject(depth, s.inv_K.double()), s.K.double(), orc.pose_matrix(aa.double(), tr.double(), invert=True), h, w)
    px = ((pix[..., 0] + 1) * w - 1) / 2
    py = ((pix[..., 1] + 1) * h - 1) / 2
    band = ((px - px.round()).abs() < TAP_BAND) | ((py - py.round()).abs() < TAP_BAND)
    band = band.unsqueeze(1)
    r = reference(chain_fn(ORACLE_OPS, s.K, s.inv_K, frames[1], frames[0], h, w, band), [s.disp, aa, tr], [True, True, True], [torch.ones(())])
    r.scene, r.frames, r.band, r.aa, r.tr = s, frames, band, aa, tr
    return r
