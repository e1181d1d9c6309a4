"""depth_metrics_kernel (dd_depth_metrics / dd_depth_metrics_masked, csrc/dd_metrics.hip) through the C ABI against the reference's
DepthMetrics and compute_errors in float64 on the CPU, stage by stage: the keep rule and the sampled depth of every point read back from
the workspace, the four error metrics and the three accuracy counts overall and per label, the batch mean.  Cases: identity,
x2 / x4 dyadic (bit equality with ATen), a non-integer up-scale, a down-scale, 1x1 / 1x13 / 13x1 disparities, two gt_dim in a batch, white
noise; points on every crop and depth bound and one step either side; n = 1, 2, 3, even n, equal values, duplicates across the middle,
ground truth and disparity that differ in one byte of the bit pattern, fifteen exponents, M = 1, 63, 1024, 1025, 2500; scaled predictions on and beyond both
clamp bounds; th exactly on every threshold; all 256 labels, single-point labels, a label under dropped points, n = 0 inside a masked
batch, a mask smaller than the ground truth.  Contracts: a sample alone or inside a batch, two launches, untouched slack, argument
checks, a NaN disparity.

The kernel keeps its two medians to itself.  What dm_select returns is held by the identity-geometry cases, where everything up to
abs_rel, sq_rel and rms is one correctly rounded fp32 operation after another: those three must lie within one fp32 ulp of that chain
restated in numpy (stage `fp32`), so a median one ulp off in the low bytes, one unit of the byte under test off, or the upper one fails.

tests/metrics_case.py holds the cases, the oracle and the criterion (nothing in a bound from the kernel's output);
tests/test_metrics_inputs.py asserts on the CPU that the inputs are what is claimed here.

Every case prints one `worst:` line (run with -s); profiles/metrics_parity.txt keeps those of one MI355X run as a record.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import metrics_case as MC

gpu = pytest.mark.gpu
HIP_ERROR_INVALID_VALUE = 1
SLACK = 64                    # floats of NaN behind every output and the workspace
NAN_BITS = 0x7FC00000


def _nan(n):
    return torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")


class Run:
    """one launch on case `c` (all of it), every output and the workspace pre-filled with NaN and followed by SLACK NaNs"""

    def __init__(self, c, masked=None):
        from hipops import abi
        from hipops import lib as L
        lib = L.load()
        self.c, self.masked = c, (c.mask is not None) if masked is None else masked
        B, M = c.B, c.M
        self.dev = [c.disp.cuda(), c.lidar.cuda().contiguous(), c.valid.cuda().contiguous(), c.gt_dim.cuda().contiguous()]
        self.mask = c.mask.cuda().contiguous() if self.masked else None
        self.bound = (C.c_double * 4)(*c.bound)
        self.nbytes = int((lib.dd_depth_metrics_masked_workspace_bytes if self.masked else lib.dd_depth_metrics_workspace_bytes)(B, M))
        assert self.nbytes == B * (3 if self.masked else 2) * M * 4
        self.sizes = {"per": B * 8, "mean": 7, "ws": self.nbytes // 4, "per_label": B * 256 * 8 if self.masked else 0}
        self.buf = {k: _nan(n + SLACK) for k, n in self.sizes.items()}
        self.abi, self.lib, self.L = abi, lib, L

    def args(self):
        p, c, d = self.abi.ptr, self.c, self.dev
        head = [p(d[0]), c.B, c.H, c.W, p(d[1]), p(d[2]), c.M, p(d[3]), self.bound, c.min_depth, c.max_depth]
        if self.masked:
            return head + [p(self.mask), self.mask.shape[1], self.mask.shape[2], p(self.buf["per"]), p(self.buf["mean"]), p(self.buf["per_label"]),
                           p(self.buf["ws"]), self.nbytes, self.L.current_stream()]
        return head + [p(self.buf["per"]), p(self.buf["mean"]), p(self.buf["ws"]), self.nbytes, self.L.current_stream()]

    def fn(self):
        return self.lib.dd_depth_metrics_masked if self.masked else self.lib.dd_depth_metrics

    def launch(self):
        self.L.check(self.fn()(*self.args()), "dd_depth_metrics")
        torch.cuda.synchronize()
        return self.read()

    def read(self):
        c, k = self.c, 3 if self.masked else 2
        host = {name: t.cpu().numpy() for name, t in self.buf.items()}
        self.host = host
        ws = host["ws"][:self.sizes["ws"]].reshape(c.B, k, c.M)
        out = {"per": host["per"][:c.B * 8].reshape(c.B, 8), "mean": host["mean"][:7], "gt": ws[:, 0], "pd": ws[:, 1],
               "label": ws[:, 2].view(np.int32) if self.masked else None,
               "per_label": host["per_label"][:c.B * 2048].reshape(c.B, 256, 8) if self.masked else None}
        return out

    def slack_untouched(self):
        return all(bool((self.host[k][n:].view(np.uint32) == NAN_BITS).all()) for k, n in self.sizes.items())

    def bytes(self):
        return b"".join(self.host[k].tobytes() for k in sorted(self.host))


def judge_run(c, os_, out, j, masked):
    for b, o in enumerate(os_):
        j.points(b, o, out["gt"][b], out["pd"][b], out["label"][b] if masked else None)
        j.sample(b, o, out["per"][b])
        if masked:
            j.labels(b, o, out["per_label"][b])
    j.mean(out["per"], out["mean"])


@gpu
@pytest.mark.parametrize("ci", range(len(MC.CASES)), ids=MC.CASE_IDS)
def test_depth_metrics(ci):
    """every case through the entry point it is made for (masked if it has a mask), judged stage by stage; a second launch gives the
    same bytes; the slack behind per_sample, mean, per_label and the workspace stays NaN.  The cases with a mask also run unmasked."""
    c, os_ = MC.CASES[ci], MC.oracle(ci)
    fails = []
    for masked in ((True, False) if c.mask is not None else (False,)):
        run = Run(c, masked)
        out = run.launch()
        j = MC.Judge(c, "dd_depth_metrics_masked" if masked else "dd_depth_metrics")
        judge_run(c, os_, out, j, masked)
        j.same("counts", run.slack_untouched(), "the slack behind an output or the workspace was written")
        first = run.bytes()
        again = Run(c, masked)
        again.launch()
        j.same("counts", again.bytes() == first, "a second launch gives other bytes")
        fails += j.finish()
    assert not fails, fails


@gpu
@pytest.mark.parametrize("name", ["two-gt-dims", "median-small-n", "masked-labels"])
def test_a_sample_alone_gives_the_row_it_gives_inside_a_batch(name):
    c = MC.by_name(name)
    whole = Run(c).launch()
    for b in range(c.B):
        alone = Run(MC.slice_case(c, b)).launch()
        assert np.array_equal(alone["per"][0].view(np.uint32), whole["per"][b].view(np.uint32)), (name, b, alone["per"][0], whole["per"][b])
        assert np.array_equal(alone["gt"][0].view(np.uint32), whole["gt"][b].view(np.uint32))
        assert np.array_equal(alone["pd"][0].view(np.uint32), whole["pd"][b].view(np.uint32))
        if c.mask is not None:
            assert np.array_equal(alone["per_label"][0].view(np.uint32), whole["per_label"][b].view(np.uint32))


@gpu
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
def test_argument_checks_return_invalid_value_and_write_nothing(masked):
    """each NULL pointer, B < 1, M < 1, a workspace one byte short: hipErrorInvalidValue, and every output and the workspace stay NaN"""
    c = MC.by_name("masked-small-mask")
    run = Run(c, masked)
    good = run.args()
    pointers = [i for i, a in enumerate(good[:-1]) if isinstance(a, C.c_void_p) or a is run.bound]
    assert len(pointers) == (10 if masked else 8)
    size_at = len(good) - 2
    variants = [(i, None) for i in pointers] + [(1, 0), (1, -1), (6, 0), (6, -3), (size_at, run.nbytes - 1), (size_at, 0)]
    for i, v in variants:
        a = list(good)
        a[i] = v
        err = run.fn()(*a)
        torch.cuda.synchronize()
        assert err == HIP_ERROR_INVALID_VALUE, (i, v, err)
    run.read()
    for k in run.host:
        assert bool((run.host[k].view(np.uint32) == NAN_BITS).all()), k
    run.launch()                                     # the untouched argument list is a good one
    assert bool(np.isfinite(run.host["per"][:8]).all())


@gpu
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
def test_nan_disparity_under_a_kept_point_gives_nan_errors(masked):
    """the sample's four error metrics are NaN, never a finite-looking number; the other samples' rows are the ones without the NaN.
    a1..a3 of that sample stay finite, and that is the contract written down here: the NaN prediction is left out of dm_select's
    histogram while n still counts it, so the ratio is finite; the NaN point compares false with every threshold and every other point
    is counted as usual, against n kept points"""
    import copy
    c = copy.copy(MC.by_name("masked-labels"))
    clean = Run(c, masked).launch()
    o = MC.oracle(MC.CASE_IDS.index("masked-labels"))[0]
    c.disp = c.disp.clone()
    c.disp[0, 0, int(o.y0[5]), int(o.x0[5])] = float("nan")              # a tap of kept point 5, weight > 0
    out = Run(c, masked).launch()
    assert bool(np.isnan(out["per"][0, :4]).all()), out["per"][0]
    assert out["per"][0, 7] == o.n
    assert bool(np.isfinite(out["per"][0, 4:7]).all()) and bool((out["per"][0, 4:7] >= 0).all()) and bool((out["per"][0, 4:7] < 1).all())
    assert np.array_equal(out["per"][1:].view(np.uint32), clean["per"][1:].view(np.uint32))
    if masked:
        lab = int(o.labels[5])
        assert bool(np.isnan(out["per_label"][0, lab, :4]).all())
        assert np.array_equal(out["per_label"][1:].view(np.uint32), clean["per_label"][1:].view(np.uint32))
