"""dd_export_depth / dd_export_plane_u8 on the device against the numpy definition (hipops/export.py), bit for bit: every output and
every subset of outputs at the shapes of export_case.SHAPES, with and without the flip post-processing, the value cases (NaN, 0, 1,
rounding ties) embedded; the arguments the wrappers and the entry points refuse; nothing written outside a requested output."""
import numpy as np
import pytest
import torch

import export_case as EC

pytestmark = pytest.mark.gpu

IDS = ["x".join(str(v) for v in s) for s in EC.SHAPES]


def same_bits(got, want):
    """Equal bit for bit; float NaNs equal as NaNs (their payload is not part of the definition)."""
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    if got.dtype == np.float32:
        nan = np.isnan(want)
        return np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))
    return np.array_equal(got, want)


@pytest.mark.parametrize("flip", [False, True], ids=["plain", "pp"])
@pytest.mark.parametrize("shape", EC.SHAPES, ids=IDS)
def test_export_depth_is_the_host_definition(shape, flip):
    from hipops.export import depth_params, export_depth
    B, h, w, H, W = shape
    disp, flipped = (torch.from_numpy(a.copy()).cuda() for a in EC.disparities(B, h, w))
    want = EC.host_reference(B, h, w, H, W, flip)
    assert not np.isnan(want["depth"]).all()
    if h * w > 1 and H >= h and W >= w:
        assert np.isnan(want["depth"]).any() and (want["depth16"] == 0).any()       # the embedded NaN reaches the output
    for subset in EC.SUBSETS:
        got = export_depth(disp.unsqueeze(1), H, W, disp_flipped=flipped if flip else None, min_depth=EC.MIN_DEPTH, max_depth=EC.MAX_DEPTH, want=subset)
        assert sorted(got) == sorted(subset)
        for name in subset:
            assert got[name].is_cuda and same_bits(got[name], want[name]), (shape, flip, subset, name)
    if (H, W) == (h, w) and not flip:                       # same size: the blend passes s through, depth is 1 / s exactly
        lo, span = depth_params(EC.MIN_DEPTH, EC.MAX_DEPTH)
        s = (lo + span * EC.disparities(B, h, w)[0]).astype(np.float32)
        clean = ~np.isnan(want["depth"])
        with np.errstate(all="ignore"):
            assert same_bits(got["depth"].cpu().numpy()[clean], (np.float32(1) / s)[clean])


@pytest.mark.parametrize("shape", EC.SHAPES, ids=IDS)
def test_export_plane_u8_is_the_host_definition(shape):
    from hipops.export import export_plane_u8
    B, h, w, H, W = shape
    plane = torch.from_numpy(EC.disparities(B, h, w)[0] * 1.5 - 0.2).cuda()
    want = EC.host_reference(B, h, w, H, W, False)["plane_u8"]
    for p in (plane, plane.unsqueeze(1)):
        assert same_bits(export_plane_u8(p, H, W), want), shape
    if h * w > 8 and H >= h and W >= w:                     # both clamps are exercised (down-scaling steps over the embedded 0 and 1)
        assert want.min() == 0 and want.max() == 255


def test_depth_scale_and_colour_range():
    """Another depth_scale (saturation at 65535) and another colour range than the defaults."""
    from hipops.export import export_depth, export_depth_host
    B, h, w, H, W = EC.SHAPES[4]
    disp = EC.disparities(B, h, w, values=False)[0].copy()
    disp[0, :3, :5] = 0.0                                    # depth 100: beyond 65535 at a scale of 1000
    kwargs = dict(min_depth=EC.MIN_DEPTH, max_depth=EC.MAX_DEPTH, depth_scale=1000.0, vmin=0.1, vmax=0.7)
    want = export_depth_host(disp, H, W, **kwargs)
    got = export_depth(torch.from_numpy(disp.copy()).cuda(), H, W, want=EC.SUBSETS[-1], **kwargs)
    assert (want["depth16"] == 65535).any() and (want["depth16"] < 65535).any()
    assert all(same_bits(got[k], want[k]) for k in want)


def test_bad_arguments_are_refused():
    from hipops import abi, lib as L
    from hipops.export import export_depth, export_plane_u8
    from hipops.lib import DynamoHipError
    disp = torch.rand(2, 1, 4, 6, device="cuda")
    kw = dict(min_depth=0.1, max_depth=100.0)
    for bad in (lambda: export_depth(disp.cpu(), 8, 12, **kw),
                lambda: export_depth(disp, 8, 12, disp_flipped=disp.cpu(), **kw),
                lambda: export_depth(disp, 8, 12, disp_flipped=disp[:, :, :, :5], **kw),
                lambda: export_depth(disp, 8, 12, disp_flipped=disp[:1], **kw),
                lambda: export_depth(disp, 0, 12, **kw),
                lambda: export_depth(disp, 8, 0, **kw),
                lambda: export_depth(disp, 8, 12, want=(), **kw),
                lambda: export_depth(disp, 8, 12, want=("depth", "flow"), **kw),
                lambda: export_depth(disp.double(), 8, 12, **kw),
                lambda: export_depth(disp, 8, 12, min_depth=0.0, max_depth=100.0),
                lambda: export_plane_u8(disp.cpu(), 8, 12),
                lambda: export_plane_u8(disp, 8, 0),
                lambda: export_plane_u8(disp[0, 0, 0], 8, 12)):
        with pytest.raises(DynamoHipError):
            bad()
    # the entry points themselves: every refusal returns hipErrorInvalidValue and leaves the poisoned outputs alone
    lib, s = L.load(), L.current_stream()
    d = disp[:, 0].contiguous()
    mask, lut = torch.zeros(6, device="cuda"), torch.zeros(256, dtype=torch.int32, device="cuda")
    depth = torch.full((2, 8, 12), 7.0, device="cuda")
    d16 = torch.full((2, 8, 12), 7, dtype=torch.int16, device="cuda")
    rgb = torch.full((2, 8, 12, 3), 7, dtype=torch.uint8, device="cuda")
    P = abi.ptr
    good = [P(d), None, None, 2, 4, 6, 8, 12, 0.1, 100.0, 256.0, P(lut), 0.0, 1.0, P(depth), P(d16), P(rgb)]

    def call(**change):
        names = ["disp", "flip", "mask", "B", "h", "w", "H", "W", "min_depth", "max_depth", "scale", "lut", "vmin", "vmax", "depth", "d16", "rgb"]
        args = list(good)
        for k, v in change.items():
            args[names.index(k)] = v
        return lib.dd_export_depth(*args, s)

    off = lambda t, n: abi.C.c_void_p(t.data_ptr() + n)           # noqa: E731
    assert call(disp=None) == 1 and call(flip=P(d)) == 1 and call(mask=P(mask)) == 1 and call(lut=None) == 1 and call(rgb=None) == 1
    assert call(depth=None, d16=None, rgb=None, lut=None) == 1
    assert all(call(**{k: 0}) == 1 for k in ("B", "h", "w", "H", "W")) and call(H=-3) == 1
    assert call(H=65536, W=32768) == 1 and call(h=65536, w=32768) == 1            # 2**31 pixels
    assert call(min_depth=0.0) == 1 and call(max_depth=float("nan")) == 1
    assert call(disp=off(d, 2)) == 1 and call(depth=off(depth, 2)) == 1 and call(d16=off(d16, 1)) == 1 and call(lut=off(lut, 1)) == 1
    assert call(flip=P(d), mask=off(mask, 2)) == 1
    out = torch.full((2, 8, 12), 7, dtype=torch.uint8, device="cuda")
    assert lib.dd_export_plane_u8(None, 2, 4, 6, 8, 12, P(out), s) == 1 and lib.dd_export_plane_u8(P(d), 2, 4, 6, 8, 12, None, s) == 1
    assert lib.dd_export_plane_u8(P(d), 2, 4, 6, 0, 12, P(out), s) == 1 and lib.dd_export_plane_u8(off(d, 1), 2, 4, 6, 8, 12, P(out), s) == 1
    torch.cuda.synchronize()
    assert bool((depth == 7).all()) and bool((d16 == 7).all()) and bool((rgb == 7).all()) and bool((out == 7).all())
    assert call() == 0 and lib.dd_export_plane_u8(P(d), 2, 4, 6, 8, 12, P(out), s) == 0
    torch.cuda.synchronize()
    assert not bool((depth == 7).any()) and bool((d16 != 7).any()) and bool((rgb != 7).any())


@pytest.mark.parametrize("shape", [EC.SHAPES[1], EC.SHAPES[4]], ids=[IDS[1], IDS[4]])
def test_only_the_requested_output_is_written(shape):
    """The raw entry points on outputs inside one poisoned arena, each at an odd distance from the arena's start (unaligned rows and a
    W that is no multiple of 4): every byte outside the requested output keeps the poison, every byte inside equals the definition."""
    from hipops import abi, lib as L
    from hipops.vis import lut_words
    B, h, w, H, W = shape
    lib, s = L.load(), L.current_stream()
    disp = torch.from_numpy(EC.disparities(B, h, w)[0].copy()).cuda()
    want = EC.host_reference(B, h, w, H, W, False)
    lut = torch.from_numpy(lut_words()[0].astype(np.int32)).cuda()
    n = B * H * W
    for name, item, lead in (("depth", 4, 36), ("depth16", 2, 38), ("rgb", 3, 37), ("plane_u8", 1, 39)):
        size = n * item
        arena = torch.full((lead + size + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        at = abi.C.c_void_p(arena.data_ptr() + lead)
        if name == "plane_u8":
            plane = (disp * 1.5 - 0.2).contiguous()
            code = lib.dd_export_plane_u8(abi.ptr(plane), B, h, w, H, W, at, s)
        else:
            code = lib.dd_export_depth(abi.ptr(disp), None, None, B, h, w, H, W, EC.MIN_DEPTH, EC.MAX_DEPTH, 256.0, abi.ptr(lut) if name == "rgb" else None,
                                       0.0, 1.0, at if name == "depth" else None, at if name == "depth16" else None, at if name == "rgb" else None, s)
        assert code == 0, name
        host = arena.cpu().numpy()
        assert (host[:lead] == 0xA5).all() and (host[lead + size:] == 0xA5).all(), name
        got = host[lead:lead + size].copy().view(want[name].dtype).reshape(want[name].shape)
        assert same_bits(got, want[name]), name
