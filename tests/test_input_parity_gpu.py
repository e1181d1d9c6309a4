"""The input-side kernels on hard content (tests/input_case.py; tests/test_input_inputs.py asserts on the CPU that the cases are what
they claim): dd_jpeg_decode against PIL bit for bit, dd_prepare_frames and dd_pyramid_down2 against float64.

dd_jpeg_decode (csrc/dd_jpeg.hip): one decode_batch call per geometry carries every content (noise, 0/255 edges, saturated halves,
primaries), quality 1 .. 100, standard and optimised Huffman tables, every restart interval and the custom quantisation tables of
that geometry, so that images 0 and 1 never share their tables; sizes from 1x1 (less than one MCU) up; a scan behind 70 KB of
metadata.  The bytes behind each file's end are not zero (what the bit reader feeds itself at the end of a stream), and the output
and the workspace lie between guard bands.
dd_prepare_frames / dd_pyramid_down2 (csrc/dd_input.hip): judged by float64, the own error beside the float32 oracle's where the
bound is relative to it, outputs between NaN guard bands."""
import ctypes as C

import numpy as np
import pytest
import torch

import input_case as IC
from test_mlp_stage3_gpu import _guarded, _intact

pytestmark = pytest.mark.gpu

BAND = 4096                                # bytes of 0xA5 around the decoder's output and workspace (keeps their 16-byte alignment)
OVERREAD_GEOMETRIES = [g for g in IC.JPEG_GEOMETRIES if g[:3] in ((17, 33, 3), (101, 67, 3))]
GUARDED_GEOMETRIES = [g for g in IC.JPEG_GEOMETRIES if g[:3] == (101, 67, 3) or g[2] == 1]


def _upload(files, fill):
    """the files of a batch side by side in one (n, cap) buffer, `fill` behind each file's end (at least 64 bytes of it), and
    their header records"""
    from hipops import jpeg
    recs, geoms = zip(*[jpeg.parse_header(f.data) for f in files])
    assert len(set(geoms)) == 1
    cap = (max(len(f.data) for f in files) + 64 + 4095) // 4096 * 4096
    buf = np.full((len(files), cap), fill, np.uint8)
    for i, f in enumerate(files):
        buf[i, :len(f.data)] = np.frombuffer(f.data, np.uint8)
    return torch.from_numpy(buf).cuda(), torch.from_numpy(np.stack(recs)).cuda(), geoms[0]


def _decode(files, fill=0):
    from hipops import jpeg
    data, hdrs, (w, h, nc, hs, vs) = _upload(files, fill)
    out = jpeg.decode_batch(data, hdrs, h, w, nc, hs, vs)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _same(got, want, files, what=""):
    """bit for bit; on a mismatch: max |diff|, the share of differing pixels, the first differing (image, y, x) and its file"""
    assert got.shape == want.shape, (got.shape, want.shape)
    if np.array_equal(got, want):
        return
    diff = np.abs(got.astype(np.int32) - want.astype(np.int32)).max(-1)
    img, y, x = (int(v) for v in np.argwhere(diff > 0)[0])
    pytest.fail("%s max |diff| %d, %.4f of the pixels differ in %d of %d images, first at (image %d, y %d, x %d) of '%s': %s != PIL's %s" % (
        what, diff.max(), float((diff > 0).mean()), int((diff.reshape(len(diff), -1).max(1) > 0).sum()), len(diff), img, y, x,
        files[img].label, got[img, y, x].tolist(), want[img, y, x].tolist()))


@pytest.mark.parametrize("geom", IC.JPEG_GEOMETRIES, ids=IC.batch_id)
def test_jpeg_decoder_equals_pil(geom):
    files = IC.jpeg_batches()[geom]
    _same(_decode(files), IC.pil_batch(geom), files)


@pytest.mark.parametrize("geom", OVERREAD_GEOMETRIES, ids=IC.batch_id)
def test_jpeg_decoder_ignores_the_bytes_behind_a_file(geom):
    """zeros are what the bit reader feeds itself at the end of a stream, so only other bytes behind data_end show a read past it"""
    files = IC.jpeg_batches()[geom]
    for fill in (0xA5, 0xFF):
        _same(_decode(files, fill), IC.pil_batch(geom), files, "with 0x%02X behind the files:" % fill)


@pytest.mark.parametrize("geom", GUARDED_GEOMETRIES, ids=IC.batch_id)
def test_jpeg_decoder_stays_inside_its_buffers(geom):
    """dd_jpeg_workspace_bytes / dd_jpeg_decode through the C ABI: rgb between two 0xA5 bands, the workspace (0xA5-filled, not zeroed)
    between two more, the second one past workspace_bytes.  Pre-filled with 0x00 and then with 0xFF, rgb must be PIL's both times:
    a byte the kernels skip keeps a value that is wrong in one of the two runs."""
    from hipops import lib as L
    lib = L.load()
    files = IC.jpeg_batches()[geom]
    data, hdrs, (w, h, nc, hs, vs) = _upload(files, 0xA5)
    n = len(files)
    hv = (C.c_int * 3)(*hs), (C.c_int * 3)(*vs)
    need = int(lib.dd_jpeg_workspace_bytes(n, h, w, nc, hv[0], hv[1]))
    assert need > 0
    size = n * h * w * 3
    for prefill in (0x00, 0xFF):
        out = torch.full((BAND + size + BAND,), 0xA5, dtype=torch.uint8, device="cuda")
        out[BAND:BAND + size] = prefill
        ws = torch.full((BAND + need + BAND,), 0xA5, dtype=torch.uint8, device="cuda")
        L.check(lib.dd_jpeg_decode(C.c_void_p(data.data_ptr()), data.shape[1], C.c_void_p(hdrs.data_ptr()), n, h, w, nc, hv[0], hv[1],
                                   C.c_void_p(out.data_ptr() + BAND), C.c_void_p(ws.data_ptr() + BAND), need, L.current_stream()), "dd_jpeg_decode")
        torch.cuda.synchronize()
        for name, buf, inner in (("rgb", out, size), ("workspace", ws, need)):
            assert bool((buf[:BAND] == 0xA5).all()), "%s: the band in front was written (pre-fill 0x%02X)" % (name, prefill)
            assert bool((buf[BAND + inner:] == 0xA5).all()), "%s: the band behind was written (pre-fill 0x%02X)" % (name, prefill)
        _same(out[BAND:BAND + size].view(n, h, w, 3).cpu().numpy(), IC.pil_batch(geom), files, "pre-fill 0x%02X:" % prefill)


@pytest.mark.parametrize("shape", IC.JITTER_CASES, ids=str)
def test_prepare_frames_against_float64(shape):
    """color = u8 / 255 flipped and color_aug = color where apply = 0, bit for bit; elsewhere the own distance from the float64
    jitter is at most twice the float32 oracle's, with the floor of tests/test_mlp_narrow_train_gpu.py (2e-6; values in [0,1])."""
    from hipops import lib as L
    lib = L.load()
    B, F, H, W = shape
    case, ref = IC.jitter_case(shape), IC.jitter_ref(shape)
    frames, params, flip = case.frames.cuda().contiguous(), case.params.cuda().contiguous(), case.flip.cuda().contiguous()
    n = F * B * 3 * H * W
    n_ws = int(lib.dd_prepare_frames_workspace_bytes(B, F)) // 4
    assert n_ws >= 1
    (cbuf, color), (abuf, aug), (wbuf, ws) = _guarded(n), _guarded(n), _guarded(n_ws)
    L.check(lib.dd_prepare_frames(C.c_void_p(frames.data_ptr()), C.c_void_p(params.data_ptr()), C.c_void_p(flip.data_ptr()), B, F, H, W,
                                  C.c_void_p(color.data_ptr()), C.c_void_p(aug.data_ptr()), C.c_void_p(ws.data_ptr()), L.current_stream()), "dd_prepare_frames")
    torch.cuda.synchronize()
    assert _intact(cbuf, n) and _intact(abuf, n) and _intact(wbuf, n_ws)
    assert not bool(torch.isnan(color).any()) and not bool(torch.isnan(aug).any()) and not bool(torch.isnan(ws).any())
    color, aug = color.view(F, B, 3, H, W).cpu(), aug.view(F, B, 3, H, W).cpu()
    assert torch.equal(color, ref.color)
    idle = ~ref.applied
    assert torch.equal(aug[idle], ref.color[idle])
    on = ref.applied
    e_own = float((aug[on].double() - ref.aug64[on]).abs().max())
    e_oracle = float((ref.aug32[on].double() - ref.aug64[on]).abs().max())
    print("prepare_frames %s: color_aug against float64: own %.2e  float32 oracle %.2e" % (shape, e_own, e_oracle))
    assert e_own <= max(2.0 * e_oracle, 2e-6), (e_own, e_oracle)


@pytest.mark.parametrize("H,W", IC.PYRAMID_SHAPES)
def test_pyramid_against_float64(H, W):
    """every plane count and content of the shape: within 2e-6 of clamp(float64 restatement, 0, 1) (values in [0,1]; output width 1
    included, where torch is no reference); all-zero input gives exactly zero; the destination between NaN guard bands"""
    from hipops import lib as L
    lib = L.load()
    h, w = H // 2, W // 2
    worst = 0.0
    for planes in IC.PYRAMID_PLANES:
        for kind in IC.PYRAMID_KINDS:
            x = IC.pyramid_input(H, W, planes, kind).cuda().contiguous()
            n = planes * h * w
            buf, dst = _guarded(n)
            L.check(lib.dd_pyramid_down2(C.c_void_p(x.data_ptr()), planes, H, W, C.c_void_p(dst.data_ptr()), L.current_stream()), "dd_pyramid_down2")
            torch.cuda.synchronize()
            assert _intact(buf, n) and not bool(torch.isnan(dst).any()), (planes, kind)
            got = dst.view(1, planes, h, w).cpu().numpy()
            if kind == "zero":
                assert not got.any(), planes
                continue
            err = float(np.abs(got.astype(np.float64) - np.clip(IC.pyramid_ref(H, W, planes, kind), 0.0, 1.0)).max())
            worst = max(worst, err)
            assert err <= 2e-6, (planes, kind, err)
    print("pyramid_down2 (%d,%d): worst error against float64 %.2e" % (H, W, worst))
