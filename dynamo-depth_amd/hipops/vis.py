"""Segment visualisation panels on the device (csrc/dd_vis.hip): the tiles image | disparity | ego flow | independent
flow | motion mask of the reference's eval/visualize.py (get_vis / combine_vis), as (N, R*H, C*W, 3) uint8 frames.

One launch per frame (`add_frame`: the tiles that do not depend on the segment's largest flow magnitude, every flow tile's
magnitude and hue into a side buffer, the running maxima) and one per segment (`finish`: the flow tiles, normalised by the
maximum the device holds).  Nothing is copied to the host before the caller's one `.cpu()` of the finished panel.

The colour-map tiles follow matplotlib's Normalize and Colormap.__call__ on fp32 data; the two tables below are
(uint8)(lut * 255) of matplotlib 3.10's 256-entry `plasma` and `hot` tables (tests/test_vis.py holds them to the installed
matplotlib): data, so that rendering needs no matplotlib."""
import ctypes as C

import numpy as np

from . import abi
from . import lib as L

FLOW_TILES = ("ego_flow", "ind_flow", "comp_flow", "samp_flow")

_PLASMA = (
    "0c078610078713068915068a18068b1b068c1d068d1f058e21058f2305902505912705922905932b05942d04942f04953104963304973404983604983804993a"
    "049a3b039a3d039b3f039c40039c42039d44039e45039e47029f49029f4a02a04c02a14e02a14f02a25101a25201a35401a35601a35701a45901a45a00a55c00"
    "a55e00a55f00a66100a66200a66400a76500a76700a76800a76a00a76c00a86d00a86f00a87000a87200a87300a87500a87601a87801a87901a87b02a87c02a7"
    "7e03a77f03a78104a78204a78405a68506a68607a68807a58908a58b09a48c0aa48e0ca48f0da3900ea3920fa29310a19511a19612a09713a099149f9a159e9b"
    "179e9d189d9e199c9f1a9ba01b9ba21c9aa31d99a41e98a51f97a72197a82296a92395aa2494ac2593ad2692ae2791af2890b02a8fb12b8fb22c8eb42d8db52e"
    "8cb62f8bb7308ab83289b93388ba3487bb3586bc3685bd3784be3883bf3982c03b81c13c80c23d80c33e7fc43f7ec5407dc6417cc7427bc8447ac94579ca4678"
    "cb4777cc4876cd4975ce4a75cf4b74d04d73d14e72d14f71d25070d3516fd4526ed5536dd6556dd7566cd7576bd8586ad95969da5a68db5b67dc5d66dc5e66dd"
    "5f65de6064df6163df6262e06461e16560e26660e3675fe3685ee46a5de56b5ce56c5be66d5ae76e5ae87059e87158e97257ea7356ea7455eb7654ec7754ec78"
    "53ed7952ed7b51ee7c50ef7d4fef7e4ef0804df0814df1824cf2844bf2854af38649f38748f48947f48a47f58b46f58d45f68e44f68f43f69142f79241f79341"
    "f89540f8963ff8983ef9993df99a3cfa9c3bfa9d3afa9f3afaa039fba238fba337fba436fca635fca735fca934fcaa33fcac32fcad31fdaf31fdb030fdb22ffd"
    "b32efdb52dfdb62dfdb82cfdb92bfdbb2bfdbc2afdbe29fdc029fdc128fdc328fdc427fdc626fcc726fcc926fccb25fccc25fcce25fbd024fbd124fbd324fad5"
    "24fad624fad824f9d924f9db24f8dd24f8df24f7e024f7e225f6e425f6e525f5e726f5e926f4ea26f3ec26f3ee26f2f026f2f126f1f326f0f525f0f623eff821"
)
_HOT = (
    "0a00000d00000f00001200001500001700001a00001c00001f00002200002400002700002a00002c00002f00003100003400003700003900003c00003f000041"
    "00004400004600004900004c00004e00005100005400005600005900005b00005e00006100006300006600006900006b00006e00007000007300007600007800"
    "007b00007e00008000008300008500008800008b00008d00009000009300009500009800009a00009d0000a00000a20000a50000a80000aa0000ad0000af0000"
    "b20000b50000b70000ba0000bd0000bf0000c20000c40000c70000ca0000cc0000cf0000d20000d40000d70000d90000dc0000df0000e10000e40000e70000e9"
    "0000ec0000ee0000f10000f40000f60000f90000fc0000fe0000ff0200ff0500ff0700ff0a00ff0c00ff0f00ff1200ff1400ff1700ff1a00ff1c00ff1f00ff21"
    "00ff2400ff2700ff2900ff2c00ff2f00ff3100ff3400ff3600ff3900ff3c00ff3e00ff4100ff4400ff4600ff4900ff4b00ff4e00ff5100ff5300ff5600ff5900"
    "ff5b00ff5e00ff6000ff6300ff6600ff6800ff6b00ff6e00ff7000ff7300ff7500ff7800ff7b00ff7d00ff8000ff8300ff8500ff8800ff8a00ff8d00ff9000ff"
    "9200ff9500ff9700ff9a00ff9d00ff9f00ffa200ffa500ffa700ffaa00ffac00ffaf00ffb200ffb400ffb700ffba00ffbc00ffbf00ffc100ffc400ffc700ffc9"
    "00ffcc00ffcf00ffd100ffd400ffd600ffd900ffdc00ffde00ffe100ffe400ffe600ffe900ffeb00ffee00fff100fff300fff600fff900fffb00fffe00ffff02"
    "ffff06ffff0affff0effff12ffff16ffff1affff1effff22ffff26ffff2affff2effff32ffff36ffff3affff3effff41ffff45ffff49ffff4dffff51ffff55ff"
    "ff59ffff5dffff61ffff65ffff69ffff6dffff71ffff75ffff79ffff7dffff80ffff84ffff88ffff8cffff90ffff94ffff98ffff9cffffa0ffffa4ffffa8ffff"
    "acffffb0ffffb4ffffb8ffffbcffffbfffffc3ffffc7ffffcbffffcfffffd3ffffd7ffffdbffffdfffffe3ffffe7ffffebffffeffffff3fffff7fffffbffffff"
)


def cmap_bytes(name):
    """(256, 3) uint8: byte = (uint8)(entry * 255) of the colour map's float table."""
    return np.frombuffer(bytes.fromhex({"plasma": _PLASMA, "hot": _HOT}[name]), dtype=np.uint8).reshape(256, 3).copy()


def lut_words():
    """(2, 256) int32 r | g << 8 | b << 16: the disparity tile's table (plasma), then the mask tile's (hot)."""
    t = np.stack([cmap_bytes("plasma"), cmap_bytes("hot")]).astype(np.int32)
    return t[..., 0] | (t[..., 1] << 8) | (t[..., 2] << 16)


def tile_list(arrangement):
    """[(kind, row, col), ...], R, C of a 2-D arrangement of tile names (rows may differ in length; the gaps stay black)."""
    if isinstance(arrangement, (str, bytes)) or len(arrangement) < 1 or any(isinstance(r, (str, bytes)) or len(r) < 1 for r in arrangement):
        raise L.DynamoHipError("an arrangement is a non-empty list of non-empty rows of tile names")
    tiles = []
    for r, row in enumerate(arrangement):
        for c, name in enumerate(row):
            if name not in abi.DD_VIS_KINDS:
                raise L.DynamoHipError("Arrangement name (={}) not recognized.".format(name))
            tiles.append((abi.DD_VIS_KINDS[name], r, c))
    if len(tiles) > abi.DD_VIS_MAX_TILES:
        raise L.DynamoHipError("an arrangement holds at most {} tiles, not {}".format(abi.DD_VIS_MAX_TILES, len(tiles)))
    return tiles, len(arrangement), max(len(row) for row in arrangement)


class SegmentRenderer:
    """Renders the frames of one segment after another into one device buffer; `reset()` starts the next segment on the same buffers."""

    def __init__(self, arrangement, H, W, max_frames, *, flow_mag_factor=1.0, mask_max_mag=1.0, consistent_flow=True, device="cuda"):
        import torch
        self.arrangement = [list(row) for row in arrangement] if not isinstance(arrangement, (str, bytes)) else arrangement
        tiles, self.R, self.C = tile_list(self.arrangement)
        if not (int(H) >= 1 and int(W) >= 1 and 1 <= int(max_frames) <= 65535):
            raise L.DynamoHipError("SegmentRenderer: H, W >= 1 and 1 <= max_frames <= 65535")
        if not (float(flow_mag_factor) > 0 and float(mask_max_mag) > 0):
            raise L.DynamoHipError("SegmentRenderer: flow_mag_factor and mask_max_mag are positive")
        self.H, self.W, self.max_frames = int(H), int(W), int(max_frames)
        self.flow_mag_factor, self.mask_max_mag, self.consistent_flow = float(flow_mag_factor), float(mask_max_mag), bool(consistent_flow)
        self.names = [name for row in self.arrangement for name in row]
        self.n_tiles, self.n_flow = len(tiles), sum(name in FLOW_TILES for name in self.names)
        self._tiles = (C.c_int * (3 * len(tiles)))(*[v for t in tiles for v in t])
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise L.DynamoHipError("SegmentRenderer renders on the GPU")
        L.load()
        self.panel = torch.zeros((self.max_frames, self.R * self.H, self.C * self.W, 3), dtype=torch.uint8, device=self.device)
        self.side = torch.empty((self.max_frames, max(self.n_flow, 1), 2, self.H, self.W), dtype=torch.float32, device=self.device) if self.n_flow else None
        self._maxima = torch.zeros(self.max_frames + 1, dtype=torch.float32, device=self.device)
        self._lut = torch.from_numpy(lut_words()).to(self.device)
        self.n_frames = 0

    def reset(self):
        """The next segment: zero running maximum, zero per-frame maxima, no frames."""
        self._maxima.zero_()
        self.n_frames = 0

    @property
    def maxima(self):
        """(1 + frames) fp32 on the device: the segment's largest flow magnitude, then every frame's."""
        return self._maxima[:1 + self.n_frames]

    def _plane(self, t, channels, what, needed):
        if t is None:
            if needed:
                raise L.DynamoHipError("SegmentRenderer.add_frame: the arrangement needs `{}`".format(what))
            return None
        import torch
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.numel() == channels * self.H * self.W
                and tuple(t.shape[-2:]) == (self.H, self.W)):
            raise L.DynamoHipError("SegmentRenderer.add_frame: `{}` must be a ({}, {}, {}) fp32 tensor on the GPU".format(what, channels, self.H, self.W))
        return t.contiguous()

    def _matrix(self, t, what, needed):
        if t is None:
            if needed:
                raise L.DynamoHipError("SegmentRenderer.add_frame: the arrangement needs `{}`".format(what))
            return None
        import torch
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.numel() == 16 and tuple(t.shape[-2:]) == (4, 4)):
            raise L.DynamoHipError("SegmentRenderer.add_frame: `{}` must be a (4, 4) fp32 tensor on the GPU".format(what))
        return t.contiguous()

    def add_frame(self, *, color=None, disp=None, motion_mask=None, complete_flow=None, K=None, inv_K=None, cam_T_cam=None, ref_color=None,
                  min_depth=0.1, max_depth=100.0):
        """One frame's tensors, where they lie on the device ((C,H,W) or (1,C,H,W)): one launch on the current stream, no host sync.
        A tensor that no tile of the arrangement reads may be left out."""
        if self.n_frames >= self.max_frames:
            raise L.DynamoHipError("SegmentRenderer.add_frame: frame {} of a renderer for {} frames".format(self.n_frames + 1, self.max_frames))
        if not (float(min_depth) > 0 and float(max_depth) > 0):
            raise L.DynamoHipError("SegmentRenderer.add_frame: min_depth and max_depth are positive")
        names = set(self.names)
        flow = self.n_flow > 0
        motion = bool(names & {"ind_flow", "comp_flow", "samp_flow"})
        color = self._plane(color, 3, "color", "img" in names)
        ref_color = self._plane(ref_color, 3, "ref_color", "ref_img" in names)
        disp = self._plane(disp, 1, "disp", flow or "disp" in names)
        motion_mask = self._plane(motion_mask, 1, "motion_mask", motion or "mask" in names)
        complete_flow = self._plane(complete_flow, 3, "complete_flow", motion)
        K, inv_K, cam_T_cam = self._matrix(K, "K", flow), self._matrix(inv_K, "inv_K", flow), self._matrix(cam_T_cam, "cam_T_cam", flow)
        L.check(L.load().dd_vis_frame(abi.ptr(color), abi.ptr(ref_color), abi.ptr(disp), abi.ptr(motion_mask), abi.ptr(complete_flow), abi.ptr(K),
                                      abi.ptr(inv_K), abi.ptr(cam_T_cam), float(min_depth), float(max_depth), self.H, self.W, self._tiles, self.n_tiles,
                                      self.R, self.C, abi.ptr(self._lut), 0.0, 1.0, 0.0, self.mask_max_mag, self.n_frames, self.max_frames,
                                      abi.ptr(self.panel), abi.ptr(self.side), abi.ptr(self._maxima), L.current_stream()), "dd_vis_frame")
        self.n_frames += 1

    def finish(self):
        """Colours the flow tiles of every frame added since `reset()` (one launch) and returns the (N, R*H, C*W, 3) uint8 frames on
        the device: a view of the renderer's buffer, valid until the next segment is rendered into it."""
        if self.n_frames < 1:
            raise L.DynamoHipError("SegmentRenderer.finish: no frame was added")
        L.check(L.load().dd_vis_flow_tiles(abi.ptr(self.side), abi.ptr(self._maxima), self._tiles, self.n_tiles, self.R, self.C, self.H, self.W,
                                           self.n_frames, self.flow_mag_factor, int(self.consistent_flow), abi.ptr(self.panel), L.current_stream()),
                "dd_vis_flow_tiles")
        return self.panel[:self.n_frames]
