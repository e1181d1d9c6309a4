"""The definition of the visualisation panels on the host, in torch on the CPU: what csrc/dd_vis.hip computes, restated from the
reference's eval/visualize.py:24-124 (get_vis / combine_vis), Trainer.py:574-605 (vis_motion) and utils.py:103-164 (cart2polar,
hsv_to_rgb, score_map_vis).  The flow tiles in fp32 or fp64 by argument; the image tiles and the colour-map tiles ALWAYS in fp32:
their bytes are defined on fp32 data (numpy's (x * 255).astype(uint8) on the fp32 image, matplotlib's Normalize and
Colormap.__call__ on the fp32 map), and a wider product would truncate differently next to an integer.

Also the seeded scenes the tests share."""
import math

import numpy as np
import torch

FLOW_TILES = ("ego_flow", "ind_flow", "comp_flow", "samp_flow")
MIN_DEPTH, MAX_DEPTH = 0.1, 100.0
GOLDEN_ARRANGEMENT = [["img", "disp", "ego_flow", "ind_flow", "mask"]]
SECOND_ARRANGEMENT = [["ref_img", "comp_flow", "samp_flow"], ["img", "ego_flow", "ind_flow"]]


# ---------------------------------------------------------------------------------------------------------------------------------
# tiles
def image_bytes(img):
    """(3,H,W) fp32 in [0,1] -> (H,W,3) uint8, truncating."""
    x = img.reshape(3, *img.shape[-2:]).float().clamp(0, 1)
    return (x * 255).to(torch.uint8).permute(1, 2, 0)


def cmap_index(x, vmin=0.0, vmax=1.0):
    """matplotlib's Normalize(vmin, vmax) then Colormap.__call__ (N = 256) on fp32 data: the table entry per element, -1 for NaN."""
    x = x.float()
    lo, hi = torch.tensor(vmin, dtype=torch.float32), torch.tensor(vmax, dtype=torch.float32)
    s = ((x - lo) / (hi - lo)) * 256
    idx = s.clamp(0, 255).nan_to_num(0.0).to(torch.int64)       # truncation; s == 256 and everything above it -> 255, below 0 -> 0
    return torch.where(torch.isnan(s), torch.full_like(idx, -1), idx)


def cmap_bytes(x, table, vmin=0.0, vmax=1.0):
    """(H,W) fp32 -> (H,W,3) uint8 through a (256,3) uint8 table; NaN is black."""
    idx = cmap_index(x, vmin, vmax)
    out = torch.as_tensor(table)[idx.clamp(min=0)]
    return torch.where((idx < 0).unsqueeze(-1), torch.zeros_like(out), out)


def _project(q, K, H, W):
    """tools.py Project3D after the transform: q (4,N) -> (H,W,2) in [-1,1]."""
    cam = K[:3, :] @ q
    pix = cam[:2] / (cam[2:3] + 1e-7)
    pix = pix.reshape(2, H, W).permute(1, 2, 0)
    pix = torch.stack([pix[..., 0] / (W - 1), pix[..., 1] / (H - 1)], -1)
    return (pix - 0.5) * 2


def flow_planes(kind, disp, motion_mask, complete_flow, K, inv_K, T, min_depth=MIN_DEPTH, max_depth=MAX_DEPTH, dtype=torch.float32):
    """(mag, hue), each (H,W), of one flow tile of one frame."""
    H, W = disp.shape[-2:]
    disp, K, inv_K, T = disp.reshape(1, H * W).to(dtype), K.reshape(4, 4).to(dtype), inv_K.reshape(4, 4).to(dtype), T.reshape(4, 4).to(dtype)
    min_disp, max_disp = 1 / max_depth, 1 / min_depth
    depth = 1 / (min_disp + (max_disp - min_disp) * disp)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=dtype), torch.arange(W, dtype=dtype), indexing="ij")
    grid = torch.stack([xs.reshape(-1), ys.reshape(-1), torch.ones(H * W, dtype=dtype)])
    P = depth * (inv_K[:3, :3] @ grid)                                                    # (3,N)
    ones = torch.ones(1, H * W, dtype=dtype)
    ident = torch.stack([(torch.arange(W, dtype=dtype) / W * 2 - 1).unsqueeze(0).repeat(H, 1),
                         (torch.arange(H, dtype=dtype) / H * 2 - 1).unsqueeze(1).repeat(1, W)], -1)
    err = _project(torch.cat([P, ones]), K, H, W) - ident
    q = P
    if kind != "ego_flow":
        m = complete_flow.reshape(3, H * W).to(dtype)
        if kind in ("ind_flow", "samp_flow"):
            ego3d = (T @ torch.cat([P, ones]))[:3] - P
            m = motion_mask.reshape(1, H * W).to(dtype) * (m - ego3d)
        q = P + m
    q = torch.cat([q, ones])
    if kind in ("ego_flow", "samp_flow"):
        q = T @ q
    raw = _project(q, K, H, W) - ident - err
    # utils.cart2polar on the last dimension (x, y): it names them "y, x" and divides the first by the second
    mag = torch.sqrt(torch.sum(raw ** 2, -1))
    theta = torch.atan(raw[..., 0] / raw[..., 1])
    theta = torch.where(torch.isnan(theta), torch.zeros_like(theta), theta)
    theta = theta + (raw[..., 1] < 0) * math.pi
    theta = (5 * math.pi / 2 - theta) % (2 * math.pi)
    hue = (theta - math.pi / 4) % (2 * math.pi) / (2 * math.pi)
    return mag, hue


def flow_bytes(mag, hue, top):
    """1 - hsv_to_rgb(hue, 1, clamp(mag / top, 0, 1)) as (H,W,3) uint8; the sector table of utils.hsv_to_rgb."""
    v = torch.clamp(mag / top, 0, 1)
    s = torch.ones_like(v)
    hi = torch.floor(hue * 6) % 6
    f = ((hue * 6) % 6) - hi
    p, q, t = v * (1 - s), v * (1 - f * s), v * (1 - (1 - f) * s)
    hi = hi.long()
    table = torch.stack((v, q, p, p, t, v, t, v, v, q, p, p, p, p, t, v, v, q), dim=0)
    rgb = torch.gather(table, 0, torch.stack([hi, hi + 6, hi + 12], dim=0))
    return ((1 - rgb) * 255).to(torch.uint8).permute(1, 2, 0)


def render(frames, arrangement, *, dtype=torch.float32, min_depth=MIN_DEPTH, max_depth=MAX_DEPTH, flow_mag_factor=1.0, mask_max_mag=1.0,
           consistent_flow=True):
    """frames: a list of dicts color, ref_color, disp, motion_mask, complete_flow, K, inv_K, cam_T_cam (CPU tensors).
    -> (panel (N, R*H, C*W, 3) uint8, maxima (1 + N,) of `dtype`: the segment's largest flow magnitude, then every frame's)."""
    from hipops.vis import cmap_bytes as table_of
    plasma, hot = table_of("plasma"), table_of("hot")
    H, W = frames[0]["disp"].shape[-2:]
    R, C = len(arrangement), max(len(row) for row in arrangement)
    panel = torch.zeros(len(frames), R * H, C * W, 3, dtype=torch.uint8)
    planes, frame_max = {}, torch.zeros(len(frames), dtype=dtype)
    for n, fr in enumerate(frames):
        for r, row in enumerate(arrangement):
            for c, name in enumerate(row):
                if name in FLOW_TILES:
                    planes[n, r, c] = flow_planes(name, fr["disp"], fr["motion_mask"], fr["complete_flow"], fr["K"], fr["inv_K"], fr["cam_T_cam"],
                                                  min_depth, max_depth, dtype)
                    frame_max[n] = torch.maximum(frame_max[n], planes[n, r, c][0].max())
                    continue
                if name == "img":
                    tile = image_bytes(fr["color"])
                elif name == "ref_img":
                    tile = image_bytes(fr["ref_color"])
                elif name == "disp":
                    tile = cmap_bytes(fr["disp"].reshape(H, W), plasma, 0.0, 1.0)
                elif name == "mask":
                    tile = cmap_bytes(fr["motion_mask"].reshape(H, W), hot, 0.0, mask_max_mag)
                else:
                    raise Exception("Arrangement name (={}) not recognized.".format(name))
                panel[n, r * H:(r + 1) * H, c * W:(c + 1) * W] = tile
    seg_max = frame_max.max() if len(planes) else torch.zeros((), dtype=dtype)
    for (n, r, c), (mag, hue) in planes.items():
        top = flow_mag_factor * ((seg_max if consistent_flow else frame_max[n]) + 1e-8)
        panel[n, r * H:(r + 1) * H, c * W:(c + 1) * W] = flow_bytes(mag, hue, top)
    return panel, torch.cat([seg_max.reshape(1), frame_max])


# ---------------------------------------------------------------------------------------------------------------------------------
# comparisons
def tile_of(panel, arrangement, name, H, W):
    for r, row in enumerate(arrangement):
        for c, a in enumerate(row):
            if a == name:
                return panel[:, r * H:(r + 1) * H, c * W:(c + 1) * W]
    raise KeyError(name)


def compare(got, want, arrangement, H, W):
    """-> (largest level difference anywhere, share of the flow-tile bytes that differ, whether every other tile is identical)."""
    got, want = torch.as_tensor(got).to(torch.int16), torch.as_tensor(want).to(torch.int16)
    assert got.shape == want.shape, (got.shape, want.shape)
    worst, off, total, rest_equal = int((got - want).abs().max()), 0, 0, True
    for row in arrangement:
        for name in row:
            d = tile_of(got, arrangement, name, H, W) - tile_of(want, arrangement, name, H, W)
            if name in FLOW_TILES:
                off, total = off + int((d != 0).sum()), total + d.numel()
            else:
                rest_equal = rest_equal and not bool(d.any())
    return worst, (off / total if total else 0.0), rest_equal


# ---------------------------------------------------------------------------------------------------------------------------------
# scenes
def intrinsics(H, W):
    K = np.array([[0.58 * W, 0, 0.5 * W, 0], [0, 1.92 * H, 0.5 * H, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=np.float32)     # KITTI-like
    return torch.from_numpy(K), torch.from_numpy(np.linalg.pinv(K).astype(np.float32))


def pose(tx, ty, tz, yaw):
    c, s = math.cos(yaw), math.sin(yaw)
    return torch.tensor([[c, 0, s, tx], [0, 1, 0, ty], [-s, 0, c, tz], [0, 0, 0, 1]], dtype=torch.float32)


def scene(N, H, W, seed=0, flow=0.2, step=0.05):
    """N frames: disp in [0.002, 0.05] (depth 2 .. 33 m at 0.1 / 100), complete flow within +-flow, motion mask in [0,1), a camera
    translation that grows with the frame index, scaled (x1, x2, x0.5, ...) so that the segment's largest flow is the middle
    frame's, and a small yaw."""
    g = torch.Generator().manual_seed(seed)
    K, inv_K = intrinsics(H, W)
    gain = [1.0, 2.0, 0.5]
    frames = []
    for n in range(N):
        t = step * (n + 1) * gain[n % 3]
        frames.append({
            "color": torch.rand(3, H, W, generator=g), "ref_color": torch.rand(3, H, W, generator=g),
            "disp": 0.002 + 0.048 * torch.rand(1, H, W, generator=g),
            "motion_mask": torch.rand(1, H, W, generator=g),
            "complete_flow": flow * (2 * torch.rand(3, H, W, generator=g) - 1),
            "K": K.clone(), "inv_K": inv_K.clone(), "cam_T_cam": pose(0.3 * t, -0.1 * t, t, 0.004 * (n + 1))})
    return frames


def to_device(frames, device="cuda"):
    return [{k: v.to(device) for k, v in fr.items()} for fr in frames]
