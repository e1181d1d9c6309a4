"""What the preparation scripts share (prepare_data/nuScenes.py, prepare_data/waymo.py): JPEG files' bytes to frames on the device or
by Pillow, the area down-sample as a step with a host twin, and the small file helpers their thread pools run."""
import io

import numpy as np
from PIL import Image

JPEG_QUALITY = 95               # cv2.imwrite's default
MAX_THREADS = 16


def pil_decode(data):
    with Image.open(io.BytesIO(data)) as img:
        return np.asarray(img.convert("RGB"))


def host_decode(datas):
    """JPEG files' bytes -> (H, W, 3) uint8 frames, by Pillow."""
    return [pil_decode(d) for d in datas]


def device_decode(datas):
    """The same on the device for the files hipops.jpeg's geometry check accepts (frames stay on the GPU), by Pillow for the rest."""
    import ctypes as C

    import torch

    from hipops import jpeg
    from hipops import lib as L
    lib = L.load()
    out, groups = [None] * len(datas), {}
    for n, data in enumerate(datas):
        try:
            rec, (w, h, ncomp, hs, vs) = jpeg.parse_header(data)
        except jpeg.UnsupportedJpeg:
            rec = None
        if rec is None or ncomp != 3 or not lib.dd_jpeg_workspace_bytes(1, h, w, ncomp, (C.c_int * 3)(*hs), (C.c_int * 3)(*vs)):
            out[n] = pil_decode(data)
        else:
            groups.setdefault((h, w, ncomp, hs, vs), []).append((n, rec))
    for geom, members in groups.items():
        cap = (max(len(datas[n]) for n, _ in members) + 4095) // 4096 * 4096
        buf = np.zeros((len(members), cap), dtype=np.uint8)
        for k, (n, _) in enumerate(members):
            buf[k, :len(datas[n])] = np.frombuffer(datas[n], dtype=np.uint8)
        frames = jpeg.decode_batch(torch.from_numpy(buf).cuda(), torch.from_numpy(np.stack([rec for _, rec in members])).cuda(), *geom)
        for k, (n, _) in enumerate(members):
            out[n] = frames[k]
    return out


def host_resize(frames, height, width):
    from hipops import resize
    return resize.resize_area_host(np.stack(frames), height, width)


def device_resize(frames, height, width):
    """Equal-sized frames (GPU tensors or host arrays) -> (n, height, width, 3) uint8 on the host, one launch."""
    import torch

    from hipops import resize
    stack = torch.stack([f if torch.is_tensor(f) else torch.from_numpy(np.ascontiguousarray(f)).cuda() for f in frames])
    return resize.resize_area_batch(stack, height, width).cpu().numpy()


def read_bytes(path):
    with open(path, "rb") as fh:
        return fh.read()


def save_jpeg(job):
    Image.fromarray(job[1]).save(job[0], quality=JPEG_QUALITY)


def chunks(items, size):
    return [items[i:i + size] for i in range(0, len(items), size)]
