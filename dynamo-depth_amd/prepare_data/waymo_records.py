"""The host side of the Waymo preparation's input (prepare_data/waymo.py): the TFRecord container without TensorFlow, and the one
function that touches the Waymo messages.

Container: every record is a little-endian uint64 length, a uint32 masked CRC32C of those eight bytes, the payload, and a uint32
masked CRC32C of the payload.  The length's CRC is always checked (eight bytes: it catches a truncated or misaligned file), the
payload's only on request, since a CRC in Python over the gigabyte of a segment is too slow to be the default.

Messages: `waymo_open_dataset.dataset_pb2` is imported where a Frame is first needed; it needs protobuf only.  No field number is
written down here: `frame_to_arrays` reads attributes of message objects, whatever class they come from, and returns plain Python
and numpy data (`FrameArrays`); everything downstream takes only that."""
import io
import struct
import zlib
from dataclasses import dataclass, field

import numpy as np

CAMERA_NAMES = {1: "FRONT", 2: "FRONT_LEFT", 3: "FRONT_RIGHT", 4: "SIDE_LEFT", 5: "SIDE_RIGHT"}      # dataset.proto CameraName.Name

_CRC_TABLE = []
for _n in range(256):
    _c = _n
    for _ in range(8):
        _c = (_c >> 1) ^ 0x82F63B78 if _c & 1 else _c >> 1
    _CRC_TABLE.append(_c)


def crc32c(data):
    crc = 0xFFFFFFFF
    table = _CRC_TABLE
    for byte in data:
        crc = table[(crc ^ byte) & 0xFF] ^ (crc >> 8)
    return crc ^ 0xFFFFFFFF


def masked_crc(data):
    crc = crc32c(data)
    return ((((crc >> 15) | (crc << 17)) & 0xFFFFFFFF) + 0xA282EAD8) & 0xFFFFFFFF


def read_records(path, check_data=False):
    """Yields the payloads of a TFRecord file.  ValueError, with the file and the offset, for a short read or a CRC that differs."""
    with open(path, "rb") as fh:
        offset = 0
        while True:
            head = fh.read(12)
            if not head:
                return
            if len(head) < 12:
                raise ValueError("{}: truncated record header at offset {}".format(path, offset))
            length, crc = struct.unpack("<QI", head)
            if masked_crc(head[:8]) != crc:
                raise ValueError("{}: bad length checksum at offset {}".format(path, offset))
            body = fh.read(length + 4)
            if len(body) < length + 4:
                raise ValueError("{}: truncated record of {} bytes at offset {}".format(path, length, offset))
            if check_data and masked_crc(body[:length]) != struct.unpack("<I", body[length:])[0]:
                raise ValueError("{}: bad payload checksum at offset {}".format(path, offset))
            yield body[:length]
            offset += 16 + length


def message_classes():
    """(Frame, MatrixFloat, MatrixInt32) of the Waymo package."""
    try:
        from waymo_open_dataset import dataset_pb2
    except ImportError as err:
        raise RuntimeError("prepare_data/waymo.py reads the segments with waymo_open_dataset.dataset_pb2 (it needs protobuf only, neither "
                           "TensorFlow nor OpenCV), and that module is not installed: {}".format(err))
    return dataset_pb2.Frame, dataset_pb2.MatrixFloat, dataset_pb2.MatrixInt32


@dataclass
class FrameArrays:
    pose: np.ndarray                                # frame.pose.transform, float64 (4, 4)
    cameras: dict = field(default_factory=dict)     # camera name -> {code, image, pose, intrinsic, extrinsic, width, height, panoptic, divisor}
    lasers: list = field(default_factory=list)      # ascending laser name: {name, range, cp, pose, inclinations, extrinsic}
    labels: list = field(default_factory=list)      # laser labels: {box [7], speed [3], accel [3], type}


def _matrix(cls, compressed, last, what):
    m = cls()
    m.ParseFromString(zlib.decompress(compressed))
    dims = [int(d) for d in m.shape.dims]
    if len(dims) != 3 or dims[2] != last:
        raise ValueError("{} of shape {}: the last dimension should be {}".format(what, dims, last))
    data = np.asarray(m.data)
    if data.size != dims[0] * dims[1] * dims[2]:
        raise ValueError("{} of shape {} holds {} values".format(what, dims, data.size))
    return data.reshape(dims)


def decode_panoptic(png, divisor):
    """(semantic, instance) (H, W, 1) of a 16-bit PNG panoptic label, uint8 where the maximum allows it, as the reference stores them."""
    from PIL import Image
    if int(divisor) <= 0:
        raise ValueError("panoptic label divisor {}".format(divisor))
    with Image.open(io.BytesIO(png)) as img:
        label = np.asarray(img).astype(np.int32)
    if label.ndim != 2:
        raise ValueError("a panoptic label of shape {}".format(label.shape))
    out = []
    for part in (label // int(divisor), label % int(divisor)):
        out.append((part.astype(np.uint8) if part.max() < 256 else part)[:, :, None])
    return out[0], out[1]


def frame_to_arrays(frame, cams, MatrixFloat=None, MatrixInt32=None):
    """The only function that touches message objects: a Frame -> FrameArrays with the cameras named in `cams`.  Only the first
    return of every laser is used; the laser whose first return carries a compressed per-pixel pose (TOP) gets it decoded."""
    from hipops import lidar
    if MatrixFloat is None or MatrixInt32 is None:
        _, MatrixFloat, MatrixInt32 = message_classes()
    out = FrameArrays(pose=np.array(list(frame.pose.transform), dtype=np.float64).reshape(4, 4))
    images = {CAMERA_NAMES.get(int(img.name)): img for img in frame.images}
    for cal in frame.context.camera_calibrations:
        name = CAMERA_NAMES.get(int(cal.name))
        if name not in cams:
            continue
        intrinsic = [float(v) for v in cal.intrinsic]
        if len(intrinsic) != 9:
            raise ValueError("camera {}: an intrinsic of {} values, not 9".format(name, len(intrinsic)))
        if name not in images:
            raise ValueError("camera {} has a calibration and no image".format(name))
        img = images[name]
        seg = img.camera_segmentation_label
        out.cameras[name] = {"code": int(cal.name), "image": bytes(img.image), "pose": [float(v) for v in img.pose.transform], "intrinsic": intrinsic,
                             "extrinsic": [float(v) for v in cal.extrinsic.transform], "width": int(cal.width), "height": int(cal.height),
                             "panoptic": bytes(seg.panoptic_label) or None, "divisor": int(seg.panoptic_label_divisor)}
    missing = [c for c in cams if c not in out.cameras]
    if missing:
        raise ValueError("the frame has no camera {}".format(missing))
    calibrations = {int(c.name): c for c in frame.context.laser_calibrations}
    for laser in sorted(frame.lasers, key=lambda l: int(l.name)):
        name = int(laser.name)
        if name not in calibrations:
            raise ValueError("laser {} has no calibration".format(name))
        cal, ret = calibrations[name], laser.ri_return1
        rng = _matrix(MatrixFloat, ret.range_image_compressed, 4, "range image of laser {}".format(name))
        cp = _matrix(MatrixInt32, ret.camera_projection_compressed, 6, "camera projection of laser {}".format(name))
        if cp.shape[:2] != rng.shape[:2]:
            raise ValueError("laser {}: range image {} and camera projection {}".format(name, rng.shape, cp.shape))
        pose = None
        if len(ret.range_image_pose_compressed):
            pose = _matrix(MatrixFloat, ret.range_image_pose_compressed, 6, "per-pixel pose of laser {}".format(name)).astype(np.float32)
            if pose.shape[:2] != rng.shape[:2]:
                raise ValueError("laser {}: range image {} and per-pixel pose {}".format(name, rng.shape, pose.shape))
        out.lasers.append({"name": name, "range": np.ascontiguousarray(rng[:, :, 0], dtype=np.float32), "cp": np.ascontiguousarray(cp[:, :, :3], dtype=np.int32),
                           "pose": pose, "extrinsic": np.array(list(cal.extrinsic.transform), dtype=np.float64).reshape(4, 4),
                           "inclinations": lidar.inclination_table(rng.shape[0], list(cal.beam_inclinations), cal.beam_inclination_min,
                                                                   cal.beam_inclination_max)})
    for lbl in frame.laser_labels:
        box, meta = lbl.camera_synced_box, lbl.metadata
        out.labels.append({"box": [box.center_x, box.center_y, box.center_z, box.length, box.width, box.height, box.heading],
                           "speed": [meta.speed_x, meta.speed_y, meta.speed_z], "accel": [meta.accel_x, meta.accel_y, meta.accel_z], "type": lbl.type})
    return out
