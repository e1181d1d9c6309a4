"""Generated inputs and independent restatements for the Waymo preparation's tests (test_waymo_prepare.py, test_waymo_prepare_gpu.py).

Nothing of the Waymo package can be executed where these tests run, so the restatements below guard against transcription errors in
hipops/lidar.py range_image_points_host and hipops/undistort.py undistort_host, not against a misremembered convention: they follow
the same description, written another way -- 4x4 homogeneous matrices, scipy's Rotation.from_euler, np.linalg.inv and
boolean masks instead of step-by-step sums and compaction; a scalar loop over pixels in Python integers for the undistortion.

The message classes here stand in for the Waymo package's: real protobuf messages of a schema built at import time, with the
attribute names prepare_data/waymo_records.py frame_to_arrays reads and field numbers of this file's own."""
import io
import os
import struct
import zlib
from types import SimpleNamespace as NS

import numpy as np
from PIL import Image

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
FIXTURE = os.path.join(ROOT, "tests", "golden", "tiny_waymo", "val", "segment-1024360143612057520_3580_000_3600_000", "FRONT")
PAIR = os.path.join(ROOT, "tests", "golden", "waymo_prepare")
MOVEABLE = (2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 16, 27)
NUSCENES_AREA_FIGURE = 1.388        # the area down-sample against the reference's own nuScenes down-samples, grey levels


# ---------------------------------------------------------------------------------------------------------------- the record container
def _crc32c_bitwise(data):
    crc = 0xFFFFFFFF
    for byte in data:
        crc ^= byte
        for _ in range(8):
            crc = (crc >> 1) ^ (0x82F63B78 & -(crc & 1))
    return crc ^ 0xFFFFFFFF


def _masked(data):
    crc = _crc32c_bitwise(data)
    return (((crc >> 15) | (crc << 17)) + 0xA282EAD8) & 0xFFFFFFFF


def write_tfrecord(path, payloads):
    """A TFRecord file of the payloads; returns the offset of every record."""
    offsets, at = [], 0
    with open(path, "wb") as fh:
        for p in payloads:
            head = struct.pack("<Q", len(p))
            fh.write(head + struct.pack("<I", _masked(head)) + p + struct.pack("<I", _masked(p)))
            offsets.append(at)
            at += 16 + len(p)
    return offsets


# ------------------------------------------------------------------------------------------------------------- stand-in message classes
# A schema built at import time with protobuf's descriptor pool: real protobuf messages (wire format, repeated containers, bytes
# fields) with the attribute NAMES frame_to_arrays reads.  The field numbers are this file's own, counted from 1 in the order below;
# they are not the Waymo package's and nothing outside the tests uses them.
_SCHEMA = (
    ("Transform", (("transform", "double*"),)),
    ("Shape", (("dims", "int32*"),)),
    ("MatrixFloat", (("data", "float*"), ("shape", "Shape"))),
    ("MatrixInt32", (("data", "int32*"), ("shape", "Shape"))),
    ("SegmentationLabel", (("panoptic_label", "bytes"), ("panoptic_label_divisor", "int32"))),
    ("CameraImage", (("name", "int32"), ("image", "bytes"), ("pose", "Transform"), ("camera_segmentation_label", "SegmentationLabel"))),
    ("CameraCalibration", (("name", "int32"), ("intrinsic", "double*"), ("extrinsic", "Transform"), ("width", "int32"), ("height", "int32"))),
    ("LaserCalibration", (("name", "int32"), ("beam_inclinations", "double*"), ("beam_inclination_min", "double"), ("beam_inclination_max", "double"),
                          ("extrinsic", "Transform"))),
    ("Context", (("camera_calibrations", "CameraCalibration*"), ("laser_calibrations", "LaserCalibration*"))),
    ("Box", tuple((n, "double") for n in ("center_x", "center_y", "center_z", "length", "width", "height", "heading"))),
    ("Metadata", tuple((n, "double") for n in ("speed_x", "speed_y", "speed_z", "accel_x", "accel_y", "accel_z"))),
    ("Label", (("camera_synced_box", "Box"), ("metadata", "Metadata"), ("type", "int32"))),
    ("RangeImage", (("range_image_compressed", "bytes"), ("camera_projection_compressed", "bytes"), ("range_image_pose_compressed", "bytes"))),
    ("Laser", (("name", "int32"), ("ri_return1", "RangeImage"))),
    ("Frame", (("images", "CameraImage*"), ("context", "Context"), ("laser_labels", "Label*"), ("pose", "Transform"), ("lasers", "Laser*"))),
)


def _message_classes():
    from google.protobuf import descriptor_pb2, descriptor_pool, message_factory
    F = descriptor_pb2.FieldDescriptorProto
    scalars = {"double": F.TYPE_DOUBLE, "float": F.TYPE_FLOAT, "int32": F.TYPE_INT32, "bytes": F.TYPE_BYTES}
    fdp = descriptor_pb2.FileDescriptorProto(name="waymo_prepare_case.proto", package="ddtest", syntax="proto2")
    for name, fields in _SCHEMA:
        m = fdp.message_type.add(name=name)
        for number, (fname, kind) in enumerate(fields, 1):
            repeated, kind = kind.endswith("*"), kind.rstrip("*")
            f = m.field.add(name=fname, number=number, label=F.LABEL_REPEATED if repeated else F.LABEL_OPTIONAL)
            if kind in scalars:
                f.type = scalars[kind]
                if repeated:
                    f.options.packed = True
            else:
                f.type, f.type_name = F.TYPE_MESSAGE, ".ddtest." + kind
    pool = descriptor_pool.DescriptorPool()
    pool.Add(fdp)
    return {name: message_factory.GetMessageClass(pool.FindMessageTypeByName("ddtest." + name)) for name, _ in _SCHEMA}


_CLASSES = _message_classes()
Frame, MatrixFloat, MatrixInt32 = _CLASSES["Frame"], _CLASSES["MatrixFloat"], _CLASSES["MatrixInt32"]
MESSAGES = (Frame, MatrixFloat, MatrixInt32)


def to_message(cls, tree):
    """A message of class `cls` from a tree of SimpleNamespace objects, lists and scalars with the same attribute names."""
    from google.protobuf.descriptor import FieldDescriptor
    msg = cls()
    for f in cls.DESCRIPTOR.fields:
        value = getattr(tree, f.name)
        repeated = f.is_repeated if hasattr(f, "is_repeated") else f.label == FieldDescriptor.LABEL_REPEATED
        if f.message_type is not None:
            sub = _CLASSES[f.message_type.name]
            if repeated:
                for item in value:
                    getattr(msg, f.name).append(to_message(sub, item))
            else:
                getattr(msg, f.name).CopyFrom(to_message(sub, value))
        elif repeated:
            getattr(msg, f.name).extend(value)
        else:
            setattr(msg, f.name, value)
    return msg


def _compressed(array):
    a = np.asarray(array)
    cls = MatrixFloat if a.dtype.kind == "f" else MatrixInt32
    return zlib.compress(to_message(cls, NS(data=a.reshape(-1).tolist(), shape=NS(dims=list(a.shape)))).SerializeToString())


def _transform(M):
    return NS(transform=[float(v) for v in np.asarray(M, dtype=np.float64).reshape(-1)])


# --------------------------------------------------------------------------------------------------------------------- the lidar case
def rigid(yaw, pitch, roll, t):
    from scipy.spatial.transform import Rotation
    M = np.eye(4)
    M[:3, :3] = Rotation.from_euler("xyz", [roll, pitch, yaw]).as_matrix()
    M[:3, 3] = t
    return M


CAM_W, CAM_H = 96, 64
CAM_INTRINSIC = [40.0, 41.0, 47.3, 31.6, 0.0, 0.0, 0.0, 0.0, 0.0]
CAM_EXTRINSIC = rigid(0.003, -0.002, 0.009, [1.54, -0.02, 2.12])
TOP_SHAPE, SIDE_SHAPE = (8, 40), (5, 12)
GLOBAL = 5.0e4                      # metres: the magnitude of the fixture's odometry


def lidar_frame(seed, frame_pose=None):
    """One generated frame as plain data: {pose, lasers: [{name, range (H, W, 4), cp (H, W, 6), pose (H, W, 6) or None, extrinsic,
    beam_inclinations, min, max}]}.  TOP 8x40 with listed inclinations and a per-pixel pose near the frame pose, four 5x12 images with
    uniform inclinations; about a third of the ranges <= 0, image 4 entirely invalid, image 5 valid only behind the vehicle."""
    rng = np.random.default_rng(seed)
    if frame_pose is None:
        frame_pose = rigid(0.7 + 0.01 * seed, 0.02, -0.01, [GLOBAL - 100.0 * seed, -0.6 * GLOBAL, 31.0])
    euler = [-0.01, 0.02, 0.7 + 0.01 * seed]
    lasers = []
    for name in (1, 2, 3, 4, 5):
        H, W = TOP_SHAPE if name == 1 else SIDE_SHAPE
        rho = rng.uniform(4.0, 60.0, size=(H, W)).astype(np.float32)
        dead = rng.uniform(size=(H, W)) < 0.33
        rho[dead] = np.where(rng.uniform(size=int(dead.sum())) < 0.5, 0.0, -1.0)
        if name == 4:
            rho[:] = np.where(rng.uniform(size=(H, W)) < 0.5, 0.0, -1.0)
        if name == 5:
            rho[:, 2:W - 2] = -1.0
            rho[:, [0, 1, W - 2, W - 1]] = rng.uniform(4.0, 60.0, size=(H, 4))
        image = np.zeros((H, W, 4), dtype=np.float32)
        image[:, :, 0] = rho
        image[:, :, 1:] = rng.uniform(size=(H, W, 3))
        cp = np.zeros((H, W, 6), dtype=np.int32)
        cp[:, :, 0], cp[:, :, 3] = rng.integers(0, 3, size=(H, W)), rng.integers(0, 3, size=(H, W))
        cp[:, :, 1], cp[:, :, 2] = rng.integers(0, CAM_W, size=(H, W)), rng.integers(0, CAM_H, size=(H, W))
        cp[:, :, 4], cp[:, :, 5] = rng.integers(0, CAM_W, size=(H, W)), rng.integers(0, CAM_H, size=(H, W))
        pose = None
        if name == 1:
            pose = np.zeros((H, W, 6), dtype=np.float32)
            pose[:, :, :3] = np.array(euler) + rng.uniform(-1e-3, 1e-3, size=(H, W, 3))
            pose[:, :, 3:] = frame_pose[:3, 3] + rng.uniform(-0.05, 0.05, size=(H, W, 3))
        yaw = {1: -2.6, 2: 0.01, 3: 1.57, 4: -1.56, 5: 3.13}[name]
        extrinsic = rigid(yaw, 0.004 * name, -0.003, [1.43 - 0.5 * name, 0.1 * name - 0.3, 2.18 - 0.3 * name])
        lasers.append({"name": name, "range": image, "cp": cp, "pose": pose, "extrinsic": extrinsic,
                       "beam_inclinations": (np.linspace(-0.30, 0.04, H) + rng.uniform(-0.005, 0.005, size=H)).tolist() if name == 1 else [],
                       "min": -0.9 + 0.01 * name, "max": 0.4})
    return {"pose": frame_pose, "lasers": lasers}


def restate_points(frame, cam_extrinsic=CAM_EXTRINSIC, intrinsic=CAM_INTRINSIC, width=CAM_W, height=CAM_H):
    """Per laser (points (n, 3), cp (n, 3), rows (m, 3)) of one frame of `lidar_frame`, restated with homogeneous matrices."""
    from scipy.spatial.transform import Rotation
    swap = np.array([[0, 0, 1, 0], [-1, 0, 0, 0], [0, -1, 0, 0], [0, 0, 0, 1]], dtype=np.float64)
    P = np.zeros((3, 4))
    P[0, 0], P[1, 1], P[0, 2], P[1, 2], P[2, 2] = intrinsic[0], intrinsic[1], intrinsic[2], intrinsic[3], 1.0
    P = P @ np.linalg.inv(np.asarray(cam_extrinsic) @ swap)
    out = []
    for laser in frame["lasers"]:
        H, W = laser["range"].shape[:2]
        E = np.asarray(laser["extrinsic"], dtype=np.float64)
        if laser["beam_inclinations"]:
            incl = np.array(laser["beam_inclinations"], dtype=np.float64)
        else:
            incl = np.array([(0.5 + i) / H * (laser["max"] - laser["min"]) + laser["min"] for i in range(H)])
        incl = incl[::-1]
        az = np.array([((W - c - 0.5) / W * 2 - 1) * np.pi for c in range(W)]) - np.arctan2(E[1, 0], E[0, 0])
        rho = laser["range"][:, :, 0].astype(np.float64)
        homog = np.ones((H, W, 4))
        homog[:, :, 0] = rho * np.cos(az)[None, :] * np.cos(incl)[:, None]
        homog[:, :, 1] = rho * np.sin(az)[None, :] * np.cos(incl)[:, None]
        homog[:, :, 2] = rho * np.sin(incl)[:, None]
        M = np.broadcast_to(E, (H, W, 4, 4))
        if laser["pose"] is not None:
            pose = laser["pose"].astype(np.float64)
            T = np.zeros((H, W, 4, 4))
            T[:, :, :3, :3] = Rotation.from_euler("xyz", pose[:, :, :3].reshape(-1, 3)).as_matrix().reshape(H, W, 3, 3)
            T[:, :, :3, 3] = pose[:, :, 3:]
            T[:, :, 3, 3] = 1.0
            M = np.linalg.inv(frame["pose"]) @ T @ E
        vehicle = np.einsum("hwij,hwj->hwi", M, homog)
        pix = np.einsum("ij,hwj->hwi", P, vehicle)
        valid = laser["range"][:, :, 0] > 0
        with np.errstate(all="ignore"):
            u, v = pix[:, :, 0] / pix[:, :, 2], pix[:, :, 1] / pix[:, :, 2]
            keep = valid & (pix[:, :, 2] > 0) & (u >= 0) & (u < width) & (v >= 0) & (v < height)
        out.append((vehicle[valid][:, :3], laser["cp"][valid][:, :3], np.stack([u[keep], v[keep], pix[:, :, 2][keep]], axis=1)))
    return out


def definition_inputs(frames, cam_extrinsic=CAM_EXTRINSIC, intrinsic=CAM_INTRINSIC, width=CAM_W, height=CAM_H):
    """(ranges, cps, poses, trigs, params) of hipops.lidar.range_image_points{,_host} for a list of `lidar_frame`s."""
    from hipops import lidar
    K = np.array([[intrinsic[0], 0, intrinsic[2]], [0, intrinsic[1], intrinsic[3]], [0, 0, 1.0]])
    e2c = lidar.vehicle_to_camera(cam_extrinsic)
    ranges, cps, poses, trigs, params = [], [], [], [], []
    for frame in frames:
        for laser in frame["lasers"]:
            H, W = laser["range"].shape[:2]
            incl = lidar.inclination_table(H, laser["beam_inclinations"], laser["min"], laser["max"])
            ranges.append(np.ascontiguousarray(laser["range"][:, :, 0]))
            cps.append(np.ascontiguousarray(laser["cp"][:, :, :3]))
            poses.append(laser["pose"])
            trigs.append(lidar.range_image_trig(incl, W, laser["extrinsic"]))
            params.append(lidar.range_image_params(laser["extrinsic"], frame["pose"] if laser["pose"] is not None else None, e2c, K, width, height))
    return ranges, cps, poses, trigs, np.stack(params)


def points_bound():
    """64 * 2^-52 * (G + 75) metres: a few float64 roundings at the global magnitude (G the largest pose translation of the case,
    75 m the reach of a laser)."""
    return 64 * 2.0 ** -52 * (GLOBAL + 75.0)


def exact_case():
    """Points ON the thresholds, with arithmetic that is exact in float64: identity extrinsics, tables and intrinsics made of powers
    of two.  Twenty-four images of one pixel, each with its own tables (the call crosses its 16-image chunk); with
    C = inv(axis_swap) the camera sees q = (-y, -z, x), K = [[32, 0, 32], [0, 32, 16], [0, 0, 1]], 64 x 32 pixels.  Returns (inputs of
    range_image_points, per image: True kept, False valid and not kept, None not valid)."""
    from hipops import lidar
    #        rho              cos az sin az  sin incl  expected
    cols = [(8.0,             0.5,   0.5,    0.0,      True),      # y = x: u = 0, kept
            (8.0,             0.5,   -0.5,   0.0,      False),     # y = -x: u = 64 = width
            (8.0,             0.5,   0.0,    0.25,     True),      # z = x / 2: v = 0, kept
            (8.0,             0.5,   0.0,    -0.25,    False),     # v = 32 = height
            (8.0,             0.0,   0.5,    0.0,      False),     # x = 0: a_z = 0
            (0.0,             0.5,   0.0,    0.0,      None),      # rho = 0: not valid
            (-0.0,            0.5,   0.0,    0.0,      None),
            (2.0 ** -126,     0.5,   0.0,    0.0,      True),      # the smallest normal range: valid, u = 32, v = 16
            (float("nan"),    0.5,   0.0,    0.0,      None),
            (8.0,             0.5,   -0.4375, 0.0,     True),      # u = 60
            (8.0,             -0.5,  0.0,    0.0,      False),     # behind the camera
            (4.0,             0.25,  0.0,    0.0,      True)]
    cols = cols + cols
    W = len(cols)
    rng = np.array([[c[0] for c in cols]], dtype=np.float32)
    cp = np.arange(W * 3, dtype=np.int32).reshape(1, W, 3)
    ranges, cps, trigs = [], [], []
    for k in range(W):
        ranges.append(rng[:, k:k + 1])
        cps.append(cp[:, k:k + 1])
        trigs.append(np.array([1.0, cols[k][3], cols[k][1], cols[k][2]]))
    K = np.array([[32.0, 0, 32.0], [0, 32.0, 16.0], [0, 0, 1.0]])
    p = lidar.range_image_params(np.eye(4), None, lidar.vehicle_to_camera(np.eye(4)), K, 64, 32)
    return (ranges, cps, [None] * W, trigs, np.stack([p] * W)), [c[4] for c in cols]


# ----------------------------------------------------------------------------------------------------------------------- undistortion
def restate_undistort_pixel(frame, intrinsic, u, v):
    """One destination pixel of the definition in Python floats and integers."""
    fu, fv, cu, cv, k1, k2, p1, p2, k3 = (float(t) for t in intrinsic)
    H, W = frame.shape[:2]
    x, y = (u - cu) / fu, (v - cv) / fv
    r2 = x * x + y * y
    k = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
    xd = (x * k + ((2 * p1) * x) * y) + p2 * (r2 + 2 * (x * x))
    yd = (y * k + p1 * (r2 + 2 * (y * y))) + ((2 * p2) * x) * y
    ix, iy = round((fu * xd + cu) * 32), round((fv * yd + cv) * 32)         # Python rounds halves to even
    sx, sy, a, b = ix >> 5, iy >> 5, ix & 31, iy & 31
    total = [512, 512, 512]
    for dx, dy, wt in ((0, 0, (32 - a) * (32 - b)), (1, 0, a * (32 - b)), (0, 1, (32 - a) * b), (1, 1, a * b)):
        if 0 <= sx + dx < W and 0 <= sy + dy < H:
            for ch in range(3):
                total[ch] += wt * int(frame[sy + dy, sx + dx, ch])
    return [t >> 10 for t in total]


def checkerboard(n, H, W, cell=4, seed=0):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    board = (((yy // cell) + (xx // cell)) % 2).astype(np.uint8)
    frames = np.zeros((n, H, W, 3), dtype=np.uint8)
    for k in range(n):
        lo, hi = rng.integers(0, 100, size=3), rng.integers(156, 256, size=3)
        frames[k] = np.where(board[:, :, None] == 1, hi, lo).astype(np.uint8)
    frames[:, ::7, ::5] = rng.integers(0, 256, size=frames[:, ::7, ::5].shape, dtype=np.uint8)
    return frames


def calibration(H, W, strength):
    """An intrinsic for an H x W frame: 'none', 'k1' (pure radial) or 'strong' (border taps leave the image on all four sides)."""
    base = [0.9 * W, 0.95 * W, W / 2 - 0.3, H / 2 + 0.4]
    return base + {"none": [0.0] * 5, "k1": [-0.21, 0.0, 0.0, 0.0, 0.0], "strong": [0.45, 0.12, 0.004, -0.006, 0.02]}[strength]


# ------------------------------------------------------------------------------------------------------------------- the whole script
SEGMENT = "segment-123_000_with_camera_labels.tfrecord"
SEGMENT_NAME = "segment-123_000"
SCRIPT_INTRINSIC = [40.0, 41.0, 47.3, 31.6, 0.04, -0.3, 0.001, -0.0015, 0.0]
OBJECT_LABELS = (1, 3, 2)           # the motion labels the reader should paint: a moving car, a car nothing hits, a static pedestrian


def instance_image():
    """(semantic, instance, [(class, object mask)] in the pickle's order) of the labelled frame: two cars (class 2), one of them a ring,
    and a pedestrian (class 9) on a CAM_H x CAM_W frame of road (class 20)."""
    sem = np.full((CAM_H, CAM_W), 20, dtype=np.int32)
    ins = np.zeros((CAM_H, CAM_W), dtype=np.int32)
    sem[8:31, 10:41], ins[8:31, 10:41] = 2, 0                      # car 0: a block ...
    sem[14:22, 20:30], ins[14:22, 20:30] = 20, 0                    # ... with a hole
    sem[40:44, 60:63], ins[40:44, 60:63] = 2, 1                     # car 1: small, no point lands on it
    sem[36:60, 70:90], ins[36:60, 70:90] = 9, 0                     # the pedestrian
    objects = [(2, (sem == 2) & (ins == 0)), (2, (sem == 2) & (ins == 1)), (9, sem == 9)]
    return sem, ins, objects


def script_frames():
    """Three frames as message trees (the second one with a panoptic label and two laser labels) and what the test expects."""
    from hipops import lidar
    sem, ins, objects = instance_image()
    rng = np.random.default_rng(3)
    frames, plain = [], []
    for k in range(3):
        data = lidar_frame(10 + k, frame_pose=rigid(0.3, 0.0, 0.0, [GLOBAL + 2.0 * k, 7.0, 1.0]))
        for laser in data["lasers"]:
            cp = laser["cp"]
            on_small_car = objects[1][1][cp[:, :, 2], cp[:, :, 1]]
            cp[:, :, 0][on_small_car] = 2                            # seen by another camera
        top = data["lasers"][0]["cp"]
        top[:, 0:8, 0], top[:, 0:8, 1], top[:, 0:8, 2] = 1, 12 + np.arange(8)[None, :], 9 + np.arange(8)[:, None]         # on car 0
        top[:, 8:16, 0], top[:, 8:16, 1], top[:, 8:16, 2] = 1, 72 + np.arange(8)[None, :], 40 + np.arange(8)[:, None]      # on the pedestrian
        data["lasers"][0]["range"][:, 0:16, 0] = rng.uniform(5.0, 50.0, size=(8, 16)).astype(np.float32)
        plain.append(data)
    found, _ = lidar.range_image_points_host(*definition_inputs([plain[1]], intrinsic=SCRIPT_INTRINSIC))
    points, cp = np.concatenate([f[0] for f in found]), np.concatenate([f[1] for f in found])
    boxes = []
    for (lo_x, lo_y), speed in (((12, 9), 3.0), ((72, 40), 0.1)):
        hit = (cp[:, 0] == 1) & (cp[:, 1] >= lo_x) & (cp[:, 1] < lo_x + 8) & (cp[:, 2] >= lo_y) & (cp[:, 2] < lo_y + 8)
        centre = points[hit][0]
        boxes.append(NS(camera_synced_box=NS(center_x=float(centre[0]), center_y=float(centre[1]), center_z=float(centre[2]), length=4.0, width=2.0,
                                             height=1.5, heading=0.4),
                        metadata=NS(speed_x=speed, speed_y=0.0, speed_z=0.0, accel_x=0.1, accel_y=0.0, accel_z=0.0), type=1 if speed > 1 else 2))
    panoptic = io.BytesIO()
    Image.fromarray((sem * 1000 + ins).astype(np.uint16)).save(panoptic, format="PNG")
    images = checkerboard(3, CAM_H, CAM_W, cell=6, seed=5)
    for k, data in enumerate(plain):
        jpeg = io.BytesIO()
        Image.fromarray(images[k]).save(jpeg, format="JPEG", quality=92)
        cam_pose = rigid(0.3, 0.0, 0.0, [GLOBAL + 2.0 * k + 0.25, 7.0, 1.0])
        seg = NS(panoptic_label=panoptic.getvalue() if k == 1 else b"", panoptic_label_divisor=1000 if k == 1 else 0)
        lasers, lcals = [], []
        for laser in reversed(data["lasers"]):                       # not in ascending name: the reader sorts them
            ret = NS(range_image_compressed=_compressed(laser["range"]), camera_projection_compressed=_compressed(laser["cp"]),
                     range_image_pose_compressed=_compressed(laser["pose"]) if laser["pose"] is not None else b"")
            lasers.append(NS(name=laser["name"], ri_return1=ret))
            lcals.append(NS(name=laser["name"], beam_inclinations=laser["beam_inclinations"], beam_inclination_min=laser["min"],
                            beam_inclination_max=laser["max"], extrinsic=_transform(laser["extrinsic"])))
        frames.append(NS(images=[NS(name=2, image=b"", pose=_transform(np.eye(4)), camera_segmentation_label=NS(panoptic_label=b"", panoptic_label_divisor=0)),
                                 NS(name=1, image=jpeg.getvalue(), pose=_transform(cam_pose), camera_segmentation_label=seg)],
                         context=NS(camera_calibrations=[NS(name=1, intrinsic=list(SCRIPT_INTRINSIC), extrinsic=_transform(CAM_EXTRINSIC), width=CAM_W,
                                                            height=CAM_H)],
                                    laser_calibrations=lcals),
                         laser_labels=boxes if k == 1 else [], pose=_transform(data["pose"]), lasers=lasers))
    return [to_message(Frame, f) for f in frames], plain, images, (sem, ins, objects)


def write_records(record_dir):
    """<record_dir>/{train,val}: one segment of three frames under val, nothing under train.  Returns script_frames()'s expectations."""
    frames, plain, images, labels = script_frames()
    os.makedirs(os.path.join(record_dir, "train"), exist_ok=True)
    os.makedirs(os.path.join(record_dir, "val"), exist_ok=True)
    write_tfrecord(os.path.join(record_dir, "val", SEGMENT), [f.SerializeToString() for f in frames])
    return frames, plain, images, labels


def host_steps():
    from hipops import lidar
    from prepare_data import waymo
    return dict(decode=waymo.host_decode, undistort=waymo.host_undistort, resize=waymo.host_resize, points=lidar.range_image_points_host,
                fit=lidar.box_fit_host, messages=MESSAGES)
