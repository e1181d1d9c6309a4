"""Case builder of the nuScenes preparation tests (tests/test_nuscenes_prepare.py on the host, tests/test_nuscenes_prepare_gpu.py on the
device): a generated <data_root> in the raw nuScenes layout -- two scenes, three CAM_FRONT frames each (key, sweep, key), 50x25
JPEG frames (16x8 down-samples), four 200-point LIDAR_TOP scans per scene (one sweep lies nearer in time to the last key frame than
the sample's own scan: the override of the association), two annotation boxes per sample and panoptic files -- with what the script
has to make of it, the boundary scan of the mask thresholds, and the seeded frames of the resize comparison."""
import io
import json
import os
import os.path as osp

import numpy as np
from PIL import Image

# 50 / 16 = 25 / 8 = 3.125 on both axes, the scale of the real frames: every weight is a multiple of 1/25, so a sum is a multiple of 1/625
# and never closer to a half-integer than 1/1250 -- the fp32 sums of the device round as the float64 sums of the definition do, and
# the two runs of the script can be compared byte for byte (at 32 rows the scale would be 16/5 and sums could hit .5 exactly)
W, H = 50, 25
DOWN_W, DOWN_H = 16, 8
N_POINTS = 200
SCENES = ("scene-0001", "scene-0002")
K = [[40.0, 0.0, 25.0], [0.0, 40.0, 12.5], [0.0, 0.0, 1.0]]
CAM_CS = {"translation": [1.7, 0.016, 1.51], "rotation": [0.4998, -0.5030, 0.4998, -0.4974]}
LIDAR_CS = {"translation": [0.94, 0.0, 1.84], "rotation": [0.7077, -0.0064, 0.0107, -0.7064]}
CATEGORIES = (("noise", 0), ("human.pedestrian.adult", 2), ("vehicle.car", 17), ("flat.driveable_surface", 24), ("vehicle.ego", 31))
LABELS = ((17001, 40), (17002, 30), (17003, 20), (2001, 10), (24000, 100))     # panoptic label, points: 200 per scan
# what the key frames' points must get: the moving box, the parked box, a car outside every box, a pedestrian without a box, the road
MOTION_OF = {17001: 1, 17002: 2, 17003: 3, 2001: 3, 24000: 0}


def quat_yaw(a):
    return [float(np.cos(a / 2)), 0.0, 0.0, float(np.sin(a / 2))]


def rigid(rec):
    from hipops import lidar
    return lidar.transform_matrix(rec["translation"], rec["rotation"])


def ego_pose(scene, step):
    """The ego pose `step` tenths of a second into the scene."""
    return {"translation": [400.0 + 300.0 * scene + 0.8 * step, 900.0 + 0.05 * step, 0.0], "rotation": quat_yaw(0.3 + 0.4 * scene + 0.01 * step)}


def box_of(scene, which):
    """An annotation box in the ego frame of step 0 carried to the global frame: (translation, size wlh, rotation)."""
    T = rigid(ego_pose(scene, 0))
    centre = T @ np.array([[12.0, 2.5, 1.0, 1.0], [9.0, -3.0, 0.9, 1.0]][which])
    yaw = 0.3 + 0.4 * scene + (0.2, -0.5)[which]
    return [float(v) for v in centre[:3]], [1.9, 4.4, 1.6], quat_yaw(yaw)


def scan_points(rng, scene, pose):
    """200 points in the sensor frame of a scan taken at `pose`: the two boxes' points inside them, a car far from both, a pedestrian,
    the road; every one in front of the camera."""
    from hipops import lidar
    parts = []
    for which, n in ((0, LABELS[0][1]), (1, LABELS[1][1])):
        centre, (w, l, h), rot = box_of(scene, which)
        local = rng.uniform(-0.45, 0.45, size=(n, 3)) * np.array([l, w, h])
        parts.append(local @ lidar.quaternion_matrix(rot).T + np.array(centre))
    T0 = rigid(ego_pose(scene, 0))
    for n, lo, hi in ((20, (20.0, -1.0, 0.2), (24.0, 1.0, 1.5)), (10, (6.0, 0.5, 0.2), (7.0, 1.0, 1.8)), (100, (4.0, -6.0, 0.0), (30.0, 6.0, 0.3))):
        local = np.concatenate([rng.uniform(lo, hi, size=(n, 3)), np.ones((n, 1))], axis=1)
        parts.append((local @ T0.T)[:, :3])
    g = np.concatenate(parts)
    to_sensor = np.linalg.inv(rigid(pose) @ rigid(LIDAR_CS))
    pts = (np.concatenate([g, np.ones((g.shape[0], 1))], axis=1) @ to_sensor.T)[:, :3]
    return np.concatenate([pts, rng.uniform(0, 255, size=(g.shape[0], 1)), np.zeros((g.shape[0], 1))], axis=1).astype(np.float32)


def frame(rng, w, h):
    """A smooth frame with some texture: what a JPEG keeps."""
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([xx * 4 + yy, 255 - yy * 6, (xx + yy) * 3], axis=-1) + rng.integers(-20, 20, size=(h, w, 3))
    return np.clip(base, 0, 255).astype(np.uint8)


def write_tree(root, seed=7):
    """Writes the raw tree under `root`; returns {scene: {"cams": [...], "lidar_of": [file per camera frame], "key": [bool]}}."""
    rng = np.random.default_rng(seed)
    tables = {name: [] for name in ("scene", "sample", "sample_data", "calibrated_sensor", "ego_pose", "sensor", "attribute", "sample_annotation",
                                    "instance", "panoptic")}
    tables["category"] = [{"token": "cat_" + name, "name": name, "index": index, "description": ""} for name, index in CATEGORIES]
    tables["attribute"] = [{"token": "attr_moving", "name": "vehicle.moving"}, {"token": "attr_parked", "name": "vehicle.parked"}]
    tables["sensor"] = [{"token": "sensor_cam", "channel": "CAM_FRONT", "modality": "camera"}, {"token": "sensor_lidar", "channel": "LIDAR_TOP", "modality": "lidar"}]
    tables["calibrated_sensor"] = [dict(CAM_CS, token="cs_cam", sensor_token="sensor_cam", camera_intrinsic=K),
                                   dict(LIDAR_CS, token="cs_lidar", sensor_token="sensor_lidar", camera_intrinsic=[])]
    for d in ("v1.0-trainval", "samples/CAM_FRONT", "sweeps/CAM_FRONT", "samples/LIDAR_TOP", "sweeps/LIDAR_TOP", "panoptic/v1.0-trainval"):
        os.makedirs(osp.join(root, d), exist_ok=True)
    expect = {}
    for k, name in enumerate(SCENES):
        t0 = 1_500_000_000_000_000 + k * 1_000_000_000
        samples = ["s{}_{}".format(k, n) for n in range(2)]
        tables["scene"].append({"token": "scene{}".format(k), "name": name, "log_token": "log", "nbr_samples": 2, "first_sample_token": samples[0],
                                "last_sample_token": samples[1]})
        for n, tok in enumerate(samples):
            tables["sample"].append({"token": tok, "timestamp": t0 + n * 150_000, "scene_token": "scene{}".format(k), "prev": samples[n - 1] if n else "",
                                     "next": samples[n + 1] if n + 1 < len(samples) else ""})
        for which in range(2):
            tables["instance"].append({"token": "inst{}_{}".format(k, which), "category_token": "cat_vehicle.car"})
            for n, tok in enumerate(samples):
                centre, size, rot = box_of(k, which)
                tables["sample_annotation"].append({"token": "ann{}_{}_{}".format(k, which, n), "sample_token": tok, "instance_token": "inst{}_{}".format(k, which),
                                                    "attribute_tokens": ["attr_moving" if which == 0 else "attr_parked"], "translation": centre, "size": size,
                                                    "rotation": rot})
        # camera frames: key (step 0), sweep (+100 ms), key (+150 ms)
        cams = [(0, True, samples[0]), (100_000, False, samples[1]), (150_000, True, samples[1])]
        # scans: the first sample's, a sweep, a sweep at the very time of the last key frame, the second sample's 3 ms later
        lidars = [(2_000, True, samples[0]), (98_000, False, samples[1]), (150_000, False, samples[1]), (153_000, True, samples[1])]
        info = {"cams": [], "lidar_of": [], "key": [c[1] for c in cams], "stamps": [c[0] for c in cams]}
        for chain, prefix, ext in ((cams, "cam", ".jpg"), (lidars, "lidar", ".pcd.bin")):
            for n, (dt, key, sample) in enumerate(chain):
                tok = "{}{}_{}".format(prefix, k, n)
                folder = ("samples" if key else "sweeps") + ("/CAM_FRONT/" if prefix == "cam" else "/LIDAR_TOP/")
                rel = folder + "{}_{}{}".format(name, tok, ext)
                pose = ego_pose(k, dt / 100_000.0)
                tables["ego_pose"].append(dict(pose, token="pose_" + tok, timestamp=t0 + dt))
                tables["sample_data"].append({"token": tok, "sample_token": sample, "ego_pose_token": "pose_" + tok, "calibrated_sensor_token": "cs_" + prefix,
                                              "timestamp": t0 + dt, "fileformat": ext[1:], "is_key_frame": key, "height": H if prefix == "cam" else 0,
                                              "width": W if prefix == "cam" else 0, "filename": rel, "prev": "{}{}_{}".format(prefix, k, n - 1) if n else "",
                                              "next": "{}{}_{}".format(prefix, k, n + 1) if n + 1 < len(chain) else ""})
                if prefix == "cam":
                    Image.fromarray(frame(rng, W, H)).save(osp.join(root, rel), quality=92)
                    info["cams"].append(rel)
                else:
                    scan_points(rng, k, pose).tofile(osp.join(root, rel))
                    if key:
                        pan = "panoptic/v1.0-trainval/{}_panoptic.npz".format(tok)
                        np.savez_compressed(osp.join(root, pan), data=np.concatenate([np.full(c, v, dtype=np.uint16) for v, c in LABELS]))
                        tables["panoptic"].append({"token": tok, "sample_data_token": tok, "filename": pan})
        info["lidar_of"] = ["samples/LIDAR_TOP/{}_lidar{}_0.pcd.bin".format(name, k), "sweeps/LIDAR_TOP/{}_lidar{}_1.pcd.bin".format(name, k),
                            "samples/LIDAR_TOP/{}_lidar{}_3.pcd.bin".format(name, k)]
        info["cam_steps"] = [0.0, 1.0, 1.5]
        info["lidar_steps"] = [0.02, 0.98, 1.53]
        expect[name] = info
    for name, rows in tables.items():
        with open(osp.join(root, "v1.0-trainval", name + ".json"), "w") as fh:
            json.dump(rows, fh)
    return expect


def direct_rows(scan, lidar_pose, cam_pose):
    """[u, v, depth] of a scan by the composition of the four 4x4 matrices in float64, and the reference's mask."""
    M = np.linalg.inv(rigid(CAM_CS)) @ np.linalg.inv(rigid(cam_pose)) @ rigid(lidar_pose) @ rigid(LIDAR_CS)
    p = np.concatenate([scan[:, :3].astype(np.float64), np.ones((scan.shape[0], 1))], axis=1) @ M.T
    uv = p[:, :3] @ np.array(K).T
    u, v, d = uv[:, 0] / uv[:, 2], uv[:, 1] / uv[:, 2], p[:, 2]
    keep = (d > 1.0) & (u > 1) & (u < W - 1) & (v > 1) & (v < H - 1)
    return np.stack([u, v, d], axis=1)[keep], keep


def check_tree(root, expect, scenes=SCENES, rgb=True, depth=True, mask=True):
    """Every file the script writes for `scenes`, against the raw tree and the direct definitions."""
    for k, name in enumerate(SCENES):
        base = osp.join(root, "scenes", name, "FRONT")
        if name not in scenes:
            assert not osp.exists(base)
            continue
        info = expect[name]
        for ii, rel in enumerate(info["cams"]):
            org, dwn = osp.join(base, "rgb", "original", "{:06}.jpg".format(ii)), osp.join(base, "rgb", "downsample", "{:06}.jpg".format(ii))
            assert osp.exists(org) == rgb and osp.exists(dwn) == rgb
            if rgb:
                assert osp.islink(org) and os.readlink(org) == osp.realpath(osp.join(root, rel))
                with Image.open(dwn) as img:
                    assert img.size == (DOWN_W, DOWN_H) and img.mode == "RGB"
            dpath, mpath = osp.join(base, "depth", "{:06}.npy".format(ii)), osp.join(base, "mask", "{:06}.npz".format(ii))
            scan = np.fromfile(osp.join(root, info["lidar_of"][ii]), dtype=np.float32).reshape(-1, 5)
            want, keep = direct_rows(scan, ego_pose(k, info["lidar_steps"][ii]), ego_pose(k, info["cam_steps"][ii]))
            assert 20 < want.shape[0] < N_POINTS                        # the case keeps some points and drops some
            assert osp.exists(dpath) == depth
            if depth:
                got = np.load(dpath)
                assert got.dtype == np.float64 and got.shape == want.shape
                assert np.allclose(got, want, rtol=0, atol=1e-8)         # float64 round-off of two orders of the same sums, coordinates <= 1e3
            assert osp.exists(mpath) == (mask and info["key"][ii])
            if mask and info["key"][ii]:
                with np.load(mpath, allow_pickle=True) as z:
                    assert sorted(z.files) == ["motion_label", "panoptic2ann", "panoptic_label"]
                    pan, motion, p2a = z["panoptic_label"], z["motion_label"], z["panoptic2ann"].item()
                labels = np.concatenate([np.full(c, v, dtype=np.uint16) for v, c in LABELS])[keep]
                assert pan.dtype == np.uint16 and np.array_equal(pan, labels)
                assert motion.dtype == np.uint8 and np.array_equal(motion, np.array([MOTION_OF[int(v)] for v in labels], dtype=np.uint8))
                present = set(int(v) for v in labels)
                assert set(int(u) for u in p2a) == present & {17001, 17002, 17003, 2001}
                for label, which in ((17001, 0), (17002, 1)):
                    if label in present:
                        assert p2a[label] == {"token": "ann{}_{}_{}".format(k, which, 0 if ii == 0 else 1), "fit": 1.0}
                for label in (17003, 2001):
                    if label in present:
                        assert p2a[label] == {"token": None, "fit": 0}
        with open(osp.join(base, "rgb", "cam.json")) as fh:
            cam = json.load(fh)
        assert list(cam) == ["camera_intrinsic", "translation", "rotation", "dim", "intrinsic_mat"]
        assert cam["camera_intrinsic"] == K and cam["dim"] == [H, W] and cam["translation"] == CAM_CS["translation"] and cam["rotation"] == CAM_CS["rotation"]
        assert cam["intrinsic_mat"] == [[40.0 / W, 0.0, 25.0 / W], [0.0, 40.0 / H, 12.5 / H], [0.0, 0.0, 1.0]]
        with open(osp.join(base, "rgb", "ts.json")) as fh:
            assert json.load(fh) == [100, 50]
        with open(osp.join(base, "odometry.txt")) as fh:
            lines = fh.read().split("\n")
        assert len(lines) == 4 and lines[3] == ""
        for ii in range(3):
            vals = lines[ii].split(" ")
            assert len(vals) == 16 and vals[12:] == ["0.0", "0.0", "0.0", "1.0"]
            assert np.array_equal(np.array([float(v) for v in vals]).reshape(4, 4), rigid(ego_pose(k, info["cam_steps"][ii])))
            assert all(v == str(np.float64(float(v))) for v in vals)


def boundary_scan(params):
    """Points in the sensor frame whose images under `params` lie on and next to every mask threshold (u = 1 and u = W - 1 exactly
    in exact arithmetic, depth = 1, behind the camera) and the rows of the host definition tell which side round-off put them."""
    from hipops import lidar
    q = np.asarray(params)
    Wq, Hq = q[57], q[58]
    Kq = q[48:57].reshape(3, 3)
    cam = []
    for u, v, d in ((1.0, 8.0, 5.0), (Wq - 1.0, 8.0, 5.0), (10.0, 1.0, 5.0), (10.0, Hq - 1.0, 5.0), (10.0, 8.0, 1.0), (10.0, 8.0, 1.0 + 1e-6), (10.0, 8.0, -3.0),
                    (1.0 + 1e-4, 8.0, 5.0), (1.0 - 1e-4, 8.0, 5.0), (Wq - 1.0 - 1e-4, 8.0, 2.0), (10.0, Hq - 1.0 + 1e-4, 2.0), (10.0, 8.0, 0.0)):
        cam.append([(u - Kq[0, 2]) * d / Kq[0, 0], (v - Kq[1, 2]) * d / Kq[1, 1], d])
    p = np.array(cam, dtype=np.float64)
    R1, R2, R3, R4 = (q[a:a + 9].reshape(3, 3) for a in (0, 12, 27, 39))
    p = p @ R4 + q[36:39]               # the inverse of p = R4 (p - t4), R4 orthogonal
    p = p @ R3 + q[24:27]
    p = (p - q[21:24]) @ R2
    p = (p - q[9:12]) @ R1
    return np.concatenate([p, np.zeros((p.shape[0], 1))], axis=1).astype(np.float32)


def exact_params():
    from hipops import lidar
    ident = {"rotation": [1.0, 0.0, 0.0, 0.0], "translation": [0.0, 0.0, 0.0]}
    return lidar.pose_params(ident, ident, ident, ident, [[32.0, 0.0, 16.0], [0.0, 32.0, 8.0], [0.0, 0.0, 1.0]], 32, 16)


def host_steps():
    from hipops import lidar
    from prepare_data import nuScenes
    return dict(decode=nuScenes.host_decode, resize=nuScenes.host_resize, pose_rows=nuScenes.host_pose_rows, fit=lidar.box_fit_host)


def resize_frames(kind, n, h, w, seed):
    if kind == "noise":
        return np.random.default_rng(seed).integers(0, 256, size=(n, h, w, 3), dtype=np.uint8)
    if kind == "white":
        return np.full((n, h, w, 3), 255, dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    return np.broadcast_to((((yy + xx) & 1) * 255).astype(np.uint8)[None, :, :, None], (n, h, w, 3)).copy()
