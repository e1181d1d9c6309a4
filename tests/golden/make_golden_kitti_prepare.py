"""Golden vectors for the KITTI preparation (tests/test_kitti_prepare.py, tests/test_lidar_depth_gpu.py).

Executes the UNMODIFIED reference prepare_data/kitti_util.py::generate_depth_map(..., vel_depth=True) (imported from where it lies)
on temporary calibration directories and .bin scans, followed by the `np.where(depth > 0)` stacking of the reference's
prepare_data/kitti.py:112-114.  The one stand-in, installed here: `np.int = int` (numpy removed the alias in 1.24).  Only data is
stored: per case the two calibration files' text, the points, P (2, 3, 4) for cameras 2 and 3, H, W and the reference's rows.

    python tests/golden/make_golden_kitti_prepare.py        ->  tests/golden/kitti_prepare.npz

Cases:
  real_calib  tiny_kitti's calibration texts (375x1242); a seeded 64-beam scan of the forward sector: ground plane and wall with
              range noise, and a few points behind the car
  dense       24x40, 6 000 points with x in [-2, 40]: the first 50 have x = 0, ten x = -0.0, ten are exact duplicates of ten others,
              some hold NaN or inf, some have a_2 = 0 or a_2 < 0 with x >= 0
  alias       8x6, hand-placed points in the shared buckets (r, W-1) / (r+1, 0) in both index orders, the minimum coming from the
              other pixel, pixel (0, 0) (bucket -1) and the last bucket hit twice
  ties        8x12, P = [[0,-16,0,0],[0,0,-16,0],[1,0,0,0]]: x a power of two, y and z odd multiples of x/32, so every product and sum
              is exact in any order and u, v are -0.5, 0.5, 1.5, 2.5, W-0.5, W+0.5 (and the same in H): half-to-even at both bounds
  empty       a scan of length 0 and a scan without a valid point, under every case's calibration: no rows

The script refuses to write unless (a) outside `ties` no kept point with u in [-2, W+2] and v in [-2, H+2] has u or v within 1e-9
of a half-integer (inside that band the reference's BLAS product and the left-to-right definition could round apart: change the
seed), and (b) hipops.lidar.depth_points_host equals the reference on every case and camera, nothing excluded.
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.normpath(os.path.join(HERE, "..", ".."))
for p in (HERE, os.path.join(ROOT, "dynamo-depth_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
import _refshim  # noqa: E402
from hipops import lidar  # noqa: E402

np.int = int                                                        # the stand-in: kitti_util.py:86 predates numpy 1.24
sys.path.insert(0, os.path.join(_refshim.REFERENCE_ROOT, "prepare_data"))
import kitti_util  # noqa: E402

CAMS = (2, 3)
EYE = np.eye(3)
AXES = np.array([[0.0, -1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]])     # velodyne (forward, left, up) -> camera (right, down, forward)


def fmt(values):
    return " ".join("{:.6e}".format(float(v)) for v in np.asarray(values, dtype=np.float64).reshape(-1))


def calib_texts(H, W, P2, P3, R_rect=EYE, R=EYE, T=(0.0, 0.0, 0.0)):
    cam2cam = "calib_time: 01-Jan-2024 00:00:00\ncorner_dist: 1.000000e-01\nS_rect_02: {}\nR_rect_00: {}\nP_rect_02: {}\nP_rect_03: {}\n".format(
        fmt([W, H]), fmt(R_rect), fmt(P2), fmt(P3))
    velo2cam = "calib_time: 01-Jan-2024 00:00:00\nR: {}\nT: {}\ndelta_f: 0.000000e+00 0.000000e+00\n".format(fmt(R), fmt(T))
    return cam2cam, velo2cam


def real_calib():
    d = os.path.join(_refshim.REFERENCE_ROOT, "assets", "tiny_kitti", "2011_09_26", "2011_09_26_drive_0001_sync")
    texts = tuple(open(os.path.join(d, f)).read() for f in ("calib_cam_to_cam.txt", "calib_velo_to_cam.txt"))
    rng = np.random.default_rng(20110926)
    el = np.deg2rad(np.linspace(2.0, -24.8, 64))[:, None]
    az = np.deg2rad(np.linspace(-60.0, 60.0, 500))[None, :]
    ray = np.stack(np.broadcast_arrays(np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el) + 0 * az), axis=-1).reshape(-1, 3)
    with np.errstate(divide="ignore"):
        ground = np.where(ray[:, 2] < 0, -1.73 / ray[:, 2], np.inf)
    wall = 25.0 / ray[:, 0]
    rng_m = np.minimum(ground, wall)
    hit = rng_m < 80.0
    rng_m = rng_m[hit] + rng.normal(0.0, 0.02, int(hit.sum()))
    xyz = ray[hit] * rng_m[:, None]
    behind = rng.uniform(-30.0, 30.0, (200, 3)) * np.array([1.0, 1.0, 0.05])
    behind[:, 0] = -np.abs(behind[:, 0]) - 0.1
    xyz = np.concatenate([xyz, behind])
    xyz = xyz[rng.permutation(xyz.shape[0])]
    pts = np.concatenate([xyz, rng.uniform(0, 1, (xyz.shape[0], 1))], axis=1).astype(np.float32)
    return texts, pts


def dense():
    H, W = 24, 40
    texts = calib_texts(H, W, [[30, 0, 20, 0.5], [0, 30, 12, 0.25], [0, 0, 1, 0]], [[30, 0, 20, -16], [0, 30, 12, 0.25], [0, 0, 1, -0.25]], R=AXES)
    rng = np.random.default_rng(24040)
    n = 6000
    x = rng.uniform(-2.0, 40.0, n)
    pts = np.stack([x, x * rng.uniform(-0.9, 0.9, n), x * rng.uniform(-0.6, 0.6, n), rng.uniform(0, 1, n)], axis=1).astype(np.float32)
    pts[:60, 1:3] = rng.uniform(-1.0, 1.0, (60, 2))
    pts[:50, 0] = 0.0                                               # a_2 = 0 for camera 2, a_2 < 0 for camera 3
    pts[50:60, 0] = -0.0
    pts[200] = (np.nan, 1, 1, 0)
    pts[201] = (5, np.nan, 0, 0)
    pts[202] = (5, 0, np.inf, 0)
    pts[203] = (np.inf, 1, 1, 0)
    pts[204] = (-np.inf, 1, 1, 0)
    pts[205] = (5, -np.inf, 0, 0)
    pts[206] = (np.inf, np.inf, 0, 0)
    pts[300:310, 0] = rng.uniform(0.01, 0.24, 10)                   # camera 3: a_2 = x - 0.25 < 0 with x >= 0
    pts[300:310, 1:3] = rng.uniform(-0.2, 0.2, (10, 2))
    pts[310] = (0.25, 0.1, 0.1, 0)                                  # camera 3: a_2 = 0
    pts[n - 10:] = pts[100:110]                                     # exact duplicates
    return texts, pts


def pixel_points(hits):
    """(d, -(c + 1) d, -(r + 1) d): under P = [[0,-1,0,0],[0,0,-1,0],[1,0,0,0]] the point lands on pixel (r, c) with depth d."""
    return np.array([[d, -(c + 1) * d, -(r + 1) * d, 0.5] for r, c, d in hits], dtype=np.float32)


def alias():
    H, W = 8, 6
    texts = calib_texts(H, W, [[0, -1, 0, 0], [0, 0, -1, 0], [1, 0, 0, 0]], [[1, -1, 0, 0], [0, 0, -1, 0], [1, 0, 0, 0]])
    hits = [
        (2, 5, 5.0), (3, 0, 3.0),                                   # first at (r, W-1), the minimum from (r+1, 0)
        (5, 0, 7.0), (4, 5, 2.0),                                   # first at (r+1, 0), the minimum from (r, W-1)
        (0, 5, 9.0), (1, 0, 4.0), (0, 5, 6.0),                      # three in the bucket; the last writer of (0, 5) is overruled
        (0, 0, 8.0), (0, 0, 10.0),                                  # bucket -1, the later point is farther
        (3, 3, 2.5), (3, 3, 5.5),                                   # an ordinary pixel, the later point is farther
        (3, 2, 5.25), (3, 2, 2.75),                                 # ... and nearer
        (6, 5, 11.0),                                               # alone in a shared bucket
        (1, 5, 3.5), (2, 0, 6.5),                                   # the first is already the minimum
        (7, 5, 4.0), (7, 5, 1.0),                                   # the last bucket, H (W - 1) - 1
        (7, 0, 1.5), (6, 5, 0.75),                                  # a second pass over (6, 5) / (7, 0): now three points, first at (6, 5)
        (4, 4, 12.0), (4, 4, 12.0),                                 # an exact duplicate counts as two
        (8, 0, 1.0), (0, 6, 1.0), (-1, 2, 1.0), (2, -1, 1.0),       # just outside
    ]
    return texts, pixel_points(hits)


def ties():
    H, W = 8, 12
    texts = calib_texts(H, W, [[0, -16, 0, 0], [0, 0, -16, 0], [1, 0, 0, 0]], [[0, -16, 0, 0], [0, 0, 16, 0], [1, 0, 0, 0]])
    pts = []
    k = 0
    for mu in (-1, 1, 3, 5, 2 * W - 1, 2 * W + 1):                  # u = mu / 2
        for mv in (-1, 1, 3, 5, 2 * H - 1, 2 * H + 1):              # v = mv / 2 for camera 2, -mv / 2 for camera 3
            for sign in (1, -1):
                x = 2.0 ** (k % 7 - 1)
                pts.append((x, -mu * x / 32, -sign * mv * x / 32, 0.0))
                k += 1
    return texts, np.array(pts, dtype=np.float32)


def empties():
    none_valid = np.array([[-1, 0, 0, 0], [-0.5, 1, 1, 0], [np.nan, 0, 0, 0], [1, 1e6, 0, 0], [1, 0, 1e6, 0], [1, -1e6, -1e6, 0], [-np.inf, 0, 0, 0],
                           [2, np.nan, np.nan, 0]], dtype=np.float32)
    return np.zeros((0, 4), dtype=np.float32), none_valid


def reference_rows(texts, pts, cam):
    """kitti.py:111-114 on a temporary date directory."""
    with tempfile.TemporaryDirectory() as d:
        for name, text in zip(("calib_cam_to_cam.txt", "calib_velo_to_cam.txt"), texts):
            with open(os.path.join(d, name), "w") as fh:
                fh.write(text)
        scan = os.path.join(d, "scan.bin")
        np.ascontiguousarray(pts, dtype=np.float32).tofile(scan)
        with np.errstate(all="ignore"):
            depth_map = kitti_util.generate_depth_map(d, scan, cam=cam, vel_depth=True)
        h_ind, w_ind = np.where(depth_map > 0)
        rows = np.stack([h_ind, w_ind, depth_map[h_ind, w_ind]]).transpose((1, 0))
        # the reference's own matrix, from its own reader (kitti_util.py:50-62)
        cam2cam = kitti_util.read_calib_file(os.path.join(d, "calib_cam_to_cam.txt"))
        velo2cam = kitti_util.read_calib_file(os.path.join(d, "calib_velo_to_cam.txt"))
        velo2cam = np.hstack((velo2cam["R"].reshape(3, 3), velo2cam["T"][..., np.newaxis]))
        velo2cam = np.vstack((velo2cam, np.array([0, 0, 0, 1.0])))
        R_cam2rect = np.eye(4)
        R_cam2rect[:3, :3] = cam2cam["R_rect_00"].reshape(3, 3)
        P_ref = np.dot(np.dot(cam2cam["P_rect_0" + str(cam)].reshape(3, 4), R_cam2rect), velo2cam)
        P, H, W = lidar.projection(d, cam)
    assert depth_map.shape == (H, W) and np.array_equal(P, P_ref), "projection() differs from the reference's expression"
    return np.ascontiguousarray(rows, dtype=np.float64), P, H, W


def guard_band(pts, P, H, W):
    """Kept points inside the band whose u or v lies within 1e-9 of a half-integer."""
    kept = pts[pts[:, 0] >= 0].astype(np.float64)
    with np.errstate(all="ignore"):
        a = [((P[k, 0] * kept[:, 0] + P[k, 1] * kept[:, 1]) + P[k, 2] * kept[:, 2]) + P[k, 3] for k in range(3)]
        u, v = a[0] / a[2], a[1] / a[2]
        near = (u >= -2) & (u <= W + 2) & (v >= -2) & (v <= H + 2)
        frac = np.minimum(np.abs(u - np.floor(u) - 0.5), np.abs(v - np.floor(v) - 0.5))
    return int((near & (frac <= 1e-9)).sum())


def main():
    out = {}
    empty_a, empty_b = empties()
    for name, make in (("real_calib", real_calib), ("dense", dense), ("alias", alias), ("ties", ties)):
        texts, pts = make()
        mats = []
        for cam in CAMS:
            rows, P, H, W = reference_rows(texts, pts, cam)
            if name != "ties":
                assert guard_band(pts, P, H, W) == 0, "{} camera {}: a projection within 1e-9 of a half-integer -- change the seed".format(name, cam)
            got, dense_map = lidar.depth_points_host(pts, P, H, W)
            assert got.dtype == rows.dtype and got.shape == rows.shape and np.array_equal(got, rows), "{} camera {}: the host definition differs".format(name, cam)
            for scan in (empty_a, empty_b):
                none, _, _, _ = reference_rows(texts, scan, cam)
                assert none.shape == (0, 3) and lidar.depth_points_host(scan, P, H, W)[0].shape == (0, 3), "{} camera {}: an empty scan has rows".format(name, cam)
            out["{}/rows{}".format(name, cam)] = rows
            mats.append(P)
            hit, shared = int((dense_map > 0).sum()), np.bincount((rows[:, 0] * (W - 1) + rows[:, 1]).astype(np.int64))
            print("{:10s} camera {}: {}x{}, {:6d} points, {:6d} rows ({} of {} pixels), {} buckets with two listed pixels".format(
                name, cam, H, W, pts.shape[0], rows.shape[0], hit, H * W, int((shared > 1).sum())))
        out[name + "/cam2cam"], out[name + "/velo2cam"] = np.array(texts[0]), np.array(texts[1])
        out[name + "/points"], out[name + "/P"], out[name + "/HW"] = pts, np.stack(mats), np.array([H, W], dtype=np.int64)
    out["empty/points_a"], out["empty/points_b"], out["empty/rows"] = empty_a, empty_b, np.zeros((0, 3), dtype=np.float64)
    path = os.path.join(HERE, "kitti_prepare.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 1000000, size
    print("wrote", path, size, "bytes")


if __name__ == "__main__":
    main()
