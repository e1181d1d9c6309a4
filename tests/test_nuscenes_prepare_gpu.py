"""The device steps of the nuScenes preparation (csrc/dd_resize_area.hip, csrc/dd_lidar.hip through hipops.resize and hipops.lidar;
DESIGN 4.22) against their numpy definitions, and prepare_data/nuScenes.py with the device callables against the host callables.

dd_resize_area sums in fp32, the definition in float64: every byte is equal except where the float64 sum lies within 1e-4 of a
half-integer (the fp32 sum of at most 6 + 6 fused taps of values up to 255 is within 12 * 2^-17 = 9.2e-5 of it); those bytes are
left out, at most 0.1 % of a case (tests/test_nuscenes_prepare.py checks the cases against that cap on the host).
dd_lidar_pose_points computes the definition's float64 operations in the definition's order: values within 4 ulp, the same rows in
the same order; a point whose host margin to a mask threshold is below 1e-9 may fall on either side, at most 0.1 % of a batch.
dd_box_fit counts in integers: equality."""
import os
import os.path as osp

import numpy as np
import pytest
import torch

import nuscenes_prepare_case as nc

pytestmark = pytest.mark.gpu

EXCLUDED_CAP = 1e-3

RESIZE_CASES = [((2, 900, 1600, 288, 512), "noise", 11)] + [(shape, kind, seed) for shape in ((1, 7, 9, 3, 2), (3, 25, 50, 8, 16), (1, 10, 16, 10, 16), (2, 33, 47, 8, 12))
                                                            for kind, seed in (("noise", 11), ("white", 0), ("checker", 0))]


@pytest.mark.parametrize("shape,kind,seed", RESIZE_CASES)
def test_resize_area_equals_the_definition(shape, kind, seed):
    from hipops import resize
    n, hs, ws, hd, wd = shape
    frames = nc.resize_frames(kind, n, hs, ws, seed)
    sums = resize.resize_area_sums(frames, hd, wd)
    want = np.clip(np.rint(sums), 0, 255).astype(np.uint8)
    got = resize.resize_area_batch(torch.from_numpy(frames).cuda(), hd, wd)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (n, hd, wd, 3)
    got = got.cpu().numpy()
    near = np.abs(sums - np.floor(sums) - 0.5) < 1e-4
    wrong = (got != want) & ~near
    print("{} {}: {} bytes, {} near a half-integer, {} of them differ, {} others differ".format(shape, kind, got.size, int(near.sum()),
                                                                                             int(((got != want) & near).sum()), int(wrong.sum())))
    assert float(near.mean()) <= EXCLUDED_CAP
    assert not wrong.any(), np.argwhere(wrong)[:5]
    if (hs, ws) == (hd, wd):
        assert np.array_equal(got, frames)


def test_resize_area_refuses_what_it_cannot_do():
    from hipops import resize
    from hipops.lib import DynamoHipError
    x = torch.zeros((1, 4, 4, 3), dtype=torch.uint8, device="cuda")
    for bad in (lambda: resize.resize_area_batch(x, 5, 4), lambda: resize.resize_area_batch(x.cpu(), 2, 2), lambda: resize.resize_area_batch(x.float(), 2, 2)):
        with pytest.raises(DynamoHipError):
            bad()


def general_params(k):
    from hipops import lidar
    return lidar.pose_params(nc.LIDAR_CS, nc.ego_pose(k % 2, 0.2 * k), nc.ego_pose(k % 2, 0.2 * k + 0.5), nc.CAM_CS, nc.K, nc.W, nc.H)


def random_scan(rng, n, params):
    """n points spread over the camera's view and beyond it, carried back to the sensor frame."""
    cam = np.stack([rng.uniform(-12, 12, n), rng.uniform(-8, 8, n), rng.uniform(-5, 20, n)], axis=1)
    q = params
    R1, R2, R3, R4 = (q[a:a + 9].reshape(3, 3) for a in (0, 12, 27, 39))
    p = ((((cam @ R4 + q[36:39]) @ R3 + q[24:27]) - q[21:24]) @ R2 - q[9:12]) @ R1
    return np.concatenate([p, rng.uniform(0, 1, (n, 1))], axis=1).astype(np.float32)


def pose_batch(which):
    rng = np.random.default_rng(5)
    if which == "one":
        p = general_params(0)
        return [np.concatenate([random_scan(rng, 1988, p), nc.boundary_scan(p)])], [p]
    scans, params = [], []
    for k, n in enumerate((0, 1, 63, 64, 65)):
        p = general_params(k)
        scans.append(random_scan(rng, n, p))
        params.append(p)
    for k in range(13):                                               # 18 scans: the call crosses its 16-scan chunk
        p = general_params(5 + k)
        scans.append(nc.boundary_scan(p) if k % 2 else random_scan(rng, 2000 if k == 0 else 70 + k, p))
        params.append(p)
    return scans, params


def run_pose(scans, params):
    from hipops import lidar
    offsets = np.concatenate([[0], np.cumsum([s.shape[0] for s in scans])]).astype(np.int64)
    points = torch.from_numpy(np.ascontiguousarray(np.concatenate(scans)[:, :4])).cuda()
    rows, counts = lidar.pose_points(points, offsets, torch.from_numpy(np.stack(params)).cuda())
    assert rows.dtype == torch.float64 and tuple(rows.shape) == (int(offsets[-1]), 6) and counts.dtype == torch.int32 and tuple(counts.shape) == (len(scans), 1)
    return [r[0] for r in lidar.split_rows(rows, counts, offsets)]


def same(a, b):
    return bool((np.abs(a - b) <= 4 * np.spacing(np.abs(b))).all())


@pytest.mark.parametrize("which", ("one", "five_and_more"))
def test_pose_points_equal_the_definition(which):
    from hipops import lidar
    scans, params = pose_batch(which)
    got = run_pose(scans, params)
    total = ambiguous_total = kept_total = 0
    for s, (scan, p, rows) in enumerate(zip(scans, params, got)):
        want, full, kept = lidar.pose_points_host(scan, p)
        with np.errstate(all="ignore"):
            margin = np.nanmin(np.abs(np.stack([full[:, 2] - 1.0, full[:, 0] - 1.0, full[:, 0] - (p[57] - 1.0), full[:, 1] - 1.0, full[:, 1] - (p[58] - 1.0)])), axis=0) \
                if scan.shape[0] else np.zeros(0)
        ambiguous = ~(margin >= 1e-9)
        total, ambiguous_total, kept_total = total + scan.shape[0], ambiguous_total + int(ambiguous.sum()), kept_total + int(kept.sum())
        if not ambiguous.any():
            assert rows.shape == want.shape, (s, rows.shape, want.shape)
        j = 0
        for i in range(scan.shape[0]):                                # the device's rows are the host's kept points, in order
            with np.errstate(all="ignore"):
                hit = j < rows.shape[0] and same(rows[j], full[i])
            if hit and (kept[i] or ambiguous[i]):
                j += 1
            elif kept[i] and not ambiguous[i]:
                raise AssertionError("scan {} point {}: kept by the definition, missing or different on the device".format(s, i))
        assert j == rows.shape[0], (s, j, rows.shape)
    print("{}: {} points, {} kept, {} within 1e-9 of a threshold".format(which, total, kept_total, ambiguous_total))
    assert kept_total > total // 20 and ambiguous_total <= EXCLUDED_CAP * total


def test_pose_points_on_the_exact_thresholds():
    """Identity poses and power-of-two intrinsics: no operation rounds, so the thresholds themselves decide, strictly."""
    from hipops import lidar
    params = nc.exact_params()
    scan = nc.boundary_scan(params)
    rows = run_pose([scan, scan[:0], scan], [params] * 3)
    want = lidar.pose_points_host(scan, params)[0]
    assert want.shape == (3, 6) and np.array_equal(rows[0], want) and rows[1].shape == (0, 6) and np.array_equal(rows[2], want)


def box_case(rng, n, n_labels, B):
    from hipops import lidar
    pts = rng.uniform(-10, 10, size=(n, 3))
    cuts = np.sort(rng.integers(0, n + 1, size=n_labels - 1)) if n_labels > 1 else np.zeros(0, dtype=np.int64)
    if n_labels > 2:
        cuts[1] = cuts[0]                                             # an empty label
    seg = np.concatenate([[0], cuts, [n]]).astype(np.int32)
    label_cat = rng.choice([17, 2, 9], size=n_labels)
    corners, box_cat = [], []
    for b in range(B):
        if b % 5 == 1:                                                # the same box twice: a tie, the first one wins
            corners.append(corners[-1])
            box_cat.append(box_cat[-1])
            continue
        yaw = rng.uniform(0, np.pi)
        corners.append(lidar.box_corners(rng.uniform(-6, 6, 3), rng.uniform(4, 14, 3), [np.cos(yaw / 2), 0, 0, np.sin(yaw / 2)]))
        box_cat.append(int(rng.choice([17, 2])))
    return pts, seg, label_cat, lidar.box_params(np.array(corners).reshape(-1, 8, 3)), np.array(box_cat, dtype=np.int32)


@pytest.mark.parametrize("B", (0, 1, 40))
@pytest.mark.parametrize("n", (1, 64, 3000))
@pytest.mark.parametrize("n_labels", (1, 17))
def test_box_fit_equals_the_definition(n_labels, n, B):
    from hipops import lidar
    case = box_case(np.random.default_rng(1000 * n_labels + 10 * B + n), n, n_labels, B)
    want_counts, want_best = lidar.box_fit_host(*case)
    counts, best = lidar.box_fit(*case)
    assert counts.dtype == np.int32 and best.dtype == np.int32
    assert np.array_equal(counts, want_counts) and np.array_equal(best, want_best)
    sizes = np.diff(case[1])
    with np.errstate(all="ignore"):
        assert np.array_equal(np.where(sizes > 0, best[:, 1] / sizes, 0.0), np.where(sizes > 0, want_best[:, 1] / sizes, 0.0))
    if B == 40 and n == 3000:
        assert (want_best[:, 0] >= 0).any() and (want_counts > 0).sum() > 10
        ties = [l for l in range(n_labels) if want_best[l, 0] >= 0 and (want_counts[l] == want_best[l, 1]).sum() > 1]
        assert n_labels == 1 or ties, "the case holds no tie"


def tree_files(root):
    out = {}
    for d, _, files in os.walk(osp.join(root, "scenes")):
        for f in files:
            out[osp.relpath(osp.join(d, f), root)] = osp.join(d, f)
    return out


def test_script_with_the_device_steps_writes_the_host_steps_files(tmp_path):
    from prepare_data import nuScenes
    roots = [str(tmp_path / "host"), str(tmp_path / "device")]
    expect = nc.write_tree(roots[0])
    nc.write_tree(roots[1])
    nuScenes.prepare(roots[0], batch=2, num_workers=3, log=lambda s: None, **nc.host_steps())
    nuScenes.prepare(roots[1], batch=2, num_workers=3, log=lambda s: None)
    nc.check_tree(roots[1], expect)
    a, b = tree_files(roots[0]), tree_files(roots[1])
    assert sorted(a) == sorted(b) and len(a) == 2 * (3 + 3 + 3 + 2 + 3)
    for rel in a:
        if rel.endswith(".npy"):
            assert np.array_equal(np.load(a[rel]), np.load(b[rel])), rel
        elif rel.endswith(".npz"):
            with np.load(a[rel], allow_pickle=True) as x, np.load(b[rel], allow_pickle=True) as y:
                assert x.files == y.files
                assert np.array_equal(x["panoptic_label"], y["panoptic_label"]) and np.array_equal(x["motion_label"], y["motion_label"])
                assert x["panoptic2ann"].item() == y["panoptic2ann"].item()
        elif "original" not in rel:
            assert open(a[rel], "rb").read() == open(b[rel], "rb").read(), rel
