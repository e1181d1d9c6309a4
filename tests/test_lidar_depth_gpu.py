"""dd_lidar_depth_points (csrc/dd_lidar.hip through hipops.lidar) on the device against the reference's own rows
(tests/golden/kitti_prepare.npz) and the numpy definition's dense maps: equality only.  Every golden case and both cameras in one
batched call per image size -- scans of different lengths with the empty ones between them, 18 scans for the small images so that the
call crosses its 16-scan chunk; the same call twice; the outputs inside poisoned buffers; the invalid arguments; one drive through
prepare_data/kitti.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import kitti_prepare_case as kc

pytestmark = pytest.mark.gpu

POISON = 0xA5
_host = {}


def batch(g, case):
    """[(scan, golden key or None)]: the case's scan, the two empty ones, a prefix of the scan (its rows from the host definition)."""
    pts = g[case + "/points"]
    unit = [(pts, case), (g["empty/points_a"], "empty"), (pts[:pts.shape[0] * 2 // 3 + 1], None), (g["empty/points_b"], "empty")]
    if case == "real_calib":
        return unit
    return (unit * 5)[:18]


def expected(g, case):
    """Per scan of `batch`: ([rows per camera], [map per camera]); the host definition runs once per distinct scan."""
    if case not in _host:
        from hipops import lidar
        H, W = (int(v) for v in g[case + "/HW"])
        seen, out = {}, []
        for scan, key in batch(g, case):
            tag = (scan.shape[0], key)
            if tag not in seen:
                both = [lidar.depth_points_host(scan, g[case + "/P"][c], H, W) for c in range(2)]
                rows = [b[0] for b in both]
                if key == case:
                    rows = [g["{}/rows{}".format(case, cam)] for cam in kc.CAMS]            # the reference's
                elif key == "empty":
                    rows = [g["empty/rows"]] * 2
                seen[tag] = (rows, [b[1] for b in both])
            out.append(seen[tag])
        _host[case] = out
    return _host[case]


def upload(g, case):
    scans = [s for s, _ in batch(g, case)]
    offsets = np.concatenate([[0], np.cumsum([s.shape[0] for s in scans])]).astype(np.int32)
    return torch.from_numpy(np.concatenate(scans)).cuda(), offsets, torch.from_numpy(np.array(g[case + "/P"])).cuda()


@pytest.mark.parametrize("case", kc.CASES)
def test_rows_counts_and_maps_equal_the_golden(golden_dir, case):
    from hipops import lidar
    g = kc.golden(golden_dir)
    H, W = (int(v) for v in g[case + "/HW"])
    points, offsets, P = upload(g, case)
    rows, counts, maps = lidar.depth_points(points, offsets, P, H, W, return_maps=True)
    assert rows.shape == (2 * points.shape[0], 3) and rows.dtype == torch.float64 and counts.dtype == torch.int32 and maps.dtype == torch.float32
    jobs = lidar.split_rows(rows, counts, offsets)
    counts, maps = counts.cpu().numpy(), maps.cpu().numpy()
    want = expected(g, case)
    assert len(jobs) == len(want) == offsets.size - 1
    for s, (want_rows, want_maps) in enumerate(want):
        for c in range(2):
            assert int(counts[s, c]) == want_rows[c].shape[0], (s, c, int(counts[s, c]), want_rows[c].shape[0])
            assert jobs[s][c].dtype == np.float64 and jobs[s][c].shape == want_rows[c].shape and np.array_equal(jobs[s][c], want_rows[c]), (s, c)
            assert np.array_equal(maps[s, c], want_maps[c]), (s, c)
            assert not np.signbit(maps[s, c]).any()


def raw_call(g, case, with_maps=True):
    """The C call with every output at an odd element offset inside a poisoned buffer: (code, rows, counts, maps buffers as bytes on the host)."""
    from hipops import lib as L
    lib = L.load()
    H, W = (int(v) for v in g[case + "/HW"])
    points, offsets, P = upload(g, case)
    S, n_total = offsets.size - 1, int(points.shape[0])
    sizes = {"rows": 2 * n_total * 24, "counts": S * 2 * 4, "maps": S * 2 * H * W * 4}
    at = {"rows": 7 * 8, "counts": 3 * 4, "maps": 5 * 4}
    bufs = {k: torch.full((at[k] + sizes[k] + 64,), POISON, dtype=torch.uint8, device="cuda") for k in sizes}
    need = int(lib.dd_lidar_depth_points_workspace_bytes(S, 2, H, W))
    work = torch.full((need + 64,), POISON, dtype=torch.uint8, device="cuda")
    ptr = {k: C.c_void_p(bufs[k].data_ptr() + at[k]) for k in sizes}
    code = lib.dd_lidar_depth_points(C.c_void_p(points.data_ptr()), n_total, offsets.ctypes.data_as(C.POINTER(C.c_int32)), S, C.c_void_p(P.data_ptr()), 2,
                                     H, W, ptr["counts"], ptr["rows"], ptr["maps"] if with_maps else None, C.c_void_p(work.data_ptr()), need, L.current_stream())
    torch.cuda.synchronize()
    host = {k: bufs[k].cpu().numpy() for k in sizes}
    host["work_tail"] = work[need:].cpu().numpy()
    return code, host, at, sizes, offsets


@pytest.mark.parametrize("case", ("dense", "alias", "real_calib"))
def test_same_call_twice_and_nothing_outside_the_extents(golden_dir, case):
    g = kc.golden(golden_dir)
    H, W = (int(v) for v in g[case + "/HW"])
    code, first, at, sizes, offsets = raw_call(g, case)
    code2, second, _, _, _ = raw_call(g, case)
    assert code == 0 and code2 == 0
    for k in first:
        assert np.array_equal(first[k], second[k]), k                 # bit-identical, poison included
    want = expected(g, case)
    written = {k: np.zeros(first[k].size, dtype=bool) for k in sizes}
    written["counts"][at["counts"]:at["counts"] + sizes["counts"]] = True
    written["maps"][at["maps"]:at["maps"] + sizes["maps"]] = True
    counts = first["counts"][at["counts"]:at["counts"] + sizes["counts"]].view(np.int32).reshape(-1, 2)
    rows = first["rows"][at["rows"]:at["rows"] + sizes["rows"]].view(np.float64).reshape(-1, 3)
    for s, (want_rows, _) in enumerate(want):
        n = int(offsets[s + 1] - offsets[s])
        for c in range(2):
            start = 2 * int(offsets[s]) + c * n                     # the job's segment: n rows, the first counts[s, c] of them written
            assert int(counts[s, c]) == want_rows[c].shape[0] <= n
            assert np.array_equal(rows[start:start + counts[s, c]], want_rows[c]), (s, c)
            written["rows"][at["rows"] + 24 * start:at["rows"] + 24 * (start + int(counts[s, c]))] = True
    for k in sizes:
        assert (first[k][~written[k]] == POISON).all(), k
    assert (first["work_tail"] == POISON).all()
    code3, third, _, _, _ = raw_call(g, case, with_maps=False)      # without the maps: the same rows, the maps buffer untouched
    assert code3 == 0 and np.array_equal(third["rows"], first["rows"]) and np.array_equal(third["counts"], first["counts"])
    assert (third["maps"] == POISON).all()


def test_invalid_arguments_return_1_and_launch_nothing(golden_dir):
    from hipops import lib as L
    lib = L.load()
    g = kc.golden(golden_dir)
    H, W = (int(v) for v in g["alias/HW"])
    scans = [g["alias/points"], g["empty/points_a"], g["alias/points"][:9]]
    offsets = np.concatenate([[0], np.cumsum([s.shape[0] for s in scans])]).astype(np.int32)
    points = torch.from_numpy(np.concatenate(scans)).cuda()
    P = torch.from_numpy(np.array(g["alias/P"])).cuda()
    S, n_total = 3, int(points.shape[0])
    need = int(lib.dd_lidar_depth_points_workspace_bytes(S, 2, H, W))
    out = {k: torch.full((8192,), POISON, dtype=torch.uint8, device="cuda") for k in ("rows", "counts", "maps", "work")}
    assert need <= 8192 and 2 * n_total * 24 <= 8192 and S * 2 * H * W * 4 <= 8192
    decreasing = np.array([0, offsets[2], offsets[1] - 1, offsets[3]], dtype=np.int32)
    good = dict(points=C.c_void_p(points.data_ptr()), n_total=n_total, offsets=offsets, S=S, P=C.c_void_p(P.data_ptr()), C=2, H=H, W=W,
                counts=C.c_void_p(out["counts"].data_ptr()), rows=C.c_void_p(out["rows"].data_ptr()), maps=C.c_void_p(out["maps"].data_ptr()),
                work=C.c_void_p(out["work"].data_ptr()), bytes=need)

    def call(**change):
        a = dict(good, **change)
        off = None if a["offsets"] is None else a["offsets"].ctypes.data_as(C.POINTER(C.c_int32))
        code = lib.dd_lidar_depth_points(a["points"], a["n_total"], off, a["S"], a["P"], a["C"], a["H"], a["W"], a["counts"], a["rows"], a["maps"], a["work"],
                                         a["bytes"], L.current_stream())
        torch.cuda.synchronize()
        return code

    bad = [dict(points=None), dict(offsets=None), dict(P=None), dict(counts=None), dict(rows=None), dict(work=None), dict(S=0), dict(S=-1), dict(C=0),
           dict(H=0), dict(W=1), dict(H=65536, W=32768), dict(n_total=2 ** 31), dict(n_total=n_total + 1), dict(offsets=decreasing),
           dict(offsets=offsets + 1), dict(bytes=need - 1), dict(bytes=0)]
    for change in bad:
        assert call(**change) == 1, change
        for k, t in out.items():
            assert bool((t == POISON).all()), (change, k)
    assert call() == 0                                              # and the unchanged arguments are accepted
    assert not bool((out["counts"] == POISON).all())


def test_hipops_wrapper_refuses_what_it_cannot_launch():
    from hipops import lidar
    from hipops.lib import DynamoHipError
    pts, P = torch.zeros((4, 4), device="cuda"), torch.zeros((2, 3, 4), dtype=torch.float64, device="cuda")
    for args in ((pts.cpu(), [0, 4], P, 8, 6), (pts, [0, 4], P.float(), 8, 6), (pts, torch.tensor([0, 4]).cuda(), P, 8, 6), (pts, [0, 5], P, 8, 6),
                 (pts, [0, 4], P, 8, 1), (pts, [4], P, 8, 6)):
        with pytest.raises(DynamoHipError):
            lidar.depth_points(*args)
    rows, counts = lidar.depth_points(pts[:0], [0, 0, 0], P, 8, 6)      # a batch of empty scans
    assert rows.shape == (0, 3) and counts.cpu().tolist() == [[0, 0], [0, 0]]


def test_script_on_the_device_path(golden_dir, tmp_path, capsys):
    from prepare_data import kitti
    g = kc.golden(golden_dir)
    raw, out = str(tmp_path / "raw"), str(tmp_path / "out")
    scans = kc.write_raw_tree(raw, g)
    kitti.main([raw, out, "--height", str(kc.OUT_H), "--width", str(kc.OUT_W), "--batch", "2", "--num_workers", "3"])
    kc.check_tree(raw, out, scans, g, capsys.readouterr().out)
    kc.check_reader(out, scans, g)
