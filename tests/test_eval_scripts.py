"""The host side of eval/depth.py and eval/odometry.py, no GPU: the snippet rule restated in tests/odometry_case.py against the
reference's recorded results (tests/golden/odometry.npz), dd_odom_snippet_count's formula, odometry.txt parsing, the names of the
output files and the line formats of both scripts, and the three new names in the ABI list."""
import ctypes
import os
import re

import numpy as np
import pytest

import odometry_case as oc

NUM = r"-?\d+\.\d{3}"


@pytest.fixture(scope="module")
def golden(golden_dir):
    z = np.load(os.path.join(golden_dir, "odometry.npz"))
    names = sorted(set(k.split("/")[0] for k in z.files))
    return {n: {k: z["{}/{}".format(n, k)] for k in ("pred", "gt", "ates", "speeds", "track_length")} for n in names}


def test_golden_holds_the_cases(golden):
    by_n = {c["pred"].shape[0] for c in golden.values() if int(c["track_length"]) == 5}
    assert {2, 3, 4, 5, 9, 70} <= by_n
    assert {int(c["track_length"]) for c in golden.values() if c["pred"].shape[0] == 9} >= {2, 3, 5}
    assert any(c["gt"].shape[1] == 3 for c in golden.values())                                  # a 12-column file
    mags = [np.linalg.norm(c["gt"][0, :3, 3]) for c in golden.values()]
    assert any(3e4 < m < 5e4 for m in mags) and any(5e2 < m < 2e3 for m in mags)                # Waymo and nuScenes magnitudes
    assert any(np.isnan(c["ates"]).all() and len(c["ates"]) for c in golden.values())           # the all-zero prediction
    for c in golden.values():
        assert c["pred"].dtype == np.float32 and c["gt"].dtype == np.float64 and c["ates"].dtype == np.float64 and c["speeds"].dtype == np.float64


def test_restatement_reproduces_the_reference(golden):
    worst = 0.0
    for name, c in golden.items():
        ates, speeds, ext = oc.snippets(c["pred"], c["gt"], int(c["track_length"]))
        assert ates.shape == c["ates"].shape and speeds.shape == c["speeds"].shape, name
        if len(ates) == 0:
            continue
        ua, us = oc.units(ates, c["ates"], c["gt"], ext), oc.units(speeds, c["speeds"], c["gt"], ext)
        print("{:14s} restatement vs reference: ate {:.3f} speed {:.3f} units (bound {:.3f})".format(name, ua.max(), us.max(), oc.BOUND_UNITS))
        assert ua.max() <= oc.BOUND_UNITS and us.max() <= oc.BOUND_UNITS, (name, ua.max(), us.max())
        assert np.array_equal(np.isnan(ates), np.isnan(c["ates"])), name
        worst = max(worst, ua.max(), us.max())
    assert worst > 0                # not a comparison of the golden with itself


def test_reference_error_is_the_recorded_one(golden):
    """REFERENCE_ERROR_UNITS is the measured distance of the reference's float64 results from extended precision: re-measured here
    where the platform's long double is wider than double."""
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        return                      # long double is double on this platform: nothing to measure with
    worst = 0.0
    for c in golden.values():
        ates, speeds, ext = oc.snippets(c["pred"], c["gt"], int(c["track_length"]), np.longdouble)
        if len(ates):
            worst = max(worst, oc.units(c["ates"], ates, c["gt"], ext).max(), oc.units(c["speeds"], speeds, c["gt"], ext).max())
    print("reference float64 vs long double: {:.4f} units".format(worst))
    assert abs(worst - oc.REFERENCE_ERROR_UNITS) <= 0.01 * oc.REFERENCE_ERROR_UNITS


def test_short_last_snippet(golden):
    """N = 3 at track length 5: one snippet of four points; every segment's last snippet is one point short."""
    c = golden["n3"]
    assert len(c["ates"]) == 1 and len(golden["n2"]["ates"]) == 0
    full = oc.snippets(golden["n9"]["pred"], golden["n9"]["gt"], 5)[1]
    # the last kept snippet's speed averages three steps, not four: dropping the segment's last pose changes nothing before it
    cut = oc.snippets(golden["n9"]["pred"][:8], golden["n9"]["gt"][:9], 5)[1]
    assert len(full) == 7 and len(cut) == 6 and np.array_equal(full[:5], cut[:5]) and full[5] != cut[5]


def _count_functions():
    fns = [oc.snippet_count]
    from tools import OdometryMetrics
    fns.append(lambda n, t: OdometryMetrics(t).snippet_count(n) if 2 <= t <= 16 else -1)
    try:
        from hipops import abi, lib
        so = ctypes.CDLL(lib.LIB_PATH)
        abi.declare(so)
        fns.append(so.dd_odom_snippet_count)
    except (OSError, AttributeError):
        pass                        # the library does not load without a GPU runtime here: the pure-Python twins stand in
    return fns


def test_snippet_count_formula(golden):
    for fn in _count_functions():
        for c in golden.values():
            assert fn(c["pred"].shape[0], int(c["track_length"])) == len(c["ates"])
        for n in range(1, 40):
            for t in range(2, 17):
                kept = sum(1 for i in range(n) if min(t - 1, n - i) + 1 >= t - 1)           # the reference's loop and its `continue`
                assert fn(n, t) == kept, (n, t)
        assert fn(0, 5) == -1 and fn(5, 1) == -1 and fn(5, 17) == -1 and fn(-3, 5) == -1


@pytest.mark.parametrize("columns", [12, 16])
def test_odometry_txt_parsing(tmp_path, columns):
    from eval import odometry as od
    gt = oc.trajectory(7, 1e3, seed=3)                      # 7 frame files: 5 evaluated frames, 6 poses after the first
    path = tmp_path / "odometry.txt"
    np.savetxt(path, gt.reshape(7, 16)[:, :columns], fmt="%.17e")
    read = od.read_odometry(str(path), 5)
    assert read.shape == (6, columns // 4, 4) and read.dtype == np.float64
    assert np.array_equal(oc.pad_global(read), gt[1:])
    with pytest.raises(AssertionError, match="pose rows"):
        od.read_odometry(str(path), 4)


def test_odometry_output_names_and_lines(tmp_path):
    from eval import odometry as od
    from options import DynamoOptions
    opt = DynamoOptions().parse(args=["-d", "waymo", "-l", "logs/run7/models/weights_19", "--eval_dir", str(tmp_path)])
    txt, npy = od.output_paths(opt, 5)
    assert txt == str(tmp_path / "run7_waymo" / "odometry" / "record_weights_19-5.txt")
    assert npy == str(tmp_path / "run7_waymo" / "odometry" / "record_weights_19-5.npy") and os.path.isdir(os.path.dirname(txt))
    ates, speeds = np.array([0.5, 0.25, 0.75]), np.array([1.0, 2.0, 3.0])
    line = od.segment_line("segment-1", 5, ates, speeds, 12)
    assert line == "{:50s} Track=5 ATE: 0.500 ± 0.204,  Speed: 2.000 ± 0.816,  Len: 12".format("segment-1")
    assert re.fullmatch(r"segment-1 {41} Track=5 ATE: NUM ± NUM,  Speed: NUM ± NUM,  Len: \d+".replace("NUM", NUM), line)
    empty = od.segment_line("segment-2", 5, ates[:0], speeds[:0], 12)
    assert re.fullmatch(r"segment-2 {41} Track=5 ATE: nan ± nan,  Speed: nan ± nan,  Len: 12", empty)
    lines = od.summary_lines(ates, speeds, 5)
    assert lines == ["\nATE Trajectory error (Track=5):  ", "Mean:   0.5", "std:    {}".format(np.std(ates)), "--", "Min:    0.25", "Median: 0.5",
                     "Max:    0.75", "==", "\nSpeed:  ", "Mean:   2.0", "std:    {}".format(np.std(speeds)), "--", "Min:    1.0", "Median: 2.0",
                     "Max:    3.0", "--", "len:    3"]
    assert od.summary_lines(ates[:0], speeds[:0], 5)[1] == "Mean:   nan"


def test_depth_output_name_and_lines(tmp_path):
    from eval import depth as dp
    from options import DynamoOptions
    opt = DynamoOptions().parse(args=["-d", "nuscenes", "-l", "logs/run7/models/weights_19", "--eval_dir", str(tmp_path)])
    assert dp.output_path(opt) == str(tmp_path / "run7_nuscenes" / "depth" / "weights_19.txt")
    names = ["de:abs_rel", "de:sq_rel", "de:rms", "de:log_rms", "da:a1", "da:a2", "da:a3"]
    header = dp.display_str(["Split"] + names)
    assert len(header) == 8 * 15 and header.split() == ["Split"] + names
    values = [0.1234, 1.0, 6.5, 0.2, 0.85, 0.95, 0.99]
    res = {"overall": dict(zip(names, values)), "num": 10, "skipped": 2,
           "by_label": {0: dict(zip(names, values)), 1: dict(zip(names, [2 * v for v in values]))}}
    row = dp.overall_row(res, names)
    assert row == "    OVERALL        & 0.123        & 1.000        & 6.500        & 0.200        & 0.850        & 0.950        & 0.990    "
    assert re.fullmatch(r" *OVERALL *(& {} *){{7}}".format(NUM), row) and len(row) == 8 * 15
    bg, static, mot = dp.split_rows(res, names)
    assert re.fullmatch(r" *BG *(& {} *){{7}}".format(NUM), bg) and "& 0.123" in bg
    assert re.fullmatch(r" *STATIC *(& nan *){7}", static)                                   # label 2 saw no LiDAR point
    assert re.fullmatch(r" *MOT *(& {} *){{7}}".format(NUM), mot) and "& 0.247" in mot
    assert re.search(r"\b2 of 12 samples\b", dp.skipped_line(res))


def test_new_entry_points_are_listed():
    from hipops import abi
    for name in ("dd_depth_metrics_accumulate", "dd_odom_snippet_count", "dd_odom_snippets"):
        assert name in abi.EXPORTED
    assert abi.DD_ABI_VERSION == 2
