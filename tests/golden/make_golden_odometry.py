"""Golden vectors for the odometry evaluation (tests/test_eval_scripts.py, tests/test_odometry_gpu.py).

Executes the UNMODIFIED reference eval/odometry.py::eval_odom (loaded from where it lies by _refshim) on a stand-in trainer that
replays canned pose-head outputs, over a temporary segment directory of empty frame files and a generated odometry.txt.  Only data
is stored: per case the frame-pair matrices the reference formed (fp32), the global poses it read (float64), its `ates` and `speeds`
(float64) and the track length.

    python tests/golden/make_golden_odometry.py        ->  tests/golden/odometry.npz

Cases: N = 2, 3, 4, 5, 9, 70 frame pairs at track length 5; N = 9 also at track lengths 2 and 3; a 12-column (3x4) file; a track at
Waymo magnitudes (|t| ~ 4e4 m) and one at nuScenes magnitudes (~1e3 m); an all-zero prediction.
"""
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.normpath(os.path.join(HERE, "..", ".."))
for p in (HERE, ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "dynamo-depth_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
import _refshim  # noqa: E402
import odometry_case as oc  # noqa: E402

# name: (N, track_length, |t| of the first pose, columns of odometry.txt, all-zero prediction, seed)
CASES = {
    "n2": (2, 5, 1e3, 16, False, 1),
    "n3": (3, 5, 1e3, 16, False, 2),
    "n4": (4, 5, 1e3, 16, False, 3),
    "n5": (5, 5, 1e3, 16, False, 4),
    "n9": (9, 5, 1e3, 16, False, 5),
    "n9_track2": (9, 2, 1e3, 16, False, 5),
    "n9_track3": (9, 3, 1e3, 16, False, 5),
    "n9_cols12": (9, 5, 1e3, 12, False, 6),
    "n70_waymo": (70, 5, 4e4, 16, False, 7),
    "n40_nuscenes": (40, 5, 1e3, 16, False, 8),
    "n9_zero_pred": (9, 5, 4e4, 16, True, 9),
}


def load_odometry(ref):
    """The reference's eval/odometry.py as a module, its top-level imports resolving to the reference's own modules."""
    tops = _refshim._REF_TOPLEVEL
    saved = {k: sys.modules.pop(k) for k in list(sys.modules) if k.split(".")[0] in tops}
    sys.path.insert(0, _refshim.REFERENCE_ROOT)
    try:
        for name in ("options", "tools", "utils", "networks", "datasets", "Trainer"):
            sys.modules[name] = getattr(ref, name)
        spec = importlib.util.spec_from_file_location("_ref_odometry", os.path.join(_refshim.REFERENCE_ROOT, "eval", "odometry.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod
    finally:
        while _refshim.REFERENCE_ROOT in sys.path:
            sys.path.remove(_refshim.REFERENCE_ROOT)
        for k in list(sys.modules):
            if k.split(".")[0] in tops:
                del sys.modules[k]
        sys.modules.update(saved)


class Frames(torch.utils.data.Dataset):
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return {"index": torch.tensor(i)}


def run_case(odom, N, track_length, magnitude, columns, zero_pred, seed):
    axisangle, translation = oc.pose_parameters(N, seed)
    if zero_pred:
        axisangle, translation = np.zeros_like(axisangle), np.zeros_like(translation)
    gt = oc.trajectory(N + 2, magnitude, seed)               # one pose per frame file; the reference drops the first row
    with tempfile.TemporaryDirectory() as root:
        seg, cam = "segment-0", "FRONT"
        rgb = os.path.join(root, seg, cam, "rgb", "downsample")
        os.makedirs(rgb)
        for f in range(N + 2):                               # frames 0 and N+1 are edge frames: N evaluated frames
            open(os.path.join(rgb, "{:06}.jpg".format(f)), "w").close()
        rows = gt.reshape(N + 2, 16)[:, :columns]
        np.savetxt(os.path.join(root, seg, cam, "odometry.txt"), rows, fmt="%.17e")
        opt = types.SimpleNamespace(data_path=root, cam_name=cam, eval_img_type="downsample", eval_img_ext=".jpg", frame_ids=[0, -1, 1], num_workers=0)
        replay = {"a": torch.from_numpy(axisangle), "t": torch.from_numpy(translation)}

        def model(inputs):
            i = inputs["index"]
            return {("axisangle", 0, 1): replay["a"][i], ("translation", 0, 1): replay["t"][i]}

        trainer = types.SimpleNamespace(device=torch.device("cpu"), model=model, apply_img_resize=lambda inputs: None,
                                        get_dataset=lambda filenames, **kw: Frames(len(filenames)))
        ates, speeds = odom.eval_odom(opt, trainer, seg, track_length)
        read = np.loadtxt(os.path.join(root, seg, cam, "odometry.txt"))[1:].reshape(N + 1, -1, 4)
    pred = odom.transformation_from_parameters(replay["a"], replay["t"]).numpy()
    assert pred.dtype == np.float32 and pred.shape == (N, 4, 4)
    return {"pred": pred, "gt": read, "ates": np.asarray(ates, dtype=np.float64), "speeds": np.asarray(speeds, dtype=np.float64),
            "track_length": np.int64(track_length)}


def main():
    ref = _refshim.import_reference()
    odom = load_odometry(ref)
    out = {}
    for name, spec in CASES.items():
        res = run_case(odom, *spec)
        assert len(res["ates"]) == max(oc.snippet_count(spec[0], spec[1]), 0), (name, len(res["ates"]))
        print("{:14s} N {:3d} track {} snippets {:3d} ate {:.6f} speed {:.6f}".format(
            name, spec[0], spec[1], len(res["ates"]), float(np.mean(res["ates"])) if len(res["ates"]) else float("nan"),
            float(np.mean(res["speeds"])) if len(res["speeds"]) else float("nan")))
        for k, v in res.items():
            out["{}/{}".format(name, k)] = v
    path = os.path.join(HERE, "odometry.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
