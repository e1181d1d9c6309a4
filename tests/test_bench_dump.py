"""bench.py --dump-outputs without a GPU: bench.dump_outputs on CPU tensors, in a child process (importing bench.py sets up the
MIOpen environment of a benchmark process, which the test process keeps out of)."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = """
import sys, torch
sys.path.insert(0, {root!r})
import bench
bench.DUMP_LIMIT_BYTES = 1 << 16
outputs = {{("disp", 0, 0): torch.arange(100000, dtype=torch.float32).reshape(1, 1, 100, 1000).contiguous(memory_format=torch.channels_last),
            ("cam_T_cam", 0, -1): torch.eye(4, dtype=torch.float64), "not a tensor": 3}}
losses = {{"loss": torch.tensor(0.5, requires_grad=True) * 1, "loss_term/d_ground": torch.tensor(0.25, dtype=torch.float16)}}
bench.dump_outputs(sys.argv[1], outputs, losses)
"""


def _dump(dest):
    res = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT), str(dest)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         text=True, timeout=300, env=dict(os.environ, HIP_VISIBLE_DEVICES=""))
    assert res.returncode == 0, res.stderr[-3000:]
    return {f.name: np.load(f) for f in sorted(dest.glob("*.npy"))}


def test_dump_names_dtypes_and_a_fixed_sample_within_the_limit(tmp_path):
    a, b = _dump(tmp_path / "a"), _dump(tmp_path / "b")
    assert sorted(a) == ["losses.loss.npy", "losses.loss_term-d_ground.npy", "outputs.cam_T_cam_0_-1.npy", "outputs.disp_0_0.npy"]
    assert sum(x.nbytes for x in a.values()) <= 1 << 16
    assert a["outputs.cam_T_cam_0_-1.npy"].dtype == np.float64 and np.array_equal(a["outputs.cam_T_cam_0_-1.npy"], np.eye(4))
    assert a["losses.loss.npy"].dtype == np.float32 and float(a["losses.loss.npy"]) == 0.5
    assert a["losses.loss_term-d_ground.npy"].dtype == np.float32 and float(a["losses.loss_term-d_ground.npy"]) == 0.25
    # the large tensor: a sample of its flattened values in logical order (value == flat index), the same elements in both runs
    s = a["outputs.disp_0_0.npy"]
    assert s.dtype == np.float32 and s.ndim == 1 and 0 < s.size < 100000
    assert np.all(np.diff(s) > 0) and s[0] >= 0 and s[-1] < 100000 and np.array_equal(s, np.round(s))
    assert all(np.array_equal(a[k], b[k]) for k in a)
