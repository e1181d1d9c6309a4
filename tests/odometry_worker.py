"""eval/odometry.py in a process of its own, as its launch line starts it, with seeded scratch weights (the options have no seed):

    python tests/odometry_worker.py <seed> <arguments of eval/odometry.py ...>

The script's module comes first: it sets the process's MIOpen environment (miopen_env.setup()) before torch is imported."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dynamo-depth_amd"))

from eval import odometry as od  # noqa: E402

import torch  # noqa: E402

if __name__ == "__main__":
    torch.manual_seed(int(sys.argv[1]))
    od.main(sys.argv[2:])
