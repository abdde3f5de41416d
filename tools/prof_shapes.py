"""Workload of the per-kernel table of the Synthetic Shapes feed: 10 batches of 64 at the shipped config, draw + render + feed,
no network step.  Run under `rocprofv3 --kernel-trace --stats --output-format csv -- python tools/prof_shapes.py`."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench_shapes  # noqa: E402
from semantic_superpoint_amd import shapes  # noqa: E402

loader = shapes.SyntheticShapes(bench_shapes.config(64), "train", device="cuda:0", seed=0, length=10)
for s in loader:
    pass
torch.cuda.synchronize()
