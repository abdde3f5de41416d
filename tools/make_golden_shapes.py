"""Writes tests/golden/g18_shapes_tables.npz: scene tables drawn on the GPU at the small size of tests/shapes_ref.py (one image
per primitive plus two mixed batches), so that tests/test_shapes_cpu.py can check the flip-set cap without a device."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from semantic_superpoint_amd import lib as L  # noqa: E402
from tests import shapes_ref as R  # noqa: E402

data = json.load(open(os.path.join(ROOT, "tests", "golden", "g18_shapes_config.json")))["data"]
out = {}
for k, name in enumerate(L.SHAPES_PRIMITIVES):
    out["prim%d" % k] = L.op_shapes_draw(1, 100 + k, R.small_config(data, name), "cuda").cpu().numpy()
for key, seed in R.FIXTURE_SEEDS.items():
    out[key] = L.op_shapes_draw(4, seed, R.small_config(data), "cuda").cpu().numpy()
path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "g18_shapes_tables.npz")
np.savez_compressed(path, **out)
print("wrote", path, os.path.getsize(path), "bytes")
