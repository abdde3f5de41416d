"""Measures, on the GPU, how far the float32 noise stages of ssp_op_photometric_apply stray from the float64 restatement
(tests/photometric_ref.py::noise): for every pixel whose level differs from rint(p_ref), the smallest e / base that admits it.
The test cases of tests/test_gpu_draws_exact.py hold too few pixels to meet a flipped rounding, so three populations of 4.9 M
pixels are measured beside them.  Prints the report that profiles/draws_exact_measure.txt keeps; NOISE_TAU = 4 x the largest
ratio, rounded up to a power of two.  Usage: python tools/measure_draws_noise.py [output file]"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from semantic_superpoint_amd import lib as L   # noqa: E402
from tests import draws_cases as DC            # noqa: E402
from tests import photometric_ref as P         # noqa: E402

dev = torch.device("cuda:0")
lines = []
worst = 0.0


def measure(img, rows):
    x = torch.from_numpy(img).view(1, 1, *img.shape).repeat(len(rows), 1, 1, 1).contiguous().to(dev)
    out = L.op_photometric_apply(x, torch.from_numpy(rows).to(dev)).cpu().numpy()[:, 0]
    s_all = []
    for b in range(len(rows)):
        s_all += list(P.noise_samples(img, rows[b], out[b])[0])
    return sorted(s_all)


for H, W in DC.NOISE_SIZES:
    for name, (img, rows) in DC.noise_cases(H, W).items():
        if rows[0][P.BLUR_FLAG] != 0:
            continue
        s = measure(img, rows)
        worst = max([worst] + s)
        lines.append("%dx%d %-14s pixels %8d  level != rint(p_ref) at %3d  largest e/base admitting them %.3e" %
                     (H, W, name, len(rows) * H * W, len(s), max(s) if s else 0.0))
for kw in (dict(sigma=10.0, impulse_p=0.0035), dict(sigma=10.0, contrast=1.4), dict(sigma=3.0)):
    H, W, nrow = 240, 320, 64
    rows = np.stack([P.make_row(key=(0x9E3779B97F4A7C15 * (k + 1)) & (2 ** 64 - 1), **kw) for k in range(nrow)])
    s = measure(P.case_image(H, W, seed=3), rows)
    worst = max([worst] + s)
    lines.append("%dx%d x %d rows %-40s pixels %8d  level != rint(p_ref) at %3d  largest e/base admitting them %.3e" %
                 (H, W, nrow, kw, nrow * H * W, len(s), max(s) if s else 0.0))
lines.append("largest ratio over all cases %.6e   (photometric_ref.NOISE_MEASURED %.6e, NOISE_TAU 2^%d)" %
             (worst, P.NOISE_MEASURED, int(np.log2(P.NOISE_TAU))))
print("\n".join(lines))
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
