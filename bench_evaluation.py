#!/usr/bin/env python3
"""bench_evaluation.py - pairs/s of the device evaluation (evaluation.py -r -homo without file I/O) on one MI355X.

eval: P synthetic 240x320 export pairs (~1000 points per image, tests/golden_evaluation.py-style linked descriptors with
exact inliers and gross outliers) resident on the device; a step = repeatability + matching-score count, the crossCheck
matcher and its RANSAC, the nn-1.2 matcher and its RANSAC with AP, closed by the one host read of the per-pair results
(Evaluator.run_points).  fused: DescriptorExporter.run_device followed by Evaluator.run_device on random-init weights.

`python bench_evaluation.py [--steps K] [--warmup W] [--pairs 16]` prints ONE JSON line.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=16)
    ap.add_argument("--no-fused", action="store_true", help="skip the export + evaluation measurement")
    return ap.parse_args(argv)


def _timed(fn, steps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def main(argv=None):
    args = parse_args(argv)
    import numpy as np
    import torch
    from semantic_superpoint_amd.evaluation import Evaluator, _upload
    from tests.golden_evaluation import case_pair

    assert torch.cuda.is_available(), "bench_evaluation.py needs an MI355X"
    if args.gpus != 1:
        raise SystemExit("bench_evaluation.py measures one GPU (--gpus 1)")
    dev = torch.device("cuda:0")
    datas = [case_pair(("bench", 5000 + k, 600, 200, 200, 200, 0.0, "persp"))[0] for k in range(args.pairs)]
    pts, cnt, desc = _upload(datas, dev)
    Hs = np.stack([d["homography"] for d in datas])
    ev = Evaluator(240, 320)
    dt = _timed(lambda: ev.run_points(pts, cnt, desc, Hs, list(range(args.pairs))), args.steps, args.warmup)
    out = {"metric": "evaluation_pairs_per_s", "value": round(args.pairs / dt, 2), "unit": "pairs/s",
           "ms_per_step": round(dt * 1e3, 3), "pairs_per_step": args.pairs,
           "mean_points_per_image": round(float(cnt.float().mean()), 1), "steps": args.steps, "warmup": args.warmup}
    if not args.no_fused:
        from oracle import cpu_ref as C
        from semantic_superpoint_amd import models
        from semantic_superpoint_amd.export import DescriptorExporter
        arch = "SuperPointNet_gauss2_ssmall"
        net = getattr(models, arch)()
        net.load_state_dict({k: torch.as_tensor(np.array(v)) for k, v in C.init_state_dict(arch, seed=0).items()})
        net = net.to(dev).eval()
        ex = DescriptorExporter(net, dev, conf_thresh=0.0155, nms_dist=4, subpixel=True, nn_thresh=0.7)
        rs = np.random.RandomState(0)
        pairs = []
        for _ in range(args.pairs):
            a = torch.from_numpy(rs.uniform(0, 1, (240, 320)).astype(np.float32))
            pairs.append((a.to(dev), torch.roll(a, (2, 3), (0, 1)).to(dev)))
        hom = [np.array([[1.0, 0, 3], [0, 1.0, 2], [0, 0, 1]])] * args.pairs
        dtf = _timed(lambda: ev.run_device(ex.run_device(pairs), hom, list(range(args.pairs))), args.steps, args.warmup)
        out.update(fused_pairs_per_s=round(args.pairs / dtf, 2), fused_ms_per_step=round(dtf * 1e3, 3))
    import semantic_superpoint_amd as ssp
    out["library"] = ssp.lib.build_id()[:16]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
