#!/usr/bin/env python3
"""bench_descriptor.py - pairs/s of the fused descriptor export (export.py:66-190 export_descriptor without the file I/O) on
one MI355X.

A step = P pairs (image, warped image) resident on the device: ONE eval-mode forward over the 2P images, keypoints
(flattenDetection, threshold, greedy NMS, border removal, sort, 5x5 soft-argmax), sparse descriptors and the two-way
nearest-neighbour matcher (DescriptorExporter.run_device), closed by one host read of the point and match counts.
Timed with a device synchronisation around the steps.

`python bench_descriptor.py [--steps K] [--warmup W] [--pairs 16] [--height 240 --width 320]` prints ONE JSON line.
The forward / post-processing split of the kernel time comes from a separate profiled run (tools/prof_descriptor.sh).
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
    ap.add_argument("--gpus", type=int, default=1, help="one GPU (the export shards pairs over ranks without a collective)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=16)
    ap.add_argument("--arch", default="ssp", choices=["sp", "ssp"])
    ap.add_argument("--height", type=int, default=240)
    ap.add_argument("--width", type=int, default=320)
    ap.add_argument("--thresh", type=float, default=0.0155)  # random-init logits: softmax ~ 1/65 = 0.01538
    ap.add_argument("--nn-thresh", type=float, default=0.7)
    return ap.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    import numpy as np
    import torch
    from oracle import cpu_ref as C
    from semantic_superpoint_amd import models
    from semantic_superpoint_amd.export import DescriptorExporter

    assert torch.cuda.is_available(), "bench_descriptor.py needs an MI355X"
    if args.gpus != 1:
        raise SystemExit("bench_descriptor.py measures one GPU (--gpus 1)")
    dev = torch.device("cuda:0")
    arch = {"sp": "SuperPointNet_gauss2", "ssp": "SuperPointNet_gauss2_ssmall"}[args.arch]
    net = getattr(models, arch)()
    net.load_state_dict({k: torch.as_tensor(np.array(v)) for k, v in C.init_state_dict(arch, seed=0).items()})
    net = net.to(dev).eval()
    ex = DescriptorExporter(net, dev, conf_thresh=args.thresh, nms_dist=4, subpixel=True, nn_thresh=args.nn_thresh)
    rs = np.random.RandomState(0)
    H, W = args.height, args.width
    pairs = []
    for _ in range(args.pairs):
        a = torch.from_numpy(rs.uniform(0, 1, (H, W)).astype(np.float32))
        pairs.append((a.to(dev), torch.roll(a, (2, 3), (0, 1)).to(dev)))

    def step():
        o = ex.run_device(pairs)
        return o["count"].cpu(), o["n_match"].cpu()  # the one host read of a flush

    for _ in range(args.warmup):
        counts, n_match = step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        counts, n_match = step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / args.steps
    import semantic_superpoint_amd as ssp
    print(json.dumps({
        "metric": "descriptor_export_pairs_per_s", "value": round(args.pairs / dt, 2), "unit": "pairs/s",
        "ms_per_step": round(dt * 1e3, 3), "pairs_per_step": args.pairs, "arch": arch, "height": H, "width": W,
        "conf_thresh": args.thresh, "nn_thresh": args.nn_thresh, "steps": args.steps, "warmup": args.warmup,
        "mean_points_per_image": round(float(counts.float().mean()), 1), "mean_matches_per_pair": round(float(n_match.float().mean()), 1),
        "library": ssp.lib.build_id()[:16]}))


if __name__ == "__main__":
    main()
