#!/usr/bin/env python3
"""bench_descriptor_metrics.py - the streamed descriptor metrics on one MI355X: ONE JSON line.

SuperPointNet_gauss2_ssmall with random-init weights at 240x320, B = 32 pairs, detection threshold 0.0155 (random-init
logits: softmax ~ 1/65), as bench_descriptor.py.
  val_step_ms_on / val_step_ms_off   a validation `train_val_sample` of the trainer (`ssp_device_pairs`) with
                                     `ssp_descriptor_metrics` on and off; the "on" figure includes the round's one
                                     result() read every validation_size + 2 steps, as train() makes it.  The two
                                     trainers alternate in blocks of one round, so both see the same clock.
  streaming_pairs_per_s              StreamingEvaluator.update_views on the points and descriptors of one eval
                                     forward per view, one result() per 8 steps
  run_points_pairs_per_s             Evaluator.run_points per batch on the same tensors (interleaved once, outside the
                                     timed window): the per-batch host read this work removes
Host clock around work that ends in a device synchronise.  `--repeats` windows each; median, min and max are printed.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
ARCH = "SuperPointNet_gauss2_ssmall"


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=16, help="steps per timed window (a multiple of 8 and of the round)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--height", type=int, default=240)
    ap.add_argument("--width", type=int, default=320)
    ap.add_argument("--thresh", type=float, default=0.0155)
    ap.add_argument("--validation-size", type=int, default=3)
    return ap.parse_args(argv)


def trainer_config(B, thresh, validation_size, on):
    cfg = {"data": {"semantic": True, "gaussian_label": {"enable": True},
                    "warped_pair": {"enable": True, "valid_border_margin": 3,
                                    "params": dict(translation=True, rotation=True, scaling=True, perspective=True,
                                                   scaling_amplitude=0.2, perspective_amplitude_x=0.2,
                                                   perspective_amplitude_y=0.2, patch_ratio=0.85, max_angle=1.57,
                                                   allow_artifacts=True)}},
           "model": {"name": ARCH, "params": {}, "batch_size": B, "real_batch_size": B, "learning_rate": 1e-3,
                     "lambda_loss": 1, "multi_task_loss": True, "dense_loss": {"enable": False},
                     "detector_loss": {"loss_type": "softmax"}, "detection_threshold": thresh, "nms": 4,
                     "subpixel": {"enable": True},
                     "sparse_loss": {"enable": True, "params": {"num_matching_attempts": 1000,
                                                                "num_masked_non_matches_per_match": 100, "lamda_d": 1}}},
           "validation_interval": 1000, "validation_size": validation_size, "tensorboard_interval": 1000, "retrain": True,
           "reset_iter": True, "ssp_seed": 0, "ssp_device_pairs": True}
    if on:
        cfg["ssp_descriptor_metrics"] = True
    return cfg


def jsonable(v):
    """numpy scalars / arrays as plain Python, NaN as null."""
    if hasattr(v, "tolist"):
        v = v.tolist()
    if isinstance(v, (list, tuple)):
        return [jsonable(x) for x in v]
    return None if isinstance(v, float) and v != v else v


def spread(xs, digits=3):
    return {"median": round(statistics.median(xs), digits), "min": round(min(xs), digits), "max": round(max(xs), digits)}


def main(argv=None):
    args = parse_args(argv)
    import numpy as np
    import torch
    from oracle import cpu_ref as C
    import semantic_superpoint_amd as ssp
    from semantic_superpoint_amd import lib as L
    from semantic_superpoint_amd import models
    from semantic_superpoint_amd.Train_model_heatmap_all import Train_model_heatmap_all
    from semantic_superpoint_amd.evaluation import Evaluator, StreamingEvaluator

    if not torch.cuda.is_available():
        raise SystemExit("bench_descriptor_metrics.py measures on the GPU: no HIP device found")
    if args.gpus != 1:
        raise SystemExit("bench_descriptor_metrics.py measures one GPU (--gpus 1)")
    if args.steps < 8 or args.steps % 8:
        raise SystemExit("--steps must be a multiple of 8 (one result() per 8 steps)")
    dev = torch.device("cuda:0")
    B, H, W = args.batch, args.height, args.width
    sd = {k: torch.as_tensor(np.array(v)) for k, v in C.init_state_dict(ARCH, seed=0).items()}
    out = {"bench": "descriptor_metrics", "arch": ARCH, "batch": B, "height": H, "width": W, "conf_thresh": args.thresh,
           "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats, "library": ssp.lib.build_id()[:16]}
    clock0 = L.clock_probe(5.0)

    # ---- the trainer's validation step, key on / off ----
    round_steps = args.validation_size + 2
    g = torch.Generator().manual_seed(0)
    samples = [{"image": torch.rand(B, 1, H, W, generator=g), "labels_2D": (torch.rand(B, 1, H, W, generator=g) < 0.01).float(),
                "semantic": torch.randint(0, 134, (B, H, W), generator=g)} for _ in range(2)]
    agents = {}
    for name, on in (("on", True), ("off", False)):
        a = Train_model_heatmap_all(trainer_config(B, args.thresh, args.validation_size, on), save_path=tempfile.gettempdir(), device="cuda:0")
        a.loadModel()
        a.net.load_state_dict(sd)
        a.dataParallel()
        agents[name] = a

    def val_round(name, it0):
        a = agents[name]
        if a.descriptor_metrics:
            a.reset_descriptor_eval()
        for j in range(round_steps):
            a.train_val_sample(samples[(it0 + j) % 2], n_iter=it0 + j, train=False)
        return a.descriptor_round_scalars() if a.descriptor_metrics else None

    for name in agents:
        for _ in range(max(1, args.warmup // round_steps)):
            scalars = val_round(name, 0)
        if scalars:
            out["round_scalars"] = {k: jsonable(v) for k, v in scalars.items()}
    rounds = max(1, args.steps // round_steps)
    ms = {"on": [], "off": []}
    for _ in range(args.repeats):
        for name in ("on", "off"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for r in range(rounds):
                val_round(name, r * round_steps)
            torch.cuda.synchronize()
            ms[name].append(1e3 * (time.perf_counter() - t0) / (rounds * round_steps))
    out["val_step_ms_on"], out["val_step_ms_off"] = spread(ms["on"]), spread(ms["off"])
    out["val_step_ms_added"] = round(out["val_step_ms_on"]["median"] - out["val_step_ms_off"]["median"], 3)
    del agents
    torch.cuda.empty_cache()

    # ---- StreamingEvaluator.update_views against Evaluator.run_points on the same tensors ----
    net = getattr(models, ARCH)()
    net.load_state_dict(sd)
    net = net.to(dev).eval()
    eng = net.engine(B, H, W, dev)
    rs = np.random.RandomState(0)
    a = torch.from_numpy(rs.uniform(0, 1, (B, 1, H, W)).astype(np.float32)).to(dev)
    b = torch.roll(a, (2, 3), (2, 3)).contiguous()
    with torch.no_grad():
        eng.forward(a, slot=0, train=False, want=())
        eng.forward(b, slot=1, train=False, want=())
    kw = dict(conf_thresh=args.thresh, nms_dist=4, subpixel=True, border_remove=4)
    d0, d1 = eng.describe_points(0, B, **kw), eng.describe_points(1, B, **kw)
    hn = torch.tensor([[1.0, 0.0, 2 * 3 / W], [0.0, 1.0, 2 * 2 / H], [0.0, 0.0, 1.0]], device=dev).repeat(B, 1, 1)
    out["mean_points_per_image"] = round(float(torch.cat([d0["count"], d1["count"]]).float().mean()), 1)
    ev = StreamingEvaluator(H, W, dev, 8 * B, corner_shape=(H, W))

    def streaming_window():
        for s in range(args.steps):
            ev.update_views(d0, d1, hn, subpixel=True)
            if s % 8 == 7:
                res = ev.result()
                ev.reset()
        return res

    p0, p1 = ev._points64(d0["pts"], True), ev._points64(d1["pts"], True)
    pts = torch.stack([p0, p1], 1).reshape(2 * B, p0.shape[1], 3).contiguous()
    cnt = torch.stack([d0["count"], d1["count"]], 1).reshape(2 * B).contiguous()
    desc = torch.stack([d0["desc"], d1["desc"]], 1).reshape(2 * B, p0.shape[1], 256).contiguous()
    Hpx = np.stack([np.array([[1.0, 0, 3], [0, 1.0, 2], [0, 0, 1]])] * B)
    old = Evaluator(H, W)

    def run_points_window():
        for s in range(args.steps):
            res = old.run_points(pts, cnt, desc, Hpx, list(range(B)))
        return res

    rate = {"streaming": [], "run_points": []}
    windows = (("streaming", streaming_window), ("run_points", run_points_window))
    for name, fn in windows:
        fn()  # warm-up
    for _ in range(args.repeats):
        for name, fn in windows:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = fn()
            torch.cuda.synchronize()
            rate[name].append(args.steps * B / (time.perf_counter() - t0))
            if name == "streaming":
                out["streaming_summary"] = {k: jsonable(v) for k, v in res.items() if k != "rows"}
    out["streaming_pairs_per_s"], out["run_points_pairs_per_s"] = spread(rate["streaming"], 1), spread(rate["run_points"], 1)
    out["streaming_over_run_points"] = round(out["streaming_pairs_per_s"]["median"] / out["run_points_pairs_per_s"]["median"], 3)
    clock1 = L.clock_probe(5.0)
    out["gpu_clock_mhz"] = None if clock0 is None else {"before": round(clock0, 1), "after": round(clock1, 1)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
