"""Synthetic Shapes feed benchmark: one JSON line.

  --mode all       generation at the shipped config (960x1280 -> 120x160, B = 64): images/s mixed and per primitive, the device
                   time of draw / render / feed (HIP events), and the SuperPointNet_gauss2 single-view step through
                   Train_model_heatmap_all.train_val_sample fed (a) by SyntheticShapes and (b) by one resident batch
  --mode resident  (b) alone: needs nothing of the shapes feed, so it runs on older revisions too

The augmentation block is the shipped yaml's; its motion_blur.max_kernel_size of 7 means no motion blur and a doubled impulse
noise in the reference, which the feed applies once.  There is no CPU baseline: the reference generator (tensorflow + cv2) cannot be imported where this project is built."""
import argparse
import json
import statistics
import tempfile
import time

ARCH = "SuperPointNet_gauss2"
AUG = {"photometric": {"enable": True, "enable_train": True, "enable_val": False,
                       "params": {"random_brightness": {"max_abs_change": 75}, "random_contrast": {"strength_range": [0.3, 1.8]},
                                  "additive_gaussian_noise": {"stddev_range": [0, 15]}, "additive_speckle_noise": {"prob_range": [0, 0.0035]},
                                  "additive_shade": {"transparency_range": [-0.5, 0.8], "kernel_size_range": [50, 100]},
                                  "motion_blur": {"max_kernel_size": 7}}},
       "homographic": {"enable": True, "enable_train": True, "enable_val": False, "valid_border_margin": 2,
                       "params": {"translation": True, "rotation": True, "scaling": True, "perspective": True, "scaling_amplitude": 0.2,
                                  "perspective_amplitude_x": 0.2, "perspective_amplitude_y": 0.2, "patch_ratio": 0.8, "max_angle": 1.57,
                                  "allow_artifacts": True, "translation_overflow": 0.05}}}


def config(B):
    return {"data": {"primitives": "all", "truncate": {"draw_ellipses": 0.3, "draw_stripes": 0.2, "gaussian_noise": 0.1},
                     "gaussian_label": {"enable": True}, "preprocessing": {"blur_size": 21, "resize": [120, 160]}, "augmentation": AUG,
                     "warped_pair": {"enable": False}},
            "model": {"name": ARCH, "params": {}, "batch_size": B, "eval_batch_size": B, "real_batch_size": B, "multi_task_loss": False, "learning_rate": 1e-3, "lambda_loss": 0,
                      "detector_loss": {"loss_type": "softmax"}, "dense_loss": {"enable": False},
                      "sparse_loss": {"enable": True, "params": {"num_matching_attempts": 1000, "num_masked_non_matches_per_match": 100, "lamda_d": 1}}},
            "validation_interval": 10 ** 9, "tensorboard_interval": 10 ** 9, "retrain": True, "reset_iter": True}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="all", choices=["all", "resident"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64)
    args = ap.parse_args(argv)
    import torch
    from semantic_superpoint_amd import lib as L
    from semantic_superpoint_amd.Train_model_heatmap_all import Train_model_heatmap_all as T
    if not torch.cuda.is_available():
        raise SystemExit("bench_shapes.py measures on the GPU: no HIP device found")
    dev, B, H, W = torch.device("cuda:0"), args.batch, 120, 160
    cfg = config(B)

    def clock():
        return L.clock_probe(5.0) if hasattr(L, "clock_probe") else None

    def timed(fn):
        for it in range(args.warmup):
            fn(it)
        torch.cuda.synchronize()
        c0 = clock()
        torch.cuda.synchronize()
        ms = []
        for r in range(args.repeats):
            t0 = time.perf_counter()
            for it in range(args.steps):
                fn(args.warmup + r * args.steps + it)
            torch.cuda.synchronize()
            ms.append(1e3 * (time.perf_counter() - t0) / args.steps)
        c1 = clock()
        return {"ms": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4), "images_per_s": round(B / (1e-3 * statistics.median(ms)), 1),
                "gpu_clock_mhz": None if c0 is None else {"before": round(c0, 1), "after": round(c1, 1)}}

    def events(fn, n=10):
        for i in range(3):
            fn(i)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
        for i, (a, b) in enumerate(ev):
            a.record()
            fn(3 + i)
            b.record()
        torch.cuda.synchronize()
        t = [a.elapsed_time(b) for a, b in ev]
        return {"ms": round(statistics.median(t), 4), "min": round(min(t), 4), "max": round(max(t), 4)}

    agent = T(cfg, save_path=tempfile.mkdtemp(), device="cuda:0")
    agent.loadModel()
    agent.dataParallel()
    out = {"bench": "shapes", "arch": ARCH, "batch": B, "gen": [960, 1280], "out": [H, W], "mode": args.mode,
           "build_id": L.build_id()[:16] if hasattr(L, "build_id") else None, "cpu_baseline": None}
    g = torch.Generator().manual_seed(0)
    lab = (torch.rand(B, 1, H, W, generator=g) < 0.002).float().to(dev)
    resident = {"image": torch.rand(B, 1, H, W, generator=g).to(dev), "labels_2D": lab, "valid_mask": torch.ones(B, 1, H, W, device=dev),
                "labels_2D_gaussian": lab.clone()}
    out["step_resident"] = timed(lambda it: agent.train_val_sample(resident, n_iter=1 + it, train=True))
    if args.mode == "all":
        from semantic_superpoint_amd import pairs, shapes
        loader = shapes.SyntheticShapes(cfg, "train", device=dev, seed=0, length=10 ** 9)
        p = loader.params
        out["step_fed"] = timed(lambda it: agent.train_val_sample(loader.batch(it), n_iter=1 + it, train=True))
        out["generate_mixed"] = timed(lambda it: shapes.generate(B, it, params=p, device=dev))
        out["per_primitive"] = {}
        for name in L.SHAPES_PRIMITIVES:
            q = L.shapes_params_from_config(dict(cfg["data"], primitives=[name]))
            out["per_primitive"][name] = timed(lambda it: shapes.generate(B, it, params=q, device=dev))["images_per_s"]
        tab = L.op_shapes_draw(B, 1, p, dev)
        img, pts, cnt = L.op_shapes_render(tab, p)
        out["device_ms"] = {"draw": events(lambda i: L.op_shapes_draw(B, i, p, dev)), "render": events(lambda i: L.op_shapes_render(tab, p)),
                            "feed": events(lambda i: pairs.make_single_view(img, pts, cnt, i, homographic=loader.homographic,
                                                                            photometric_draws=L.op_photometric_draw(B, H, W, i, loader.photo_params, dev)))}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
