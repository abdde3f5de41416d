#!/usr/bin/env python3
"""bench_trainer.py - the pair step THROUGH the trainer plugin, fed from the host (stand-alone; bench.py stays the headline).

One JSON line for SSp (SuperPointNet_gauss2_ssmall), 240x320, batch 32, fp32, non-logging training steps, three lines of
the same box and process:
  engine          Engine.pair_step + adam_step on resident inputs (bench.py's method), for reference
  trainer_host    Train_model_heatmap_all.train_val_sample fed PINNED host dicts with the reference loader's full key set:
                  the whole pair crosses PCIe every step (the path without `ssp_device_pairs`)
  trainer_device  `ssp_device_pairs: true`, fed pinned uint8 image, float labels_2D and uint8 semantic; reported with the
                  photometric step on (the shipped COCO augmentation block) and off
plus host-to-device bytes per step of both trainer modes (summed over the tensors each mode copies) and the device time
per step of pair generation alone and of the photometric step alone (HIP events around make_pairs / draw + apply of both views).
Each line carries the shader-clock probe before / after its timed window.  Every window is warmed up, ends in a device
synchronise and is repeated `--repeats` times (median and spread reported); the modes alternate inside one process.

`--mode host` runs on a revision without the device feed too (trainer_device: null), so that the parent's number comes from
the same script on the same box.  `python bench_trainer.py [--mode all|host|device|engine] [--steps K] [--warmup W] [--repeats R]`."""
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
AUG = {"photometric": {"enable": True, "params": {
    "random_brightness": {"max_abs_change": 50}, "random_contrast": {"strength_range": [0.5, 1.5]},
    "additive_gaussian_noise": {"stddev_range": [0, 10]}, "additive_speckle_noise": {"prob_range": [0, 0.0035]},
    "additive_shade": {"transparency_range": [-0.5, 0.5], "kernel_size_range": [100, 150]},
    "motion_blur": {"max_kernel_size": 3}}}, "homographic": {"enable": False}}
WARP = dict(translation=True, rotation=True, scaling=True, perspective=True, scaling_amplitude=0.2, perspective_amplitude_x=0.2,
            perspective_amplitude_y=0.2, patch_ratio=0.85, max_angle=1.57, allow_artifacts=True)


def config(B, device_pairs=False, photometric=False):
    cfg = {"data": {"semantic": True, "gaussian_label": {"enable": True},
                    "warped_pair": {"enable": True, "params": dict(WARP), "valid_border_margin": 3},
                    "augmentation": {"photometric": dict(AUG["photometric"], enable=bool(photometric)), "homographic": {"enable": False}}},
           "model": {"name": ARCH, "params": {}, "batch_size": B, "real_batch_size": B, "learning_rate": 1e-4, "lambda_loss": 1,
                     "multi_task_loss": True, "dense_loss": {"enable": False}, "detector_loss": {"loss_type": "softmax"},
                     "sparse_loss": {"enable": True, "params": {"num_matching_attempts": 1000,
                                                                "num_masked_non_matches_per_match": 100, "lamda_d": 1}}},
           "validation_interval": 10 ** 9, "tensorboard_interval": 10 ** 9, "retrain": True, "reset_iter": True}
    if device_pairs:
        cfg["ssp_device_pairs"] = True
    return cfg


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="all", choices=["all", "host", "device", "engine"])
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--height", type=int, default=240)
    ap.add_argument("--width", type=int, default=320)
    args = ap.parse_args(argv)
    import torch
    import semantic_superpoint_amd as ssp
    from semantic_superpoint_amd import lib as L
    from semantic_superpoint_amd import synth
    from semantic_superpoint_amd.Train_model_heatmap_all import Train_model_heatmap_all as T
    if not torch.cuda.is_available():
        raise SystemExit("bench_trainer.py measures on the GPU: no HIP device found")
    dev = torch.device("cuda:0")
    B, H, W = args.batch, args.height, args.width
    tmp = tempfile.mkdtemp()
    have_device_feed = hasattr(L, "op_photometric_apply")
    full = synth.make_pair(B, H, W, dev, seed=100, semantic=True)         # the reference loader's key set, built once

    def pin(t):
        return t.cpu().contiguous().pin_memory()

    host_sample = {k: pin(v) for k, v in full.items() if torch.is_tensor(v)}
    dev_sample = {"image": pin((full["image"] * 255).to(torch.uint8)), "labels_2D": pin(full["labels_2D"]),
                  "semantic": pin(full["semantic"].to(torch.uint8))}

    def nbytes(d):
        return int(sum(v.numel() * v.element_size() for v in d.values() if torch.is_tensor(v)))

    def agent(cfg):
        a = T(cfg, save_path=tmp, device="cuda:0")
        a.loadModel()
        a.dataParallel()
        return a

    def clock():
        return L.clock_probe(5.0) if hasattr(L, "clock_probe") else None

    def timed(step):
        """median / min / max ms per step over `repeats` windows of `steps` steps, each closed by a synchronise"""
        for it in range(args.warmup):
            step(1 + it)
        torch.cuda.synchronize()
        c0 = clock()
        torch.cuda.synchronize()
        ms = []
        for r in range(args.repeats):
            t0 = time.perf_counter()
            for it in range(args.steps):
                step(1 + args.warmup + r * args.steps + it)      # n_iter >= 1: never the logging branch
            torch.cuda.synchronize()
            ms.append(1e3 * (time.perf_counter() - t0) / args.steps)
        c1 = clock()
        out = {"ms_per_step": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4),
               "pairs_per_s": round(B / (1e-3 * statistics.median(ms)), 1), "windows": args.repeats, "steps_per_window": args.steps}
        if c0 is not None and c1 is not None:
            out["gpu_clock_mhz"] = {"before": round(c0, 1), "after": round(c1, 1)}
        return out

    out = {"bench": "trainer", "arch": ARCH, "batch": B, "height": H, "width": W, "dtype": "fp32", "mode": args.mode,
           "build_id": L.build_id()[:16] if hasattr(L, "build_id") else None,
           "engine": None, "trainer_host": None, "trainer_device": None}
    if args.mode in ("all", "engine"):
        a = agent(config(B))
        eng = a._engine_for(B, H, W)

        def engine_step(it):
            eng.zero_grad()
            eng.pair_step(full, indices=None, seed=it, train=True, lambda_loss=1.0, lamda_d=1.0, multi_task=True, gaussian=True)
            eng.adam_step(1e-4)
        out["engine"] = timed(engine_step)
    if args.mode in ("all", "host"):
        a = agent(config(B))
        out["trainer_host"] = dict(timed(lambda it: a.train_val_sample(host_sample, n_iter=it, train=True)),
                                   h2d_bytes_per_step=nbytes(host_sample), keys=sorted(host_sample))
    if args.mode in ("all", "device") and have_device_feed:
        from semantic_superpoint_amd import pairs
        res = {"h2d_bytes_per_step": nbytes(dev_sample), "keys": sorted(dev_sample)}
        for name, photo in (("photometric_on", True), ("photometric_off", False)):
            a = agent(config(B, device_pairs=True, photometric=photo))
            res[name] = timed(lambda it: a.train_val_sample(dev_sample, n_iter=it, train=True))
        # device time of the two new stages alone (HIP events; resident inputs)
        img = dev_sample["image"].to(dev)
        lab, sem = dev_sample["labels_2D"].to(dev), dev_sample["semantic"].to(dev)
        raw = img.float() / 255.0
        pp = L.photometric_params_from_config(AUG)

        def events(fn, n=20):
            for _ in range(3):
                fn(0)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(n):
                fn(i)
            e1.record()
            torch.cuda.synchronize()
            return round(e0.elapsed_time(e1) / n, 4)

        raw2 = torch.cat((raw, raw))

        def photo(i):  # as make_pairs runs it: two draw tables, both views in one apply
            L.op_photometric_apply(raw2, torch.cat([L.op_photometric_draw(B, H, W, 2 * i + v, pp, dev) for v in (0, 1)]))
        draws = L.op_photometric_draw(B, H, W, 1, pp, dev)
        noshade = torch.cat((draws, draws))
        noshade[:, L.PHOTO_KSIZE] = 0
        res["pair_generation_ms_per_step"] = events(lambda i: pairs.make_pairs(img, lab, seed=i, warp_params=WARP, erosion_radius=3, semantic=sem))
        res["photometric_ms_per_step"] = events(photo)
        res["photometric_without_shade_ms_per_step"] = events(lambda i: L.op_photometric_apply(raw2, noshade))
        out["trainer_device"] = res
    if out["engine"] and out["trainer_device"]:
        out["device_fed_fraction_of_engine"] = {k: round(out["engine"]["ms_per_step"] / out["trainer_device"][k]["ms_per_step"], 4)
                                                for k in ("photometric_on", "photometric_off")}
    if out["engine"] and out["trainer_host"]:
        out["host_fed_fraction_of_engine"] = round(out["engine"]["ms_per_step"] / out["trainer_host"]["ms_per_step"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
