"""Segmentation read-out benchmark: one JSON line at B = 32, 240x320, 133 classes.

  sem_predict_pred_us        Engine.sem_predict, class map only
  sem_predict_pred_conf_us   Engine.sem_predict, class map + confusion matrix (labels constant on 16x16 blocks, like a segmentation map)
  sem_predict_conf_random_us the same with uniformly random labels (the worst case of the key merge)
  torch_composition_us       what a user had to write before: the [B,133,H,W] fp32 logits of Engine.forward(want=(..., "sem")) - the
                             upsample kernel's share of that call, taken as the difference to the same forward without "sem" - plus
                             argmax(1) plus bincount(label * C + pred) in torch, on the same device in the same run
  sem_ce_forward_us          the fused upsample + cross-entropy loss forward (ssp_op_sem_loss without gradient), for scale

Times are device times between two HIP events around `--steps` back-to-back calls, median over `--repeats` windows after `--warmup`
calls.  There is no CPU baseline: the read-out runs on the device only."""
import argparse
import ctypes
import json
import statistics

ARCH = "SuperPointNet_gauss2_ssmall"


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--height", type=int, default=240)
    ap.add_argument("--width", type=int, default=320)
    args = ap.parse_args(argv)
    import torch
    from semantic_superpoint_amd import lib as L
    if not torch.cuda.is_available():
        raise SystemExit("bench_semantic.py measures on the GPU: no HIP device found")
    dev, B, H, W, NC = torch.device("cuda:0"), args.batch, args.height, args.width, 133

    def timed(fn, steps=args.steps):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        us = []
        for _ in range(args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(steps):
                fn()
            b.record()
            torch.cuda.synchronize()
            us.append(1e3 * a.elapsed_time(b) / steps)
        return {"us": round(statistics.median(us), 2), "min": round(min(us), 2), "max": round(max(us), 2)}

    eng = L.Engine(ARCH, B, H, W, dev, with_grad=False)
    g = torch.Generator().manual_seed(0)
    from oracle import cpu_ref as C
    eng.load_state_dict(C.init_state_dict(ARCH, seed=1))   # untrained weights: the class map is lively, which is the harder case
    x = torch.rand(B, 1, H, W, generator=g).to(dev)
    coarse = torch.randint(0, NC + 1, (B, H // 16, W // 16), generator=g)
    lab_blocks = coarse.repeat_interleave(16, 1).repeat_interleave(16, 2).contiguous().to(dev)
    lab_random = torch.randint(0, NC + 1, (B, H, W), generator=g).to(dev)
    clock0 = L.clock_probe(5.0)
    out = eng.forward(x, train=True, want=("semi", "desc", "sem"))
    sem = out["sem"]
    conf = torch.zeros(NC, NC, dtype=torch.int64, device=dev)
    pred, _ = eng.sem_predict(0, B, H, W, labels=lab_blocks, confusion=conf)
    # same result as the torch composition (ties and last-bit differences aside: counted, not asserted)
    pred_t = sem.argmax(1)
    agree = float((pred_t == pred.long()).double().mean())
    ok = lab_blocks < NC
    conf_t = torch.bincount(lab_blocks[ok] * NC + pred.long()[ok], minlength=NC * NC).view(NC, NC)
    assert torch.equal(conf, conf_t), "confusion matrix differs from bincount"
    res = {"bench": "semantic", "arch": ARCH, "batch": B, "height": H, "width": W, "n_classes": NC, "build_id": L.build_id()[:16],
           "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats, "argmax_agreement": round(agree, 6),
           "classes_predicted": int(torch.unique(pred).numel()), "cpu_baseline": None}
    res["sem_predict_pred_us"] = timed(lambda: eng.sem_predict(0, B, H, W))
    res["sem_predict_pred_conf_us"] = timed(lambda: eng.sem_predict(0, B, H, W, labels=lab_blocks, confusion=conf))
    res["sem_predict_conf_only_us"] = timed(lambda: eng.sem_predict(0, B, H, W, labels=lab_blocks, want_pred=False, confusion=conf))
    res["sem_predict_conf_random_us"] = timed(lambda: eng.sem_predict(0, B, H, W, labels=lab_random, confusion=conf))
    del sem, out, pred_t
    few = max(3, args.steps // 10)
    f_with = timed(lambda: eng.forward(x, train=True, want=("semi", "desc", "sem")), few)
    f_without = timed(lambda: eng.forward(x, train=True, want=("semi", "desc")), few)
    sem = eng.forward(x, train=True, want=("semi", "desc", "sem"))["sem"]
    t_argmax = timed(lambda: sem.argmax(1), few)
    pl = pred.long()
    t_bincount = timed(lambda: torch.bincount(lab_blocks[ok] * NC + pl[ok], minlength=NC * NC), few)
    up = round(f_with["us"] - f_without["us"], 2)
    res["torch_composition_us"] = {"us": round(up + t_argmax["us"] + t_bincount["us"], 2), "engine_upsample_us": up,
                                   "forward_with_sem": f_with, "forward_without_sem": f_without, "argmax": t_argmax,
                                   "bincount": t_bincount, "logits_bytes": sem.numel() * 4}
    del sem
    # the loss forward on the same logits (NHWC, channel stride 136), for scale
    cs = (NC + 3) // 4 * 4
    y = eng.debug_buffer(0, "Y13", (B, (H // 8) * (W // 8), cs))
    scratch = torch.empty(65536, dtype=torch.uint8, device=dev)
    loss = torch.zeros(1, device=dev)
    raw = L.load_library()

    def ce():
        L._check(raw.ssp_op_sem_loss(L._ptr(y), cs, L._ptr(lab_blocks), B, H, W, NC, 0, L._ptr(scratch), scratch.numel(), L._ptr(loss),
                                     None, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    res["sem_ce_forward_us"] = timed(ce)
    clock1 = L.clock_probe(5.0)
    res["gpu_clock_mhz"] = None if clock0 is None else {"before": round(clock0, 1), "after": round(clock1, 1)}
    res["faster_than_torch"] = bool(res["sem_predict_pred_us"]["us"] < res["torch_composition_us"]["us"]
                                    and res["sem_predict_pred_conf_us"]["us"] < res["torch_composition_us"]["us"])
    res["conf_over_pred"] = round(res["sem_predict_pred_conf_us"]["us"] / res["sem_predict_pred_us"]["us"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
