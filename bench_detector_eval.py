"""Detector-evaluation benchmark: one JSON line, for 120x160 and 240x320.

A validation set of `--images` images in batches of `--batch`, as dense heat maps (about 78 % of the pixels above remove_zero,
as a softmax heat map has) and as NMS point lists (`--points` points per image):
  update_dense_us / update_points_us   DetectorEvaluator.update per batch (HIP events around one pass over the set)
  finalize_dense_ms / finalize_points_ms   the first result(): state read, torch.sort of the keys, the curve kernels (wall
                                       clock around a synchronise)
  device_total_ms                      a whole pass, updates + finalisation, dense input
against the two ways a user had before, timed on the first `--baseline-images` images of the same data (per image; the
`*_total_ms` entries scale that to the whole set and say so):
  host_numpy_ms_per_image   copy of the heat map and labels to the host + the numpy restatement of the reference's loop
                            (tests/detector_eval_ref.py)
  torch_ms_per_image        a torch composition on the device (nonzero, cdist, argsort, a per-image loop) + the global curve
`same_mAP`: the three agree on the baseline subset."""
import argparse
import json
import statistics
import time


def torch_composition(torch, prob, lab, remove_zero, thresh):
    """compute_tp_fp + compute_pr + compute_mAP with torch ops on the device, one image at a time."""
    tps, ps, n_gt = [], [], 0
    for b in range(prob.shape[0]):
        pred = torch.nonzero(prob[b] > remove_zero)
        p = prob[b][pred[:, 0], pred[:, 1]]
        gt = torch.nonzero(lab[b])
        n_gt += gt.shape[0]
        order = torch.argsort(p, stable=True).flip(0)
        pred, p = pred[order], p[order]
        tp = torch.zeros(p.shape[0], dtype=torch.bool, device=prob.device)
        if gt.shape[0] and p.shape[0]:
            m = torch.cdist(pred.double(), gt.double()) <= thresh
            hit = m.any(1)
            g = m.int().argmax(1)
            idx = torch.arange(p.shape[0], device=prob.device)
            first = torch.full((gt.shape[0],), p.shape[0], dtype=torch.int64, device=prob.device)
            first = first.scatter_reduce(0, g[hit], idx[hit], "amin")
            tp[first[first < p.shape[0]]] = True
        tps.append(tp.flip(0))   # position order of equal probabilities is restored by the stable global sort below
        ps.append(p.flip(0))
    tp, p = torch.cat(tps), torch.cat(ps)
    order = torch.argsort(p, stable=True).flip(0)
    tp = tp[order]
    tp_cum = torch.cumsum(tp, 0).double()
    n = torch.arange(1, tp.shape[0] + 1, device=prob.device).double()
    recall = tp_cum / n_gt if n_gt else (tp_cum == 0).double()
    z = torch.zeros(1, dtype=torch.float64, device=prob.device)
    recall = torch.cat([z, recall, z + 1])
    precision = torch.cat([z, tp_cum / n, z])
    precision = torch.cummax(precision.flip(0), 0).values.flip(0)
    return float(torch.dot(precision[1:], torch.diff(recall)).item())


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=1000)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--points", type=int, default=300)
    ap.add_argument("--baseline-images", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sizes", default="120x160,240x320")
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    from semantic_superpoint_amd import lib as L
    from semantic_superpoint_amd.detector_evaluation import DetectorEvaluator
    from tests import detector_eval_ref as R
    if not torch.cuda.is_available():
        raise SystemExit("bench_detector_eval.py measures on the GPU: no HIP device found")
    dev = torch.device("cuda:0")
    res = {"bench": "detector_eval", "images": args.images, "batch": args.batch, "points": args.points,
           "baseline_images": args.baseline_images, "repeats": args.repeats, "build_id": L.build_id()[:16], "sizes": {}}
    clock0 = L.clock_probe(5.0)
    for size in args.sizes.split(","):
        H, W = (int(v) for v in size.split("x"))
        gen = torch.Generator(device=dev).manual_seed(H * 1000 + W)
        sizes = [min(args.batch, args.images - i) for i in range(0, args.images, args.batch)]
        probs = [torch.rand(b, H, W, device=dev, generator=gen) ** 6 for b in sizes]
        labs = [(torch.rand(b, H, W, device=dev, generator=gen) < 5e-4).to(torch.uint8) for b in sizes]
        cap = 2 * args.points
        pts = []
        for b in sizes:
            t = torch.zeros(b, cap, 5, device=dev)
            t[:, :, 0] = torch.randint(0, W, (b, cap), device=dev, generator=gen).float()
            t[:, :, 1] = torch.randint(0, H, (b, cap), device=dev, generator=gen).float()
            t[:, :, 2] = torch.rand(b, cap, device=dev, generator=gen) * 0.9 + 0.015
            pts.append((t, torch.full((b,), args.points, dtype=torch.int32, device=dev)))
        out = {"batches": len(sizes)}

        def one_pass(ev, dense):
            ev.reset()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for k in range(len(sizes)):
                if dense:
                    ev.update(prob=probs[k], labels=labs[k])
                else:
                    ev.update(pts=pts[k][0], count=pts[k][1], labels=labs[k])
            b.record()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = ev.result()
            torch.cuda.synchronize()
            return 1e3 * a.elapsed_time(b) / len(sizes), 1e3 * (time.perf_counter() - t0), r

        for name, dense, capacity in (("dense", True, args.images * H * W), ("points", False, args.images * cap)):
            ev = DetectorEvaluator(H, W, dev, capacity)
            one_pass(ev, dense)  # warm-up
            runs = [one_pass(ev, dense) for _ in range(args.repeats)]
            out["update_%s_us" % name] = {"us": round(statistics.median(r[0] for r in runs), 1), "min": round(min(r[0] for r in runs), 1),
                                          "max": round(max(r[0] for r in runs), 1)}
            out["finalize_%s_ms" % name] = {"ms": round(statistics.median(r[1] for r in runs), 3), "min": round(min(r[1] for r in runs), 3),
                                            "max": round(max(r[1] for r in runs), 3)}
            out["records_%s" % name] = int(runs[0][2]["prob"].numel())
            out["mAP_%s" % name] = runs[0][2]["mAP"]
            if dense:
                out["device_total_ms"] = round(out["update_dense_us"]["us"] * len(sizes) / 1e3 + out["finalize_dense_ms"]["ms"], 3)
            del ev
        # baselines on the first images of the same data
        nb = min(args.baseline_images, sizes[0])
        ev = DetectorEvaluator(H, W, dev, nb * H * W)
        ev.update(prob=probs[0][:nb].contiguous(), labels=labs[0][:nb].contiguous())
        m_dev = ev.result()["mAP"]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pm, kp = probs[0][:nb].cpu().numpy(), labs[0][:nb].cpu().numpy()
        host = R.evaluate([(pm[i], kp[i]) for i in range(nb)])
        out["host_numpy_ms_per_image"] = round(1e3 * (time.perf_counter() - t0) / nb, 3)
        torch_composition(torch, probs[0][:2], labs[0][:2], 1e-4, 2.0)  # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m_torch = torch_composition(torch, probs[0][:nb], labs[0][:nb], 1e-4, 2.0)
        torch.cuda.synchronize()
        out["torch_ms_per_image"] = round(1e3 * (time.perf_counter() - t0) / nb, 3)
        n = len(host["prob"])
        out["same_mAP"] = bool(abs(host["mAP"] - m_dev) <= n * 2.0 ** -52 and abs(m_torch - m_dev) <= n * 2.0 ** -52)
        out["host_numpy_total_ms_scaled"] = round(out["host_numpy_ms_per_image"] * args.images, 1)
        out["torch_total_ms_scaled"] = round(out["torch_ms_per_image"] * args.images, 1)
        out["host_over_device"] = round(out["host_numpy_total_ms_scaled"] / out["device_total_ms"], 1)
        out["torch_over_device"] = round(out["torch_total_ms_scaled"] / out["device_total_ms"], 1)
        res["sizes"][size] = out
        del probs, labs, pts, ev
        torch.cuda.empty_cache()
    clock1 = L.clock_probe(5.0)
    res["gpu_clock_mhz"] = None if clock0 is None else {"before": round(clock0, 1), "after": round(clock1, 1)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
