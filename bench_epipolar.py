"""Epipolar-check benchmark: one JSON line.

  epi_ransac_us      ssp_epi_ransac per call for `--pairs` (1 and 16) pairs of about 500 and 1200 matches (70 % inliers, 0.3 px of
                     noise), for every `--groups` value (0 = the library's default) - the 2000 hypotheses of a pair split over
                     that many workgroups - and eval_ransac_us, the yardstick: ssp_eval_ransac (the homography RANSAC, one
                     workgroup per pair) on the same matches and pairs
  sequence_step_us   SequenceTracker.step per frame at `--height` x `--width` on a shifted noise image with the check off (the
                     path without any of this), "homography" and "fundamental"

Device times are between two HIP events around `--steps` back-to-back calls, median over `--repeats` windows after `--warmup`
calls; the variants of one shape are measured in turn inside one run.  The clock probe before and after reports the clock the
device grants."""
import argparse
import json
import statistics

ARCH = "SuperPointNet_gauss2_ssmall"


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--pairs", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--matches", type=int, nargs="+", default=[500, 1200])
    ap.add_argument("--groups", type=int, nargs="+", default=[1, 2, 4, 8, 16, 32, 0])
    ap.add_argument("--height", type=int, default=240)
    ap.add_argument("--width", type=int, default=320)
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    from oracle import cpu_ref as C
    from semantic_superpoint_amd import lib as L
    from semantic_superpoint_amd import models
    from semantic_superpoint_amd.export import SequenceTracker
    from tests import epipolar_ref as E
    if not torch.cuda.is_available():
        raise SystemExit("bench_epipolar.py measures on the GPU: no HIP device found")
    dev = torch.device("cuda:0")

    def window(fn):
        """median device microseconds per call of fn(k)"""
        k = 0
        for _ in range(args.warmup):
            fn(k)
            k += 1
        torch.cuda.synchronize()
        us = []
        for _ in range(args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.steps):
                fn(k)
                k += 1
            b.record()
            torch.cuda.synchronize()
            us.append(1e3 * a.elapsed_time(b) / args.steps)
        return {"us": round(statistics.median(us), 2), "min": round(min(us), 2), "max": round(max(us), 2)}

    res = {"bench": "epipolar", "build_id": L.build_id()[:16], "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats}
    clock0 = L.clock_probe(5.0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    ops = []
    for n in args.matches:
        cap = (n + 63) // 64 * 64
        for P in args.pairs:
            rng = np.random.RandomState(n + P)
            pts1, pts2 = np.zeros((P, cap, 3)), np.zeros((P, cap, 3))
            match = np.zeros((P, cap, 3), dtype=np.float32)
            for p in range(P):
                sc = E.make_scene(1000 * n + p, int(0.7 * n), n - int(0.7 * n), noise=0.3)
                pts1[p], pts2[p], match[p] = E.as_arrays(sc["m"], cap, 3, rng)
            a1, a2, m = t(pts1), t(pts2), t(match)
            nm = torch.full((P,), n, dtype=torch.int32, device=dev)
            seeds = torch.arange(P, dtype=torch.int64, device=dev) + 77
            row = {"pairs": P, "matches": n, "cap": cap, "epi_ransac_us": {}}
            row["eval_ransac_us"] = window(lambda k: L.op_eval_ransac(a1, a2, m, nm, seeds))
            for g in args.groups:
                row["epi_ransac_us"]["default" if g == 0 else str(g)] = window(
                    lambda k: L.op_epipolar_ransac(a1, a2, m, nm, seeds, groups=g))
            o = L.op_epipolar_ransac(a1, a2, m, nm, seeds)
            row["inliers_mean"] = round(float(o["n_inliers"].double().mean()), 1)
            row["err_px_mean"] = round(float(o["err"].mean()), 4)
            timed = {k: v["us"] for k, v in row["epi_ransac_us"].items() if k != "default"}
            row["fastest_groups"] = int(min(timed, key=timed.get))
            row["eval_over_epi_default"] = round(row["eval_ransac_us"]["us"] / row["epi_ransac_us"]["default"]["us"], 2) \
                if "default" in row["epi_ransac_us"] else None
            ops.append(row)
    res["operator"] = ops

    H, W = args.height, args.width
    net = getattr(models, ARCH)()
    net.load_state_dict({k: torch.as_tensor(np.array(v)) for k, v in C.init_state_dict(ARCH, seed=21).items()})
    net = net.to(dev).eval()
    big = torch.from_numpy(np.random.RandomState(5).uniform(0, 1, (H, W + 16)).astype(np.float32)).to(dev)
    ims = [big[:, 2 * k:2 * k + W].contiguous() for k in range(8)]
    step = {"height": H, "width": W}
    for mode in (None, "homography", "fundamental"):
        seq = SequenceTracker(net, dev, conf_thresh=0.0155, nms_dist=4, subpixel=True, nn_thresh=0.7, max_length=5,
                              geometric_check=mode)
        step["off" if mode is None else mode] = window(lambda k: seq.step(ims[k % len(ims)]))
        g = seq.tracker.last_geometry()
        if g is not None:
            step["%s_inliers" % mode] = int(g["n_inliers"][0])
            step["%s_status" % mode] = int(g["status"][0])
        step["matches_%s" % ("off" if mode is None else mode)] = int(seq.tracker.get_matches().shape[1])
    res["sequence_step_us"] = step
    clock1 = L.clock_probe(5.0)
    res["gpu_clock_mhz"] = None if clock0 is None else {"before": round(clock0, 1), "after": round(clock1, 1)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
