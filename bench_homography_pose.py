"""Homography pose benchmark: one JSON line.

  homography_pose_us   ssp_pose_from_homography per call for `--pairs` (1 and 16) pairs of `--matches` (500 and 1131) matches of
                       a planar scene (70 % on the plane, 0.3 px of noise), fed the scene's homography and the true rows as the mask,
                       without and with a prior
  model_select_us      ssp_model_select per call on the same pairs, with the scene's fundamental matrix beside the homography
  sequence_step_us     SequenceTracker.step per frame at `--height` x `--width` on a shifted noise image with intrinsics, under
                       geometric_check="fundamental" and under "auto" (a second RANSAC and the two calls above per frame)

Device times are between two HIP events around `--steps` back-to-back calls, median over `--repeats` windows after `--warmup`
calls; the variants of one shape are measured in turn inside one run.  The clock probe before and after reports the clock the
device grants.  Nothing about speed is asserted."""
import argparse
import json
import statistics


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--pairs", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--matches", type=int, nargs="+", default=[500, 1131])
    ap.add_argument("--height", type=int, default=240)
    ap.add_argument("--width", type=int, default=320)
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    from oracle import cpu_ref as C
    from semantic_superpoint_amd import lib as L
    from semantic_superpoint_amd import models
    from semantic_superpoint_amd.export import SequenceTracker
    from tests import pose_h_ref as H
    if not torch.cuda.is_available():
        raise SystemExit("bench_homography_pose.py measures on the GPU: no HIP device found")
    dev = torch.device("cuda:0")

    def window(fn):
        """median device microseconds per call of fn()"""
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        us = []
        for _ in range(args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.steps):
                fn()
            b.record()
            torch.cuda.synchronize()
            us.append(1e3 * a.elapsed_time(b) / args.steps)
        return {"us": round(statistics.median(us), 2), "min": round(min(us), 2), "max": round(max(us), 2)}

    res = {"bench": "homography_pose", "build_id": L.build_id()[:16], "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats}
    clock0 = L.clock_probe(5.0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    rows = []
    for n in args.matches:
        cap = (n + 63) // 64 * 64
        n_in = int(0.7 * n)
        for n_pairs in args.pairs:
            pts1, pts2 = np.zeros((n_pairs, cap, 2)), np.zeros((n_pairs, cap, 2))
            match = np.zeros((n_pairs, cap, 3), dtype=np.float32)
            intr = np.zeros((n_pairs, 2, 4))
            hm, fm = np.zeros((n_pairs, 3, 3)), np.zeros((n_pairs, 3, 3))
            mask = np.zeros((n_pairs, cap), dtype=np.uint8)
            for p in range(n_pairs):
                seq = H.make_sequence(1000 * n + p, ("side",), n_in, n - n_in, noise=0.3)
                pr = seq["pairs"][0]
                pts1[p, :n], pts2[p, :n], match[p, :n], intr[p] = seq["pts"][0], seq["pts"][1], pr["match"], pr["intr"]
                hm[p], fm[p], mask[p, :n] = pr["H"], pr["F"], pr["truth"]
            a1, a2, m, kd = t(pts1), t(pts2), t(match), t(intr)
            nm = torch.full((n_pairs,), n, dtype=torch.int32, device=dev)
            n_inl = torch.full((n_pairs,), n_in, dtype=torch.int32, device=dev)
            zero = torch.zeros(n_pairs, dtype=torch.int32, device=dev)
            gh = {"H": t(hm), "mask": t(mask), "n_inliers": n_inl, "status": zero}
            gf = {"F": t(fm), "mask": t(mask), "n_inliers": n_inl, "status": zero}
            o = L.op_homography_pose(gh, a1, a2, m, nm, kd)
            prior = o["normals2"].clone()
            s = L.op_model_select(gf, gh, a1, a2, m, nm)
            row = {"pairs": n_pairs, "matches": n, "cap": cap,
                   "homography_pose_us": window(lambda: L.op_homography_pose(gh, a1, a2, m, nm, kd)),
                   "homography_pose_prior_us": window(lambda: L.op_homography_pose(gh, a1, a2, m, nm, kd, prior=prior)),
                   "model_select_us": window(lambda: L.op_model_select(gf, gh, a1, a2, m, nm))}
            row["front_mean"] = round(float(o["n_front"].double().mean()), 1)
            row["model"] = sorted(set(int(v) for v in o["model"].cpu()))
            row["status"] = sorted(set(int(v) for v in o["status"].cpu()))
            row["use_h_mean"] = round(float(s["use_h"].double().mean()), 3)
            row["ratio_mean"] = round(float((s["scores"][:, 0] / s["scores"].sum(dim=1)).mean()), 4)
            rows.append(row)
    res["operator"] = rows

    Hh, W = args.height, args.width
    arch = "SuperPointNet_gauss2_ssmall"
    net = getattr(models, arch)()
    net.load_state_dict({k: torch.as_tensor(np.array(v)) for k, v in C.init_state_dict(arch, seed=21).items()})
    net = net.to(dev).eval()
    big = torch.from_numpy(np.random.RandomState(5).uniform(0, 1, (Hh, W + 16)).astype(np.float32)).to(dev)
    ims = [big[:, 2 * k:2 * k + W].contiguous() for k in range(8)]
    step = {"height": Hh, "width": W}
    count = [0]

    def stepper(seq):
        def fn():
            seq.step(ims[count[0] % len(ims)])
            count[0] += 1
        return fn

    for name in ("fundamental", "auto"):
        seq = SequenceTracker(net, dev, conf_thresh=0.0155, nms_dist=4, subpixel=True, nn_thresh=0.7, max_length=5,
                              geometric_check=name, intrinsics=(0.9 * W, 0.9 * W, W / 2.0, Hh / 2.0))
        step[name] = window(stepper(seq))
        g = seq.tracker.last_geometry()
        step["%s_inliers" % name], step["%s_pose_status" % name] = int(g["n_inliers"][0]), int(g["pose_status"][0])
        if name == "auto":
            step["model"], step["scores"] = int(g["model"][0]), [round(float(v), 1) for v in g["scores"][0]]
    step["auto_share_us"] = round(step["auto"]["us"] - step["fundamental"]["us"], 2)
    res["sequence_step_us"] = step
    clock1 = L.clock_probe(5.0)
    res["gpu_clock_mhz"] = None if clock0 is None else {"before": round(clock0, 1), "after": round(clock1, 1)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
