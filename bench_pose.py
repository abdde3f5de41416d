"""Two-view pose benchmark: one JSON line.

  two_view_pose_us   ssp_pose_from_fundamental per call for `--pairs` (1 and 16) pairs of `--matches` (500 and 1131) matches
                     (70 % inliers, 0.3 px of noise), fed the fundamental matrices and masks of ssp_epi_ransac; epi_ransac_us,
                     the call it follows, on the same pairs
  pose_chain_us      ssp_pose_chain per call on two consecutive pairs of a sequence with that many matches
  sequence_step_us   SequenceTracker.step per frame at `--height` x `--width` on a shifted noise image with
                     geometric_check="fundamental", without and with `intrinsics`

Device times are between two HIP events around `--steps` back-to-back calls, median over `--repeats` windows after `--warmup`
calls; the variants of one shape are measured in turn inside one run.  The clock probe before and after reports the clock the
device grants.  Nothing about speed is asserted."""
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
    from tests import pose_ref as P
    if not torch.cuda.is_available():
        raise SystemExit("bench_pose.py measures on the GPU: no HIP device found")
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

    res = {"bench": "pose", "build_id": L.build_id()[:16], "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats}
    clock0 = L.clock_probe(5.0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    ops, chains = [], []
    for n in args.matches:
        cap = (n + 63) // 64 * 64
        n_in = int(0.7 * n)
        for n_pairs in args.pairs:
            pts1, pts2 = np.zeros((n_pairs, cap, 2)), np.zeros((n_pairs, cap, 2))
            match = np.zeros((n_pairs, cap, 3), dtype=np.float32)
            intr = np.zeros((n_pairs, 2, 4))
            for p in range(n_pairs):
                seq = P.make_sequence(1000 * n + p, 2, n_in, n - n_in, noise=0.3)
                pts1[p, :n], pts2[p, :n], match[p, :n], intr[p] = seq["pts"][0], seq["pts"][1], seq["pairs"][0]["match"], seq["pairs"][0]["intr"]
            a1, a2, m, kd = t(pts1), t(pts2), t(match), t(intr)
            nm = torch.full((n_pairs,), n, dtype=torch.int32, device=dev)
            seeds = torch.arange(n_pairs, dtype=torch.int64, device=dev) + 77
            g = L.op_epipolar_ransac(a1, a2, m, nm, seeds)
            row = {"pairs": n_pairs, "matches": n, "cap": cap,
                   "epi_ransac_us": window(lambda k: L.op_epipolar_ransac(a1, a2, m, nm, seeds)),
                   "two_view_pose_us": window(lambda k: L.op_two_view_pose(g, a1, a2, m, nm, kd))}
            o = L.op_two_view_pose(g, a1, a2, m, nm, kd)
            row["inliers_mean"] = round(float(g["n_inliers"].double().mean()), 1)
            row["front_mean"] = round(float(o["n_front"].double().mean()), 1)
            row["status"] = sorted(set(int(s) for s in o["status"].cpu()))
            ops.append(row)
        seq = P.make_sequence(7000 + n, 3, n_in, n - n_in, noise=0.3)
        pts = np.zeros((3, cap, 2))
        match = np.zeros((2, cap, 3), dtype=np.float32)
        for f in range(3):
            pts[f, :n] = seq["pts"][f]
        for k in range(2):
            match[k, :n] = seq["pairs"][k]["match"]
        pd, m = t(pts), t(match)
        nm = torch.full((2,), n, dtype=torch.int32, device=dev)
        g = L.op_epipolar_ransac(pd[:2], pd[1:], m, nm, torch.arange(2, dtype=torch.int64, device=dev) + 5)
        o = L.op_two_view_pose(g, pd[:2], pd[1:], m, nm, t(np.stack([pr["intr"] for pr in seq["pairs"]])))
        prev, cur = ({k: v[i:i + 1] for k, v in o.items()} for i in range(2))
        state, table = L.pose_state(dev), L.pose_table(8, dev)
        row = {"matches": n, "cap": cap,
               "pose_chain_us": window(lambda k: L.op_pose_chain(prev, cur, m[0:1], m[1:2], nm[0:1], nm[1:2], state, table))}
        st, tb = L.pose_state(dev), L.pose_table(8, dev)
        L.op_pose_chain(prev, cur, m[0:1], m[1:2], nm[0:1], nm[1:2], st, tb)
        row["n_shared"], row["flags"], row["ratio"] = int(tb[0, 13]), int(tb[0, 14]), round(float(tb[0, 15]), 4)
        row["true_ratio"] = round(seq["pairs"][1]["length"] / seq["pairs"][0]["length"], 4)
        chains.append(row)
    res["operator"], res["chain"] = ops, chains

    H, W = args.height, args.width
    net = getattr(models, ARCH)()
    net.load_state_dict({k: torch.as_tensor(np.array(v)) for k, v in C.init_state_dict(ARCH, seed=21).items()})
    net = net.to(dev).eval()
    big = torch.from_numpy(np.random.RandomState(5).uniform(0, 1, (H, W + 16)).astype(np.float32)).to(dev)
    ims = [big[:, 2 * k:2 * k + W].contiguous() for k in range(8)]
    step = {"height": H, "width": W}
    for name, intr in (("fundamental", None), ("fundamental_intrinsics", (0.9 * W, 0.9 * W, W / 2.0, H / 2.0))):
        seq = SequenceTracker(net, dev, conf_thresh=0.0155, nms_dist=4, subpixel=True, nn_thresh=0.7, max_length=5,
                              geometric_check="fundamental", intrinsics=intr)
        step[name] = window(lambda k: seq.step(ims[k % len(ims)]))
        g = seq.tracker.last_geometry()
        step["%s_inliers" % name] = int(g["n_inliers"][0])
        if intr is not None:
            step["pose_status"], step["n_front"] = int(g["pose_status"][0]), int(g["n_front"][0])
            step["trajectory_rows"] = int(seq.trajectory()[1])
    step["pose_share_us"] = round(step["fundamental_intrinsics"]["us"] - step["fundamental"]["us"], 2)
    res["sequence_step_us"] = step
    clock1 = L.clock_probe(5.0)
    res["gpu_clock_mhz"] = None if clock0 is None else {"before": round(clock0, 1), "after": round(clock1, 1)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
