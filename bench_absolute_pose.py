"""Absolute pose benchmark: one JSON line.

  operator           ssp_op_landmark_matches + ssp_pnp_ransac per call for `--problems` (1 and 16) problems of `--rows` (500 and
                     1131) correspondences (70 % inliers, 0.3 px of noise, the rest salted); the join runs once per problem
  groups             ssp_pnp_ransac alone with 1, 2, 8, 16 and 32 workgroups per problem (and 0, the library's choice)
  sequence_step_us   SequenceTracker.step per frame at `--height` x `--width` on a shifted noise image with
                     geometric_check="fundamental" and intrinsics: absolute_pose None (the step as it was before section 27: no
                     new code runs), "observe" and "repair"

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
    ap.add_argument("--problems", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--rows", type=int, nargs="+", default=[500, 1131])
    ap.add_argument("--groups", type=int, nargs="+", default=[1, 2, 8, 16, 32, 0])
    ap.add_argument("--height", type=int, default=240)
    ap.add_argument("--width", type=int, default=320)
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    from oracle import cpu_ref as C
    from semantic_superpoint_amd import lib as L
    from semantic_superpoint_amd import models
    from semantic_superpoint_amd.export import SequenceTracker
    from tests import landmarks_ref as LR
    from tests import pnp_ref as R
    from tests import pose_ref as P
    if not torch.cuda.is_available():
        raise SystemExit("bench_absolute_pose.py measures on the GPU: no HIP device found")
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

    res = {"bench": "absolute_pose", "build_id": L.build_id()[:16], "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats}
    clock0 = L.clock_probe(5.0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    ops = []
    for n in args.rows:
        cap = (n + 63) // 64 * 64
        for n_problems in args.problems:
            lms, matches, pts, ks = [], [], [], []
            for p in range(n_problems):
                seq = P.make_sequence(1000 * n + p, 2, n, 0, zoom=False)
                X = LR.scene_points(1000 * n + p, 2, n, "side", False)
                Rws, Cs = LR.true_poses(seq)
                corr, _ = R.make_problem(X, Rws[1], Cs[1], seq["intr"][1], 0.3, 0.3, 0, 0, p)
                lm = np.zeros((cap, L.LANDMARK_WORDS))
                lm[:n, 1:4], lm[:n, 7] = corr[:, 0:3], np.arange(n)
                m = np.zeros((cap, 3), dtype=np.float32)
                m[:n, 0] = m[:n, 1] = np.arange(n)
                px = np.zeros((cap, 2))
                px[:n] = corr[:, 3:5]
                lms.append(t(lm)), matches.append(t(m)), pts.append(t(px)), ks.append(seq["intr"][1])
            cnt = torch.full((1,), n, dtype=torch.int32, device=dev)
            bufs = [L.pnp_buffers(1, cap, dev) for _ in range(n_problems)]
            out = L.pnp_buffers(n_problems, cap, dev)
            kd = t(np.stack(ks))
            nn = torch.full((n_problems,), n, dtype=torch.int32, device=dev)
            seeds = torch.arange(n_problems, dtype=torch.int64, device=dev) + 77

            def both(k, groups=0):
                for p in range(n_problems):
                    corr, _ = L.op_landmark_matches(lms[p], cnt, matches[p], cnt, pts[p], out=bufs[p])
                    out["corr"][p].copy_(corr)
                return L.op_pnp_ransac(out["corr"], nn, kd, seeds, groups=groups, out=out)

            o = both(0)
            row = {"problems": n_problems, "rows": n, "cap": cap, "join_and_ransac_us": window(both),
                   "join_us": window(lambda k: L.op_landmark_matches(lms[0], cnt, matches[0], cnt, pts[0], out=bufs[0])),
                   "ransac_us": {str(g): window(lambda k: L.op_pnp_ransac(out["corr"], nn, kd, seeds, groups=g, out=out)) for g in args.groups},
                   "inliers_mean": round(float(o["n_inliers"].double().mean()), 1), "rms_mean": round(float(o["rms"].mean()), 4),
                   "status": sorted(set(int(s) for s in o["status"].cpu()))}
            ops.append(row)
    res["operator"] = ops

    H, W = args.height, args.width
    net = getattr(models, ARCH)()
    net.load_state_dict({k: torch.as_tensor(np.array(v)) for k, v in C.init_state_dict(ARCH, seed=21).items()})
    net = net.to(dev).eval()
    big = torch.from_numpy(np.random.RandomState(5).uniform(0, 1, (H, W + 16)).astype(np.float32)).to(dev)
    ims = [big[:, 2 * k:2 * k + W].contiguous() for k in range(8)]
    step = {"height": H, "width": W}
    for mode in (None, "observe", "repair"):
        seq = SequenceTracker(net, dev, conf_thresh=0.0155, nms_dist=4, subpixel=True, nn_thresh=0.7, max_length=5,
                              geometric_check="fundamental", intrinsics=(0.9 * W, 0.9 * W, W / 2.0, H / 2.0), absolute_pose=mode)
        step[str(mode)] = window(lambda k: seq.step(ims[k % len(ims)]))
        g = seq.tracker.last_geometry()
        step["%s_inliers" % mode] = int(g["n_inliers"][0])
        if mode is not None:
            step["%s_abs" % mode] = {"status": int(g["abs_status"][0]), "n_corr": int(g["abs_n_corr"][1]), "n_inliers": int(g["abs_n_inliers"][0])}
    step["observe_share_us"] = round(step["observe"]["us"] - step["None"]["us"], 2)
    step["repair_share_us"] = round(step["repair"]["us"] - step["None"]["us"], 2)
    res["sequence_step_us"] = step
    clock1 = L.clock_probe(5.0)
    res["gpu_clock_mhz"] = None if clock0 is None else {"before": round(clock0, 1), "after": round(clock1, 1)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
