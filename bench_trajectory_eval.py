"""Trajectory evaluation benchmark: one JSON line, also written to `--out`.

  operators     each of ssp_op_traj_align / ape / stats / rpe_delta / rpe_segments per call, and the full
                TrajectoryEvaluator.evaluate_many (align, ape, two stats, rpe + two stats per delta, segments: ten launches), for
                `--frames` (64, 1 024, 4 541: the length of KITTI 00) frames and `--problems` (1, 11) tables against one ground truth
  host_ms       the host route for one table that is on the device: its copy to the host plus the numpy restatement
                tests/traj_eval_ref.evaluate (one run; it loops in Python over segments and frames)
  sequence_step_us   SequenceTracker.step per frame at `--height` x `--width` on a shifted noise image: trajectory_eval None (no new
                code runs) against "observe", twice in turn

Device times are between two HIP events around `--steps` back-to-back calls, median over `--repeats` windows after `--warmup`
calls.  The clock probe before and after reports the clock the device grants.  Nothing about speed is asserted."""
import argparse
import json
import os
import statistics
import time


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--frames", type=int, nargs="+", default=[64, 1024, 4541])
    ap.add_argument("--problems", type=int, nargs="+", default=[1, 11])
    ap.add_argument("--no-host", action="store_true", help="skip the host route")
    ap.add_argument("--height", type=int, default=240)
    ap.add_argument("--width", type=int, default=320)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", "bench_trajectory_eval.json"))
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    from oracle import cpu_ref as C
    from semantic_superpoint_amd import lib as L
    from semantic_superpoint_amd import models
    from semantic_superpoint_amd.export import SequenceTracker
    from semantic_superpoint_amd.trajectory_evaluation import TrajectoryEvaluator
    from tests import traj_eval_cases as TC
    from tests import traj_eval_ref as R
    if not torch.cuda.is_available():
        raise SystemExit("bench_trajectory_eval.py measures on the GPU: no HIP device found")
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

    res = {"bench": "trajectory_eval", "build_id": L.build_id()[:16], "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats}
    clock0 = L.clock_probe(5.0)
    rows = []
    for n in args.frames:
        gt = TC.truth(n, length=0.8 * n)   # steps of 0.8 m: the KITTI lengths 100 .. 800 m find segments from about 1 000 frames on
        base = TC.estimate(gt, 0.037, TC.ROT_A, (5.0, -3.0, 2.0), 0.02 / 0.037, 0.01, seed=n)
        host_ms = None
        if not args.no_host:
            on_device = torch.as_tensor(base).to(dev)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            R.evaluate(on_device.cpu().numpy(), n, gt)
            host_ms = round(1e3 * (time.perf_counter() - t0), 1)
        for P in args.problems:
            tables = torch.as_tensor(np.stack([base] * P)).to(dev)
            ev = TrajectoryEvaluator(gt, capacity=n, device=dev)
            out = ev.evaluate_many(tables, n)
            traj = L.traj_eval_buffers(n, P, len(L.KITTI_LENGTHS), 10, dev)
            traj["lengths"].copy_(torch.tensor(L.KITTI_LENGTHS, dtype=torch.float64))
            nf = torch.full((P,), n, dtype=torch.int32, device=dev)
            L.op_traj_align(tables, nf, ev.gt, traj)
            row = {"frames": n, "problems": P, "host_ms": host_ms, "n_valid": int(out["sim"][0, 13].item()),
                   "segments": int(out["info"][0, 0].item())}
            row["align"] = window(lambda: L.op_traj_align(tables, nf, ev.gt, traj))
            row["ape"] = window(lambda: L.op_traj_ape(tables, nf, ev.gt, traj))
            row["stats"] = window(lambda: L.op_traj_stats(traj["err_t"], traj["valid"], traj["stats"][0]))
            row["rpe_delta"] = window(lambda: L.op_traj_rpe_delta(tables, nf, ev.gt, traj, scale=traj["sim"]))
            row["rpe_segments"] = window(lambda: L.op_traj_rpe_segments(tables, nf, ev.gt, traj, scale=traj["sim"]))
            row["evaluate"] = window(lambda: ev.evaluate_many(tables, nf))
            rows.append(row)
    res["rows"] = rows
    H, W = args.height, args.width
    net = getattr(models, "SuperPointNet_gauss2_ssmall")()
    net.load_state_dict({k: torch.as_tensor(np.array(v)) for k, v in C.init_state_dict("SuperPointNet_gauss2_ssmall", seed=21).items()})
    net = net.to(dev).eval()
    big = torch.from_numpy(np.random.RandomState(5).uniform(0, 1, (H, W + 16)).astype(np.float32)).to(dev)
    ims = [big[:, 2 * k:2 * k + W].contiguous() for k in range(8)]
    step = {"height": H, "width": W}
    for mode in (None, "observe", None, "observe"):
        kw = {} if mode is None else dict(ground_truth=TC.truth(4096), trajectory_eval=mode)
        seq = SequenceTracker(net, dev, conf_thresh=0.0155, nms_dist=4, subpixel=True, nn_thresh=0.7, max_length=5,
                              geometric_check="fundamental", intrinsics=(0.9 * W, 0.9 * W, W / 2.0, H / 2.0), **kw)
        counter = [0]

        def one():
            seq.step(ims[counter[0] % len(ims)])
            counter[0] += 1
        key = str(mode) + ("_again" if str(mode) in step else "")
        step[key] = window(one)
    step["observe_share_us"] = round(step["observe"]["us"] - step["None"]["us"], 2)
    step["observe_share_again_us"] = round(step["observe_again"]["us"] - step["None_again"]["us"], 2)
    res["sequence_step_us"] = step
    res["clock_mhz"] = [clock0, L.clock_probe(5.0)]
    line = json.dumps(res)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
