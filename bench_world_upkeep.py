"""World map upkeep benchmark: one JSON line, also written to `--out`.

  operator           ssp_op_world_upkeep per call on a map of `--map-rows` (4 096, 16 384, 65 536) rows of which `--dying` (0, 10,
                     50 %) are culled, at random slots, beside a torch composition on the device (the cull mask, nonzero, then
                     index_select and a copy back per array; nonzero synchronises with the host).  A call compacts the map, so every
                     call of a window is preceded by a restore of the three arrays that decide who dies (n_views, last_frame, state:
                     0.5 MB at 65 536 rows); restore_us is that restore alone and upkeep_us the difference.  moved_mb: the bytes
                     the two move kernels read and write (1 072 B per surviving row from the first dead slot on, twice over),
                     move_gbs: that over upkeep_us
  sequence_step_us   SequenceTracker.step per frame at `--height` x `--width` on a shifted noise image with world_map="relocalise":
                     world_upkeep None (no new code runs) against "on"

Device times are between two HIP events around `--steps` back-to-back calls, median over `--repeats` windows after `--warmup`
calls; the variants of one shape are measured in turn inside one run.  The clock probe before and after reports the clock the
device grants.  Nothing about speed is asserted."""
import argparse
import json
import os
import statistics

ARCH = "SuperPointNet_gauss2_ssmall"
ROW_BYTES = 1024 + 24 + 8 + 16     # descriptor, X, rms, four int32 columns


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--map-rows", type=int, nargs="+", default=[4096, 16384, 65536])
    ap.add_argument("--dying", type=int, nargs="+", default=[0, 10, 50])
    ap.add_argument("--height", type=int, default=240)
    ap.add_argument("--width", type=int, default=320)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", "bench_world_upkeep.json"))
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    from oracle import cpu_ref as C
    from semantic_superpoint_amd import lib as L
    from semantic_superpoint_amd import models
    from semantic_superpoint_amd.export import SequenceTracker
    if not torch.cuda.is_available():
        raise SystemExit("bench_world_upkeep.py measures on the GPU: no HIP device found")
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

    res = {"bench": "world_upkeep", "build_id": L.build_id()[:16], "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats}
    clock0 = L.clock_probe(5.0)
    f, age, min_views = 100, 10, 3
    cols = ("X", "desc", "tid", "n_views", "first_frame", "last_frame", "rms")
    rows = []
    for n in args.map_rows:
        w = L.world_buffers(n, 1 << 17, dev)
        up = L.world_upkeep_buffers(n, dev)
        g = torch.Generator(device=dev)
        g.manual_seed(n)
        w["desc"].copy_(torch.randn(n, 256, device=dev, generator=g))
        w["X"].copy_(torch.rand(n, 3, dtype=torch.float64, device=dev, generator=g))
        w["tid"].copy_(torch.randperm(1 << 17, device=dev, generator=g)[:n].int())
        w["slot_of_tid"][w["tid"].long()] = torch.arange(n, dtype=torch.int32, device=dev)
        match = torch.zeros(8, 3, device=dev)
        zero = torch.zeros(1, dtype=torch.int32, device=dev)
        lms = torch.zeros(8, L.LANDMARK_WORDS, dtype=torch.float64, device=dev)
        pts = torch.zeros(8, 2, dtype=torch.float64, device=dev)
        table = L.pose_table(f + 1, dev)
        table[f, 0:9] = torch.eye(3, dtype=torch.float64, device=dev).reshape(9)
        intr = torch.tensor([288.0, 288.0, 160.0, 120.0], dtype=torch.float64, device=dev)
        for pct in args.dying:
            dying = torch.rand(n, device=dev, generator=g) < pct / 100.0
            views0 = torch.where(dying, 1, 5).int()
            last0 = torch.where(dying, 0, f - 1).int()
            state0 = torch.tensor([n, 1, 0, 0, 0, 0, 0, 0], dtype=torch.int32, device=dev)

            def restore(_):
                w["n_views"].copy_(views0)
                w["last_frame"].copy_(last0)
                w["state"].copy_(state0)

            def upkeep(k):
                restore(k)
                L.op_world_upkeep(w, match, zero, lms, zero, pts, zero, table, f + 1, intr, up, merge=True, merge_thresh=2.0,
                                  cull_age=age, cull_min_views=min_views, high_water=-1)

            def composed(k):
                restore(k)
                keep = ~((w["last_frame"] < f - age) & (w["n_views"] < min_views))
                idx = keep.nonzero().squeeze(1)
                m = idx.shape[0]
                for c in cols:
                    w[c][:m] = w[c].index_select(0, idx)
                w["slot_of_tid"][w["tid"][:m].long()] = torch.arange(m, dtype=torch.int32, device=dev)
                w["state"][0] = m

            upkeep(0)
            report = up["report"].cpu().tolist()
            first_dead = int(dying.nonzero()[0]) if report[2] else n
            moved = report[4] - first_dead
            row = {"map_rows": n, "dying_pct": pct, "report": report, "rows_moved": moved, "restore_us": window(restore),
                   "restore_and_upkeep_us": window(upkeep), "restore_and_torch_us": window(composed)}
            row["upkeep_us"] = round(row["restore_and_upkeep_us"]["us"] - row["restore_us"]["us"], 2)
            row["torch_us"] = round(row["restore_and_torch_us"]["us"] - row["restore_us"]["us"], 2)
            row["moved_mb"] = round(4.0 * ROW_BYTES * moved / 1e6, 2)
            row["move_gbs"] = round(4.0 * ROW_BYTES * moved / max(row["upkeep_us"], 1e-3) / 1e3, 1)
            row["torch_over_upkeep"] = round(row["torch_us"] / max(row["upkeep_us"], 1e-3), 2)
            rows.append(row)
        del w, up
    res["operator"] = rows

    H, W = args.height, args.width
    net = getattr(models, ARCH)()
    net.load_state_dict({k: torch.as_tensor(np.array(v)) for k, v in C.init_state_dict(ARCH, seed=21).items()})
    net = net.to(dev).eval()
    big = torch.from_numpy(np.random.RandomState(5).uniform(0, 1, (H, W + 16)).astype(np.float32)).to(dev)
    ims = [big[:, 2 * k:2 * k + W].contiguous() for k in range(8)]
    step = {"height": H, "width": W}
    for mode in (None, "on", None, "on"):
        seq = SequenceTracker(net, dev, conf_thresh=0.0155, nms_dist=4, subpixel=True, nn_thresh=0.7, max_length=5,
                              geometric_check="fundamental", intrinsics=(0.9 * W, 0.9 * W, W / 2.0, H / 2.0), world_map="relocalise",
                              world_upkeep=mode)
        key = str(mode) + ("_again" if str(mode) in step else "")
        step[key] = window(lambda k: seq.step(ims[k % len(ims)]))
        step["%s_map_state" % key] = seq.world_map_device()["state"].cpu().tolist()
        if mode is not None:
            step["%s_totals" % key] = seq.world_upkeep_report().tolist()
    step["upkeep_share_us"] = round(step["on"]["us"] - step["None"]["us"], 2)
    step["upkeep_share_again_us"] = round(step["on_again"]["us"] - step["None_again"]["us"], 2)
    res["sequence_step_us"] = step
    clock1 = L.clock_probe(5.0)
    res["gpu_clock_mhz"] = None if clock0 is None else {"before": round(clock0, 1), "after": round(clock1, 1)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
