"""Bundle adjustment benchmark: one JSON line.

  tables             ssp_bundle_adjust per call on the track table of a slow sequence of `--points` points per frame (a share
                     `--drop` of the matches left out: about 3 400 rows at L = 5, 10 000 at L = 16; bench_landmarks.py's tables)
                     with 0.3 px of noise, under true cameras perturbed by 0.05 degrees and 0.02 baselines, in buffers allocated once:
                       adjust_us        iterations = 10 (info: what the call did)
                       one_iteration_us iterations = 1; per_iteration_us = (adjust_us - one_iteration_us) / 9, which is an upper
                                        bound on a live iteration only while the loop is not done before the tenth
                       idle_us          iterations = 16 on the same table with n_rows = 0: status 1 after the first iteration, so
                                        every later launch returns at once; launch_us = (idle 16 - idle 1) / 60 launches
                       numpy_ms         the numpy restatement (tests/ba_ref.py, float64) of the same call: wall clock
  sequence_step_us   SequenceTracker.step per frame at `--height` x `--width` on a shifted noise image with
                     geometric_check="fundamental" and intrinsics: bundle_adjust None (no new code runs) and "apply", the two
                     trackers measured in alternating windows of one run

Device times are between two HIP events around `--steps` back-to-back calls, median over `--repeats` windows after `--warmup`
calls.  The clock probe before and after reports the clock the device grants.  Nothing about speed is asserted."""
import argparse
import json
import math
import statistics
import time

ARCH = "SuperPointNet_gauss2_ssmall"


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--lengths", type=int, nargs="+", default=[5, 16])
    ap.add_argument("--points", type=int, default=1000)
    ap.add_argument("--drop", type=float, default=0.6)
    ap.add_argument("--height", type=int, default=240)
    ap.add_argument("--width", type=int, default=320)
    ap.add_argument("--no-numpy", action="store_true", help="skip the numpy restatement (minutes at L = 16)")
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    from oracle import cpu_ref as C
    from semantic_superpoint_amd import lib as L
    from semantic_superpoint_amd import models
    from semantic_superpoint_amd.export import SequenceTracker
    from tests import ba_ref as B
    from tests import landmarks_ref as R
    from tests import pnp_ref as PN
    if not torch.cuda.is_available():
        raise SystemExit("bench_bundle_adjust.py measures on the GPU: no HIP device found")
    dev = torch.device("cuda:0")

    def once(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.steps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return 1e3 * a.elapsed_time(b) / args.steps

    def summary(us):
        return {"us": round(statistics.median(us), 2), "min": round(min(us), 2), "max": round(max(us), 2)}

    def window(fn):
        """median device microseconds per call of fn()"""
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        return summary([once(fn) for _ in range(args.repeats)])

    res = {"bench": "bundle_adjust", "build_id": L.build_id()[:16], "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats,
           "points": args.points, "drop": args.drop}
    clock0 = L.clock_probe(5.0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    rows_out = []
    for length in args.lengths:
        n_out = args.points // 20
        seq = R.make_slow_sequence(900 + length, length, args.points - n_out, n_out, noise=0.3)
        tr = R.build_tracks(seq, length, drop=args.drop, drop_seed=length)
        point_cap = (args.points + 63) // 64 * 64
        row_cap = length * point_cap
        n = tr.ids.shape[0]
        pts, first_slot = R.ring_of(seq, length, point_cap)
        cams = R.true_cams(seq, length)
        rng = np.random.RandomState(3)
        base = float(np.linalg.norm(cams[1, 9:12] - cams[0, 9:12]))
        _, _, b, ks = B.gauge(cams)
        for c in range(1, length):
            axis = rng.randn(3)
            w = axis / np.linalg.norm(axis) * (2.0 * math.tan(math.radians(0.05) / 2.0))
            shift = rng.randn(3) * (0.02 * base)
            if c == b:
                shift[ks] = 0.0
            cams[c, 0:9], _ = PN.cayley_update(cams[c, 0:9].copy(), np.zeros(3), [w[0], w[1], w[2], 0.0, 0.0, 0.0])
            cams[c, 9:12] += shift
        ids = np.full((row_cap, length), -1, dtype=np.int32)
        ids[:n] = tr.ids
        state = np.array([n, tr.track_count] + list(tr.counts), dtype=np.int32)
        tab = {"ids": t(ids), "state": t(state), "L": length, "point_cap": point_cap, "row_cap": row_cap}
        empty = dict(tab, state=t(np.array([0, 0] + list(tr.counts), dtype=np.int32)))
        cams_d, pts_d = t(cams), t(pts)
        rows = L.op_triangulate_tracks(tab, pts_d, first_slot, cams_d)
        out = L.ba_buffers(length, row_cap, dev)
        got = {k: v.cpu().numpy() for k, v in L.op_bundle_adjust(tab, pts_d, first_slot, cams_d, rows, out=out).items()}
        info = got["info"]                                               # (copies: the windows below overwrite the buffers)
        row = {"L": length, "rows": n, "row_cap": row_cap, "point_cap": point_cap, "info": [float("%.6g" % v) for v in info],
               "workspace_bytes": int(out["ws"].numel()),
               "adjust_us": window(lambda: L.op_bundle_adjust(tab, pts_d, first_slot, cams_d, rows, 10, out=out)),
               "one_iteration_us": window(lambda: L.op_bundle_adjust(tab, pts_d, first_slot, cams_d, rows, 1, out=out)),
               "idle_16_us": window(lambda: L.op_bundle_adjust(empty, pts_d, first_slot, cams_d, rows, 16, out=out)),
               "idle_1_us": window(lambda: L.op_bundle_adjust(empty, pts_d, first_slot, cams_d, rows, 1, out=out))}
        row["per_iteration_us"] = round((row["adjust_us"]["us"] - row["one_iteration_us"]["us"]) / 9.0, 2)
        row["launch_us"] = round((row["idle_16_us"]["us"] - row["idle_1_us"]["us"]) / 60.0, 2)
        row["launch_share"] = round(42 * row["launch_us"] / row["adjust_us"]["us"], 3)
        if not args.no_numpy:
            status = rows["status"].cpu().numpy()[:n]
            X = rows["X"].cpu().numpy()[:n]
            t0 = time.perf_counter()
            ref = B.adjust(tr.ids, tr.counts, pts, first_slot, cams, X, status)
            row["numpy_ms"] = round(1e3 * (time.perf_counter() - t0), 2)
            row["equal_to_numpy"] = bool(np.array_equal(ref["info"], info) and np.array_equal(ref["cams"], got["cams"])
                                         and np.array_equal(ref["X"], got["X"][:n]) and np.array_equal(ref["rms"], got["rms"][:n]))
        rows_out.append(row)
    res["tables"] = rows_out

    H, W = args.height, args.width
    net = getattr(models, ARCH)()
    net.load_state_dict({k: torch.as_tensor(np.array(v)) for k, v in C.init_state_dict(ARCH, seed=21).items()})
    net = net.to(dev).eval()
    big = torch.from_numpy(np.random.RandomState(5).uniform(0, 1, (H, W + 16)).astype(np.float32)).to(dev)
    ims = [big[:, 2 * k:2 * k + W].contiguous() for k in range(8)]
    trackers, count = {}, {}
    for mode in (None, "apply"):
        trackers[mode] = SequenceTracker(net, dev, conf_thresh=0.0155, nms_dist=4, subpixel=True, nn_thresh=0.7, max_length=5,
                                         geometric_check="fundamental", intrinsics=(0.9 * W, 0.9 * W, W / 2.0, H / 2.0),
                                         bundle_adjust=mode)
        count[mode] = 0

    def step_of(mode):
        def fn():
            trackers[mode].step(ims[count[mode] % len(ims)])
            count[mode] += 1
        return fn

    for mode in trackers:
        for _ in range(args.warmup):
            step_of(mode)()
    torch.cuda.synchronize()
    us = {None: [], "apply": []}
    for _ in range(args.repeats):                                        # alternating windows: both see the same clock
        for mode in trackers:
            us[mode].append(once(step_of(mode)))
    step = {"height": H, "width": W, "None": summary(us[None]), "apply": summary(us["apply"])}
    step["apply_share_us"] = round(step["apply"]["us"] - step["None"]["us"], 2)
    g = trackers["apply"].tracker.last_geometry()
    step["points"] = int(trackers["apply"].tracker._counts.max())
    step["ba_info"] = [float("%.6g" % v) for v in g["ba_info"].cpu().numpy()]
    res["sequence_step_us"] = step
    clock1 = L.clock_probe(5.0)
    res["gpu_clock_mhz"] = None if clock0 is None else {"before": round(clock0, 1), "after": round(clock1, 1)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
