"""Landmark benchmark: one JSON line.

  landmarks_us     ssp_map_window + ssp_op_triangulate_tracks + ssp_op_landmarks_select per call on the track table of a
                   sequence of `--points` points per frame (a share `--drop` of the matches left out, so tracks end and start:
                   about 3 400 rows at L = 5), for every `--lengths` L, in buffers allocated once; triangulate_us: the middle
                   call alone
  numpy_ms         the numpy restatement (tests/landmarks_ref.py, float64, vectorised over the rows) on the same table: wall clock

Device times are between two HIP events around `--steps` back-to-back calls, median over `--repeats` windows after `--warmup`
calls.  The clock probe before and after reports the clock the device grants.  Nothing about speed is asserted."""
import argparse
import json
import statistics
import time


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--lengths", type=int, nargs="+", default=[5, 16])
    ap.add_argument("--points", type=int, default=1000)
    ap.add_argument("--drop", type=float, default=0.6)
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    from semantic_superpoint_amd import lib as L
    from tests import landmarks_ref as R
    if not torch.cuda.is_available():
        raise SystemExit("bench_landmarks.py measures on the GPU: no HIP device found")
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

    res = {"bench": "landmarks", "build_id": L.build_id()[:16], "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats,
           "points": args.points, "drop": args.drop}
    clock0 = L.clock_probe(5.0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    rows_out = []
    for length in args.lengths:
        n_out = args.points // 20
        seq = R.make_slow_sequence(900 + length, length, args.points - n_out, n_out)
        tr = R.build_tracks(seq, length, drop=args.drop, drop_seed=length)
        point_cap = (args.points + 63) // 64 * 64
        row_cap = length * point_cap
        n = tr.ids.shape[0]
        pts, first_slot = R.ring_of(seq, length, point_cap)
        # the trajectory of the true poses, as the chain would have written it: one camera, every scale chained
        Rw, C = R.true_poses(seq)
        table = np.zeros((length + 1, 16))
        table[:length, :9], table[:length, 9:12], table[:length, 12] = Rw.reshape(-1, 9), C, 1.0
        table[0, 14], table[1, 14] = 3.0, 2.0
        state = L.pose_state(dev)
        state[0] = length
        ids = np.full((row_cap, length), -1, dtype=np.int32)
        tid = np.zeros(row_cap, dtype=np.int32)
        ids[:n], tid[:n] = tr.ids, tr.tid
        tab = {"ids": t(ids), "tid": t(tid), "score": torch.zeros(row_cap, dtype=torch.float64, device=dev),
               "state": t(np.array([n, tr.track_count] + list(tr.counts), dtype=np.int32)), "L": length, "point_cap": point_cap,
               "row_cap": row_cap}
        table_d, intr_d, pts_d = t(table), t(seq["intr"][:1]), t(pts)
        out = L.landmark_buffers(length, row_cap, dev)

        def all_three():
            cams = L.op_map_window(state, table_d, intr_d, length, out=out)
            rows = L.op_triangulate_tracks(tab, pts_d, first_slot, cams, out=out)
            return L.op_landmarks_select(tab, rows, out=out)

        lm, n_lm = all_three()
        cams = out["cams"].clone()
        row = {"L": length, "rows": n, "row_cap": row_cap, "point_cap": point_cap, "landmarks": int(n_lm),
               "landmarks_us": window(all_three),
               "triangulate_us": window(lambda: L.op_triangulate_tracks(tab, pts_d, first_slot, cams, out=out))}
        t0 = time.perf_counter()
        cams_np = R.map_window(length, table, seq["intr"][:1], length)
        ref = R.triangulate(tr.ids, tr.counts, pts, first_slot, cams_np)
        lm_np = R.select(tr.ids, tr.tid, tr.counts, point_cap, ref)
        row["numpy_ms"] = round(1e3 * (time.perf_counter() - t0), 2)
        row["status_counts"] = np.bincount(ref["status"], minlength=5).tolist()
        row["equal_to_numpy"] = bool(np.array_equal(lm[:int(n_lm)].cpu().numpy(), lm_np))
        rows_out.append(row)
    res["tables"] = rows_out
    clock1 = L.clock_probe(5.0)
    res["gpu_clock_mhz"] = None if clock0 is None else {"before": round(clock0, 1), "after": round(clock1, 1)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
