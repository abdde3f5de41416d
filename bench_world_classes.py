"""World map classes benchmark: one JSON line.

  matcher   ssp_match_world and ssp_match_world_classes per call on the same inputs at `--map-rows` (4 096, 65 536) map rows
            against `--frame-rows` (1 131) frame rows of random unit descriptors with planted correspondences, `--classes` classes
            drawn uniformly on both sides (planted frame rows carry their map row's class), a full keep mask.  The two calls are
            timed alternately in one process, `--rounds` times each: plain_us / classes_us are the medians of the rounds' medians,
            plain_spread_us the spread (max - min) of the plain matcher's repeated medians - the margin the class-aware call is
            read against.  all_one_class: the same with every row of one class, where the two outputs must be equal.
  vote      ssp_op_track_class_votes at `--landmarks` (3 373, 10 013) landmark rows, and ssp_op_world_classes of a 65 536-row map

Device times are between two HIP events around `--steps` back-to-back calls, median over `--repeats` windows after `--warmup`
calls.  The clock probe before and after reports the clock the device grants.  Nothing about speed is asserted."""
import argparse
import json
import statistics


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--map-rows", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--frame-rows", type=int, nargs="+", default=[1131])
    ap.add_argument("--classes", type=int, default=8)
    ap.add_argument("--landmarks", type=int, nargs="+", default=[3373, 10013])
    args = ap.parse_args(argv)
    import torch
    from semantic_superpoint_amd import lib as L
    if not torch.cuda.is_available():
        raise SystemExit("bench_world_classes.py measures on the GPU: no HIP device found")
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
        return statistics.median(us)

    res = {"bench": "world_classes", "build_id": L.build_id()[:16], "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats,
           "rounds": args.rounds, "classes": args.classes}
    clock0 = L.clock_probe(5.0)
    thr = 0.7

    def unit(seed, n):
        g = torch.Generator(device=dev)
        g.manual_seed(seed)
        d = torch.randn(n, 256, device=dev, generator=g)
        return d / d.norm(dim=1, keepdim=True)

    def entries(cls):
        return ((3 << 8) | cls.to(torch.int32)).to(torch.int16).view(torch.uint16)     # (three votes each)

    rows = []
    for n1 in args.map_rows:
        for n2 in args.frame_rows:
            d1, d2 = unit(n1, n1), unit(7 * n2 + 1, n2)
            k = min(n1, n2) // 2
            src = torch.randperm(n1, device=dev)[:k]
            noisy = d1[src] + 0.02 * torch.randn(k, 256, device=dev)
            d2[:k] = noisy / noisy.norm(dim=1, keepdim=True)
            c1 = torch.randint(0, args.classes, (n1,), device=dev).to(torch.uint8)
            c2 = torch.randint(0, args.classes, (n2,), device=dev).to(torch.uint8)
            c2[:k] = c1[src]
            w = L.world_buffers(n1, n1, dev)
            w["desc"].copy_(d1)
            w["tid"].copy_(torch.arange(n1, dtype=torch.int32, device=dev))
            w["state"][0] = n1
            classes = L.world_class_buffers(n1, dev)
            cnt = torch.full((1,), n2, dtype=torch.int32, device=dev)
            out = (torch.zeros(n2, 3, device=dev), torch.zeros(1, dtype=torch.int32, device=dev))
            out_c = (torch.zeros(n2, 3, device=dev), torch.zeros(1, dtype=torch.int32, device=dev))
            plain = lambda: L.op_match_world(w, d2, cnt, thr, out=out)
            row = {"map_rows": n1, "frame_rows": n2}
            for tag, a, b in (("", c1, c2), ("all_one_class", torch.ones_like(c1), torch.ones_like(c2))):
                classes["votes"].copy_(entries(a))
                aware = lambda: L.op_match_world_classes(w, classes, d2, b, cnt, thr, out=out_c)
                plain(), aware()
                torch.cuda.synchronize()
                p, c = [], []
                for _ in range(args.rounds):
                    p.append(window(plain))
                    c.append(window(aware))
                r = {"matches_plain": int(out[1]), "matches_classes": int(out_c[1]),
                     "plain_us": round(statistics.median(p), 2), "classes_us": round(statistics.median(c), 2),
                     "plain_spread_us": round(max(p) - min(p), 2), "classes_spread_us": round(max(c) - min(c), 2),
                     "plain_medians_us": [round(x, 2) for x in p], "classes_medians_us": [round(x, 2) for x in c]}
                r["classes_minus_plain_us"] = round(r["classes_us"] - r["plain_us"], 2)
                r["within_plain_spread"] = bool(abs(r["classes_us"] - r["plain_us"]) <= r["plain_spread_us"])
                if tag:
                    nm = int(out[1])
                    r["equal"] = bool(int(out_c[1]) == nm and torch.equal(out[0][:nm], out_c[0][:nm]))
                    row[tag] = r
                else:
                    row.update(r)
            rows.append(row)
            del w, classes, d1, d2
    res["matcher"] = rows

    votes = []
    point_cap = L.MATCH_MAX_POINTS
    cls_new = torch.randint(0, args.classes, (point_cap,), device=dev).to(torch.uint8)
    cnt = torch.full((1,), point_cap, dtype=torch.int32, device=dev)
    for n in args.landmarks:
        classes = L.world_class_buffers(1 << 22, dev)
        lm = torch.zeros(n, L.LANDMARK_WORDS, dtype=torch.float64, device=dev)
        lm[:, 0] = torch.randperm(1 << 22, device=dev)[:n]
        lm[:, 7] = torch.arange(n, device=dev) % point_cap
        nl = torch.full((1,), n, dtype=torch.int32, device=dev)
        votes.append({"landmarks": n, "vote_us": round(window(lambda: L.op_track_class_votes(classes, lm, nl, cls_new, cnt)), 2)})
    res["vote"] = votes
    w = L.world_buffers(65536, device=dev)
    w["state"][0] = 65536
    classes = L.world_class_buffers(w["tid_cap"], dev)
    out = torch.empty(65536, dtype=torch.uint8, device=dev)
    res["read_out"] = {"map_rows": 65536, "us": round(window(lambda: L.op_world_classes(w, classes, out=out)), 2)}
    clock1 = L.clock_probe(5.0)
    res["gpu_clock_mhz"] = None if clock0 is None else {"before": round(clock0, 1), "after": round(clock1, 1)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
