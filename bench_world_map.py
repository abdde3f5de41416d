"""World map benchmark: one JSON line.

  matcher            ssp_match_world per call at `--map-rows` (4 096, 16 384, 65 536) map rows against `--frame-rows` (1 131, 4 096)
                     frame rows of random unit descriptors with planted correspondences, beside a torch composition on the device
                     (mm, clamp, sqrt, both arg-mins, the mutual test and the threshold; no compaction) and, at 4 096 map rows,
                     op_match_two_way on the same data.  gflops: 2 * 256 * rows * rows over the device time; hbm_gbs: the bytes
                     of both descriptor sets, read once, over it
  insert             ssp_op_world_insert of `--landmarks` landmark rows: all new (the map is cleared before each call) and all found
  correspondences    ssp_op_world_correspondences + ssp_pnp_ransac for 1 131 match rows
  sequence_step_us   SequenceTracker.step per frame at `--height` x `--width` on a shifted noise image with
                     geometric_check="fundamental" and intrinsics: world_map None (no new code runs), "observe", "relocalise"

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
    ap.add_argument("--map-rows", type=int, nargs="+", default=[4096, 16384, 65536])
    ap.add_argument("--frame-rows", type=int, nargs="+", default=[1131, 4096])
    ap.add_argument("--landmarks", type=int, default=4096)
    ap.add_argument("--height", type=int, default=240)
    ap.add_argument("--width", type=int, default=320)
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    from oracle import cpu_ref as C
    from semantic_superpoint_amd import lib as L
    from semantic_superpoint_amd import models
    from semantic_superpoint_amd.export import SequenceTracker
    if not torch.cuda.is_available():
        raise SystemExit("bench_world_map.py measures on the GPU: no HIP device found")
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

    res = {"bench": "world_map", "build_id": L.build_id()[:16], "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats}
    clock0 = L.clock_probe(5.0)
    thr = 0.7

    def unit(seed, n):
        g = torch.Generator(device=dev)
        g.manual_seed(seed)
        d = torch.randn(n, 256, device=dev, generator=g)
        return d / d.norm(dim=1, keepdim=True)

    def torch_match(d1, d2):
        d = torch.sqrt(2.0 - 2.0 * torch.clamp(d1 @ d2.t(), -1.0, 1.0))
        dmin, j = d.min(dim=1)
        i = d.argmin(dim=0)
        return (dmin < thr) & (i[j] == torch.arange(d1.shape[0], device=dev)), j, dmin

    rows = []
    for n1 in args.map_rows:
        for n2 in args.frame_rows:
            d1, d2 = unit(n1, n1), unit(7 * n2 + 1, n2)
            k = min(n1, n2) // 2
            noisy = d1[torch.randperm(n1, device=dev)[:k]] + 0.02 * torch.randn(k, 256, device=dev)
            d2[:k] = noisy / noisy.norm(dim=1, keepdim=True)
            w = L.world_buffers(n1, 1024, dev)
            w["desc"].copy_(d1)
            w["state"][0] = n1
            cnt = torch.full((1,), n2, dtype=torch.int32, device=dev)
            out = (torch.zeros(n2, 3, device=dev), torch.zeros(1, dtype=torch.int32, device=dev))
            m, nm = L.op_match_world(w, d2, cnt, thr, out=out)
            keep, j, dmin = torch_match(d1, d2)
            torch.cuda.synchronize()
            row = {"map_rows": n1, "frame_rows": n2, "matches": int(nm), "torch_matches": int(keep.sum()),
                   "world_us": window(lambda _: L.op_match_world(w, d2, cnt, thr, out=out)),
                   "torch_us": window(lambda _: torch_match(d1, d2))}
            if n1 <= L.MATCH_MAX_POINTS and n2 <= n1:
                side2 = torch.zeros(1, n1, 256, device=dev)
                side2[0, :n2] = d2
                c1 = torch.full((1,), n1, dtype=torch.int32, device=dev)
                m2, nm2 = L.op_match_two_way(d1[None], c1, side2, cnt, thr)
                row["two_way_equal"] = bool(int(nm2) == int(nm) and torch.equal(m2[0, :int(nm)], m[:int(nm)]))
                row["two_way_us"] = window(lambda _: L.op_match_two_way(d1[None], c1, side2, cnt, thr))
                row["world_us_again"] = window(lambda _: L.op_match_world(w, d2, cnt, thr, out=out))
            row["gflops"] = round(2.0 * 256 * n1 * n2 / row["world_us"]["us"] / 1e3, 1)
            row["hbm_gbs"] = round(1024.0 * (n1 + n2) / row["world_us"]["us"] / 1e3, 1)
            row["torch_over_world"] = round(row["torch_us"]["us"] / row["world_us"]["us"], 2)
            rows.append(row)
            del w, d1, d2
    res["matcher"] = rows

    # insert
    n = args.landmarks
    cap = min(n, L.MATCH_MAX_POINTS)
    lm = torch.zeros(n, L.LANDMARK_WORDS, dtype=torch.float64, device=dev)
    lm[:, 0] = torch.arange(n, device=dev)
    lm[:, 1:4] = torch.rand(n, 3, dtype=torch.float64, device=dev)
    lm[:, 4], lm[:, 7] = 3, torch.arange(n, device=dev) % cap
    nl = torch.full((1,), n, dtype=torch.int32, device=dev)
    desc = unit(3, cap)
    cnt = torch.full((1,), cap, dtype=torch.int32, device=dev)
    table = L.pose_table(8, dev)
    w = L.world_buffers(65536, device=dev)

    def fresh(_):
        w["state"].zero_()
        L.op_world_insert(w, lm, nl, desc, cnt, table, 3)
    res["insert"] = {"landmarks": n, "clear_us": window(lambda _: w["state"].zero_()), "clear_and_append_us": window(fresh),
                     "update_us": window(lambda _: L.op_world_insert(w, lm, nl, desc, cnt, table, 3)),
                     "state": w["state"].cpu().tolist()}

    # correspondences + P3P on a map of 65 536 rows, 1 131 match rows
    nmatch, pcap = 1131, 1152
    rng = np.random.RandomState(4)
    Xw = np.stack([rng.uniform(-4, 4, 65536), rng.uniform(-3, 3, 65536), rng.uniform(3, 12, 65536)], axis=1)
    w["X"].copy_(torch.from_numpy(Xw).to(dev))
    w["state"][0] = 65536
    kk = np.array([288.0, 288.0, 160.0, 120.0])
    pick = rng.permutation(65536)[:nmatch]
    px = np.stack([kk[0] * Xw[pick, 0] / Xw[pick, 2] + kk[2], kk[1] * Xw[pick, 1] / Xw[pick, 2] + kk[3]], axis=1) + 0.3 * rng.randn(nmatch, 2)
    px[::4] = rng.uniform(0, 320, (len(px[::4]), 2))                       # a quarter of the matches are wrong
    pts = torch.zeros(pcap, 2, dtype=torch.float64, device=dev)
    pts[:nmatch] = torch.from_numpy(px).to(dev)
    match = torch.zeros(pcap, 3, device=dev)
    order = np.argsort(pick)
    match[:nmatch, 0] = torch.from_numpy(pick[order].astype(np.float32)).to(dev)
    match[:nmatch, 1] = torch.from_numpy(order.astype(np.float32)).to(dev)
    nmt = torch.full((1,), nmatch, dtype=torch.int32, device=dev)
    pc = torch.full((1,), nmatch, dtype=torch.int32, device=dev)
    buf = L.pnp_buffers(1, pcap, dev)
    kd = torch.from_numpy(kk[None]).to(dev)
    seed = torch.full((1,), 5, dtype=torch.int64, device=dev)

    def join_pnp(_):
        corr, nn = L.op_world_correspondences(w, match, nmt, pts, pc, out=buf)
        return L.op_pnp_ransac(buf["corr"], nn[0:1], kd, seed, out=buf)
    o = join_pnp(0)
    res["correspondences"] = {"rows": nmatch, "join_us": window(lambda _: L.op_world_correspondences(w, match, nmt, pts, pc, out=buf)),
                              "join_and_ransac_us": window(join_pnp), "status": int(o["status"][0]), "n_inliers": int(o["n_inliers"][0])}
    del w

    H, W = args.height, args.width
    net = getattr(models, ARCH)()
    net.load_state_dict({k: torch.as_tensor(np.array(v)) for k, v in C.init_state_dict(ARCH, seed=21).items()})
    net = net.to(dev).eval()
    big = torch.from_numpy(np.random.RandomState(5).uniform(0, 1, (H, W + 16)).astype(np.float32)).to(dev)
    ims = [big[:, 2 * k:2 * k + W].contiguous() for k in range(8)]
    step = {"height": H, "width": W}
    for mode in (None, "observe", "relocalise"):
        seq = SequenceTracker(net, dev, conf_thresh=0.0155, nms_dist=4, subpixel=True, nn_thresh=0.7, max_length=5,
                              geometric_check="fundamental", intrinsics=(0.9 * W, 0.9 * W, W / 2.0, H / 2.0), world_map=mode)
        step[str(mode)] = window(lambda k: seq.step(ims[k % len(ims)]))
        g = seq.tracker.last_geometry()
        step["%s_inliers" % mode] = int(g["n_inliers"][0])
        if mode is not None:
            step["%s_world" % mode] = {"status": int(g["world_status"][0]), "n_match": int(g["world_n_match"][0]),
                                       "n_inliers": int(g["world_n_inliers"][0]), "map_state": seq.world_map_device()["state"].cpu().tolist()}
    step["observe_share_us"] = round(step["observe"]["us"] - step["None"]["us"], 2)
    step["relocalise_share_us"] = round(step["relocalise"]["us"] - step["None"]["us"], 2)
    res["sequence_step_us"] = step
    clock1 = L.clock_probe(5.0)
    res["gpu_clock_mhz"] = None if clock0 is None else {"before": round(clock0, 1), "after": round(clock1, 1)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
