"""Loop closure benchmark: one JSON line.

  detection          ssp_op_loop_correspondences, the extra ssp_pnp_ransac and ssp_loop_edge for 1 131 match rows against a map of
                     65 536 rows: a revisit (a quarter of the rows old, an edge accepted once and refused inside the cooldown after
                     that) and the idle case (no old row: the P3P still runs its two launches on zero valid rows)
  pose_graph         ssp_pose_graph at `--nodes` (64, 1 024, 4 095) free nodes with 0 and 8 both-ends-free edges, `--iterations`
                     Levenberg-Marquardt steps on tests/loop_ref.py's planted drift, beside the host wall clock of that file's numpy
                     restatement on the same inputs (once per shape)
  apply              ssp_loop_apply over a map of 65 536 rows and 4 095 trajectory rows
  sequence_step_us   SequenceTracker.step per frame at `--height` x `--width` with world_map="observe": loop_closure None (no new
                     code runs), "observe", "apply", in one process

Device times are between two HIP events around `--steps` back-to-back calls, median over `--repeats` windows after `--warmup`
calls.  The clock probe before and after reports the clock the device grants.  Nothing about speed is asserted."""
import argparse
import json
import statistics
import time

ARCH = "SuperPointNet_gauss2_ssmall"


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--nodes", type=int, nargs="+", default=[64, 1024, 4095])
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--height", type=int, default=240)
    ap.add_argument("--width", type=int, default=320)
    ap.add_argument("--no-host", action="store_true", help="skip the numpy restatement's wall clock")
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    from oracle import cpu_ref as C
    from semantic_superpoint_amd import lib as L
    from semantic_superpoint_amd import models
    from semantic_superpoint_amd.export import SequenceTracker
    from tests import loop_ref as G
    if not torch.cuda.is_available():
        raise SystemExit("bench_loop_closure.py measures on the GPU: no HIP device found")
    dev = torch.device("cuda:0")

    def window(fn, steps=None):
        """median device microseconds per call of fn(k)"""
        steps = args.steps if steps is None else steps
        k = 0
        for _ in range(args.warmup):
            fn(k)
            k += 1
        torch.cuda.synchronize()
        us = []
        for _ in range(args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(steps):
                fn(k)
                k += 1
            b.record()
            torch.cuda.synchronize()
            us.append(1e3 * a.elapsed_time(b) / steps)
        return {"us": round(statistics.median(us), 2), "min": round(min(us), 2), "max": round(max(us), 2)}

    res = {"bench": "loop_closure", "build_id": L.build_id()[:16], "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats}
    clock0 = L.clock_probe(5.0)

    # detection: 1 131 match rows against 65 536 map rows
    nmatch, pcap, n_map, f, gap = 1131, 1152, 65536, 300, 32
    rng = np.random.RandomState(4)
    Xw = np.stack([rng.uniform(-4, 4, n_map), rng.uniform(-3, 3, n_map), rng.uniform(3, 12, n_map)], axis=1)
    kk = np.array([288.0, 288.0, 160.0, 120.0])
    pick = np.sort(rng.permutation(n_map)[:nmatch])
    px = np.stack([kk[0] * Xw[pick, 0] / Xw[pick, 2] + kk[2], kk[1] * Xw[pick, 1] / Xw[pick, 2] + kk[3]], axis=1) + 0.3 * rng.randn(nmatch, 2)
    w = L.world_buffers(n_map, 1024, dev)
    w["X"].copy_(torch.from_numpy(Xw).to(dev))
    w["state"][0] = n_map
    last = np.full(n_map, f - 3, dtype=np.int32)
    last[pick[::4]] = rng.randint(0, 40, len(pick[::4]))                  # a quarter of the matched rows are old
    pts = torch.zeros(pcap, 2, dtype=torch.float64, device=dev)
    pts[:nmatch] = torch.from_numpy(px).to(dev)
    match = torch.zeros(pcap, 3, device=dev)
    match[:nmatch, 0] = torch.from_numpy(pick.astype(np.float32)).to(dev)
    match[:nmatch, 1] = torch.arange(nmatch, device=dev)
    nmt = torch.full((1,), nmatch, dtype=torch.int32, device=dev)
    lms = torch.zeros(4096, L.LANDMARK_WORDS, dtype=torch.float64, device=dev)
    lms[:nmatch, 0] = torch.arange(nmatch, device=dev)
    lms[:nmatch, 1:4] = torch.from_numpy(Xw[pick]).to(dev)               # the chained frame is the map's: sigma 1
    lms[:nmatch, 7] = torch.arange(nmatch, device=dev)
    nl = torch.full((1,), nmatch, dtype=torch.int32, device=dev)
    table = L.pose_table(4096, dev)
    table[:, 0], table[:, 4], table[:, 8] = 1.0, 1.0, 1.0
    table[:, 9] = 1e-3 * torch.arange(4096, device=dev)
    table[f, 9] = 0.0
    lp = L.loop_buffers(pcap, 4096, dev)
    buf = L.pnp_buffers(1, pcap, dev)
    kd = torch.from_numpy(kk[None]).to(dev)
    seed = torch.full((1,), 5, dtype=torch.int64, device=dev)
    det = {"rows": nmatch, "map_rows": n_map}
    for name, col in (("revisit", last), ("idle", np.full(n_map, f - 3, dtype=np.int32))):
        w["last_frame"].copy_(torch.from_numpy(col).to(dev))
        lp["state"].zero_()
        join = lambda _: L.op_loop_correspondences(w, match, nmt, pts, nmt, lms, nl, f, gap, lp)
        pnp = lambda _: L.op_pnp_ransac(lp["corr"], lp["n"][0:1], kd, seed, thresh=2.0, min_inliers=12, out=buf)
        edge = lambda _: L.op_loop_edge(w, buf, table, f, lp, 12, 32, 1.0)
        join(0), pnp(0), edge(0)
        torch.cuda.synchronize()
        det[name] = {"n": lp["n"].cpu().tolist(), "status": int(buf["status"][0]), "n_inliers": int(buf["n_inliers"][0]),
                     "cand": [round(x, 6) for x in lp["cand"][:9].cpu().tolist()], "join_us": window(join), "pnp_us": window(pnp),
                     "edge_us": window(edge)}
        det[name]["total_us"] = round(sum(det[name][k]["us"] for k in ("join_us", "pnp_us", "edge_us")), 2)
    res["detection"] = det

    # apply: 65 536 map rows, rows 2 .. 4095
    lp["state"].zero_()
    lp["state"][4], lp["state"][5] = 1, 1
    lp["info"].zero_()
    lp["Rw"].copy_(table[:, 0:9])
    lp["C"].copy_(table[:, 9:12])
    lp["sigma"].fill_(1.0)
    w["last_frame"].copy_(torch.from_numpy(rng.randint(0, 4096, n_map).astype(np.int32)).to(dev))
    st = L.pose_state(dev)
    res["apply"] = {"map_rows": n_map, "rows": 4094, "us": window(lambda _: L.op_loop_apply(w, st, table, 4095, lp))}
    del w, lp

    # the pose graph
    graphs = []
    for m in args.nodes:
        for n_inner in (0, 8):
            truth, tab, edges, state, fr = G.graph_case(m, n_inner, capacity=max(m + 3, 8))
            lp = L.loop_buffers(4, tab.shape[0], dev)
            lp["edges"].copy_(torch.from_numpy(edges).to(dev))
            lp["state"].copy_(torch.from_numpy(state).to(dev))
            td = torch.from_numpy(tab).to(dev)
            L.op_pose_graph(td, fr, lp, args.iterations)
            torch.cuda.synchronize()
            row = {"nodes": m, "inner_edges": n_inner, "iterations": args.iterations, "info": lp["info"].cpu().tolist(),
                   "device_us": window(lambda _: L.op_pose_graph(td, fr, lp, args.iterations), steps=max(1, min(args.steps, 4)))}
            if not args.no_host:
                t0 = time.perf_counter()
                want = G.pose_graph(tab, edges, state, fr, args.iterations)
                row["host_restatement_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
                row["host_over_device"] = round(1e3 * row["host_restatement_ms"] / row["device_us"]["us"], 1)
                row["centres_against_restatement"] = float(np.abs(lp["C"].cpu().numpy() - want[1]).max())
            graphs.append(row)
            del lp
    res["pose_graph"] = graphs

    H, W = args.height, args.width
    net = getattr(models, ARCH)()
    net.load_state_dict({k: torch.as_tensor(np.array(v)) for k, v in C.init_state_dict(ARCH, seed=21).items()})
    net = net.to(dev).eval()
    big = torch.from_numpy(np.random.RandomState(5).uniform(0, 1, (H, W + 16)).astype(np.float32)).to(dev)
    ims = [big[:, 2 * k:2 * k + W].contiguous() for k in range(8)]
    step = {"height": H, "width": W}
    for mode in (None, "observe", "apply", None):
        seq = SequenceTracker(net, dev, conf_thresh=0.0155, nms_dist=4, subpixel=True, nn_thresh=0.7, max_length=5,
                              geometric_check="fundamental", intrinsics=(0.9 * W, 0.9 * W, W / 2.0, H / 2.0), world_map="observe",
                              loop_closure=mode)
        key = str(mode) if str(mode) not in step else str(mode) + "_again"
        step[key] = window(lambda k: seq.step(ims[k % len(ims)]))
        if mode is not None:
            g = seq.tracker.last_geometry()
            step["%s_loop" % mode] = {"n": g["loop_n_corr"].cpu().tolist(), "state": g["loop_state"].cpu().tolist()}
    step["observe_share_us"] = round(step["observe"]["us"] - step["None"]["us"], 2)
    step["apply_share_us"] = round(step["apply"]["us"] - step["None"]["us"], 2)
    step["off_spread_us"] = round(abs(step["None_again"]["us"] - step["None"]["us"]), 2)
    res["sequence_step_us"] = step
    clock1 = L.clock_probe(5.0)
    res["gpu_clock_mhz"] = None if clock0 is None else {"before": round(clock0, 1), "after": round(clock1, 1)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
