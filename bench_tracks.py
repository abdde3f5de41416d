"""Point-track benchmark: one JSON line.

  update_device_L5_us / _L2_us   PointTracker.update_device per frame (match + track update, no host copy) at `--points` points
                                 per frame with 40 % of them continuing, max_length 5 and 2, with its split: match_us
                                 (ssp_match_two_way) and tracks_us (ssp_op_track_update)
  numpy_update_L5_us / _L2_us    tests/tracks_ref.update on the SAME matches (host wall clock): the comparison target, because
                                 there was no device track path before
  sequence_step_us               SequenceTracker.step at `--height` x `--width` on a shifted noise image, and its split: forward
                                 (eval forward of one image), describe (ssp_describe_points), match, tracks

Device times are between two HIP events around `--steps` back-to-back frames, median over `--repeats` windows after `--warmup`
frames; the frames cycle through a pre-uploaded sequence so that the table is in its steady state.  The clock probe before and
after reports the clock the device grants."""
import argparse
import json
import statistics
import time

ARCH = "SuperPointNet_gauss2_ssmall"


def make_frames(n_points, n_frames, keep, seed):
    """[(xy float64 [n,2], desc float32 [n,256])]: every frame continues `keep` of the previous frame's points (descriptor
    rotated to a distance of 0.06-0.49), the rest are fresh unit vectors."""
    import numpy as np
    from tests.golden_tracks import rotated, unit32
    rs = np.random.RandomState(seed)
    out, prev = [], None
    for _ in range(n_frames):
        d = rs.randn(256, n_points)
        d /= np.linalg.norm(d, axis=0, keepdims=True)
        if prev is not None:
            k = int(keep * n_points)
            dst, src = rs.permutation(n_points)[:k], rs.permutation(n_points)[:k]
            d[:, dst] = rotated(rs, prev[:, src].astype(np.float64), 0.06, 0.49)
        d = unit32(d)
        out.append((rs.uniform(4, 300, (n_points, 2)), np.ascontiguousarray(d.T)))
        prev = d
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--points", type=int, default=1000)
    ap.add_argument("--height", type=int, default=240)
    ap.add_argument("--width", type=int, default=320)
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    from oracle import cpu_ref as C
    from semantic_superpoint_amd import lib as L
    from semantic_superpoint_amd import models
    from semantic_superpoint_amd.export import PointTracker, SequenceTracker
    from tests import tracks_ref as TR
    if not torch.cuda.is_available():
        raise SystemExit("bench_tracks.py measures on the GPU: no HIP device found")
    dev = torch.device("cuda:0")
    N = args.points

    def window(frame_fn, frames):
        """median device microseconds per frame of frame_fn(k) over the cycling frame index k"""
        k = 0
        for _ in range(args.warmup):
            frame_fn(k % frames)
            k += 1
        torch.cuda.synchronize()
        us = []
        for _ in range(args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.steps):
                frame_fn(k % frames)
                k += 1
            b.record()
            torch.cuda.synchronize()
            us.append(1e3 * a.elapsed_time(b) / args.steps)
        return {"us": round(statistics.median(us), 2), "min": round(min(us), 2), "max": round(max(us), 2)}

    res = {"bench": "tracks", "points": N, "keep": 0.4, "build_id": L.build_id()[:16], "steps": args.steps, "warmup": args.warmup,
           "repeats": args.repeats}
    clock0 = L.clock_probe(5.0)
    frames = make_frames(N, 8, 0.4, 1950)
    cnt = torch.tensor([N], dtype=torch.int32, device=dev)
    up = [(torch.from_numpy(xy).to(dev), torch.from_numpy(d).to(dev)) for xy, d in frames]
    def match(k0, k1):
        return L.op_match_two_way(up[k0][1][None], cnt, up[k1][1][None], cnt, 0.7)

    for ml in (5, 2):
        t = PointTracker(ml, 0.7, dev)
        res["update_device_L%d_us" % ml] = window(lambda k: t.update_device(up[k][0], cnt, up[k][1]), len(up))
        res["rows_L%d" % ml] = int(t.tracks.shape[0])
        # the split: a table that holds frames 0-6 and the matches of frame 7 against frame 6, pushed again and again
        t3 = PointTracker(ml, 0.7, dev)
        for xy, d in up[:7]:
            t3.update_device(xy, cnt, d)
        m, nm = match(6, 7)
        res["update_device_L%d_us" % ml]["match_us"] = window(lambda k: match(6, 7), 1)["us"]
        spare = L.track_table(ml, t3.table["point_cap"], dev)
        mm = torch.zeros(t3.table["point_cap"], 3, dtype=torch.float32, device=dev)
        mm[:N] = m[0]
        res["update_device_L%d_us" % ml]["tracks_us"] = window(
            lambda k: L.op_track_update(t3.table, mm, nm, cnt, out=spare), 1)["us"]
        # the host restatement on the same matches, frame by frame (wall clock, steady state after one pass)
        t2 = PointTracker(ml, 0.7, dev)
        matches = []
        for f in range(2 * len(up)):
            k = f % len(up)
            t2.update_device(up[k][0], cnt, up[k][1])
            if f:
                mf, nf = match((k - 1) % len(up), k)
                matches.append(mf[0, :int(nf.item())].cpu().numpy().astype(np.float64).T.copy())
            else:
                matches.append(np.zeros((3, 0)))
        ref = TR.Tracks(ml)
        for mt in matches[:len(up)]:
            TR.update(ref, N, mt)
        t0 = time.perf_counter()
        for mt in matches[len(up):]:
            TR.update(ref, N, mt)
        host_us = 1e6 * (time.perf_counter() - t0) / len(up)
        res["numpy_update_L%d_us" % ml] = round(host_us, 1)
        same = np.array_equal(ref.matrix()[:, [0] + list(range(2, ml + 2))], t2.tracks[:, [0] + list(range(2, ml + 2))])
        res["same_table_L%d" % ml] = bool(same)
        res["numpy_over_device_tracks_L%d" % ml] = round(host_us / res["update_device_L%d_us" % ml]["tracks_us"], 1)

    # SequenceTracker.step and its split
    H, W = args.height, args.width
    net = getattr(models, ARCH)()
    net.load_state_dict({k: torch.as_tensor(np.array(v)) for k, v in C.init_state_dict(ARCH, seed=21).items()})
    net = net.to(dev).eval()
    seq = SequenceTracker(net, dev, conf_thresh=0.0155, nms_dist=4, subpixel=True, nn_thresh=0.7, max_length=5)
    big = torch.from_numpy(np.random.RandomState(5).uniform(0, 1, (H, W + 16)).astype(np.float32)).to(dev)
    ims = [big[:, 2 * k:2 * k + W].contiguous() for k in range(8)]
    step = window(lambda k: seq.step(ims[k]), len(ims))
    x = ims[0][None, None].contiguous()
    eng = net.engine(1, H, W, dev)

    def fwd(k):
        with torch.no_grad():
            eng.forward(x, slot=0, train=False, want=())
    step["forward_us"] = window(fwd, 1)["us"]
    step["describe_us"] = window(lambda k: eng.describe_points(0, 1, conf_thresh=0.0155, nms_dist=4, subpixel=True), 1)["us"]
    # the split of match and tracks: the table holds ims[0] as its newest frame, the matches are those of ims[1] against it
    tr = seq.tracker
    prev = {k: v.clone() for k, v in seq.step(ims[0]).items() if k in ("desc", "count")}
    cur = {k: v.clone() for k, v in seq.describe(ims[1]).items() if k in ("desc", "count")}

    def seq_match():
        return L.op_match_two_way(prev["desc"], prev["count"], cur["desc"], cur["count"], 0.7)
    m, nm = seq_match()
    step["match_us"] = window(lambda k: seq_match(), 1)["us"]
    pc = tr.table["point_cap"]
    spare = L.track_table(5, pc, dev)
    mm = torch.zeros(max(pc, m.shape[1]), 3, dtype=torch.float32, device=dev)
    mm[:m.shape[1]] = m[0]
    c1 = cur["count"][0:1]
    step["tracks_us"] = window(lambda k: L.op_track_update(tr.table, mm, nm, c1, out=spare), 1)["us"]
    step["points_per_frame"] = int(c1.item())
    step["rows"] = int(tr.tracks.shape[0])
    step["height"], step["width"] = H, W
    res["sequence_step_us"] = step
    clock1 = L.clock_probe(5.0)
    res["gpu_clock_mhz"] = None if clock0 is None else {"before": round(clock0, 1), "after": round(clock1, 1)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
