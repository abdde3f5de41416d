"""Semantic-keypoint benchmark: one JSON line for Semantic-SuperPoint at 240x320 with the keypoints of
Engine.describe_points at the threshold bench_tracks.py uses (about 1000 per image), two images (a frame and the next one).

  point_classes_us        Engine.point_classes: the class of every keypoint straight from the coarse logits
  classes_composition_us  what a user had to write before: Engine.sem_predict's class map + the gather pred[k, y, x]
  filter_us               lib.op_filter_points (drop the most frequent class), no host synchronisation
  filter_torch_us         torch boolean indexing of pts / desc / cls per image, which has to learn the new count on the host
  match_classes_us        lib.op_match_two_way with cls1 / cls2 (ssp_match_two_way_classes), frame against next frame
  match_plain_us          lib.op_match_two_way on the same descriptors

Every figure is the host clock around `--steps` back-to-back calls that end in a device synchronise, per call, median over
`--repeats` windows after `--warmup` calls (min and max give the spread).  There is no CPU baseline: the operators run on the
device only."""
import argparse
import json
import statistics
import time

ARCH = "SuperPointNet_gauss2_ssmall"


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--height", type=int, default=240)
    ap.add_argument("--width", type=int, default=320)
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    from oracle import cpu_ref as C
    from semantic_superpoint_amd import lib as L
    if not torch.cuda.is_available():
        raise SystemExit("bench_point_classes.py measures on the GPU: no HIP device found")
    dev, B, H, W, NC = torch.device("cuda:0"), 2, args.height, args.width, 133

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        us = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            for _ in range(args.steps):
                fn()
            torch.cuda.synchronize()
            us.append(1e6 * (time.perf_counter() - t0) / args.steps)
        return {"us": round(statistics.median(us), 2), "min": round(min(us), 2), "max": round(max(us), 2)}

    eng = L.Engine(ARCH, B, H, W, dev, with_grad=False)
    eng.load_state_dict(C.init_state_dict(ARCH, seed=21))   # untrained weights, as in bench_tracks.py
    big = torch.from_numpy(np.random.RandomState(5).uniform(0, 1, (H, W + 16)).astype(np.float32))
    x = torch.stack([big[:, 0:W], big[:, 2:2 + W]])[:, None].contiguous().to(dev)   # a frame and the same scene 2 px on
    clock0 = L.clock_probe(5.0)
    eng.forward(x, slot=0, train=False, want=())
    o = eng.describe_points(0, B, conf_thresh=0.0155, nms_dist=4, subpixel=True, classes=True)
    pts, count, desc, cls = o["pts"], o["count"], o["desc"], o["cls"]
    counts = count.cpu().tolist()
    cap = pts.shape[1]
    res = {"bench": "point_classes", "arch": ARCH, "images": B, "height": H, "width": W, "n_classes": NC, "cap": cap,
           "points": counts, "build_id": L.build_id()[:16], "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats,
           "cpu_baseline": None}

    # (i) classes at points
    def compose_classes():
        pred, _ = eng.sem_predict(0, B, H, W)
        xy = pts[:, :, :2].long()
        # (rows past the count are uninitialised: clamped so that the gather stays inside the map)
        return torch.gather(pred.view(B, H * W), 1, xy[:, :, 1].clamp(0, H - 1) * W + xy[:, :, 0].clamp(0, W - 1))
    got = compose_classes()
    same = all(torch.equal(cls[k, :counts[k]], got[k, :counts[k]]) for k in range(B))
    res["classes_equal_composition"] = bool(same)
    res["classes_at_points"] = int(torch.unique(torch.cat([cls[k, :counts[k]] for k in range(B)])).numel())
    res["point_classes_us"] = timed(lambda: eng.point_classes(0, pts, count))
    res["classes_composition_us"] = timed(compose_classes)

    # (ii) the filter: drop the most frequent class
    flat = torch.cat([cls[k, :counts[k]] for k in range(B)]).long()
    top = int(torch.bincount(flat, minlength=NC).argmax())
    mask = L.class_mask(drop=[top], n_classes=NC)
    rows = torch.arange(cap, device=dev)

    def filter_torch():
        out = []
        for k in range(B):
            keep = (cls[k] != top) & (rows < count[k])
            out.append((pts[k][keep], desc[k][keep], cls[k][keep]))   # the new count is the shape: a host synchronisation each
        return out
    f = L.op_filter_points(pts, count, desc, cls, mask)
    ft = filter_torch()
    new = f["count"].cpu().tolist()
    res["filter_dropped_class"] = top
    res["filter_points_kept"] = new
    res["filter_equal_torch"] = bool(all(new[k] == ft[k][0].shape[0] and torch.equal(f["pts"][k, :new[k]], ft[k][0])
                                         and torch.equal(f["desc"][k, :new[k]], ft[k][1]) for k in range(B)))
    res["filter_us"] = timed(lambda: L.op_filter_points(pts, count, desc, cls, mask))
    res["filter_torch_us"] = timed(filter_torch)

    # (iii) the matcher: frame 0 against frame 1 (alternating windows would need two processes; the two are timed back to back, twice)
    d1, c1, d2, c2 = desc[0:1], count[0:1], desc[1:2], count[1:2]
    k1, k2 = cls[0:1].contiguous(), cls[1:2].contiguous()
    m_p, n_p = L.op_match_two_way(d1, c1, d2, c2, 0.7)
    m_c, n_c = L.op_match_two_way(d1, c1, d2, c2, 0.7, cls1=k1, cls2=k2)
    m_s, n_s = L.op_match_two_way(d1, c1, d2, c2, 0.7, cls1=torch.zeros_like(k1), cls2=torch.zeros_like(k2))
    res["matches_plain"], res["matches_classes"] = int(n_p[0]), int(n_c[0])
    res["match_equal_classes_is_plain"] = bool(torch.equal(n_s, n_p) and torch.equal(m_s[0, :int(n_p[0])], m_p[0, :int(n_p[0])]))
    plain = lambda: L.op_match_two_way(d1, c1, d2, c2, 0.7)  # noqa: E731
    classes = lambda: L.op_match_two_way(d1, c1, d2, c2, 0.7, cls1=k1, cls2=k2)  # noqa: E731
    res["match_plain_us"], res["match_classes_us"] = timed(plain), timed(classes)
    res["match_plain_again_us"], res["match_classes_again_us"] = timed(plain), timed(classes)
    clock1 = L.clock_probe(5.0)
    res["gpu_clock_mhz"] = None if clock0 is None else {"before": round(clock0, 1), "after": round(clock1, 1)}
    res["classes_speedup"] = round(res["classes_composition_us"]["us"] / res["point_classes_us"]["us"], 2)
    res["filter_speedup"] = round(res["filter_torch_us"]["us"] / res["filter_us"]["us"], 2)
    res["match_classes_over_plain"] = round(res["match_classes_us"]["us"] / res["match_plain_us"]["us"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
