"""Inputs of the G20 detector-evaluation fixture (shared by tools/make_golden_detector_eval.py, the tests and
bench_detector_eval.py): image sets regenerated from fixed seeds, pinned by a checksum the fixture stores.

A set is a list of images (prob float32 [H,W], prob_nms float32 [H,W], keypoint_map uint8 [H,W]): about 300 pixels above
remove_zero and about 30 ground-truth pixels each.  prob_nms keeps the 3x3 local maxima of prob (a stand-in for the exporter's
NMS: the `prob_nms` entry of the reference's files).  The generator makes the reference's undefined orders irrelevant: every
nonzero probability is unique across a set, and none lies within 4 ulp of remove_zero or prob_thresh."""
import numpy as np

REMOVE_ZERO, PROB_THRESH = 1e-4, 0.5
SETS = {"A": dict(seed=2001, n=6, H=24, W=32), "B": dict(seed=2002, n=4, H=23, W=37)}  # B: odd sizes
VARIANTS = ("dense", "nms")
SIMPLIFIED = (False, True)
DISTANCE_THRESH = (2, 3)


def _near(v, t):
    """float32 values within 4 ulp of float32(t)."""
    t = np.float32(t)
    lo = hi = t
    for _ in range(4):
        lo, hi = np.nextafter(lo, np.float32(0)), np.nextafter(hi, np.float32(2))
    return (v >= lo) & (v <= hi)


def make_set(name):
    spec = SETS[name]
    rs = np.random.RandomState(spec["seed"])
    n, H, W = spec["n"], spec["H"], spec["W"]
    prob = (rs.random_sample((n, H, W)) ** 6).astype(np.float32)
    prob[rs.random_sample((n, H, W)) < 0.5] = 0
    while True:  # redraw duplicates and values next to a threshold
        flat = prob.reshape(-1)
        nz = np.flatnonzero(flat)
        _, first, cnt = np.unique(flat[nz], return_index=True, return_counts=True)
        dup = np.ones(len(nz), bool)
        dup[first[cnt == 1]] = False
        bad = nz[dup | _near(flat[nz], REMOVE_ZERO) | _near(flat[nz], PROB_THRESH)]
        if not len(bad):
            break
        flat[bad] = (rs.random_sample(len(bad)) ** 6).astype(np.float32) + np.float32(1e-3)
    kp = (rs.random_sample((n, H, W)) < 0.04).astype(np.uint8)
    pad = np.pad(prob, ((0, 0), (1, 1), (1, 1)))
    neigh = np.max([pad[:, dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)], axis=0)
    prob_nms = np.where(prob >= neigh, prob, np.float32(0)).astype(np.float32)
    return [(prob[i], prob_nms[i], kp[i]) for i in range(n)]


def checksum(images):
    """float64 [3]: pins the regenerated inputs."""
    p = np.stack([im[0] for im in images]).astype(np.float64)
    q = np.stack([im[1] for im in images]).astype(np.float64)
    k = np.stack([im[2] for im in images]).astype(np.float64)
    w = 1.0 + np.arange(p.size).reshape(p.shape) % 97
    return np.array([(p * w).sum(), (q * w).sum(), (k * w).sum()])


def point_list(prob_nms, cap=None):
    """The exporter's point-list form of a sparse map: rows (x, y, confidence, 2, 2) in descending confidence, count."""
    ys, xs = np.nonzero(prob_nms)
    o = np.argsort(-prob_nms[ys, xs], kind="stable")
    rows = np.stack([xs[o], ys[o], prob_nms[ys, xs][o], np.full(len(o), 2), np.full(len(o), 2)], axis=-1).astype(np.float32)
    if cap is not None:
        out = np.zeros((cap, 5), np.float32)
        out[:len(rows)] = rows
        return out, len(rows)
    return rows, len(rows)


def case_key(name, variant, simplified=None, dt=None):
    k = "%s/%s" % (name, variant)
    if simplified is not None:
        k += "/s%d" % int(simplified)
    if dt is not None:
        k += "/d%d" % dt
    return k
