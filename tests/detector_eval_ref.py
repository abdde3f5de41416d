"""numpy restatement of the detector evaluation (compute_tp_fp, compute_pr, compute_mAP, compute_loc_error), written from the
rules of DESIGN.md section 19.  tests/test_detector_eval_cpu.py pins it to the real reference's results (G20); the GPU tests use
it as the reference for inputs the fixture does not cover.

Rules.  Ground truth: the nonzero pixels of the label map, row-major.  Candidates: the pixels with prob > float32(remove_zero)
(or the rows of a point list with confidence above it), each at a position: its row-major pixel index (its list position).
A candidate matches when a ground-truth pixel lies within distance_thresh (integer offsets: d2 <= r2, r2 the largest integer
with sqrt(float64(r2)) <= distance_thresh); it is assigned to the FIRST such pixel in row-major order.  Order: descending
probability, among equals the later record first, i.e. np.argsort(kind="stable")[::-1]; a record's index is image order, then
position.  A candidate is a true positive iff it is the first, in that order, of the candidates assigned to its pixel.
simplified: tp = matched, n_gt = number of ground-truth pixels within range of some candidate (the reference's flag)."""
import numpy as np


def r2_of(distance_thresh):
    r2 = int(float(distance_thresh) ** 2) + 1
    while r2 >= 0 and not np.sqrt(np.float64(r2)) <= np.float64(distance_thresh):
        r2 -= 1
    return r2


def order_of(prob):
    """Descending probability, among equals the later record first."""
    return np.argsort(prob, kind="stable")[::-1]


def _records(yx, prob, keypoint_map, distance_thresh, simplified):
    """tp (in POSITION order) and n_gt for candidates yx int [n,2] with probabilities prob [n]."""
    gy, gx = np.nonzero(keypoint_map)
    gt = np.stack([gy, gx], axis=-1).astype(np.int64)
    n_gt = len(gt)
    d2 = ((yx[:, None, :].astype(np.int64) - gt[None, :, :]) ** 2).sum(-1)
    matches = d2 <= r2_of(distance_thresh)
    hit = matches.any(axis=1) if n_gt else np.zeros(len(yx), bool)
    if simplified:
        return hit, int(matches.any(axis=0).sum())
    g = matches.argmax(axis=1) if n_gt else np.zeros(len(yx), np.int64)
    tp = np.zeros(len(yx), bool)
    taken = set()
    for i in order_of(prob):
        if hit[i] and g[i] not in taken:
            taken.add(g[i])
            tp[i] = True
    return tp, n_gt


def candidates(prob_map, remove_zero=1e-4):
    ys, xs = np.nonzero(prob_map > np.float32(remove_zero))
    return np.stack([ys, xs], axis=-1), prob_map[ys, xs]


def point_candidates(pts, remove_zero=1e-4):
    """pts: rows (x, y, confidence, ..) in list order -> (yx, prob) of the rows above remove_zero."""
    pts = np.asarray(pts, np.float32).reshape(-1, pts.shape[-1])
    keep = pts[:, 2] > np.float32(remove_zero)
    return np.stack([pts[keep, 1], pts[keep, 0]], axis=-1).astype(np.int64), pts[keep, 2]


def tp_fp_records(yx, prob, keypoint_map, distance_thresh=2, simplified=False):
    """One image: (tp, prob) in position order and n_gt."""
    tp, n_gt = _records(yx, prob, keypoint_map, distance_thresh, simplified)
    return tp, prob, n_gt


def compute_tp_fp(prob_map, keypoint_map, remove_zero=1e-4, distance_thresh=2, simplified=False):
    """The reference's return value for one image: tp, fp, prob sorted in the stated order, n_gt."""
    yx, p = candidates(prob_map, remove_zero)
    tp, p, n_gt = tp_fp_records(yx, p, keypoint_map, distance_thresh, simplified)
    o = order_of(p)
    return tp[o], ~tp[o], p[o], n_gt


def compute_pr(records):
    """records: [(tp, prob, n_gt)] per image in image order, each in position order -> precision, recall [n+2], prob [n], tp [n].
    Record k of the sorted set (k = 1 .. n) has hits(k) true positives among the first k: precision k is hits / k, recall k
    is hits / n_gt, and for a set without ground truth 1 while hits is 0 and 0 after.  Element 0 and element n + 1 are the
    padding (recall 0 and 1, precision 0 and 0); every precision is then raised to the largest one at or to the right of it."""
    tp = np.zeros(0, bool)
    prob = np.zeros(0, np.float32)
    n_gt = 0
    for r in records:
        tp = np.append(tp, np.asarray(r[0], bool))
        prob = np.append(prob, np.asarray(r[1], np.float32))
        n_gt += int(r[2])
    o = order_of(prob)
    tp, prob = tp[o], prob[o]
    n = len(tp)
    hits = np.add.accumulate(tp.astype(np.int64)).astype(np.float64)
    recall = np.empty(n + 2, np.float64)
    precision = np.empty(n + 2, np.float64)
    recall[0], recall[n + 1] = 0.0, 1.0
    precision[0], precision[n + 1] = 0.0, 0.0
    recall[1:n + 1] = hits / np.float64(n_gt) if n_gt else (hits == 0).astype(np.float64)
    precision[1:n + 1] = hits / np.arange(1, n + 1, dtype=np.float64)
    for k in range(n, -1, -1):
        precision[k] = max(precision[k], precision[k + 1])
    return precision, recall, prob, tp


def compute_mAP(precision, recall):
    """The area under the padded curve: each recall step times the precision at its right end."""
    step = np.diff(np.asarray(recall, np.float64))
    return (np.asarray(precision, np.float64)[1:] * step).sum()


def loc_distances(yx, prob, keypoint_map, prob_thresh=0.5, distance_thresh=2):
    """One image: the distances to the nearest ground-truth pixel, of the candidates above prob_thresh, that are <= distance_thresh."""
    gy, gx = np.nonzero(keypoint_map)
    keep = prob > np.float32(prob_thresh)
    if not len(gy) or not keep.any():
        return np.zeros(0)
    gt = np.stack([gy, gx], axis=-1).astype(np.int64)
    d2 = ((yx[keep][:, None, :].astype(np.int64) - gt[None, :, :]) ** 2).sum(-1).min(axis=1)
    d = np.sqrt(d2.astype(np.float64))
    return d[d <= distance_thresh]


def compute_loc_error(images, prob_thresh=0.5, distance_thresh=2):
    """images: [(yx, prob, keypoint_map)] -> the mean of the kept distances (nan without any)."""
    d = [loc_distances(yx, p, kp, prob_thresh, distance_thresh) for yx, p, kp in images]
    d = np.concatenate(d) if d else np.zeros(0)
    return np.float64(np.nan) if not len(d) else np.mean(d)


def evaluate(images, remove_zero=1e-4, distance_thresh=2, prob_thresh=0.5, simplified=False):
    """images: [(prob_map, keypoint_map)] (dense) or [((pts,), keypoint_map)] with pts rows (x, y, confidence, ..) in a 1-tuple.
    Returns the dict DetectorEvaluator.result() returns, as numpy."""
    cand = []
    for src, kp in images:
        yx, p = point_candidates(src[0], remove_zero) if isinstance(src, tuple) else candidates(src, remove_zero)
        cand.append((yx, p, kp))
    recs = [tp_fp_records(yx, p, kp, distance_thresh, simplified) for yx, p, kp in cand]
    precision, recall, prob, tp = compute_pr(recs)
    return {"precision": precision, "recall": recall, "prob": prob, "tp": tp, "n_gt": sum(int(r[2]) for r in recs),
            "mAP": compute_mAP(precision, recall), "loc_error": compute_loc_error(cand, prob_thresh, distance_thresh)}
