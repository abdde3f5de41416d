"""Inputs of the G15 fixtures, regenerated from the stored seeds (shared by tools/make_golden_descriptor.py and the tests).

descriptor_case_images(seed) returns the image pair of g15_descriptor_ssp_120x160.npz.  Each match case is
(name, seed, n1, n2, nn_thresh); match_case_inputs() returns the two float32 descriptor sets [256, N] (unit columns) the
reference's PointTracker.nn_match_two_way saw."""
import numpy as np

DESC_H, DESC_W = 120, 160
DESC_SHIFT = (3, 2)  # the warped image: the image translated by (dx, dy) pixels, fresh noise where it enters


def descriptor_case_images(seed):
    """(image, warped_image, homography) of the descriptor case: uniform noise, the warped image translated by DESC_SHIFT."""
    dx, dy = DESC_SHIFT
    rs = np.random.RandomState(1500 + seed)
    big = rs.uniform(0, 1, (DESC_H + dy, DESC_W + dx)).astype(np.float32)
    img = big[dy:, dx:].copy()
    warped = big[:DESC_H, :DESC_W].copy()  # warped(x, y) = img(x - dx, y - dy)
    hom = np.array([[1, 0, dx], [0, 1, dy], [0, 0, 1]], np.float64)
    return img, warped, hom

# (name, seed, n1, n2, nn_thresh)
MATCH_CASES = (
    ("large", 1501, 700, 900, 0.7),   # ~700 x 900 at D = 256, noisy copies + distractors
    ("dup", 1502, 300, 240, 1.0),     # exact duplicate rows on both sides: first-index ties
    ("clip", 1503, 200, 200, 0.7),    # identical unit vectors: the dot rounds above 1, the clip gives d = 0
    ("thresh", 1504, 400, 400, 0.9),  # scores spread across nn_thresh
    ("empty1", 1505, 0, 50, 0.7),     # an empty side
    ("empty2", 1506, 50, 0, 0.7),
    ("cap", 1507, 2048, 2048, 0.8),   # the largest pair the exporter meets at 240x320 with top-k 2048
)


def _unit(a):
    a = a.astype(np.float32)
    return (a / np.linalg.norm(a, axis=0, keepdims=True)).astype(np.float32)


def match_case_inputs(name, seed, n1, n2):
    rs = np.random.RandomState(seed)
    if n1 == 0 or n2 == 0:
        return np.zeros((256, n1), np.float32), np.zeros((256, n2), np.float32)
    d1 = _unit(rs.randn(256, n1))
    if name == "dup":
        d2 = _unit(rs.randn(256, n2))
        src = rs.choice(n1, n2 // 2, replace=False)
        d2[:, : n2 // 2] = _unit(d1[:, src] + 0.02 * rs.randn(256, n2 // 2))
        for a, b in ((3, 17), (5, 40), (8, 9), (60, 61)):     # duplicate columns of d2: d1 rows tie between them
            d2[:, b] = d2[:, a]
        for a, b in ((2, 100), (7, 8), (30, 250)):             # duplicate columns of d1: d2 columns tie between them
            d1[:, b] = d1[:, a]
        return d1, d2
    if name == "clip":
        d2 = _unit(rs.randn(256, n2))
        d2[:, : n2 // 2] = d1[:, rs.permutation(n1)[: n2 // 2]]
        return d1, d2
    if name == "thresh":
        d2 = _unit(rs.randn(256, n2))
        m = min(n1, n2) * 3 // 4
        noise = rs.uniform(0.2, 1.0, size=(1, m))          # spreads the matched distances across the threshold
        d2[:, :m] = _unit(d1[:, :m] + noise * rs.randn(256, m) / 16.0 * 1.5)
        return d1, d2[:, rs.permutation(n2)]
    # "large", "cap": noisy copies of a subset plus distractors
    d2 = _unit(rs.randn(256, n2))
    m = min(n1, n2) // 2
    src = rs.choice(n1, m, replace=False)
    dst = rs.choice(n2, m, replace=False)
    d2[:, dst] = _unit(d1[:, src] + 0.05 * rs.randn(256, m))
    return d1, d2


def ambiguous_rows(d1, d2, nn_thresh, eps=1e-5):
    """Rows i of d1 whose match the reference may decide by its BLAS summation order: the best and second-best fp64
    distances of row i (or of the column that row i picks, over d1) differ by < eps, or the best distance lies within eps of
    nn_thresh.  Exact duplicate columns / rows tie in every summation order and count once."""
    n1, n2 = d1.shape[1], d2.shape[1]
    if n1 == 0 or n2 == 0:
        return np.zeros(n1, bool)

    def dist(a, b):
        return np.sqrt(np.maximum(2 - 2 * np.clip(a.astype(np.float64).T @ b.astype(np.float64), -1, 1), 0))

    def margin(m, ax):
        if m.shape[ax] < 2:
            return np.full(m.shape[1 - ax], np.inf)
        s = np.sort(m, axis=ax)
        return np.take(s, 1, axis=ax) - np.take(s, 0, axis=ax)

    dm = dist(d1, d2)
    row_m = margin(dist(d1, np.unique(d2, axis=1)), 1)
    col_m = margin(dist(np.unique(d1, axis=1), d2), 0)
    best_j = np.argmin(dm, axis=1)
    best = dm[np.arange(n1), best_j]
    return (row_m < eps) | (col_m[best_j] < eps) | (np.abs(best - nn_thresh) < eps)
