"""numpy restatement of the semantic-keypoint operators, pinned to the rules the project already
states: the x8 align_corners=False bilinear upsample and first-occurrence arg-max of section 16 evaluated at points, a stable
class filter, and nn_match_two_way (section 15's matcher) with the pairs of unequal class masked out.  Everything is fp64."""
import numpy as np

CLASS_NONE = 255


def _axis(dst, in_size):
    """PyTorch's area_pixel_compute_source_index at scale 1/8, align_corners=False: (i0, i1, weight of i1)."""
    src = max((dst + 0.5) / 8.0 - 0.5, 0.0)
    i0 = min(int(np.floor(src)), in_size - 1)
    i1 = min(i0 + 1, in_size - 1)
    return i0, i1, src - i0


def logits_at(sout, k, x, y):
    """fp64 upsampled logits [C] of image k at pixel (y, x); sout [B,C,Hc,Wc]."""
    s = np.asarray(sout, dtype=np.float64)
    y0, y1, wy = _axis(int(y), s.shape[2])
    x0, x1, wx = _axis(int(x), s.shape[3])
    return ((1 - wy) * ((1 - wx) * s[k, :, y0, x0] + wx * s[k, :, y0, x1])
            + wy * ((1 - wx) * s[k, :, y1, x0] + wx * s[k, :, y1, x1]))


def point_classes(sout, pts, count, n_classes=None):
    """sout [B,C,Hc,Wc], pts [B,cap,>=2] rows starting (x, y), count [B] -> uint8 [B,cap]: np.argmax (first occurrence) of the
    fp64 logits over the first n_classes channels at the rows below the count (clamped to cap), CLASS_NONE past it.  Points
    outside the image are clamped into it."""
    sout, pts = np.asarray(sout), np.asarray(pts)
    B, C, Hc, Wc = sout.shape
    C = C if n_classes is None else n_classes
    cap = pts.shape[1]
    out = np.full((B, cap), CLASS_NONE, dtype=np.uint8)
    for k in range(B):
        for r in range(min(max(int(count[k]), 0), cap)):
            x = min(max(int(pts[k, r, 0]), 0), 8 * Wc - 1)
            y = min(max(int(pts[k, r, 1]), 0), 8 * Hc - 1)
            out[k, r] = np.argmax(logits_at(sout, k, x, y)[:C])
    return out


def mask_bits(mask):
    """eight 32-bit words -> bool [256]"""
    return np.array([(int(mask[c >> 5]) >> (c & 31)) & 1 for c in range(256)], dtype=bool)


def filter_points(pts, count, desc, cls, mask):
    """Stable per-image filter: the rows below the count whose class bit is set, in their order.  Returns (pts, count, desc,
    cls) of the input shapes; rows past the new count are zero (CLASS_NONE in cls)."""
    pts, desc, cls = np.asarray(pts), np.asarray(desc), np.asarray(cls)
    keep_bit = mask_bits(mask)
    po, do = np.zeros_like(pts), np.zeros_like(desc)
    co = np.full_like(cls, CLASS_NONE)
    no = np.zeros(len(count), dtype=np.int32)
    for k in range(pts.shape[0]):
        n = min(max(int(count[k]), 0), pts.shape[1])
        rows = [r for r in range(n) if keep_bit[cls[k, r]]]
        no[k] = len(rows)
        po[k, :len(rows)], do[k, :len(rows)], co[k, :len(rows)] = pts[k, rows], desc[k, rows], cls[k, rows]
    return po, no, do, co


def distances(d1, d2):
    """fp64 nn_match_two_way distances of unit rows d1 [N1,D], d2 [N2,D]"""
    dm = np.asarray(d1, dtype=np.float64) @ np.asarray(d2, dtype=np.float64).T
    return np.sqrt(2.0 - 2.0 * np.clip(dm, -1.0, 1.0))


def match_two_way_classes(d1, d2, c1, c2, nn_thresh):
    """Masked mutual nearest neighbour: the pairs with c1[i] != c2[j] are no candidates (distance +inf); a row or column
    without a candidate has no match; np.argmin ties (first index); keep = d < nn_thresh and mutual.  Returns float64 [M,3]
    rows (i, j, d) in ascending i."""
    n1, n2 = len(d1), len(d2)
    if n1 == 0 or n2 == 0:
        return np.zeros((0, 3))
    d = distances(d1, d2)
    d[np.asarray(c1)[:, None] != np.asarray(c2)[None, :]] = np.inf
    out = []
    for i in range(n1):
        if not np.isfinite(d[i]).any():
            continue
        j = int(np.argmin(d[i]))
        if d[i, j] < nn_thresh and int(np.argmin(d[:, j])) == i:
            out.append((i, j, d[i, j]))
    return np.array(out, dtype=np.float64).reshape(-1, 3)


def best_second_gaps(d1, d2, c1, c2):
    """Smallest gap between the best and the second-best candidate over all rows and columns that have two candidates (the
    masked fp64 distances): the margin by which the restatement's arg-mins are decided."""
    d = distances(d1, d2)
    d[np.asarray(c1)[:, None] != np.asarray(c2)[None, :]] = np.inf
    worst = np.inf
    for m in (d, d.T):
        s = np.sort(m, axis=1)
        two = np.isfinite(s[:, 1]) if s.shape[1] > 1 else np.zeros(len(s), dtype=bool)
        if two.any():
            worst = min(worst, float((s[two, 1] - s[two, 0]).min()))
    return worst


def unit_rows(rng, n, dim=256):
    d = rng.standard_normal((n, dim)).astype(np.float32)
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
