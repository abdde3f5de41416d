"""numpy fp64 restatement of eval_repeat_kernel (csrc/eval_kernels.hip.h; DESIGN.md sections 13 and 34): the reference's
compute_repeatability (evaluations/detector_evaluation.py:153-275) and the matching score's unwarped-point count
(evaluation.py:194-216), written from their formulas.  No torch, nothing imported from the product.

Every product and every sum below is one rounded operation in the stated order (no np.dot: a BLAS with FMA rounds
differently), so the integer outputs can be compared with == and the two sums to the bound of their summation order.

`mutant` (tests/test_evaluation_ref_cpu.py only) switches one rule to a plausible wrong one; None is the restatement."""
import numpy as np

F = np.float64
MUTANTS = ("le_at_border", "topk_before_filter", "ties_high", "side2_warped", "lt_thresh", "minima_swapped",
           "count_unclamped", "stride_ignored", "round_unwarped", "wh_swapped")


def warp(M, x, y):
    """warp_keypoints (detector_evaluation.py:139-150): [x, y, 1] . M^T row by row as (x m0 + y m1) + m2, then the two
    divisions by the third row.  A zero third row gives inf or NaN, as numpy does."""
    M = np.asarray(M, F).reshape(9)
    x, y = np.asarray(x, F), np.asarray(y, F)
    w0 = (x * M[0] + y * M[1]) + M[2]
    w1 = (x * M[3] + y * M[4]) + M[5]
    w2 = (x * M[6] + y * M[7]) + M[8]
    with np.errstate(divide="ignore", invalid="ignore"):
        return w0 / w2, w1 / w2


def _inside(u, v, height, width, mutant):
    W, H = (F(height), F(width)) if mutant == "wh_swapped" else (F(width), F(height))
    with np.errstate(invalid="ignore"):
        if mutant == "le_at_border":
            return (u >= 0) & (u <= W) & (v >= 0) & (v <= H)
        return (u >= 0) & (u < W) & (v >= 0) & (v < H)


def _select(conf, inside, keep_k, mutant):
    """Indices of the keep_k most confident inside points, best first; ties to the lower index (a stable sort of the
    negated confidence: -0.0 and +0.0 tie)."""
    conf = np.asarray(conf, F)
    if mutant == "topk_before_filter":
        order = np.argsort(-conf, kind="stable")[:keep_k]
        return order[inside[order]]
    idx = np.nonzero(inside)[0]
    if mutant == "ties_high":
        return idx[::-1][np.argsort(-conf[idx[::-1]], kind="stable")[:keep_k]]
    return idx[np.argsort(-conf[idx], kind="stable")[:keep_k]]


def _border_margin(u, v, height, width):
    """Least non-zero distance of a finite u to 0 and W and of a finite v to 0 and H."""
    m = np.inf
    for a, lim in ((u, F(width)), (v, F(height))):
        a = a[np.isfinite(a)]
        for d in (np.abs(a), np.abs(a - lim)):
            d = d[d > 0]
            if d.size:
                m = min(m, float(d.min()))
    return m


def _minima(A, B, thresh, mutant):
    """For every row of A the least squared distance to a row of B, its root and the `<= thresh` decision.
    -> (count, the kept roots in row order, margin of the roots to thresh).  A root is exact by construction - and
    leaves the margin alone - when both points have integer coordinates and the squared distance is a perfect square
    (the 3-4-5 pairs: every operation up to the comparison is then exact in every order)."""
    if A.shape[0] == 0 or B.shape[0] == 0:
        return 0, np.zeros(0, F), np.inf
    dx = A[:, None, 0] - B[None, :, 0]
    dy = A[:, None, 1] - B[None, :, 1]
    d2 = dx * dx + dy * dy
    j = np.argmin(d2, axis=1)
    m2 = d2[np.arange(A.shape[0]), j]
    d = np.sqrt(m2)
    keep = d < thresh if mutant == "lt_thresh" else d <= thresh
    ints = np.all(A == np.floor(A), axis=1) & np.all(B[j] == np.floor(B[j]), axis=1)
    exact = ints & (np.floor(d) == d)
    gap = np.abs(d - F(thresh))[~exact]
    gap = gap[gap > 0]
    return int(keep.sum()), d[keep], float(gap.min()) if gap.size else np.inf


def unwarped_count(p2, H_inv, height, width, mutant=None):
    """The matching score's count (evaluation.py:194-216): warped_prob[:, [1, 0]] truncated to integers (.long()),
    warped by float32(inv(H)) as if it were (x, y), kept when 0 <= p <= [W, H] - 1.  float32 throughout."""
    f = np.float32
    Fm = np.asarray(H_inv, F).reshape(9).astype(f)
    p2 = np.asarray(p2, F).reshape(-1, 3)
    cut = np.rint if mutant == "round_unwarped" else np.trunc
    a, b = cut(p2[:, 1]).astype(f), cut(p2[:, 0]).astype(f)
    with np.errstate(divide="ignore", invalid="ignore"):
        w0 = (Fm[0] * a + Fm[1] * b) + Fm[2]
        w1 = (Fm[3] * a + Fm[4] * b) + Fm[5]
        w2 = (Fm[6] * a + Fm[7] * b) + Fm[8]
        u, v = w0 / w2, w1 / w2
        wm1, hm1 = f(width) - f(1), f(height) - f(1)
        if mutant == "wh_swapped":
            wm1, hm1 = hm1, wm1
        return int(np.sum((u >= 0) & (u <= wm1) & (v >= 0) & (v <= hm1)))


def seq_sum(d):
    """One rounded addition per term, in order, from 0.0."""
    s = F(0.0)
    for t in d:
        s = s + t
    return s


def repeatability(p1, p2, H, H_inv, height, width, keep_k, thresh, mutant=None):
    """p1 / p2: [n,3] rows (x, y, confidence) of the image / of the warped image.
    -> (N1, N2, count1, count2, sum1, sum2, n_unwarped, margin); margin: the smallest decision margin in pixels (the
    least non-zero distance of a warped coordinate to 0, W, H and of a kept minimum distance to thresh; inf when no
    decision is open)."""
    p1, p2 = np.asarray(p1, F).reshape(-1, 3), np.asarray(p2, F).reshape(-1, 3)
    thresh = F(thresh)
    # side 1: the image's points warped by H, filtered, the keep_k best (select_k_best runs AFTER the filter)
    u1, v1 = warp(H, p1[:, 0], p1[:, 1])
    k1 = _select(p1[:, 2], _inside(u1, v1, height, width, mutant), keep_k, mutant)
    A = np.stack([u1[k1], v1[k1]], 1)
    # side 2: the warped image's points whose inv(H) image is inside, at their own coordinates
    u2, v2 = warp(H_inv, p2[:, 0], p2[:, 1])
    k2 = _select(p2[:, 2], _inside(u2, v2, height, width, mutant), keep_k, mutant)
    B = np.stack([u2[k2], v2[k2]], 1) if mutant == "side2_warped" else p2[k2, :2]
    margin = min(_border_margin(u1, v1, height, width), _border_margin(u2, v2, height, width))
    c1, d1, g1 = _minima(A, B, thresh, mutant)
    c2, d2, g2 = _minima(B, A, thresh, mutant)
    if mutant == "minima_swapped":
        c1, d1, c2, d2 = c2, d2, c1, d1
    return (len(k1), len(k2), c1, c2, seq_sum(d1), seq_sum(d2), unwarped_count(p2, H_inv, height, width, mutant),
            min(margin, g1, g2))


def entry_rows(pts, counts, cap, entry, mutant=None):
    """The rows the kernel reads of entry `entry` of pts [E, cap, 3]: the first min(count, cap)."""
    n = int(counts[entry])
    if mutant != "count_unclamped":
        return pts[entry, :min(n, cap)]
    flat = np.concatenate([pts.reshape(-1, 3)[entry * cap:], np.zeros((max(n, cap), 3))])  # runs on into the next entry
    return flat[:n]


def repeatability_call(call, mutant=None):
    """One launch over the P pairs of `call` (tests/evaluation_cases.py): pair p uses entry p * pair_stride of both
    sides.  -> float64 [P,8] in the kernel's layout (slot 7 is 0) and the margins [P]."""
    P, s, cap = call["n_pairs"], call["pair_stride"], call["cap"]
    out, margins = np.zeros((P, 8)), np.zeros(P)
    for p in range(P):
        e = p if mutant == "stride_ignored" else p * s
        r = repeatability(entry_rows(call["pts1"], call["n1"], cap, e, mutant), entry_rows(call["pts2"], call["n2"], cap, e, mutant),
                          call["H"][p], call["H_inv"][p], call["height"], call["width"], call["keep_k"], call["thresh"], mutant)
        out[p, :7], margins[p] = r[:7], r[7]
    return out, margins
