"""numpy restatement of the device RANSAC + AP (csrc/eval_kernels.hip.h, eval_ransac_kernel): the same counter-based
hypothesis stream, degeneracy test, normalised 4-point DLT, scoring, refit and Gauss-Newton steps.  It is the reference
of the kernel, which cannot be checked against OpenCV here ("parity unpinned").  The hypothesis
solves repeat the kernel's operation order, so they agree with it to the last bit; the refit's sums run in another order
(agreement to rounding), and a second time in the kernel's own (lane_sum: lane-strided by 64, then the butterfly of
wave_sum).  The spread between the two refits is this restatement's own floor."""
import numpy as np

HYPOTHESES = 2000
GN_STEPS = 5
SAMPLE_DRAWS = 64
FLT_EPS = 1.1920928955078125e-07
M64 = (1 << 64) - 1


def _mix(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def draw(seed, h, c, n):
    r = _mix((seed & M64) ^ _mix((h << 8) | c))
    return ((r >> 32) * n) >> 32


def sample(seed, h, n):
    """The 4 indices of hypothesis h (None when the draws do not give 4 distinct ones)."""
    if n == 4:
        return [0, 1, 2, 3]
    c = 0
    ids = []
    for k in range(4):
        while True:
            v = draw(seed, h, c, n)
            c += 1
            if v not in ids or c >= SAMPLE_DRAWS:
                break
        ids.append(v)
    return ids if len(set(ids)) == 4 else None


def _collinear(a, b, c):
    dx1, dy1, dx2, dy2 = b[0] - a[0], b[1] - a[1], c[0] - a[0], c[1] - a[1]
    return abs(dx2 * dy1 - dy2 * dx1) <= FLT_EPS * (((abs(dx1) + abs(dy1)) + abs(dx2)) + abs(dy2))


def solve8(a, pivots=None):
    """Batched [B,8,9] elimination in the kernel's order (eval_solve8).  Returns (h [B,8], ok [B]).  pivots: a list that
    receives the pivot magnitudes [B] of every step."""
    a = np.array(a, dtype=np.float64)
    B = a.shape[0]
    ok = np.ones(B, dtype=bool)
    with np.errstate(all="ignore"):
        for k in range(8):
            for r in range(k + 1, 8):
                sw = np.abs(a[:, r, k]) > np.abs(a[:, k, k])
                t = a[sw, k, k:].copy()
                a[sw, k, k:] = a[sw, r, k:]
                a[sw, r, k:] = t
            ok &= np.abs(a[:, k, k]) > 1e-12
            if pivots is not None:
                pivots.append(np.abs(a[:, k, k]))
            inv = 1.0 / a[:, k, k]
            for r in range(k + 1, 8):
                f = a[:, r, k] * inv
                for c in range(k + 1, 9):
                    a[:, r, c] = a[:, r, c] - f * a[:, k, c]
        h = np.zeros((B, 8))
        for k in range(7, -1, -1):
            s = a[:, k, 8].copy()
            for c in range(k + 1, 8):
                s = s - a[:, k, c] * h[:, c]
            h[:, k] = s / a[:, k, k]
    return h, ok


def denorm(hn, tp, tq):
    """eval_denorm: inv(Tq) * Hn * Tp scaled to H[8] = 1; hn [B,8], tp / tq = (s, cx, cy) arrays [B]."""
    sp, cpx, cpy = tp
    sq, cqx, cqy = tq
    hv = np.concatenate([hn, np.ones((hn.shape[0], 1))], axis=1)
    ox, oy = -(sp * cpx), -(sp * cpy)
    Bm = np.zeros_like(hv)
    for r in range(3):
        Bm[:, 3 * r] = hv[:, 3 * r] * sp
        Bm[:, 3 * r + 1] = hv[:, 3 * r + 1] * sp
        Bm[:, 3 * r + 2] = (hv[:, 3 * r] * ox + hv[:, 3 * r + 1] * oy) + hv[:, 3 * r + 2]
    iq = 1.0 / sq
    Cm = np.zeros_like(hv)
    for c in range(3):
        Cm[:, c] = Bm[:, c] * iq + cqx * Bm[:, 6 + c]
        Cm[:, 3 + c] = Bm[:, 3 + c] * iq + cqy * Bm[:, 6 + c]
        Cm[:, 6 + c] = Bm[:, 6 + c]
    i8 = 1.0 / Cm[:, 8]
    return Cm * i8[:, None]


def resid2(H, m):
    """eval_resid2 of homographies H [B,9] on matches m [n,4] (x1, y1, x2, y2) -> [B,n]."""
    x, y, u0, v0 = (m[None, :, k] for k in range(4))
    H = H[:, :, None]
    with np.errstate(all="ignore"):
        w = (H[:, 6] * x + H[:, 7] * y) + H[:, 8]
        u = ((H[:, 0] * x + H[:, 1] * y) + H[:, 2]) / w
        v = ((H[:, 3] * x + H[:, 4] * y) + H[:, 5]) / w
    du, dv = u - u0, v - v0
    return du * du + dv * dv


def hypotheses(m, seed, hs):
    """(H [len(hs),9], valid [len(hs)]) of the hypotheses hs of matches m [n,4]."""
    n = m.shape[0]
    A = np.zeros((len(hs), 8, 9))
    tps, tqs = np.ones((3, len(hs))), np.ones((3, len(hs)))
    valid = np.zeros(len(hs), dtype=bool)
    for b, h in enumerate(hs):
        ids = sample(seed, h, n)
        if ids is None:
            continue
        q = m[ids]
        bad = False
        for (a, bb, d) in ((0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3)):
            if _collinear(q[a, :2], q[bb, :2], q[d, :2]) or _collinear(q[a, 2:], q[bb, 2:], q[d, 2:]):
                bad = True
                break
        if bad:
            continue
        cpx = (((q[0, 0] + q[1, 0]) + q[2, 0]) + q[3, 0]) / 4.0
        cpy = (((q[0, 1] + q[1, 1]) + q[2, 1]) + q[3, 1]) / 4.0
        cqx = (((q[0, 2] + q[1, 2]) + q[2, 2]) + q[3, 2]) / 4.0
        cqy = (((q[0, 3] + q[1, 3]) + q[2, 3]) + q[3, 3]) / 4.0
        sp = sq = 0.0
        for k in range(4):
            sp = sp + (abs(q[k, 0] - cpx) + abs(q[k, 1] - cpy))
            sq = sq + (abs(q[k, 2] - cqx) + abs(q[k, 3] - cqy))
        if not (sp > 0.0 and sq > 0.0):
            continue
        sp, sq = 4.0 / sp, 4.0 / sq
        for k in range(4):
            x, y = (q[k, 0] - cpx) * sp, (q[k, 1] - cpy) * sp
            u, v = (q[k, 2] - cqx) * sq, (q[k, 3] - cqy) * sq
            A[b, 2 * k] = [x, y, 1.0, 0.0, 0.0, 0.0, -(x * u), -(y * u), u]
            A[b, 2 * k + 1] = [0.0, 0.0, 0.0, x, y, 1.0, -(x * v), -(y * v), v]
        tps[:, b] = (sp, cpx, cpy)
        tqs[:, b] = (sq, cqx, cqy)
        valid[b] = True
    hn, ok = solve8(A)
    H = denorm(hn, tps, tqs)
    valid &= ok & np.all(np.isfinite(H[:, :8]), axis=1)
    return H, valid


def strided_partials(terms, index, threads):
    """Partial sums [threads, ...] of terms [k, ...]: thread t adds the terms whose index is t mod threads, in index order
    (index ascending) from 0.0."""
    terms = np.asarray(terms, dtype=np.float64)
    index = np.asarray(index, dtype=np.int64)
    part = np.zeros((threads,) + terms.shape[1:])
    rnd = index // threads
    for r in np.unique(rnd):
        sel = rnd == r                      # one term per thread at most: the indexed addition adds each once
        part[index[sel] % threads] = part[index[sel] % threads] + terms[sel]
    return part


def butterfly(part):
    """wave_sum over axis 0 (64 lanes): the xor butterfly with offsets 32, 16, .., 1; every lane ends with the same value."""
    o = 32
    while o >= 1:
        part = part + part[np.arange(64) ^ o]
        o >>= 1
    return part[0]


def lane_sum(terms, index):
    """The sum of terms [k, ...] as wave 0 forms it: lane l adds its terms (those whose match index is l mod 64) in
    index order from 0.0, then the 64 partials meet in the xor butterfly of wave_sum (offsets 32, 16, .., 1)."""
    return butterfly(strided_partials(terms, index, 64))


def _norm_of(pts, index=None):
    """index None: numpy's own summation; else the match indices of the rows, for the kernel's lane order."""
    if index is None:
        c = pts.mean(axis=0)
        sa = np.sum(np.abs(pts[:, 0] - c[0]) + np.abs(pts[:, 1] - c[1]))
        return pts.shape[0] / sa, c[0], c[1]
    s = lane_sum(np.concatenate([pts, np.ones((pts.shape[0], 1))], axis=1), index)
    cx, cy = s[0] / s[2], s[1] / s[2]
    return s[2] / lane_sum(np.abs(pts[:, 0] - cx) + np.abs(pts[:, 1] - cy), index), cx, cy


def _normal_eq(m, tp, tq, geometric, h, index=None):
    x, y = (m[:, 0] - tp[1]) * tp[0], (m[:, 1] - tp[2]) * tp[0]
    u, v = (m[:, 2] - tq[1]) * tq[0], (m[:, 3] - tq[2]) * tq[0]
    z, o = np.zeros_like(x), np.ones_like(x)
    if geometric:
        iw = 1.0 / ((h[6] * x + h[7] * y) + 1.0)
        px, py = ((h[0] * x + h[1] * y) + h[2]) * iw, ((h[3] * x + h[4] * y) + h[5]) * iw
        xw, yw = x * iw, y * iw
        j0 = np.stack([xw, yw, iw, z, z, z, -(xw * px), -(yw * px)], 1)
        j1 = np.stack([z, z, z, xw, yw, iw, -(xw * py), -(yw * py)], 1)
        r0, r1 = px - u, py - v
    else:
        j0 = np.stack([x, y, o, z, z, z, -(x * u), -(y * u)], 1)
        j1 = np.stack([z, z, z, x, y, o, -(x * v), -(y * v)], 1)
        r0, r1 = -u, -v
    a = np.zeros((8, 9))
    if index is None:
        a[:, :8] = j0.T @ j0 + j1.T @ j1
        a[:, 8] = -(j0.T @ r0 + j1.T @ r1)
        return float(np.sum(r0 * r0 + r1 * r1)), a
    # the kernel's terms: a[r][c] += j0[r] j0[c] + j1[r] j1[c] (c >= r, mirrored), a[r][8] -= j0[r] r0 + j1[r] r1
    a[:, :8] = lane_sum(j0[:, :, None] * j0[:, None, :] + j1[:, :, None] * j1[:, None, :], index)
    a[:, 8] = -lane_sum(j0 * r0[:, None] + j1 * r1[:, None], index)
    return float(lane_sum(r0 * r0 + r1 * r1, index)), a


def refit(m, mask, lanes=False):
    """The refit of the winner's inliers: algebraic least squares, then Gauss-Newton steps kept while the cost falls.
    lanes: the sums in wave 0's order (lane_sum) instead of numpy's.  -> H [9], or None when the refit gives none."""
    idx = np.nonzero(mask)[0] if lanes else None
    mi = m[mask]
    tp, tq = _norm_of(mi[:, :2], idx), _norm_of(mi[:, 2:], idx)
    if not all(np.isfinite(t[0]) and t[0] > 0 for t in (tp, tq)):
        return None
    _, a = _normal_eq(mi, tp, tq, False, np.zeros(8), idx)
    h, ok = solve8(a[None])
    if not ok[0]:
        return None
    h = h[0]
    cost, a = _normal_eq(mi, tp, tq, True, h, idx)
    for _ in range(GN_STEPS):
        d, ok = solve8(a[None])
        if not ok[0]:
            break
        hn = h + d[0]
        cn, an = _normal_eq(mi, tp, tq, True, hn, idx)
        if not cn < cost:
            break
        cost, h, a = cn, hn, an
    Hr = denorm(h[None], np.array(tp)[:, None], np.array(tq)[:, None])[0]
    return Hr if np.all(np.isfinite(Hr)) else None


def ransac(m, seed, scores=None):
    """m: [n,4] float64 matches (x1, y1, x2, y2).  Returns dict(H [3,3], mask [n] bool, status 0 / 1, best hypothesis,
    H_best [3,3] (the winner before the refit), H_lanes [3,3] (the refit with its sums in wave 0's order: the spread
    between H and H_lanes is this restatement's own floor), ap when scores (the match distances) are given)."""
    m = np.asarray(m, dtype=np.float64).reshape(-1, 4)
    n = m.shape[0]
    out = {"H": np.eye(3), "mask": np.zeros(n, dtype=bool), "status": 1, "best": -1}
    if scores is not None:
        out["ap"] = 0.0
    if n < 4:
        return out
    if n == 4:
        H, valid = hypotheses(m, seed, [0])
        if not valid[0]:
            return out
        out.update(H=H[0].reshape(3, 3), mask=np.ones(4, dtype=bool), status=0, best=0, H_best=H[0].reshape(3, 3),
                   H_lanes=H[0].reshape(3, 3))
    else:
        best, best_sc, best_H = -1, -1, None
        for h0 in range(0, HYPOTHESES, 250):
            hs = list(range(h0, min(h0 + 250, HYPOTHESES)))
            H, valid = hypotheses(m, seed, hs)
            sc = np.sum(resid2(H, m) <= 9.0, axis=1)
            for b in np.nonzero(valid)[0]:
                if sc[b] > best_sc:
                    best, best_sc, best_H = hs[b], sc[b], H[b]
        if best < 0:
            return out
        mask = resid2(best_H[None], m)[0] <= 9.0
        Hf = Hl = best_H
        if mask.sum() >= 4:
            Hr, Hq = refit(m, mask), refit(m, mask, lanes=True)
            Hf = best_H if Hr is None else Hr
            Hl = best_H if Hq is None else Hq
        out.update(H=Hf.reshape(3, 3), mask=mask, status=0, best=best, H_best=best_H.reshape(3, 3), H_lanes=Hl.reshape(3, 3))
    if scores is not None:
        out["ap"] = average_precision(out["mask"], -np.asarray(scores, dtype=np.float64))
    return out


def average_precision_counting(mask, dist):
    """The same AP in the kernel's form: the sum over the inliers i of tp(d <= d_i) / n(d <= d_i) in index order, over
    the inlier count (float32 distances compared as they are)."""
    mask, dist = np.asarray(mask, dtype=bool), np.asarray(dist, dtype=np.float32)
    if not mask.any():
        return 0.0
    s = np.float64(0.0)
    for i in np.nonzero(mask)[0]:
        le = dist <= dist[i]
        s = s + np.float64(np.sum(le & mask)) / np.float64(np.sum(le))
    return float(s / np.float64(mask.sum()))


def average_precision(labels, scores):
    """sklearn.metrics.average_precision_score(labels, scores) for binary labels: descending distinct thresholds,
    -sum(diff(recall) * precision[:-1]); 0 when there is no positive (the evaluation's convention)."""
    labels = np.asarray(labels, dtype=bool)
    scores = np.asarray(scores, dtype=np.float64)
    if labels.size == 0 or not labels.any():
        return 0.0
    order = np.argsort(scores, kind="mergesort")[::-1]
    s, y = scores[order], labels[order].astype(np.float64)
    last = np.r_[np.nonzero(np.diff(s))[0], y.size - 1]
    tps = np.cumsum(y)[last]
    fps = 1 + last - tps
    precision = tps / (tps + fps)
    recall = tps / tps[-1]
    precision = np.r_[precision[::-1], 1.0]
    recall = np.r_[recall[::-1], 0.0]
    return float(-np.sum(np.diff(recall) * precision[:-1]))
