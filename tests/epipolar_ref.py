"""numpy restatement of the fundamental-matrix RANSAC (csrc/epipolar_kernels.hip.h).  There is no
reference counterpart and no OpenCV here, so this file is the specification the kernels are tested against: the same
counter-based draws (tests/eval_restatement.py's stream), the normalised 8-point solve by complete pivoting, the Sampson
score, the refit on the inliers, the Jacobi rank-2 step and the output scaling.  The hypothesis solves and the scores
repeat the kernel's operation order (equal to the last bit); the refit's sums over the inliers run in another order than
the kernel's (agreement to rounding, see `ransac(..., pairwise=)` and tests/test_gpu_epipolar.py for the measured bound), and
a third time in the kernel's own (`order="block"`: block_sum<256>, see `block_sum`).  `decisions` reports how far every
comparison of a problem is from going the other way.  Also the synthetic two-view scenes and the
fixtures the tests use."""
import functools

import numpy as np

from tests import eval_restatement as ER

HYPOTHESES = ER.HYPOTHESES
SAMPLE_DRAWS = ER.SAMPLE_DRAWS
PIVOT_EPS = 1e-12
JACOBI_SWEEPS = 8
MIN_SCORE = 8
DIRECT_N = 8          # this many matches: the one direct solve of matches 0..7
BLOCK_THREADS = 256   # EPI_THREADS
WINDOW = 1e-6         # decisions(): a squared distance within WINDOW * thresh^2 of thresh^2 is ambiguous


def sample8(seed, h, n):
    """The 8 match indices of hypothesis h (None when the draws do not give 8 distinct ones)."""
    if n == DIRECT_N:
        return list(range(8))
    c = 0
    ids = []
    for _ in range(8):
        while True:
            v = ER.draw(seed, h, c, n)
            c += 1
            if v not in ids or c >= SAMPLE_DRAWS:
                break
        ids.append(v)
    return ids if len(set(ids)) == 8 else None


def null_vector(A, trace=None, pivots=None):
    """Null vectors of B 8x9 matrices A [B,8,9] by Gaussian elimination with complete pivoting.  Returns (f [B,9], ok [B]).
    trace: a list that receives the (row, column) of every pivot of matrix 0; pivots: a list that receives the pivot
    magnitudes [B] of every step."""
    a = np.array(A, dtype=np.float64)
    B = a.shape[0]
    ar = np.arange(B)
    perm = np.tile(np.arange(9), (B, 1))
    ok = np.ones(B, dtype=bool)
    with np.errstate(all="ignore"):
        for k in range(8):
            sub = np.abs(a[:, k:, k:])
            sub = np.where(np.isnan(sub), -1.0, sub).reshape(B, -1)
            idx = np.argmax(sub, axis=1)  # first maximum in row-major order: the lowest row, then the lowest column
            pr, pc = k + idx // (9 - k), k + idx % (9 - k)
            if trace is not None:
                trace.append((int(pr[0]), int(pc[0])))
            t = a[ar, k, :].copy()
            a[ar, k, :] = a[ar, pr, :]
            a[ar, pr, :] = t
            t = a[ar, :, k].copy()
            a[ar, :, k] = a[ar, :, pc]
            a[ar, :, pc] = t
            t = perm[ar, k].copy()
            perm[ar, k] = perm[ar, pc]
            perm[ar, pc] = t
            piv = a[:, k, k]
            ok &= np.abs(piv) > PIVOT_EPS
            if pivots is not None:
                pivots.append(np.abs(piv))
            inv = 1.0 / piv
            for r in range(k + 1, 8):
                f = a[:, r, k] * inv
                for c in range(k + 1, 9):
                    a[:, r, c] = a[:, r, c] - f * a[:, k, c]
        x = np.zeros((B, 9))
        x[:, 8] = 1.0
        for k in range(7, -1, -1):
            s = a[:, k, 8].copy()
            for c in range(k + 1, 8):
                s = s + a[:, k, c] * x[:, c]
            x[:, k] = -s / a[:, k, k]
    f = np.zeros((B, 9))
    f[ar[:, None], perm] = x
    return f, ok


def denorm(fn, t1, t2):
    """F = T2^T Fn T1 for fn [B,9]; t = (s, cx, cy) arrays [B]; T = [[s, 0, -s cx], [0, s, -s cy], [0, 0, 1]]."""
    s1, c1x, c1y = t1
    s2, c2x, c2y = t2
    with np.errstate(all="ignore"):
        o1x, o1y = -(s1 * c1x), -(s1 * c1y)
        o2x, o2y = -(s2 * c2x), -(s2 * c2y)
        Bm = np.zeros_like(fn)
        for r in range(3):
            Bm[:, 3 * r] = fn[:, 3 * r] * s1
            Bm[:, 3 * r + 1] = fn[:, 3 * r + 1] * s1
            Bm[:, 3 * r + 2] = (fn[:, 3 * r] * o1x + fn[:, 3 * r + 1] * o1y) + fn[:, 3 * r + 2]
        F = np.zeros_like(fn)
        for c in range(3):
            F[:, c] = s2 * Bm[:, c]
            F[:, 3 + c] = s2 * Bm[:, 3 + c]
            F[:, 6 + c] = (o2x * Bm[:, c] + o2y * Bm[:, 3 + c]) + Bm[:, 6 + c]
    return F


def carry(F, t1, t2):
    """T2^-T F T1^-1 for one F [9] (scalars t = (s, cx, cy)); T^-1 = [[1/s, 0, cx], [0, 1/s, cy], [0, 0, 1]]."""
    s1, c1x, c1y = t1
    s2, c2x, c2y = t2
    i1, i2 = 1.0 / s1, 1.0 / s2
    Bm = np.zeros(9)
    for r in range(3):
        Bm[3 * r] = F[3 * r] * i1
        Bm[3 * r + 1] = F[3 * r + 1] * i1
        Bm[3 * r + 2] = (F[3 * r] * c1x + F[3 * r + 1] * c1y) + F[3 * r + 2]
    G = np.zeros(9)
    for c in range(3):
        G[c] = i2 * Bm[c]
        G[3 + c] = i2 * Bm[3 + c]
        G[6 + c] = (c2x * Bm[c] + c2y * Bm[3 + c]) + Bm[6 + c]
    return G


def rows_of(ax, ay, bx, by):
    """The epipolar rows [bx ax, bx ay, bx, by ax, by ay, by, ax, ay, 1] (b^T F a = 0)."""
    return np.stack([bx * ax, bx * ay, bx, by * ax, by * ay, by, ax, ay, np.ones_like(ax)], axis=-1)


def sampson2(F, m):
    """Squared Sampson distance of F [B,9] on matches m [n,4] (ax, ay, bx, by): (d2 [B,n], usable [B,n])."""
    ax, ay, bx, by = (m[None, :, k] for k in range(4))
    F = F[:, :, None]
    with np.errstate(all="ignore"):
        l0 = (F[:, 0] * ax + F[:, 1] * ay) + F[:, 2]
        l1 = (F[:, 3] * ax + F[:, 4] * ay) + F[:, 5]
        l2 = (F[:, 6] * ax + F[:, 7] * ay) + F[:, 8]
        m0 = (F[:, 0] * bx + F[:, 3] * by) + F[:, 6]
        m1 = (F[:, 1] * bx + F[:, 4] * by) + F[:, 7]
        e = (bx * l0 + by * l1) + l2
        den = ((l0 * l0 + l1 * l1) + m0 * m0) + m1 * m1
        usable = np.isfinite(den) & (den > 0.0)
        d2 = (e * e) / den
    return d2, usable


def inliers(F, m, thresh):
    d2, usable = sampson2(F, m)
    with np.errstate(all="ignore"):
        return usable & (d2 <= thresh * thresh)


def hypotheses(m, seed, hs, pivots=None):
    """(F [len(hs),9], valid [len(hs)]) of the hypotheses hs of matches m [n,4].  pivots: a list that receives (sampled
    [len(hs)] = the hypothesis reached the elimination, pivot magnitudes [8, len(hs)])."""
    n = m.shape[0]
    B = len(hs)
    q = np.zeros((B, 8, 4))
    valid = np.zeros(B, dtype=bool)
    for b, h in enumerate(hs):
        ids = sample8(seed, h, n)
        if ids is not None:
            q[b] = m[ids]
            valid[b] = True
    with np.errstate(all="ignore"):
        c = q[:, 0].copy()
        for k in range(1, 8):
            c = c + q[:, k]
        c = c / 8.0
        sp, sq = np.zeros(B), np.zeros(B)
        for k in range(8):
            sp = sp + (np.abs(q[:, k, 0] - c[:, 0]) + np.abs(q[:, k, 1] - c[:, 1]))
            sq = sq + (np.abs(q[:, k, 2] - c[:, 2]) + np.abs(q[:, k, 3] - c[:, 3]))
        valid &= (sp > 0.0) & (sq > 0.0)
        s1, s2 = 8.0 / sp, 8.0 / sq
        ax, ay = (q[:, :, 0] - c[:, None, 0]) * s1[:, None], (q[:, :, 1] - c[:, None, 1]) * s1[:, None]
        bx, by = (q[:, :, 2] - c[:, None, 2]) * s2[:, None], (q[:, :, 3] - c[:, None, 3]) * s2[:, None]
        piv = [] if pivots is not None else None
        fn, ok = null_vector(rows_of(ax, ay, bx, by), pivots=piv)
        if pivots is not None:
            pivots.append((valid.copy(), np.stack(piv)))
        F = denorm(fn, (s1, c[:, 0], c[:, 1]), (s2, c[:, 2], c[:, 3]))
    valid &= ok & np.all(np.isfinite(F), axis=1)
    return F, valid


def block_sum(terms, index, threads=BLOCK_THREADS):
    """The sum of terms [k, ...] as block_sum<threads> (csrc/geom_blocks.hip.h) forms it in epi_finish_kernel: term i goes to
    thread index[i] mod threads; each thread adds its terms in index order from 0.0; the 64 partials of each wave meet in the
    xor butterfly of wave_sum (offsets 32 .. 1); the wave partials are added in wave order.  index: the match rows of the
    terms (not their positions among the inliers), ascending."""
    part = ER.strided_partials(terms, index, threads)
    total = ER.butterfly(part[:64])
    for w in range(1, threads // 64):
        total = total + ER.butterfly(part[64 * w:64 * (w + 1)])
    return total


def _total(v, pairwise, index=None):
    """Sum over axis 0: ascending (one accumulator), pairwise (halves folded onto each other) or, with pairwise = "block",
    in the kernel's order (block_sum over the match rows `index`)."""
    v = np.asarray(v, dtype=np.float64)
    if isinstance(pairwise, str):
        assert pairwise == "block" and index is not None
        return block_sum(v, index)
    if not pairwise:
        acc = np.zeros(v.shape[1:])
        for k in range(v.shape[0]):
            acc = acc + v[k]
        return acc
    size = 1
    while size < v.shape[0]:
        size *= 2
    w = np.zeros((size,) + v.shape[1:])
    w[:v.shape[0]] = v
    while size > 1:
        size //= 2
        w = w[:size] + w[size:2 * size]
    return w[0]


def norm_of(pts, pairwise=False, index=None):
    """EvalNorm of a point set [k,2]: (s, cx, cy), s = k / sum(|x - cx| + |y - cy|)."""
    k = float(_total(np.ones(pts.shape[0]), pairwise, index))      # the kernel's count is a sum too (exact in every order)
    with np.errstate(all="ignore"):
        cx, cy = _total(pts[:, 0], pairwise, index) / k, _total(pts[:, 1], pairwise, index) / k
        sa = _total(np.abs(pts[:, 0] - cx) + np.abs(pts[:, 1] - cy), pairwise, index)
        return k / sa, cx, cy


def jacobi3(G):
    """Cyclic Jacobi on a symmetric 3x3: (diagonal [3], V [3,3]) after JACOBI_SWEEPS sweeps over (0,1), (0,2), (1,2)."""
    G = np.array(G, dtype=np.float64).reshape(3, 3)
    V = np.eye(3)
    with np.errstate(all="ignore"):
        for _ in range(JACOBI_SWEEPS):
            for (p, q) in ((0, 1), (0, 2), (1, 2)):
                gpq = G[p, q]
                if gpq == 0.0:
                    continue
                r = 3 - p - q
                theta = (G[q, q] - G[p, p]) / (2.0 * gpq)
                t = 1.0 / (abs(theta) + np.sqrt(theta * theta + 1.0))
                if theta < 0.0:
                    t = -t
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                gpp, gqq = G[p, p] - t * gpq, G[q, q] + t * gpq
                grp, grq = c * G[r, p] - s * G[r, q], s * G[r, p] + c * G[r, q]
                G[p, p], G[q, q] = gpp, gqq
                G[p, q] = G[q, p] = 0.0
                G[r, p] = G[p, r] = grp
                G[r, q] = G[q, r] = grq
                for k in range(3):
                    vp, vq = c * V[k, p] - s * V[k, q], s * V[k, p] + c * V[k, q]
                    V[k, p], V[k, q] = vp, vq
    return np.array([G[0, 0], G[1, 1], G[2, 2]]), V


def rank2(fn):
    """Fn - (Fn v) v^T with v the eigenvector of Fn^T Fn of the smallest eigenvalue (jacobi3): fn [9] -> [9]."""
    f = np.asarray(fn, dtype=np.float64)
    with np.errstate(all="ignore"):
        G = np.zeros((3, 3))
        for i in range(3):
            for j in range(3):
                G[i, j] = (f[i] * f[j] + f[3 + i] * f[3 + j]) + f[6 + i] * f[6 + j]
        d, V = jacobi3(G)
        k = 0
        for j in (1, 2):
            if d[j] < d[k]:
                k = j
        v = V[:, k]
        out = np.zeros(9)
        for r in range(3):
            w = (f[3 * r] * v[0] + f[3 * r + 1] * v[1]) + f[3 * r + 2] * v[2]
            for c in range(3):
                out[3 * r + c] = f[3 * r + c] - w * v[c]
    return out


def _argmax_abs(v):
    k = 0
    for j in range(1, len(v)):
        if abs(v[j]) > abs(v[k]):
            k = j
    return k


def sign_rule(Fd):
    """The output's sign: the largest |entry| (the lowest index on ties) is positive."""
    return -Fd if Fd[_argmax_abs(Fd)] < 0.0 else Fd


def _gap(v):
    """Relative gap between the two largest |entries| of v: what the argmax hangs on."""
    a = np.sort(np.abs(np.asarray(v, dtype=np.float64)))
    return float((a[-1] - a[-2]) / a[-1]) if a[-1] > 0.0 else 0.0


def refit(F, mi, pairwise=False, index=None, report=None):
    """The final F [9] from the winner's F [9] and its inliers mi [k,4] (None: no usable norm), and err.  pairwise: False
    (ascending sums), True (pairwise) or "block" (the kernel's order; index = the match rows of mi).  report: a dict that
    receives norm_usable, gap_G, gap_Fd (see _gap), solved (the 8x8 system was accepted) and pivots [8]."""
    with np.errstate(all="ignore"):
        t1, t2 = norm_of(mi[:, :2], pairwise, index), norm_of(mi[:, 2:], pairwise, index)
        if report is not None:
            report["norm_usable"] = all(np.isfinite(t[0]) and t[0] > 0.0 for t in (t1, t2))
        if not all(np.isfinite(t[0]) and t[0] > 0.0 for t in (t1, t2)):
            t1 = t2 = (1.0, 0.0, 0.0)
        G = carry(F, t1, t2)
        ks = _argmax_abs(G)
        A = rows_of((mi[:, 0] - t1[1]) * t1[0], (mi[:, 1] - t1[2]) * t1[0], (mi[:, 2] - t2[1]) * t2[0],
                    (mi[:, 3] - t2[2]) * t2[0])
        Mom = np.zeros((9, 9))
        for j in range(9):
            for k in range(j, 9):
                Mom[j, k] = Mom[k, j] = _total(A[:, j] * A[:, k], pairwise, index)
        idx = [j for j in range(9) if j != ks]
        a = np.zeros((8, 9))
        for r in range(8):
            for c in range(8):
                a[r, c] = Mom[idx[r], idx[c]]
            a[r, 8] = -Mom[idx[r], ks]
        piv = []
        g, ok = ER.solve8(a[None], pivots=piv)
        if report is not None:
            report.update(gap_G=_gap(G), solved=bool(ok[0] and np.all(np.isfinite(g[0]))), pivots=np.array([v[0] for v in piv]))
        fn = G
        if ok[0] and np.all(np.isfinite(g[0])):
            fn = np.zeros(9)
            fn[idx] = g[0]
            fn[ks] = 1.0
        fn = rank2(fn)
        as_b = lambda t: tuple(np.array([v]) for v in t)
        Fd = denorm(fn[None], as_b(t1), as_b(t2))[0]
        ss = 0.0
        for k in range(9):
            ss = ss + Fd[k] * Fd[k]
        nrm = np.sqrt(ss)
        if not (np.isfinite(nrm) and nrm > 0.0):
            return None, 0.0
        Fd = Fd / nrm
        if report is not None:
            report["gap_Fd"] = _gap(Fd)
        Fd = sign_rule(Fd)
        d2, usable = sampson2(Fd[None], mi)
        err = np.sqrt(_total(np.where(usable[0], d2[0], 0.0), pairwise, index) / float(mi.shape[0]))
    return Fd, float(err)


def winner_of(m, seed, thresh=1.0):
    """(winning hypothesis, its score, its F [9]) over the 2000 hypotheses; (-1, -1, None) without a valid one."""
    n = m.shape[0]
    best, best_sc, best_F = -1, -1, None
    if n < 8:
        return best, best_sc, best_F
    total = 1 if n == DIRECT_N else HYPOTHESES
    for h0 in range(0, total, 250):
        hs = list(range(h0, min(h0 + 250, total)))
        F, valid = hypotheses(m, seed, hs)
        sc = np.sum(inliers(F, m, thresh), axis=1)
        for b in np.nonzero(valid)[0]:
            if sc[b] > best_sc:
                best, best_sc, best_F = hs[b], int(sc[b]), F[b]
    return best, best_sc, best_F


def ransac(m, seed, thresh=1.0, pairwise=False, winner=None, report=None):
    """m: [n,4] float64 matches (ax, ay, bx, by).  Returns dict(F [3,3], mask [n] bool, n_inliers, status 0 / 1, winner,
    err, F_winner [3,3] = the unrefitted winner).  pairwise: the summation order of the refit (False: ascending, True:
    pairwise, "block": the kernel's); winner: a winner_of() result to reuse; report: see refit()."""
    m = np.asarray(m, dtype=np.float64).reshape(-1, 4)
    n = m.shape[0]
    out = {"F": np.zeros((3, 3)), "mask": np.zeros(n, dtype=bool), "n_inliers": 0, "status": 1, "winner": -1, "err": 0.0,
           "F_winner": np.zeros((3, 3))}
    best, best_sc, best_F = winner if winner is not None else winner_of(m, seed, thresh)
    if best < 0 or best_sc < MIN_SCORE:
        return out
    mask = inliers(best_F[None], m, thresh)[0]
    Fd, err = refit(best_F, m[mask], pairwise, np.nonzero(mask)[0], report)
    if Fd is None:
        return out
    out.update(F=Fd.reshape(3, 3), mask=mask, n_inliers=int(mask.sum()), status=0, winner=best, err=err,
               F_winner=best_F.reshape(3, 3))
    return out


def decisions(m, seed, thresh=1.0):
    """How far the problem is from every comparison going the other way.  Returns dict(
      score [H], ambiguous [H]: per hypothesis, the inliers and the matches with |d2 - t2| <= WINDOW * t2 (0 where invalid),
      valid [H],
      pivot_least_accepted: the least pivot magnitude of any hypothesis whose eight pivots are all accepted (inf: none),
      pivot_largest_refused: over the refused hypotheses, the largest of their smallest pivots, the one that holds the
          refusal (0: none; a NaN pivot is refused in every order and is not counted),
      pivot_log_margin: the least |log10(pivot / PIVOT_EPS)| of those two,
      winner, best (its score), winner_F [9],
      decided: the winner has no ambiguous match, every lower hypothesis has score + ambiguous < best and every higher one
          score + ambiguous <= best (without a valid hypothesis: True, the refusals are judged by the pivots),
      slack: how many more matches the nearest rival would need: min(best - 1 - max(score + ambiguous) below the winner,
          best - max(score + ambiguous) above it); >= 0 when decided, None without a rival).
    The refit's margins (argmax and sign gaps, its own pivots) come from ransac(..., report=)."""
    m = np.asarray(m, dtype=np.float64).reshape(-1, 4)
    n = m.shape[0]
    total = 0 if n < 8 else (1 if n == DIRECT_N else HYPOTHESES)
    score, amb, valid = (np.zeros(total, dtype=np.int64) for _ in range(3))
    valid = valid.astype(bool)
    Fs = np.zeros((total, 9))
    t2 = thresh * thresh
    least_ok, largest_bad, log_margin = np.inf, 0.0, np.inf
    for h0 in range(0, total, 250):
        hs = list(range(h0, min(h0 + 250, total)))
        piv = []
        F, v = hypotheses(m, seed, hs, pivots=piv)
        sampled, pv = piv[0]
        with np.errstate(all="ignore"):
            low = np.min(np.where(np.isnan(pv), np.inf, pv), axis=0)     # [B] the smallest pivot of each hypothesis
            accepted = sampled & np.all(pv > PIVOT_EPS, axis=0)
            acc, ref = low[accepted], low[sampled & ~accepted & (low <= PIVOT_EPS)]
            if acc.size:
                least_ok = min(least_ok, float(acc.min()))
            if ref.size:
                largest_bad = max(largest_bad, float(ref.max()))
            d2, usable = sampson2(F, m)
            inl = usable & (d2 <= t2)
            near = usable & (np.abs(d2 - t2) <= WINDOW * t2)
        sl = slice(h0, h0 + len(hs))
        valid[sl], Fs[sl] = v, F
        score[sl], amb[sl] = np.where(v, inl.sum(axis=1), 0), np.where(v, near.sum(axis=1), 0)
    with np.errstate(all="ignore"):
        if np.isfinite(least_ok):
            log_margin = min(log_margin, abs(np.log10(least_ok / PIVOT_EPS)))
        if largest_bad > 0.0:
            log_margin = min(log_margin, abs(np.log10(largest_bad / PIVOT_EPS)))
    out = {"score": score, "ambiguous": amb, "valid": valid, "pivot_log_margin": float(log_margin),
           "pivot_least_accepted": least_ok, "pivot_largest_refused": largest_bad, "winner": -1, "best": -1, "winner_F": None,
           "decided": True, "slack": None}
    if not valid.any():
        return out
    sv = np.where(valid, score, -1)
    w = int(np.argmax(sv))                                               # the first maximum: the lowest hypothesis
    best = int(sv[w])
    reach = np.where(valid, score + amb, -1)
    lower, higher = reach[:w], reach[w + 1:]
    decided = amb[w] == 0 and (lower.size == 0 or lower.max() < best) and (higher.size == 0 or higher.max() <= best)
    gaps = ([best - 1 - int(lower.max())] if lower.size else []) + ([best - int(higher.max())] if higher.size else [])
    out.update(winner=w, best=best, winner_F=Fs[w], decided=bool(decided), slack=min(gaps) if gaps else None)
    return out


def gather(pts1, pts2, match, n_match):
    """The kernel's staging: match rows (i, j, d) -> [n,4] (ax, ay, bx, by); indices clamped to the arrays."""
    cap = match.shape[0]
    n = min(max(int(n_match), 0), cap)
    i = np.clip(match[:n, 0].astype(np.int64), 0, cap - 1)
    j = np.clip(match[:n, 1].astype(np.int64), 0, cap - 1)
    return np.concatenate([pts1[i, :2], pts2[j, :2]], axis=1).astype(np.float64)


# ---- synthetic two-view scenes -----------------------------------------------------------------------------------------
# The camera translates and zooms (focal length FOCAL -> FOCAL2).  With equal intrinsics a pure translation gives an
# ANTISYMMETRIC F, whose two largest entries tie in magnitude with opposite signs: the output's sign rule ("the largest
# |entry| positive") would then hang on the last bit.  The zoom separates them by 10 %.
FOCAL, FOCAL2, WIDTH, HEIGHT = 300.0, 330.0, 320.0, 240.0
MARGIN = 25.0


def true_F(t):
    K1 = np.array([[FOCAL, 0.0, WIDTH / 2], [0.0, FOCAL, HEIGHT / 2], [0.0, 0.0, 1.0]])
    K2 = np.array([[FOCAL2, 0.0, WIDTH / 2], [0.0, FOCAL2, HEIGHT / 2], [0.0, 0.0, 1.0]])
    tx = np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])
    # camera 2 sees X - t: b ~ K2 (X - t), a ~ K1 X  =>  b^T K2^-T [-t]x K1^-1 a = 0
    return np.linalg.inv(K2).T @ (-tx) @ np.linalg.inv(K1)


def line_dist(F, a, b):
    """(distance of b from the line F a, distance of a from the line F^T b) for points [k,2]."""
    ah = np.concatenate([a, np.ones((a.shape[0], 1))], axis=1)
    bh = np.concatenate([b, np.ones((b.shape[0], 1))], axis=1)
    l = ah @ F.T
    mm = bh @ F
    e = np.abs(np.sum(bh * l, axis=1))
    return e / np.hypot(l[:, 0], l[:, 1]), e / np.hypot(mm[:, 0], mm[:, 1])


def make_scene(seed, n_in, n_out, noise=0.0, planar=False):
    """A translating camera over non-coplanar points (planar=True: all points on one plane).  Returns dict(m [n,4] matches in
    a shuffled order, truth [n] bool, F [3,3] the true matrix); inliers are exact projections (plus `noise` px of gaussian
    noise when asked), outliers lie at least MARGIN px from both of their epipolar lines."""
    rng = np.random.RandomState(seed)
    t = np.array([0.5, 0.12, 0.2]) * (1.0 + 0.2 * rng.rand())
    F = true_F(t)

    def project(X, f=FOCAL):
        return np.stack([f * X[:, 0] / X[:, 2] + WIDTH / 2, f * X[:, 1] / X[:, 2] + HEIGHT / 2], axis=1)

    a_in, b_in = np.zeros((0, 2)), np.zeros((0, 2))
    while a_in.shape[0] < n_in:
        a = np.stack([rng.uniform(8, WIDTH - 8, 4 * n_in + 8), rng.uniform(8, HEIGHT - 8, 4 * n_in + 8)], axis=1)
        z = rng.uniform(3.0, 12.0, a.shape[0])
        if planar:
            z = 6.0 / (1.0 + 0.3 * (a[:, 0] - WIDTH / 2) / FOCAL + 0.2 * (a[:, 1] - HEIGHT / 2) / FOCAL)   # 0.3 X + 0.2 Y + Z = 6
        X = np.stack([(a[:, 0] - WIDTH / 2) * z / FOCAL, (a[:, 1] - HEIGHT / 2) * z / FOCAL, z], axis=1)
        a, b = project(X), project(X - t, FOCAL2)
        ok = (b[:, 0] > 4) & (b[:, 0] < WIDTH - 4) & (b[:, 1] > 4) & (b[:, 1] < HEIGHT - 4)
        a_in, b_in = np.concatenate([a_in, a[ok]]), np.concatenate([b_in, b[ok]])
    a_in, b_in = a_in[:n_in], b_in[:n_in]
    if noise > 0.0:
        a_in = a_in + noise * rng.randn(n_in, 2)
        b_in = b_in + noise * rng.randn(n_in, 2)
    a_out, b_out = np.zeros((0, 2)), np.zeros((0, 2))
    while a_out.shape[0] < n_out:
        a = np.stack([rng.uniform(8, WIDTH - 8, 4 * n_out + 8), rng.uniform(8, HEIGHT - 8, 4 * n_out + 8)], axis=1)
        b = np.stack([rng.uniform(8, WIDTH - 8, 4 * n_out + 8), rng.uniform(8, HEIGHT - 8, 4 * n_out + 8)], axis=1)
        d1, d2 = line_dist(F, a, b)
        ok = (d1 >= MARGIN) & (d2 >= MARGIN)
        a_out, b_out = np.concatenate([a_out, a[ok]]), np.concatenate([b_out, b[ok]])
    m = np.concatenate([np.concatenate([a_in, b_in], axis=1), np.concatenate([a_out[:n_out], b_out[:n_out]], axis=1)])
    truth = np.arange(n_in + n_out) < n_in
    order = rng.permutation(n_in + n_out)
    return {"m": np.ascontiguousarray(m[order]), "truth": truth[order], "F": F}


def as_arrays(m, cap, pt_stride, rng):
    """Matches m [n,4] as the operator's inputs: pts1 [cap,pt_stride] (row i = a of match i), pts2 [cap,pt_stride] with the
    b points scattered by a permutation, match [cap,3] float32 rows (i, j, d) in ascending i."""
    n = m.shape[0]
    pts1, pts2 = np.zeros((cap, pt_stride)), np.zeros((cap, pt_stride))
    match = np.zeros((cap, 3), dtype=np.float32)
    perm = rng.permutation(n)
    pts1[:n, :2] = m[:, :2]
    pts2[perm, :2] = m[:, 2:]
    if pt_stride > 2:
        pts1[:, 2:] = rng.rand(cap, pt_stride - 2)
        pts2[:, 2:] = rng.rand(cap, pt_stride - 2)
    match[:n, 0] = np.arange(n)
    match[:n, 1] = perm
    match[:n, 2] = rng.rand(n).astype(np.float32)
    return pts1, pts2, match


# ---- the fixtures of tests/test_gpu_epipolar.py; tests/test_epipolar_cpu.py sums their refits in two orders ------------------
# name -> (scene seed, inliers, outliers, noise px, planar, RANSAC seed).  The seeds were searched with this restatement so that
# the winner's mask equals the truth on the noise-free scenes (the 25 px margin alone does not guarantee that with few
# matches); tests/test_epipolar_cpu.py asserts it for every one of them.
CASES = {
    "mixed48": (0, 32, 16, 0.0, False, 100),
    "eight": (1, 8, 0, 0.0, False, 101),
    "five": (2, 5, 0, 0.0, False, 102),
    "empty": (3, 0, 0, 0.0, False, 103),
    "n257": (0, 200, 57, 0.0, False, 100),
    "n4096": (0, 3000, 1096, 0.0, False, 100),
    "noisy": (3, 150, 100, 0.3, False, 103),
    "planar": (4, 48, 0, 0.0, True, 104),
}
NOISE_FREE = ("mixed48", "eight", "n257", "n4096")
# The fixtures whose F and err are compared.  The planar scene has none: each of its 2000 systems has rank 6 and is refused
# by the pivot rule (largest smallest-pivot 5.2e-16 against PIVOT_EPS = 1e-12), so its answer is status 1, winner -1, an
# empty mask (decisions() reports the margin; tests/test_epipolar_exact_cpu.py asserts it).
F_COMPARED = ("mixed48", "eight", "n257", "n4096", "noisy")
# The largest difference of F and err between the ascending and the pairwise refit over F_COMPARED, as
# order_difference(F_COMPARED) returned it when the fixtures were fixed (the err of "eight"), and the tolerance of the device
# results against the restatement: 16 times that.
ORDER_DIFFERENCE = 1.8371624549316226e-12
TOLERANCE = 16.0 * ORDER_DIFFERENCE


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(m [n,4], truth [n], F_true, seed, ref = ransac(ascending sums), ref_pairwise = ransac(pairwise sums)); computed
    once and shared: treat it as read-only."""
    scene_seed, n_in, n_out, noise, planar, seed = CASES[name]
    sc = make_scene(scene_seed, n_in, n_out, noise=noise, planar=planar)
    w = winner_of(sc["m"], seed)
    return {"m": sc["m"], "truth": sc["truth"], "F_true": sc["F"], "seed": seed, "ref": ransac(sc["m"], seed, winner=w),
            "ref_pairwise": ransac(sc["m"], seed, pairwise=True, winner=w)}


def order_difference(names=tuple(CASES)):
    """The largest difference of F and err between the ascending and the pairwise refit over the named fixtures."""
    worst = 0.0
    for nm in names:
        c = case(nm)
        a, b = c["ref"], c["ref_pairwise"]
        assert a["status"] == b["status"] and a["winner"] == b["winner"] and np.array_equal(a["mask"], b["mask"])
        worst = max(worst, float(np.abs(a["F"] - b["F"]).max()), abs(a["err"] - b["err"]))
    return worst
