"""numpy restatement of the absolute pose from landmarks (csrc/pnp_kernels.hip.h): the join of landmark rows
with the matches of the next frame (`join`), the P3P RANSAC (`sample4`, `p3p`, `hypotheses`, `ransac`: 512 hypotheses, quartic in
the depth ratio, roots by bracketing between the derivative's roots and bisection, pose from two orthonormal frames, the fourth
point picks the solution), the Gauss-Newton refit with the Cayley update (`refit`) and the repair of a flagged trajectory row
(`repair`).  There is no reference counterpart and no OpenCV here, so this file is the specification the kernels are tested
against.  Camera model of section 26: y = Rw (X - C), u = fx * y0 / y2 + cx.  Everything is fp64 in the parenthesisation written
here, vectorised over the hypotheses or over the rows; the sums over the rows repeat block_sum's order (`block_sum`), so the
device agrees to the last bit wherever its sqrt and division are correctly rounded.  Every function also runs in another "way"
(pose_ref.WAY2: numpy.longdouble where that is wider than float64, else the dot products in the reverse order), which is how the
tolerance of the continuous outputs is measured (`way_difference`).  Also the fixtures."""
import functools

import numpy as np

from tests import epipolar_ref as E
from tests import eval_restatement as ER
from tests import landmarks_ref as L
from tests import pose_ref as P

HYPOTHESES = 512       # fixed; see DESIGN.md section 27 for the derivation
SAMPLE_DRAWS = ER.SAMPLE_DRAWS
V_MAX = 32.0           # roots of the quartic are looked for in (0, V_MAX]: the ratio of two depths of one camera
BISECTIONS = 64
GN_STEPS = 4
PIVOT_EPS = 1e-12
FRAME_EPS = 1e-12      # |e1 x e2|^2 <= FRAME_EPS |e1|^2 |e2|^2: a collinear or coincident triple
CORR_WORDS = 8         # X, Y, Z, px, py, landmark row, valid, 0
THREADS = 256
SCALE_FRACTION = 1.0 / 64.0    # repair: a step shorter than this share of the previous scale does not set the scale
FLAG_ABSOLUTE = 4
THRESH, MIN_INLIERS = 2.0, 6   # the defaults of the public interface
WAY1, WAY2 = P.WAY1, P.WAY2


def _dot(p, q, rev=False):
    return P._dot(p, q, rev)


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


# ---- the join ------------------------------------------------------------------------------------------------------------------
def join(landmarks, n_landmarks, match, n_match, pts_new):
    """Correspondence rows [cap, CORR_WORDS] aligned with the match rows, and (n, n_valid).  landmarks [row_cap, LANDMARK_WORDS],
    match [cap, 3] rows (i, j, d) of the pair (previous, new), pts_new [point_cap, >= 2].  The landmark of a previous-frame point is
    the lowest landmark row whose eighth word names it."""
    landmarks = np.asarray(landmarks, dtype=np.float64).reshape(-1, L.LANDMARK_WORDS)
    match = np.asarray(match)
    pts_new = np.asarray(pts_new, dtype=np.float64)
    cap, point_cap = match.shape[0], pts_new.shape[0]
    nl = min(max(int(n_landmarks), 0), landmarks.shape[0])
    n = min(max(int(n_match), 0), cap)
    owner = {}
    for r in range(nl):
        w = landmarks[r, 7]
        if np.isfinite(w) and 0.0 <= w < point_cap and int(w) not in owner:
            owner[int(w)] = r
    out = np.zeros((cap, CORR_WORDS))
    n_valid = 0
    for k in range(n):
        i = min(max(int(match[k, 0]), 0), point_cap - 1)
        j = min(max(int(match[k, 1]), 0), point_cap - 1)
        if i not in owner:
            continue
        r = owner[i]
        row = [landmarks[r, 1], landmarks[r, 2], landmarks[r, 3], pts_new[j, 0], pts_new[j, 1]]
        if not all(np.isfinite(row)):
            continue
        out[k, :5], out[k, 5], out[k, 6] = row, r, 1.0
        n_valid += 1
    return out, (n, n_valid)


# ---- sampling ------------------------------------------------------------------------------------------------------------------
def total_hypotheses(n):
    return 0 if n < 4 else (1 if n == 4 else HYPOTHESES)


def sample4(seed, h, n, valid):
    """The 4 rows of hypothesis h: section 22's redraw rule, a draw that hits an invalid row is redrawn too.  None: the draws do not
    give 4 distinct valid rows."""
    if n == 4:
        ids = [0, 1, 2, 3]
    else:
        c, ids = 0, []
        for _ in range(4):
            while True:
                v = ER.draw(seed, h, c, n)
                c += 1
                if (v not in ids and valid[v]) or c >= SAMPLE_DRAWS:
                    break
            ids.append(v)
    return ids if len(set(ids)) == 4 and all(valid[v] for v in ids) else None


# ---- the minimal solve ---------------------------------------------------------------------------------------------------------
def bearing(px, py, k, rev=False):
    x, y = (px - k[2]) / k[0], (py - k[3]) / k[1]
    one = np.ones_like(x)
    nrm = np.sqrt(_dot((x, y, one), (x, y, one), rev))
    return [x / nrm, y / nrm, one / nrm]


def quartic(aa, bb, cc, ca, cb, cg):
    """(g [5] ascending, normalised by the largest |coefficient|; n [3], m [2] of u = N(v) / M(v); ok)."""
    A, Cc = aa / bb, cc / bb
    K = A - Cc
    n0, n1, n2 = -1.0 - K, (2.0 * K) * cb, 1.0 - K
    m0, m1 = -2.0 * cg, 2.0 * ca
    q0, q1, q2 = 1.0 - Cc, (2.0 * Cc) * cb, -Cc
    NN = [n0 * n0, 2.0 * (n0 * n1), 2.0 * (n0 * n2) + n1 * n1, 2.0 * (n1 * n2), n2 * n2]
    NM = [n0 * m0, n0 * m1 + n1 * m0, n1 * m1 + n2 * m0, n2 * m1]
    MM = [m0 * m0, 2.0 * (m0 * m1), m1 * m1]
    QM = [q0 * MM[0], q0 * MM[1] + q1 * MM[0], (q0 * MM[2] + q1 * MM[1]) + q2 * MM[0], q1 * MM[2] + q2 * MM[1], q2 * MM[2]]
    tc = 2.0 * cg
    g = [(NN[k] - tc * NM[k]) + QM[k] for k in range(4)] + [NN[4] + QM[4]]
    big = np.abs(g[0])
    for k in range(1, 5):
        big = np.where(np.abs(g[k]) > big, np.abs(g[k]), big)
    ok = np.isfinite(big) & (big > 0.0)
    return [gk / big for gk in g], (n0, n1, n2), (m0, m1), ok


def _horner(c, v):
    acc = c[-1]
    for k in range(len(c) - 2, -1, -1):
        acc = acc * v + c[k]
    return acc


def _bisect(c, lo, hi):
    """(root, sign change) of the polynomial c in [lo, hi]: BISECTIONS halvings, the half that keeps the sign change."""
    slo = _horner(c, lo) < 0.0
    change = slo != (_horner(c, hi) < 0.0)
    half = lo.dtype.type(0.5)
    for _ in range(BISECTIONS):
        mid = half * (lo + hi)
        same = (_horner(c, mid) < 0.0) == slo
        lo, hi = np.where(same, mid, lo), np.where(same, hi, mid)
    return half * (lo + hi), change


def _clamp(x):
    vmax = x.dtype.type(V_MAX)
    return np.where(np.isfinite(x), np.where(x < 0.0, 0.0, np.where(x > vmax, vmax, x)), 0.0).astype(x.dtype)


def quartic_roots(g):
    """(v [4], valid [4]): the roots of g in (0, V_MAX] with a sign change, one per bracket between the roots of g'."""
    zero, vmax = np.zeros_like(g[0]), np.full_like(g[0], V_MAX)
    d = [g[1], 2.0 * g[2], 3.0 * g[3], 4.0 * g[4]]
    e = [d[1], 2.0 * d[2], 3.0 * d[3]]
    disc = e[1] * e[1] - 4.0 * (e[2] * e[0])
    sq = np.sqrt(disc)
    ra, rb = _clamp((-e[1] - sq) / (2.0 * e[2])), _clamp((-e[1] + sq) / (2.0 * e[2]))
    c_lo, c_hi = np.where(rb < ra, rb, ra), np.where(rb < ra, ra, rb)
    crit = []
    for lo, hi in ((zero, c_lo), (c_lo, c_hi), (c_hi, vmax)):
        r, ch = _bisect(d, lo, hi)
        crit.append(np.where(ch, r, lo))
    roots, valid = [], []
    for lo, hi in ((zero, crit[0]), (crit[0], crit[1]), (crit[1], crit[2]), (crit[2], vmax)):
        r, ch = _bisect(g, lo, hi)
        roots.append(r)
        valid.append(ch)
    return roots, valid


def _frame(e1, e2, rev):
    """(w1, w2, w3, ok) of the triangle with the edges e1, e2 from its first corner."""
    n = _cross(e1, e2)
    l1, l2, ln = _dot(e1, e1, rev), _dot(e2, e2, rev), _dot(n, n, rev)
    ok = np.isfinite(ln) & (ln > FRAME_EPS * (l1 * l2))
    s1, sn = np.sqrt(l1), np.sqrt(ln)
    w1 = [e1[k] / s1 for k in range(3)]
    w3 = [n[k] / sn for k in range(3)]
    return w1, _cross(w3, w1), w3, ok


def view(R, C, X, px, k, rev=False):
    """(squared reprojection error, in front) of the points X (list of 3) against the pixels px (list of 2) under (R [9], C [3])."""
    q = [X[0] - C[0], X[1] - C[1], X[2] - C[2]]
    y0, y1, y2 = _dot(R[0:3], q, rev), _dot(R[3:6], q, rev), _dot(R[6:9], q, rev)
    r0, r1 = (k[0] * (y0 / y2) + k[2]) - px[0], (k[1] * (y1 / y2) + k[3]) - px[1]
    return r0 * r0 + r1 * r1, np.isfinite(y2) & (y2 > 0.0)


def p3p(X, px, k, rev=False, want_all=False):
    """The pose of B samples.  X: 4 points, each a list of 3 arrays [B]; px: 4 pixels, each a list of 2 arrays [B]; k: (fx, fy, cx,
    cy).  Returns (R [9] arrays, C [3] arrays, ok [B]); want_all: the list of the four (R, C, ok) before the fourth point picks."""
    with np.errstate(all="ignore"):
        f = [bearing(px[i][0], px[i][1], k, rev) for i in range(3)]
        d23 = [X[1][c] - X[2][c] for c in range(3)]
        d13 = [X[0][c] - X[2][c] for c in range(3)]
        d12 = [X[0][c] - X[1][c] for c in range(3)]
        aa, bb, cc = _dot(d23, d23, rev), _dot(d13, d13, rev), _dot(d12, d12, rev)
        ca, cb, cg = _dot(f[1], f[2], rev), _dot(f[0], f[2], rev), _dot(f[0], f[1], rev)
        g, (n0, n1, n2), (m0, m1), ok_q = quartic(aa, bb, cc, ca, cb, cg)
        roots, valid = quartic_roots(g)
        e1 = [X[1][c] - X[0][c] for c in range(3)]
        e2 = [X[2][c] - X[0][c] for c in range(3)]
        w1, w2, w3, ok_w = _frame(e1, e2, rev)
        zero = np.zeros_like(aa)
        best = np.full_like(aa, np.inf)
        Rb = [zero.copy() for _ in range(9)]
        Cb = [zero.copy() for _ in range(3)]
        found = np.zeros(aa.shape, dtype=bool)
        every = []
        for r in range(4):
            v = roots[r]
            D = (1.0 + v * v) - (2.0 * v) * cb
            u = ((n0 + n1 * v) + n2 * (v * v)) / (m0 + m1 * v)
            ok = valid[r] & ok_q & ok_w & np.isfinite(u) & (u > 0.0) & np.isfinite(D) & (D > 0.0) & (v > 0.0)
            s1 = np.sqrt(bb / D)
            s2, s3 = u * s1, v * s1
            Y1 = [s1 * f[0][c] for c in range(3)]
            Y2 = [s2 * f[1][c] for c in range(3)]
            Y3 = [s3 * f[2][c] for c in range(3)]
            c1, c2, c3, ok_c = _frame([Y2[c] - Y1[c] for c in range(3)], [Y3[c] - Y1[c] for c in range(3)], rev)
            R = [(c1[i] * w1[j] + c2[i] * w2[j]) + c3[i] * w3[j] for i in range(3) for j in range(3)]
            C = [X[0][j] - _dot((R[j], R[3 + j], R[6 + j]), Y1, rev) for j in range(3)]
            e4, front = view(R, C, X[3], px[3], k, rev)
            ok = ok & ok_c & front & np.isfinite(e4)
            every.append((R, C, ok))
            take = ok & (e4 < best)
            best = np.where(take, e4, best)
            found |= take
            Rb = [np.where(take, R[i], Rb[i]) for i in range(9)]
            Cb = [np.where(take, C[i], Cb[i]) for i in range(3)]
        return every if want_all else (Rb, Cb, found)


def hypotheses(corr, n, k, seed, hs, way=WAY1):
    """Hypotheses hs of one problem: (R [B,9], C [B,3], ok [B])."""
    dt, rev = way
    corr = np.asarray(corr, dtype=np.float64)
    valid = corr[:, 6] != 0.0
    k = np.asarray(k, dtype=dt)
    ids = [sample4(seed, h, n, valid) for h in hs]
    have = np.array([s is not None for s in ids], dtype=bool)
    idx = np.array([s if s is not None else [0, 0, 0, 0] for s in ids], dtype=np.int64).reshape(-1, 4)
    X = [[corr[idx[:, i], c].astype(dt) for c in range(3)] for i in range(4)]
    px = [[corr[idx[:, i], 3 + c].astype(dt) for c in range(2)] for i in range(4)]
    R, C, ok = p3p(X, px, k, rev)
    return np.stack(R, axis=1), np.stack(C, axis=1), ok & have


def inliers(R, C, corr, n, k, thresh, way=WAY1):
    """mask [B, n] of the rows under B poses (R [B,9], C [B,3]), and the squared errors."""
    dt, rev = way
    corr = np.asarray(corr, dtype=np.float64)[:n].astype(dt)
    k = np.asarray(k, dtype=dt)
    t2 = dt(thresh) * dt(thresh)
    with np.errstate(all="ignore"):
        e, front = view([R[:, i, None] for i in range(9)], [C[:, i, None] for i in range(3)],
                        [corr[None, :, c] for c in range(3)], [corr[None, :, 3 + c] for c in range(2)], k, rev)
        return (corr[None, :, 6] != 0.0) & front & (e <= t2), e


# ---- sums in block_sum's order (csrc/geom_blocks.hip.h) --------------------------------------------------------------------------------------------
def block_sum(vals, active):
    """Sum over the rows of vals [n, M] where active [n]: thread t adds rows t, t + 256, ... in order, the xor butterfly inside each
    wave of 64, the four wave partials in wave order."""
    vals = np.asarray(vals)
    part = np.zeros((THREADS,) + vals.shape[1:], dtype=vals.dtype)
    for base in range(0, vals.shape[0], THREADS):
        chunk, act = vals[base:base + THREADS], active[base:base + THREADS]
        m = chunk.shape[0]
        part[:m] = np.where(act.reshape((m,) + (1,) * (vals.ndim - 1)), part[:m] + chunk, part[:m])
    v = part.reshape((THREADS // 64, 64) + vals.shape[1:])
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lanes ^ o]
    red = v[:, 0]
    t = red[0]
    for w in range(1, THREADS // 64):
        t = t + red[w]
    return t


# ---- the refit -----------------------------------------------------------------------------------------------------------------
def solve_pivot(a, trace=None):
    """x of the N x (N+1) augmented system a (A x = last column) by Gaussian elimination with complete pivoting, the rule of
    epipolar_ref.null_vector: the largest |entry| of the remaining block, the lowest row then the lowest column on ties.  Returns
    (x [N], ok)."""
    a = np.array(a)
    dt = a.dtype.type
    N = a.shape[0]
    perm = list(range(N))
    ok = True
    with np.errstate(all="ignore"):
        for k in range(N):
            best, pr, pc = dt(-1.0), k, k
            for r in range(k, N):
                for c in range(k, N):
                    v = abs(a[r, c])
                    if v > best:
                        best, pr, pc = v, r, c
            if trace is not None:
                trace.append((pr, pc))
            a[[k, pr], :] = a[[pr, k], :]
            a[:, [k, pc]] = a[:, [pc, k]]
            perm[k], perm[pc] = perm[pc], perm[k]
            ok = ok and bool(abs(a[k, k]) > PIVOT_EPS)
            inv = dt(1.0) / a[k, k]
            for r in range(k + 1, N):
                m = a[r, k] * inv
                for c in range(k + 1, N + 1):
                    a[r, c] = a[r, c] - m * a[k, c]
        x = np.zeros(N, dtype=a.dtype)
        for k in range(N - 1, -1, -1):
            s = a[k, N]
            for c in range(k + 1, N):
                s = s - a[k, c] * x[c]
            x[k] = s / a[k, k]
    out = np.zeros(N, dtype=a.dtype)
    for c in range(N):
        out[perm[c]] = x[c]
    return out, ok and bool(np.all(np.isfinite(out)))


def cayley_update(R, t, delta, rev=False):
    """R <- orthonormalised(Cay(w) R), t <- Cay(w) t + dt for delta = (w [3], dt [3]); Cay(w) = (I - [w/2]x)^-1 (I + [w/2]x)
    = ((1 - a.a) I + 2 a a^T + 2 [a]x) / (1 + a.a), a = w / 2.  R [9], t [3] arrays of scalars."""
    dtp = R.dtype.type
    a = [dtp(0.5) * delta[0], dtp(0.5) * delta[1], dtp(0.5) * delta[2]]
    aa = _dot(a, a, rev)
    den, om = dtp(1.0) + aa, dtp(1.0) - aa
    two = dtp(2.0)
    Q = [(om + two * (a[0] * a[0])) / den, (two * (a[0] * a[1]) - two * a[2]) / den, (two * (a[0] * a[2]) + two * a[1]) / den,
         (two * (a[0] * a[1]) + two * a[2]) / den, (om + two * (a[1] * a[1])) / den, (two * (a[1] * a[2]) - two * a[0]) / den,
         (two * (a[0] * a[2]) - two * a[1]) / den, (two * (a[1] * a[2]) + two * a[0]) / den, (om + two * (a[2] * a[2])) / den]
    M = [_dot(Q[3 * i:3 * i + 3], (R[j], R[3 + j], R[6 + j]), rev) for i in range(3) for j in range(3)]
    tn = [_dot(Q[3 * i:3 * i + 3], t, rev) + delta[3 + i] for i in range(3)]
    # the renormalisation: row 0 scaled to unit length, row 1 made orthogonal to it and scaled, row 2 their cross product
    n0 = np.sqrt(_dot(M[0:3], M[0:3], rev))
    r0 = [M[0] / n0, M[1] / n0, M[2] / n0]
    p = _dot(M[3:6], r0, rev)
    w = [M[3] - p * r0[0], M[4] - p * r0[1], M[5] - p * r0[2]]
    n1 = np.sqrt(_dot(w, w, rev))
    r1 = [w[0] / n1, w[1] / n1, w[2] / n1]
    r2 = _cross(r0, r1)
    return np.array(r0 + r1 + r2, dtype=R.dtype), np.array(tn, dtype=R.dtype)


def moments(R, t, corr, mask, k, rev=False):
    """(H [6,6], g [6]) of the Gauss-Newton step over the masked rows; parameters (w [3], dt [3]) of y <- Cay(w) y + dt."""
    X = [corr[:, c] for c in range(3)]
    y0, y1, y2 = (_dot(R[3 * i:3 * i + 3], X, rev) + t[i] for i in range(3))
    un, vn = y0 / y2, y1 / y2
    r0, r1 = (k[0] * un + k[2]) - corr[:, 3], (k[1] * vn + k[3]) - corr[:, 4]
    fa, fb = k[0] / y2, k[1] / y2
    zero = np.zeros_like(y0)
    j0 = [fa * (0.0 - un * y1), fa * (y2 + un * y0), fa * (0.0 - y1), fa, zero, fa * (0.0 - un)]
    j1 = [fb * ((0.0 - y2) - vn * y1), fb * (vn * y0), fb * y0, zero, fb, fb * (0.0 - vn)]
    cols = [j0[p] * j0[q] + j1[p] * j1[q] for p in range(6) for q in range(p, 6)] + [j0[p] * r0 + j1[p] * r1 for p in range(6)]
    s = block_sum(np.stack(cols, axis=1), mask)
    H = np.zeros((6, 6), dtype=s.dtype)
    e = 0
    for p in range(6):
        for q in range(p, 6):
            H[p, q] = H[q, p] = s[e]
            e += 1
    return H, s[21:27]


def refit(R, C, corr, n, mask, k, way=WAY1):
    """GN_STEPS Gauss-Newton steps from (R [9], C [3]) over the masked rows: (R [9], C [3]).  A refused solve or a non-finite update
    keeps the current pose; the steps still run."""
    dt, rev = way
    corr = np.asarray(corr, dtype=np.float64)[:n].astype(dt)
    k = np.asarray(k, dtype=dt)
    R = np.asarray(R, dtype=dt).reshape(9)
    C = np.asarray(C, dtype=dt).reshape(3)
    with np.errstate(all="ignore"):
        t = np.array([-_dot(R[3 * i:3 * i + 3], C, rev) for i in range(3)], dtype=dt)
        for _ in range(GN_STEPS):
            H, g = moments(R, t, corr, mask, k, rev)
            delta, ok = solve_pivot(np.concatenate([H, -g[:, None]], axis=1))
            if not ok:
                continue
            Rn, tn = cayley_update(R, t, delta, rev)
            if np.all(np.isfinite(Rn)) and np.all(np.isfinite(tn)):
                R, t = Rn, tn
        C = np.array([-_dot((R[j], R[3 + j], R[6 + j]), t, rev) for j in range(3)], dtype=dt)
    return R, C


# ---- the RANSAC ----------------------------------------------------------------------------------------------------------------
def ransac(corr, n, k, seed, thresh=THRESH, min_inliers=MIN_INLIERS, way=WAY1, winner=None):
    """One problem.  corr [cap, CORR_WORDS], n rows used, k = (fx, fy, cx, cy).  Returns dict(Rw [3,3], C [3], mask [cap] bool,
    n_inliers, winner, rms, status, score: the winner's count before the refit).  winner: skip the search (the other way's)."""
    dt, rev = way
    corr = np.asarray(corr, dtype=np.float64).reshape(-1, CORR_WORDS)
    cap = corr.shape[0]
    n = min(max(int(n), 0), cap)
    out = {"Rw": np.eye(3, dtype=dt), "C": np.zeros(3, dtype=dt), "mask": np.zeros(cap, dtype=bool), "n_inliers": 0, "winner": -1,
           "rms": dt(0.0), "status": 1, "score": 0}
    total = total_hypotheses(n)
    if total == 0:
        return out
    if winner is None:
        hs = list(range(total))
        R, C, ok = hypotheses(corr, n, k, seed, hs, way)
        m, _ = inliers(R, C, corr, n, k, thresh, way)
        score = np.where(ok, m.sum(axis=1), -1)
        winner = int(np.argmax(score))             # the first maximum: the lowest h
        if score[winner] < 0:
            return out
    R, C, ok = hypotheses(corr, n, k, seed, [winner], way)
    if not ok[0]:
        return out
    m0, e0 = inliers(R, C, corr, n, k, thresh, way)
    m0, k0 = m0[0], int(m0[0].sum())
    if k0 < max(int(min_inliers), 4):
        return out
    R1, C1 = refit(R[0], C[0], corr, n, m0, k, way)
    m1, e1 = inliers(R1[None], C1[None], corr, n, k, thresh, way)
    m1, k1 = m1[0], int(m1[0].sum())
    if np.all(np.isfinite(R1)) and np.all(np.isfinite(C1)) and k1 >= k0:
        Rf, Cf, mf, ef, kf = R1, C1, m1, e1[0], k1
    else:
        Rf, Cf, mf, ef, kf = R[0], C[0], m0, e0[0], k0
    with np.errstate(all="ignore"):
        rms = np.sqrt(block_sum(ef[:, None], mf)[0] / (dt(2.0) * dt(kf)))
    mask = np.zeros(cap, dtype=bool)
    mask[:n] = mf
    out.update(Rw=Rf.reshape(3, 3), C=Cf, mask=mask, n_inliers=kf, winner=winner, rms=rms, status=0, score=k0)
    return out


# ---- the repair ----------------------------------------------------------------------------------------------------------------
def repair(absolute, state, table, way=WAY1):
    """The repaired (state [STATE_WORDS], table [capacity, ROW_WORDS]) of one sequence (copies).  absolute: dict(Rw, C, status).
    Acts on the newest row, n - 1 with 1 <= n < capacity rows in the table (a full table is left alone: its last row need not be
    the newest frame's), when that row carries flag bit 0 or 1, the absolute pose has status 0 and is finite."""
    dt, rev = way
    state, table = np.array(state, dtype=dt), np.array(table, dtype=dt).reshape(-1, P.ROW_WORDS)
    capacity = table.shape[0]
    nf = state[0]
    n = int(nf) if 0.0 <= nf < 2147483647.0 else 0
    if not (1 <= n < capacity) or int(absolute["status"]) != 0:
        return state, table
    row = table[n - 1]
    flags = int(row[14])
    Rw, C = np.asarray(absolute["Rw"], dtype=dt).reshape(9), np.asarray(absolute["C"], dtype=dt).reshape(3)
    if not (flags & 3) or not (np.all(np.isfinite(Rw)) and np.all(np.isfinite(C))):
        return state, table
    tw = np.array([-_dot(Rw[3 * i:3 * i + 3], C, rev) for i in range(3)], dtype=dt)
    s, keep = state[1], flags & 2
    if n >= 2:
        d = C - table[n - 2, 9:12]
        with np.errstate(all="ignore"):
            length = np.sqrt(_dot(d, d, rev))
        if np.isfinite(length) and length > dt(SCALE_FRACTION) * s:
            s, keep = length, 0
    row[0:9], row[9:12], row[12], row[14] = Rw, C, s, dt(keep | FLAG_ABSOLUTE)
    state[1], state[2:11], state[11:14] = s, Rw, tw
    return state, table


# ---- fixtures ------------------------------------------------------------------------------------------------------------------
SALT_MARGIN = 25.0
# name -> (scene seed, frames, points, motion, zoom, frame whose camera is solved for, noise px, share of salted rows, rows behind
# the camera, invalid rows, RANSAC seed, seed of the salt).  The seeds were searched with the restatement so that on the
# noise-free fixtures the mask equals the truth; tests/test_pnp_cpu.py asserts that before anything else.
CASES = {
    "side48": (60, 3, 48, "side", False, 2, 0.0, 0.0, 0, 0, 300, 0),
    "forward": (61, 3, 60, "forward", False, 2, 0.0, 0.0, 0, 0, 301, 0),
    "zoom": (62, 3, 60, "side", True, 2, 0.0, 0.0, 0, 0, 302, 0),
    "six": (63, 2, 6, "side", False, 1, 0.0, 0.0, 0, 0, 303, 0),
    "four": (64, 2, 4, "side", False, 1, 0.0, 0.0, 0, 0, 304, 0),
    "n257": (65, 2, 257, "side", True, 1, 0.0, 0.3, 6, 5, 305, 1),
    "n4096": (66, 2, 4096, "side", True, 1, 0.0, 0.3, 40, 11, 306, 2),
    "noisy": (67, 3, 150, "side", True, 2, 0.3, 0.0, 0, 0, 307, 0),
    "salted": (68, 3, 100, "side", False, 2, 0.0, 0.3, 5, 3, 308, 3),
}
NOISE_FREE = tuple(k for k, v in CASES.items() if v[6] == 0.0) + ("planar",)
COMPARED = ("side48", "forward", "zoom", "six", "n257", "n4096", "noisy", "salted", "planar")   # what the tolerance is measured on
PLANAR = (69, 80, 0.3, 4, 2, 309, 4)          # scene seed, points, salt, behind, invalid, RANSAC seed, salt seed


def _project(X, Rw, C, k):
    Y = (X - C) @ Rw.T
    return np.stack([k[0] * Y[:, 0] / Y[:, 2] + k[2], k[1] * Y[:, 1] / Y[:, 2] + k[3]], axis=1), Y[:, 2]


def make_problem(X, Rw, C, k, noise, salt, behind, invalid, salt_seed):
    """corr [n, CORR_WORDS] and truth [n] of the points X seen by the camera (Rw, C, k): `salt` of the rows get a pixel at least
    SALT_MARGIN from the true one, `behind` rows a point behind the camera (their pixel is the mirrored point's), `invalid` rows
    a cleared valid word; truth = none of the three."""
    rng = np.random.RandomState(7000 + salt_seed)
    n = X.shape[0]
    px, z = _project(X, Rw, C, k)
    assert (z > 0.5).all()
    if noise > 0.0:
        px = px + noise * rng.randn(n, 2)
    corr = np.zeros((n, CORR_WORDS))
    corr[:, 0:3], corr[:, 3:5], corr[:, 5], corr[:, 6] = X, px, np.arange(n), 1.0
    truth = np.ones(n, dtype=bool)
    order = rng.permutation(n)
    n_salt = int(round(salt * n))
    for r in order[:n_salt]:
        while True:
            q = np.array([rng.uniform(8, E.WIDTH - 8), rng.uniform(8, E.HEIGHT - 8)])
            if np.linalg.norm(q - px[r]) >= SALT_MARGIN:
                break
        corr[r, 3:5], truth[r] = q, False
    for r in order[n_salt:n_salt + behind]:
        Y = (X[r] - C) @ Rw.T
        corr[r, 0:3], truth[r] = C + (Y * np.array([1.0, 1.0, -1.0])) @ Rw, False
    for r in order[n_salt + behind:n_salt + behind + invalid]:
        corr[r, 6], truth[r] = 0.0, False
    return corr, truth


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(corr [n, CORR_WORDS], n, k [4], seed, truth [n], Rw, C (true), res / res2: ransac in WAY1 / WAY2 with the defaults);
    computed once: treat it as read-only."""
    if name == "planar":
        scene_seed, n, salt, behind, invalid, seed, salt_seed = PLANAR
        rng = np.random.RandomState(scene_seed)
        k = P.intrinsics_of(0, False)
        a = np.stack([rng.uniform(8, E.WIDTH - 8, n), rng.uniform(8, E.HEIGHT - 8, n)], axis=1)
        x, y = (a[:, 0] - k[2]) / k[0], (a[:, 1] - k[3]) / k[1]
        z = 6.0 / (1.0 - 0.3 * x + 0.2 * y)                       # the plane Z = 6 + 0.3 X - 0.2 Y of camera 0's frame
        X = np.stack([x * z, y * z, z], axis=1)
        Rw = P._rodrigues(np.array([2.0, -9.0, 3.0]))
        C = np.array([0.7, -0.2, 0.4])
        noise = 0.0
    else:
        scene_seed, frames, n, motion, zoom, f, noise, salt, behind, invalid, seed, salt_seed = CASES[name]
        seq = P.make_sequence(scene_seed, frames, n, 0, motion=motion, zoom=zoom)
        X = L.scene_points(scene_seed, frames, n, motion, zoom)
        Rws, Cs = L.true_poses(seq)
        Rw, C, k = Rws[f], Cs[f], seq["intr"][f]
    corr, truth = make_problem(X, Rw, C, k, noise, salt, behind, invalid, salt_seed)
    out = {"corr": corr, "n": corr.shape[0], "k": np.asarray(k, dtype=np.float64), "seed": seed, "truth": truth, "Rw": Rw, "C": C,
           "noise": noise}
    out["res"] = ransac(corr, out["n"], k, seed, way=WAY1)
    out["res2"] = ransac(corr, out["n"], k, seed, way=WAY2, winner=out["res"]["winner"] if out["res"]["status"] == 0 else None)
    return out


def result_difference(a, b):
    """The largest difference of Rw, C, rms between two results; the discrete outputs must agree."""
    assert a["status"] == b["status"] and a["n_inliers"] == b["n_inliers"] and a["winner"] == b["winner"]
    assert np.array_equal(a["mask"], b["mask"])
    worst = 0.0
    for key in ("Rw", "C", "rms"):
        x, y = np.asarray(a[key], dtype=np.longdouble), np.asarray(b[key], dtype=np.longdouble)
        worst = max(worst, float(np.abs(x - y).max()))
    return worst


def way_difference(names=COMPARED):
    return max(result_difference(case(nm)["res"], case(nm)["res2"]) for nm in names)


def truth_error(name):
    """(|Rw - true Rw| max, |C - true C| max) of a fixture's restated result."""
    c = case(name)
    r = c["res"]
    assert r["status"] == 0
    return (float(np.abs(np.asarray(r["Rw"], dtype=np.float64) - c["Rw"]).max()),
            float(np.abs(np.asarray(r["C"], dtype=np.float64) - c["C"]).max()))


# ---- a tracker's frames restated: check, two-view pose, chain, absolute pose, repair, tracks, landmarks ----------------------------
BROKEN = ("seq5_k", 2, 7)          # pose_ref case, the pair that is given too few matches, how many it keeps (true points)
SLOW = ("slow", 50, 16, 40, 4, 0.0)   # landmarks_ref's slow camera: 16 frames inside one window of L = 16


@functools.lru_cache(maxsize=None)
def broken_sequence():
    """pose_ref's seq5_k with the matches of pair BROKEN[1] cut to the BROKEN[2] lowest true point ids: too few for a fundamental
    matrix (status 1), enough for an absolute pose.  Adds "X0" and "kept" (the point ids)."""
    name, pair, keep = BROKEN
    seq = dict(L._scene(name))
    pairs = [dict(pr) for pr in seq["pairs"]]
    pr = pairs[pair]
    ids_prev = seq["ids"][pair][pr["match"][:, 0].astype(np.int64)]
    sel = ids_prev < keep
    pr["match"], pr["m"], pr["truth"] = pr["match"][sel], pr["m"][sel], pr["truth"][sel]
    seq["pairs"], seq["kept"] = pairs, keep
    return seq


def run_sequence(seq, max_length, point_cap, mode, seed0, min_inliers=16, thresh=THRESH, abs_min_inliers=MIN_INLIERS,
                 landmark_params=(L.MIN_VIEWS, L.MIN_PARALLAX_DEG, L.MAX_REPROJ), frames=None):
    """What a PointTracker(geometric_check="fundamental", intrinsics=one camera, absolute_pose=mode) computes over the frames of
    seq, restated: dict(table [frames, ROW_WORDS], absolute: per frame a ransac dict (or None), landmarks: per frame the kept
    rows, corr: per frame (corr, n, n_valid) or None).  mode: None, "observe" or "repair"."""
    from tests import tracks_ref as T
    frames = len(seq["pts"]) if frames is None else frames
    k = seq["intr"][0]
    tracks = T.Tracks(max_length)
    state = P.new_state()
    table = np.zeros((frames + 1, P.ROW_WORDS))
    prev_pose = prev_match = None
    lms = None
    out = {"absolute": [], "landmarks": [], "corr": [], "pose": []}
    mv, par, rep = landmark_params
    for f in range(frames):
        n_pts = seq["pts"][f].shape[0]
        if f == 0:
            m4, match = np.zeros((0, 4)), np.zeros((0, 3), dtype=np.float32)
        else:
            match = seq["pairs"][f - 1]["match"]
            m4 = np.concatenate([seq["pts"][f - 1][match[:, 0].astype(np.int64)], seq["pts"][f][match[:, 1].astype(np.int64)]], axis=1)
        r = E.ransac(m4, seed0 + f)
        pose = P.two_view_pose(r["F"], r["mask"], r["n_inliers"], r["status"], m4, np.stack([k, k]))
        table[f], state = P.chain_step(prev_pose, pose, prev_match, match, 0 if prev_match is None else prev_match.shape[0],
                                       match.shape[0], state, point_cap, point_cap)
        prev_pose, prev_match = pose, match
        res = cj = None
        if mode is not None and lms is not None:
            padded = np.zeros((point_cap, 3), dtype=np.float32)
            padded[:match.shape[0]] = match
            pts_new = np.zeros((point_cap, 2))
            pts_new[:n_pts] = seq["pts"][f]
            corr, (n, nv) = join(lms, lms.shape[0], padded, match.shape[0], pts_new)
            cj = (corr, n, nv)
            res = ransac(corr, n, k, seed0 + f, thresh, abs_min_inliers)
            if mode == "repair":
                w, table = repair(res, P.state_words(state), table)
                state = {"n_frames": state["n_frames"], "s": w[1], "Rw": w[2:11].reshape(3, 3).copy(), "tw": w[11:14].copy()}
        out["absolute"].append(res)
        out["corr"].append(cj)
        out["pose"].append(pose)
        keep = r["mask"] if (r["status"] == 0 and r["n_inliers"] >= min_inliers) else np.ones(match.shape[0], dtype=bool)
        T.update(tracks, n_pts, match[keep].astype(np.float64).T.reshape(3, -1))
        if f >= 1:
            cams = L.map_window(f + 1, table, seq["intr"][:1], max_length)
            ring, first_slot = L.ring_of(seq, max_length, point_cap, frames=f + 1)
            rows = L.triangulate(tracks.ids, tracks.counts, ring, first_slot, cams, mv, L.cos_of(par), rep)
            lms = L.select(tracks.ids, tracks.tid, tracks.counts, point_cap, rows)
        out["landmarks"].append(lms)
    out["table"] = table[:frames]
    out["tracks"] = tracks
    return out


def scaled_centres(table):
    """The centres of trajectory rows 1.. with the first baseline as the unit."""
    C = np.asarray(table, dtype=np.float64)[1:, 9:12]
    return C / np.linalg.norm(C[0])


def sequence_centre_error(seq, table):
    """The largest difference between the table's centres and the true ones, both scaled to a first baseline of 1."""
    want = seq["centres"][1:table.shape[0]] / np.linalg.norm(seq["centres"][1])
    return float(np.abs(scaled_centres(table) - want).max())


# ---- random samples for the minimal solve ----------------------------------------------------------------------------------------
def random_samples(seed, B):
    """B random cameras (rotations up to 25 degrees about each axis, centres within 1 of the origin), each with 4 random pixels at
    depth 3 to 12: (X: 4 points as lists of 3 arrays [B], px: 4 pixels as lists of 2 arrays, k, Rw [B,9], C [B,3])."""
    rng = np.random.RandomState(seed)
    k = P.intrinsics_of(0, False)
    Rw = np.stack([P._rodrigues(rng.uniform(-25, 25, 3)) for _ in range(B)])
    C = rng.uniform(-1, 1, (B, 3))
    a = np.stack([rng.uniform(8, E.WIDTH - 8, (B, 4)), rng.uniform(8, E.HEIGHT - 8, (B, 4))], axis=2)
    z = rng.uniform(3, 12, (B, 4))
    Y = np.stack([(a[..., 0] - k[2]) / k[0] * z, (a[..., 1] - k[3]) / k[1] * z, z], axis=2)
    X = np.einsum("bji,bkj->bki", Rw, Y) + C[:, None]            # X = Rw^T Y + C
    return ([[X[:, i, c] for c in range(3)] for i in range(4)], [[a[:, i, c] for c in range(2)] for i in range(4)], k,
            Rw.reshape(B, 9), C)


def sample_quartics(X, px, k):
    """(g [5] arrays, roots [4], valid [4]) of the samples' first three rows, as p3p computes them."""
    with np.errstate(all="ignore"):
        f = [bearing(px[i][0], px[i][1], k) for i in range(3)]
        d = lambda i, j: [X[i][c] - X[j][c] for c in range(3)]
        aa, bb, cc = (_dot(v, v) for v in (d(1, 2), d(0, 2), d(0, 1)))
        g, _, _, _ = quartic(aa, bb, cc, _dot(f[1], f[2]), _dot(f[0], f[2]), _dot(f[0], f[1]))
        roots, valid = quartic_roots(g)
    return g, roots, valid


# As way_difference(), max(truth_error(.)) over NOISE_FREE (without "four": no pose under the default min_inliers) and
# sequence_centre_error() of the repaired broken sequence returned them when the fixtures were fixed; tests/test_pnp_cpu.py repeats
# the measurements.  The bounds are 16 times these.
WAY_DIFFERENCE = 1.3265165592548689e-14       # (the six-row fixture), numpy.longdouble (80-bit) as WAY2
TRUTH_ERROR = 2.581268532253489e-15           # (the six-row fixture's centre)
SEQUENCE_CENTRE_ERROR = 3.419486915845482e-14
TOLERANCE = 16.0 * WAY_DIFFERENCE
TRUTH_BOUND = 16.0 * TRUTH_ERROR
SEQUENCE_CENTRE_BOUND = 16.0 * SEQUENCE_CENTRE_ERROR


@functools.lru_cache(maxsize=None)
def slow_problem():
    """The newest frame of landmarks_ref's slow 16-frame scene against the landmarks of the window of its first 15 frames (true
    cameras, L = 16: the camera stays inside one window): dict(landmarks [M, LANDMARK_WORDS], match [cap, 3], n_match, pts_new
    [point_cap, 2], corr, n, n_valid, truth [cap], k, seed, Rw, C (true), res)."""
    seq = L._scene(SLOW)
    frames, Lmax, point_cap = len(seq["pts"]), 16, 48
    t = L.build_tracks(seq, Lmax, frames=frames - 1)
    ring, first_slot = L.ring_of(seq, Lmax, point_cap, frames=frames - 1)
    cams = L.true_cams(seq, Lmax, frames=frames - 1)
    rows = L.triangulate(t.ids, t.counts, ring, first_slot, cams)
    lms = L.select(t.ids, t.tid, t.counts, point_cap, rows)
    pr = seq["pairs"][frames - 2]
    match = np.zeros((point_cap, 3), dtype=np.float32)
    match[:pr["match"].shape[0]] = pr["match"]
    pts_new = np.zeros((point_cap, 2))
    pts_new[:seq["pts"][-1].shape[0]] = seq["pts"][-1]
    corr, (n, nv) = join(lms, lms.shape[0], match, pr["match"].shape[0], pts_new)
    truth = np.zeros(point_cap, dtype=bool)
    truth[:n] = pr["truth"] & (corr[:n, 6] != 0.0)
    Rws, Cs = L.true_poses(seq)
    k = seq["intr"][0]
    out = {"landmarks": lms, "match": match, "n_match": pr["match"].shape[0], "pts_new": pts_new, "corr": corr, "n": n, "n_valid": nv,
           "truth": truth, "k": k, "seed": 310, "Rw": Rws[-1], "C": Cs[-1]}
    out["res"] = ransac(corr, n, k, out["seed"])
    return out
