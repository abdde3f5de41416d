"""numpy restatement of loop closure (csrc/loop_kernels.hip.h): the join of a frame's map matches with the
OLD rows of the world map and the frame's window landmarks (`correspondences`), the loop edge measured from the pose found against
those rows (`edge`), the Sim(3) pose graph over the trajectory rows since the old place was last seen (`pose_graph`, its linear
solve `solve_tridiagonal_low_rank`) and the write-back into the trajectory, the chain state and the map (`apply`).  There is no
reference counterpart, so this file is the specification the kernels are tested against.  Every function takes the number format
`dt` (float64, or numpy.longdouble to measure how far rounding alone moves a result); the sums run in one fixed order, written out."""
import functools

import numpy as np

from tests import pnp_ref as N
from tests import pose_ref as P

MAX_EDGES = 256        # rows of the edge table
EDGE_WORDS = 16        # i, j, R [9], t [3], log sigma, weight
STATE_WORDS = 8        # edges, frame of the last accepted edge, refused, dropped (full), accepted by the last call, its anchor, its inliers,
                       # map rows `apply` left unchanged because the result was not finite
N_EDGES, LAST_FRAME, REFUSED, DROPPED, ACCEPTED, ANCHOR, INLIERS, NONFINITE = range(8)
CAND_WORDS = 16        # frame, anchor, inliers, shared depths, sigma, angle of R_c, |t_c|, accepted, reason, 7 spare
MAX_INNER = 8          # both-ends-free loop edges the solve folds in
INFO_WORDS = 8         # status, cost before, cost after, nodes, edges used, accepted steps, both-ends-free edges left out, lambda
FLAG_LOOP = 32
MIN_SHARED = P.MIN_FRONT
LAMBDA0, LAMBDA_MIN, LAMBDA_MAX = 1e-4, 1e-12, 1e6
REASONS = ("accepted", "no pose", "few inliers", "scale", "anchor", "cooldown", "full")
WIDE = P.WIDE


# ---- the join --------------------------------------------------------------------------------------------------------------------
def correspondences(w, match, n_match, pts_new, count_new, landmarks, n_landmarks, f, min_gap):
    """(corr [cap, CORR_WORDS], xnew [cap, 4], (rows, valid old rows, valid old rows with a landmark)).  A match row is old iff
    last_frame[map row] <= f - min_gap; corr is world_ref.correspondences' row for the old rows and zero elsewhere; xnew = (X of the
    lowest landmark row whose eighth word is the frame point, 1) where that row exists and its X is finite."""
    from tests import world_ref as W
    match, pts_new = np.asarray(match), np.asarray(pts_new, dtype=np.float64)
    landmarks = np.asarray(landmarks, dtype=np.float64).reshape(-1, 8)
    cap, point_cap = match.shape[0], pts_new.shape[0]
    n_rows, count = W.n_rows_of(w), min(max(int(count_new), 0), point_cap)
    n = min(max(int(n_match), 0), cap)
    nl = min(max(int(n_landmarks), 0), landmarks.shape[0])
    owner = {}
    for r in range(nl):
        p = landmarks[r, 7]
        if np.isfinite(p) and 0.0 <= p < point_cap and int(p) not in owner:      # the lowest row wins
            owner[int(p)] = r
    corr, xnew = np.zeros((cap, N.CORR_WORDS)), np.zeros((cap, 4))
    n_valid = n_lm = 0
    for k in range(n):
        fi, fj = float(match[k, 0]), float(match[k, 1])
        if not (0.0 <= fi < n_rows and 0.0 <= fj < count):
            continue
        i, j = int(fi), int(fj)
        if not int(w["last_frame"][i]) <= f - min_gap:
            continue
        row = [w["X"][i, 0], w["X"][i, 1], w["X"][i, 2], pts_new[j, 0], pts_new[j, 1]]
        if not all(np.isfinite(row)):
            continue
        corr[k, :5], corr[k, 5], corr[k, 6] = row, i, 1.0
        n_valid += 1
        r = owner.get(j)
        if r is not None and all(np.isfinite(landmarks[r, 1:4])):
            xnew[k, :3], xnew[k, 3] = landmarks[r, 1:4], 1.0
            n_lm += 1
    return corr, xnew, (n, n_valid, n_lm)


# ---- small fixed-order algebra ---------------------------------------------------------------------------------------------------
def _dot3(p, q):
    return (p[0] * q[0] + p[1] * q[1]) + p[2] * q[2]


def _mm(A, B):
    """A @ B over the last two axes, the inner sum in ascending k: ((a0 b0 + a1 b1) + a2 b2) + ..."""
    acc = A[..., :, 0, None] * B[..., None, 0, :]
    for k in range(1, A.shape[-1]):
        acc = acc + A[..., :, k, None] * B[..., None, k, :]
    return acc


def _t(A):
    return np.swapaxes(A, -1, -2)


def new_state():
    return np.zeros(STATE_WORDS, dtype=np.int32)


def new_edges():
    return np.zeros((MAX_EDGES, EDGE_WORDS))


def relative(Ri, Ci, li, Rj, Cj, dt=np.float64):
    """The relative similarity of node j seen from node i as an edge stores it: R = Rj Ri^T, t = exp(-li) Ri (Cj - Ci)."""
    Ri, Rj = np.asarray(Ri, dtype=dt).reshape(3, 3), np.asarray(Rj, dtype=dt).reshape(3, 3)
    d = np.asarray(Cj, dtype=dt) - np.asarray(Ci, dtype=dt)
    R = np.array([[_dot3(Rj[r], Ri[c]) for c in range(3)] for r in range(3)], dtype=dt)
    e = np.exp(-dt(li))
    t = np.array([e * _dot3(Ri[r], d) for r in range(3)], dtype=dt)
    return R, t


# ---- the loop edge ---------------------------------------------------------------------------------------------------------------
def edge(absolute, corr, xnew, n, last_frame, table, f, min_inliers, cooldown, weight, edges, state, dt=np.float64):
    """One candidate edge from the pose of frame f against the old rows.  absolute: the ransac dict (Rw, C, mask, status); corr, xnew,
    n of `correspondences`; last_frame: the map's column; table [capacity, ROW_WORDS].  Returns (edges, state, cand) as copies."""
    edges, state = np.array(edges, dtype=np.float64), np.array(state, dtype=np.int32)
    table = np.asarray(table).reshape(-1, P.ROW_WORDS)
    capacity, cap = table.shape[0], corr.shape[0]
    rows = min(max(int(n[0]), 0), cap)
    mask = np.asarray(absolute["mask"]).reshape(-1)
    Rl, Cl = np.asarray(absolute["Rw"], dtype=dt).reshape(3, 3), np.asarray(absolute["C"], dtype=dt).reshape(3)
    posed = int(absolute["status"]) == 0 and bool(np.all(np.isfinite(Rl)) and np.all(np.isfinite(Cl))) and 0 <= f < capacity
    inl = [k for k in range(rows) if mask[k] and corr[k, 6] != 0.0]
    a = max([int(last_frame[int(corr[k, 5])]) for k in inl] + [-1])
    Rw = np.asarray(table[f, 0:9] if 0 <= f < capacity else np.eye(3).reshape(9), dtype=dt).reshape(3, 3)
    C = np.asarray(table[f, 9:12] if 0 <= f < capacity else np.zeros(3), dtype=dt)
    sa, sb, shared = dt(0.0), dt(0.0), 0
    for k in inl:
        if xnew[k, 3] == 0.0:
            continue
        dl, dn = np.asarray(corr[k, 0:3], dtype=dt) - Cl, np.asarray(xnew[k, 0:3], dtype=dt) - C
        sa = sa + _dot3(Rl[2], dl)
        sb = sb + _dot3(Rw[2], dn)
        shared += 1
    with np.errstate(all="ignore"):
        sigma = sa / sb if shared > 0 else dt(0.0)
    scale_ok = shared >= MIN_SHARED and bool(np.isfinite(sigma) and sigma > 0.0)
    n_edges = min(max(int(state[N_EDGES]), 0), MAX_EDGES)
    if not posed:
        reason = 1
    elif len(inl) < min_inliers:
        reason = 2
    elif not scale_ok:
        reason = 3
    elif not 0 <= a < f:
        reason = 4
    elif n_edges > 0 and f - int(state[LAST_FRAME]) < cooldown:
        reason = 5
    elif n_edges >= MAX_EDGES:
        reason = 6
    else:
        reason = 0
    cand = np.zeros(CAND_WORDS)
    cand[0:4] = f, a, len(inl), shared
    cand[8] = reason
    state[ACCEPTED], state[ANCHOR], state[INLIERS] = 0, a, len(inl)
    if reason in (1, 2, 3, 4, 5):
        state[REFUSED] += 1
    if reason == 6:
        state[DROPPED] += 1
    if posed and scale_ok:
        Rc = np.array([[_dot3(Rl[:, r], Rw[:, c]) for c in range(3)] for r in range(3)], dtype=dt)
        tc = np.array([Cl[r] - sigma * _dot3(Rc[r], C) for r in range(3)], dtype=dt)
        tr = (Rc[0, 0] + Rc[1, 1]) + Rc[2, 2]
        sk = np.array([Rc[2, 1] - Rc[1, 2], Rc[0, 2] - Rc[2, 0], Rc[1, 0] - Rc[0, 1]], dtype=dt)
        cand[4] = sigma
        cand[5] = np.arctan2(np.sqrt(_dot3(sk, sk)), tr - dt(1.0))
        cand[6] = np.sqrt(_dot3(tc, tc))
    if reason == 0:
        R, t = relative(table[a, 0:9], table[a, 9:12], 0.0, Rl, Cl, dt)
        row = edges[n_edges]
        row[0], row[1], row[2:11], row[11:14], row[14], row[15] = a, f, R.reshape(9), t, np.log(sigma), weight
        state[N_EDGES], state[LAST_FRAME], state[ACCEPTED] = n_edges + 1, f, 1
        cand[7] = 1.0
    return edges, state, cand


# ---- the linear solve: block tridiagonal plus low rank -------------------------------------------------------------------------
def _cholesky(A):
    """Lower factor of [..., n, n] SPD matrices, v = a; v = v - l l for ascending k; a non-positive pivot gives NaN."""
    n = A.shape[-1]
    L = np.zeros_like(A)
    with np.errstate(all="ignore"):
        for c in range(n):
            v = A[..., c, c]
            for k in range(c):
                v = v - L[..., c, k] * L[..., c, k]
            d = np.sqrt(v)
            L[..., c, c] = d
            for r in range(c + 1, n):
                v = A[..., r, c]
                for k in range(c):
                    v = v - L[..., r, k] * L[..., c, k]
                L[..., r, c] = v / d
    return L


def _chol_solve(L, B):
    """A^-1 B for [..., n, n] factors and [..., n, q] right-hand sides: forward then backward, sequential subtraction."""
    n = L.shape[-1]
    Y = np.zeros_like(B)
    with np.errstate(all="ignore"):
        for r in range(n):
            v = B[..., r, :]
            for k in range(r):
                v = v - L[..., r, k, None] * Y[..., k, :]
            Y[..., r, :] = v / L[..., r, r, None]
        X = np.zeros_like(B)
        for r in range(n - 1, -1, -1):
            v = Y[..., r, :]
            for k in range(r + 1, n):
                v = v - L[..., k, r, None] * X[..., k, :]
            X[..., r, :] = v / L[..., r, r, None]
    return X


def cyclic_reduction(D, U, B):
    """x with T x = B for the block tridiagonal SPD T of diagonal blocks D [m, 7, 7], upper blocks U [m, 7, 7] (U[k] couples k and
    k + 1; U[m - 1] is ignored; the lower blocks are their transposes) and B [m, 7, q].  Block cyclic reduction: at stride s the
    nodes j = s - 1 mod 2s are eliminated into their neighbours j - s and j + s; then back substitution from the top."""
    D, B = D.copy(), B.copy()
    m = D.shape[0]
    Up = U.copy()
    Up[m - 1] = 0
    Lo = np.zeros_like(D)
    Lo[1:] = _t(U[:m - 1])
    Lt, Ut, Bt = np.zeros_like(D), np.zeros_like(D), np.zeros_like(B)
    s, strides = 1, []
    while s - 1 < m:
        strides.append(s)
        J = np.arange(s - 1, m, 2 * s)
        F = _cholesky(D[J])
        Lt[J], Ut[J], Bt[J] = _chol_solve(F, Lo[J]), _chol_solve(F, Up[J]), _chol_solve(F, B[J])
        I = np.arange(2 * s - 1, m, 2 * s)
        if len(I):
            le, ri = I - s, I + s
            has = ri < m
            rc = np.where(has, ri, 0)
            hz = has[:, None, None]
            Dn = D[I] - _mm(Lo[I], Ut[le])
            Bn = B[I] - _mm(Lo[I], Bt[le])
            Dn = np.where(hz, Dn - _mm(Up[I], Lt[rc]), Dn)
            Bn = np.where(hz, Bn - _mm(Up[I], Bt[rc]), Bn)
            Ln = -_mm(Lo[I], Lt[le])
            Un = np.where(hz, -_mm(Up[I], Ut[rc]), np.zeros_like(Ln))
            D[I], B[I], Lo[I], Up[I] = Dn, Bn, Ln, Un
        s *= 2
    X = np.zeros_like(B)
    for s in reversed(strides):
        J = np.arange(s - 1, m, 2 * s)
        le, ri = J - s, J + s
        v = Bt[J]
        hl, hr = le >= 0, ri < m
        v = np.where(hl[:, None, None], v - _mm(Lt[J], X[np.where(hl, le, 0)]), v)
        v = np.where(hr[:, None, None], v - _mm(Ut[J], X[np.where(hr, ri, 0)]), v)
        X[J] = v
    return X


def solve_tridiagonal_low_rank(D, U, b, inner):
    """x with (T + sum_e V_e V_e^T) x = b.  T as in `cyclic_reduction`, b [m, 7]; inner: at most MAX_INNER triples (p, q, Vp [7, 7],
    Vq [7, 7]): V_e has the columns Vp[c] at node p and Vq[c] at node q.  Woodbury: T Y = [b, V], S = I + V^T Y_V (Cholesky),
    x = y_0 - Y_V S^-1 V^T y_0."""
    m, q = D.shape[0], 7 * len(inner)
    assert len(inner) <= MAX_INNER
    B = np.zeros((m, 7, 1 + q), dtype=D.dtype)
    B[:, :, 0] = b
    for e, (p, qq, Vp, Vq) in enumerate(inner):
        B[p, :, 1 + 7 * e:8 + 7 * e] += _t(Vp)      # (p != q: one term per entry)
        B[qq, :, 1 + 7 * e:8 + 7 * e] += _t(Vq)
    Y = cyclic_reduction(D, U, B)
    if q == 0:
        return Y[:, :, 0]
    VtY = np.zeros((q, 1 + q), dtype=D.dtype)
    for e, (p, qq, Vp, Vq) in enumerate(inner):
        acc = Vp[:, 0, None] * Y[p, None, 0, :]
        for r in range(1, 7):
            acc = acc + Vp[:, r, None] * Y[p, None, r, :]
        for r in range(7):
            acc = acc + Vq[:, r, None] * Y[qq, None, r, :]
        VtY[7 * e:7 * e + 7] = acc
    S = VtY[:, 1:] + np.eye(q, dtype=D.dtype)
    z = _chol_solve(_cholesky(S), VtY[:, 0:1])[:, 0]
    x = Y[:, :, 0]
    for c in range(q):
        x = x - Y[:, :, 1 + c] * z[c]
    return x


def assemble_dense(D, U, inner):
    """The dense matrix `solve_tridiagonal_low_rank` solves with (tests only)."""
    m = D.shape[0]
    A = np.zeros((7 * m, 7 * m), dtype=D.dtype)
    for k in range(m):
        A[7 * k:7 * k + 7, 7 * k:7 * k + 7] = D[k]
        if k + 1 < m:
            A[7 * k:7 * k + 7, 7 * k + 7:7 * k + 14] = U[k]
            A[7 * k + 7:7 * k + 14, 7 * k:7 * k + 7] = U[k].T
    for p, q, Vp, Vq in inner:
        V = np.zeros((7 * m, 7), dtype=D.dtype)
        V[7 * p:7 * p + 7], V[7 * q:7 * q + 7] = Vp.T, Vq.T
        A += V @ V.T
    return A


# ---- the pose graph --------------------------------------------------------------------------------------------------------------
def _residuals(Ri, Ci, li, Rj, Cj, lj, Rz, tz, lz, bz, want_jacobian=True):
    """Per edge (leading axis): r [n, 7] and the Jacobians Ji, Jj [n, 7, 7] with respect to (w, c, l) of node i and node j."""
    dt = Ri.dtype
    n = Ri.shape[0]
    Rr = _mm(Rj, _t(Ri))
    E = _mm(_t(Rz), Rr)
    half = dt.type(0.5)
    r = np.zeros((n, 7), dtype=dt)
    r[:, 0], r[:, 1], r[:, 2] = half * (E[:, 2, 1] - E[:, 1, 2]), half * (E[:, 0, 2] - E[:, 2, 0]), half * (E[:, 1, 0] - E[:, 0, 1])
    d = Cj - Ci
    ei = np.exp(-li)
    tr = ei[:, None] * _mm(Ri, d[:, :, None])[:, :, 0]
    r[:, 3:6] = (tr - tz) / bz[:, None]
    r[:, 6] = (lj - li) - lz
    if not want_jacobian:
        return r, None, None
    Ji, Jj = np.zeros((n, 7, 7), dtype=dt), np.zeros((n, 7, 7), dtype=dt)
    trace = (E[:, 0, 0] + E[:, 1, 1]) + E[:, 2, 2]
    T = trace[:, None, None] * np.eye(3, dtype=dt)
    Ji[:, 0:3, 0:3] = -half * (T - _t(E))
    Jj[:, 0:3, 0:3] = half * _mm(T - E, _t(Rz))
    ib = dt.type(1.0) / bz
    z = np.zeros(n, dtype=dt)
    cross = np.stack([np.stack([z, -tr[:, 2], tr[:, 1]], 1), np.stack([tr[:, 2], z, -tr[:, 0]], 1),
                      np.stack([-tr[:, 1], tr[:, 0], z], 1)], 1)
    Ji[:, 3:6, 0:3] = -cross * ib[:, None, None]
    Rs = Ri * (ei * ib)[:, None, None]
    Ji[:, 3:6, 3:6] = -Rs
    Jj[:, 3:6, 3:6] = Rs
    Ji[:, 3:6, 6] = -tr * ib[:, None]
    Ji[:, 6, 6], Jj[:, 6, 6] = -1.0, 1.0
    return r, Ji, Jj


def _cayley(R, w):
    """pnp_ref.cayley_update's rotation over a leading axis: the orthonormalised Cay(w) R."""
    dt = R.dtype.type
    a = dt(0.5) * w
    aa = (a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2]
    den, om, two = dt(1.0) + aa, dt(1.0) - aa, dt(2.0)
    Q = np.zeros_like(R)
    Q[:, 0, 0], Q[:, 0, 1], Q[:, 0, 2] = (om + two * (a[:, 0] * a[:, 0])) / den, (two * (a[:, 0] * a[:, 1]) - two * a[:, 2]) / den, \
        (two * (a[:, 0] * a[:, 2]) + two * a[:, 1]) / den
    Q[:, 1, 0], Q[:, 1, 1], Q[:, 1, 2] = (two * (a[:, 0] * a[:, 1]) + two * a[:, 2]) / den, (om + two * (a[:, 1] * a[:, 1])) / den, \
        (two * (a[:, 1] * a[:, 2]) - two * a[:, 0]) / den
    Q[:, 2, 0], Q[:, 2, 1], Q[:, 2, 2] = (two * (a[:, 0] * a[:, 2]) - two * a[:, 1]) / den, (two * (a[:, 1] * a[:, 2]) + two * a[:, 0]) / den, \
        (om + two * (a[:, 2] * a[:, 2])) / den
    M = _mm(Q, R)
    with np.errstate(all="ignore"):
        n0 = np.sqrt((M[:, 0, 0] * M[:, 0, 0] + M[:, 0, 1] * M[:, 0, 1]) + M[:, 0, 2] * M[:, 0, 2])
        r0 = M[:, 0] / n0[:, None]
        pj = (M[:, 1, 0] * r0[:, 0] + M[:, 1, 1] * r0[:, 1]) + M[:, 1, 2] * r0[:, 2]
        v = M[:, 1] - pj[:, None] * r0
        n1 = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
        r1 = v / n1[:, None]
    r2 = np.stack([r0[:, 1] * r1[:, 2] - r0[:, 2] * r1[:, 1], r0[:, 2] * r1[:, 0] - r0[:, 0] * r1[:, 2],
                   r0[:, 0] * r1[:, 1] - r0[:, 1] * r1[:, 0]], 1)
    return np.stack([r0, r1, r2], 1)


def graph_edges(edges, n_edges, a, f):
    """The stored edges the graph of nodes a .. f uses: (fixed-end rows, both-ends-free rows, rows left out), table order."""
    fixed, inner = [], []
    for e in range(min(max(int(n_edges), 0), MAX_EDGES)):
        i, j = int(edges[e, 0]), int(edges[e, 1])
        if not (a < j <= f and 0 <= i < j):
            continue
        (inner if i > a else fixed).append(e)
    left = inner[:max(0, len(inner) - MAX_INNER)]
    return fixed, inner[len(left):], left


def pose_graph(table, edges, state, f, iterations=10, dt=np.float64, trace=None):
    """Levenberg-Marquardt over the rows a + 1 .. f of table [capacity, ROW_WORDS] (a = the anchor the last `edge` call left in
    state, which must have accepted).  Returns (Rw [capacity, 9], C [capacity, 3], sigma [capacity], info [INFO_WORDS]): copies of
    the table's columns (sigma 1) with the free nodes replaced under status 0."""
    table = np.asarray(table).reshape(-1, P.ROW_WORDS)
    capacity = table.shape[0]
    Rw_out, C_out, sig_out = table[:, 0:9].astype(dt), table[:, 9:12].astype(dt), np.ones(capacity, dtype=dt)
    info = np.zeros(INFO_WORDS)
    info[0] = 1.0
    a = int(state[ANCHOR])
    if int(state[ACCEPTED]) == 0 or not (0 <= a < f < capacity):
        return Rw_out, C_out, sig_out, info
    m = f - a
    fixed, inner, left = graph_edges(edges, state[N_EDGES], a, f)
    R = np.asarray(table[a:f + 1, 0:9], dtype=dt).reshape(-1, 3, 3)           # node k + 1 of this array = free node k
    C = np.asarray(table[a:f + 1, 9:12], dtype=dt)
    l = np.zeros(m + 1, dtype=dt)
    one = dt(1.0)
    # measurements: the m chain edges, then the loop edges used
    Rz = np.zeros((m, 3, 3), dtype=dt)
    tz = np.zeros((m, 3), dtype=dt)
    for k in range(m):
        Rz[k], tz[k] = relative(R[k], C[k], 0.0, R[k + 1], C[k + 1], dt)
    loops = fixed + inner
    lo = np.asarray(edges, dtype=dt)[loops].reshape(-1, EDGE_WORDS)
    Rz, tz = np.concatenate([Rz, lo[:, 2:11].reshape(-1, 3, 3)]), np.concatenate([tz, lo[:, 11:14]])
    lz = np.concatenate([np.zeros(m, dtype=dt), lo[:, 14]])
    wt = np.concatenate([np.ones(m, dtype=dt), lo[:, 15]])
    with np.errstate(all="ignore"):
        bz = np.sqrt((tz[:, 0] * tz[:, 0] + tz[:, 1] * tz[:, 1]) + tz[:, 2] * tz[:, 2])
    bz = np.where(np.isfinite(bz) & (bz > 0.0), bz, one)
    ei = np.concatenate([np.arange(m), lo[:, 0].astype(np.int64) - a])       # node indices into R, C, l (0 = the anchor)
    ej = np.concatenate([np.arange(1, m + 1), lo[:, 1].astype(np.int64) - a])
    fix_R = np.asarray(table[:, 0:9], dtype=dt).reshape(-1, 3, 3)
    fix_C = np.asarray(table[:, 9:12], dtype=dt)
    is_fixed = ei <= 0                                                          # an end at or before the anchor: the table's row
    gi = lo[:, 0].astype(np.int64)
    abs_i = np.concatenate([np.arange(a, f), gi])

    def ends(Rn, Cn, ln):
        Ri = np.where(is_fixed[:, None, None], fix_R[abs_i], Rn[np.maximum(ei, 0)])
        Ci = np.where(is_fixed[:, None], fix_C[abs_i], Cn[np.maximum(ei, 0)])
        li = np.where(is_fixed, dt(0.0), ln[np.maximum(ei, 0)])
        return Ri, Ci, li, Rn[ej], Cn[ej], ln[ej]

    def cost_of(r):
        c = dt(0.0)
        for e in range(r.shape[0]):
            q = r[e] * r[e]
            c = c + wt[e] * ((((((q[0] + q[1]) + q[2]) + q[3]) + q[4]) + q[5]) + q[6])
        return c

    r0, _, _ = _residuals(*ends(R, C, l), Rz, tz, lz, bz, want_jacobian=False)
    cur = cost_of(r0)
    info[1], info[2], info[3], info[4], info[6] = cur, cur, m, m + len(loops), len(left)
    if not (cur > 0.0) or not np.isfinite(cur):
        return Rw_out, C_out, sig_out, info
    lam, accepted = dt(LAMBDA0), 0
    n_inner = len(inner)
    for it in range(iterations):
        r, Ji, Jj = _residuals(*ends(R, C, l), Rz, tz, lz, bz)
        D, U, g = np.zeros((m, 7, 7), dtype=dt), np.zeros((m, 7, 7), dtype=dt), np.zeros((m, 7), dtype=dt)
        JiT, JjT = _t(Ji), _t(Jj)
        Hii, Hjj, Hij = _mm(JiT, Ji), _mm(JjT, Jj), _mm(JiT, Jj)
        gi_, gj_ = _mm(JiT, r[:, :, None])[:, :, 0], _mm(JjT, r[:, :, None])[:, :, 0]
        # per node: the chain edge into it, the chain edge out of it, then the fixed-end loop edges in table order
        D += Hjj[:m]
        g += gj_[:m]
        D[:m - 1] += Hii[1:m]
        g[:m - 1] += gi_[1:m]
        U[:m - 1] = Hij[1:m]
        for x in range(len(fixed)):
            e = m + x
            k = ej[e] - 1
            D[k] = D[k] + wt[e] * Hjj[e]
            g[k] = g[k] + wt[e] * gj_[e]
        dfull = np.stack([D[:, c, c] for c in range(7)], 1)
        low = []
        for x in range(n_inner):
            e = m + len(fixed) + x
            p, q = ei[e] - 1, ej[e] - 1
            sw = np.sqrt(wt[e])
            low.append((p, q, sw * Ji[e], sw * Jj[e]))
            g[p] = g[p] + wt[e] * gi_[e]
            g[q] = g[q] + wt[e] * gj_[e]
            dfull[p] = dfull[p] + wt[e] * np.stack([Hii[e, c, c] for c in range(7)])
            dfull[q] = dfull[q] + wt[e] * np.stack([Hjj[e, c, c] for c in range(7)])
        for c in range(7):
            D[:, c, c] = D[:, c, c] + lam * dfull[:, c]
        delta = solve_tridiagonal_low_rank(D, U, -g, low)
        Rn, Cn, ln = R.copy(), C.copy(), l.copy()
        Rn[1:] = _cayley(R[1:], delta[:, 0:3])
        Cn[1:] = C[1:] + delta[:, 3:6]
        ln[1:] = l[1:] + delta[:, 6]
        with np.errstate(all="ignore"):
            rn, _, _ = _residuals(*ends(Rn, Cn, ln), Rz, tz, lz, bz, want_jacobian=False)
            nxt = cost_of(rn)
        fin = bool(np.isfinite(nxt) and np.all(np.isfinite(Rn)) and np.all(np.isfinite(Cn)) and np.all(np.isfinite(ln)))
        accept = fin and nxt < cur
        if trace is not None:
            trace.append((float(cur), float(nxt), float(lam), bool(accept)))
        if accept:
            R, C, l, cur = Rn, Cn, ln, nxt
            accepted += 1
            lam = max(lam / dt(10.0), dt(LAMBDA_MIN))
        else:
            lam = min(lam * dt(10.0), dt(LAMBDA_MAX))
    info[2], info[5], info[7] = cur, accepted, lam
    info[0] = 0.0 if accepted > 0 else 2.0
    if accepted > 0:
        Rw_out[a + 1:f + 1] = R[1:].reshape(-1, 9)
        C_out[a + 1:f + 1] = C[1:]
        sig_out[a + 1:f + 1] = np.exp(l[1:])
    return Rw_out, C_out, sig_out, info


# ---- apply -----------------------------------------------------------------------------------------------------------------------
def apply(info, Rw_new, C_new, sigma, loop_state, f, chain_state, table, w, apply_state=None, dt=np.float64):
    """The corrected nodes written back (under status 0 only): trajectory rows a + 1 .. f, the chain state when f is its newest
    frame and the table is not full, and the map rows last seen in (a, f].  Returns (chain_state, table, X, non-finite map rows
    left unchanged) as copies."""
    from tests import world_ref as W
    chain_state = np.array(chain_state, dtype=dt)
    table = np.array(table, dtype=dt).reshape(-1, P.ROW_WORDS)
    old = table.copy()
    X = np.array(w["X"], dtype=np.float64)
    capacity = table.shape[0]
    a = int(loop_state[ANCHOR])
    if info[0] != 0.0 or not (0 <= a < f < capacity):
        return chain_state, table, X, 0
    Rn, Cn = np.asarray(Rw_new, dtype=dt).reshape(-1, 9), np.asarray(C_new, dtype=dt).reshape(-1, 3)
    for k in range(a + 1, f + 1):
        row = table[k]
        row[0:9], row[9:12] = Rn[k], Cn[k]
        d = Cn[k] - Cn[k - 1]
        with np.errstate(all="ignore"):
            length = np.sqrt(_dot3(d, d))
        if np.isfinite(length) and length > dt(N.SCALE_FRACTION) * dt(row[12]):
            row[12] = length
        row[14] = float(int(row[14]) | FLAG_LOOP)
    nf = chain_state[0]
    count = int(nf) if 0.0 <= nf < 2147483647.0 else 0
    if count == f + 1 and count < capacity:
        R9 = Rn[f]
        chain_state[1], chain_state[2:11] = table[f, 12], R9
        chain_state[11:14] = [-_dot3(R9[3 * i:3 * i + 3], Cn[f]) for i in range(3)]
    bad = 0
    for s in range(W.n_rows_of(w)):
        k = int(w["last_frame"][s])
        if not a < k <= f:
            continue
        Ro, Co = np.asarray(old[k, 0:9], dtype=dt).reshape(3, 3), np.asarray(old[k, 9:12], dtype=dt)
        R1 = Rn[k].reshape(3, 3)
        d = np.asarray(X[s], dtype=dt) - Co
        y = [_dot3(Ro[r], d) for r in range(3)]
        sg = dt(sigma[k])
        xn = [Cn[k][c] + sg * _dot3(R1[:, c], y) for c in range(3)]
        if all(np.isfinite(xn)):
            X[s] = xn
        else:
            bad += 1
    return chain_state, table, X, bad


# ---- fixtures ------------------------------------------------------------------------------------------------------------------
def _rot(deg):
    """pose_ref._rodrigues with the zero vector allowed."""
    deg = np.asarray(deg, dtype=np.float64)
    return P._rodrigues(deg) if np.any(deg != 0.0) else np.eye(3)


def solve_case(m, n_inner, seed):
    """A random SPD block tridiagonal system of m nodes (the normal blocks of m + 1 random 7 x 14 chain Jacobians) with n_inner
    low-rank terms and one right-hand side: (D, U, b, inner)."""
    rng = np.random.RandomState(seed)
    J = rng.randn(m + 1, 14, 14)
    D, U = np.zeros((m, 7, 7)), np.zeros((m, 7, 7))
    for k in range(m + 1):
        H = J[k].T @ J[k]
        if k < m:
            D[k] += H[7:, 7:]
        if k >= 1:
            D[k - 1] += H[:7, :7]
            if k < m:
                U[k - 1] = H[:7, 7:]
    inner = []
    for _ in range(n_inner):
        p = rng.randint(0, m - 1)
        inner.append((p, rng.randint(p + 1, m), rng.randn(7, 7), rng.randn(7, 7)))
    return D, U, rng.randn(m, 7), inner


DRIFT_TWIST, DRIFT_SHIFT, DRIFT_SCALE = (0.05, -0.08, 0.03), (0.002, -0.001, 0.0015), 1.002


def _compose(A, B):
    return (A[0] * B[0], A[1] @ B[1], A[0] * (A[1] @ B[2]) + A[2])


def _inverse(A):
    return (1.0 / A[0], A[1].T, -(A[1].T @ A[2]) / A[0])


def drift_share(frames):
    return min(1.0, 64.0 / frames)


def circuit(frames, a, capacity=None, radius=3.0):
    """(truth, drifted): trajectory tables [capacity, ROW_WORDS] of a camera on a closed circuit of `frames` frames.  In `drifted`
    every edge after row a carries one more constant small similarity (DRIFT_*: a twist in degrees, a shift and a scale factor, in
    the camera's frame; past 64 frames all three shrink by 64 / frames, `drift_share`, so that a long circuit drifts as far as a
    short one), so rows a + 1 .. drift in all seven degrees of freedom."""
    capacity = frames if capacity is None else capacity
    truth = np.zeros((capacity, P.ROW_WORDS))
    for k in range(frames):
        th = 2.0 * np.pi * k / frames
        truth[k, 0:9] = _rot([0.0, np.degrees(th), 0.0]).reshape(9)
        truth[k, 9:12] = radius * np.cos(th), 0.1 * radius * np.sin(2.0 * th), radius * np.sin(th)
        truth[k, 12] = 1.0 if k == 0 else np.linalg.norm(truth[k, 9:12] - truth[k - 1, 9:12])
    drift = truth.copy()
    node = lambda row: (1.0, row[0:9].reshape(3, 3).T, row[9:12])
    share = drift_share(frames)
    step = (DRIFT_SCALE ** share, _rot(np.array(DRIFT_TWIST) * share), np.array(DRIFT_SHIFT) * (radius / 3.0 * share))
    T = node(truth[a])
    for k in range(a + 1, frames):
        T = _compose(_compose(T, _compose(_inverse(node(truth[k - 1])), node(truth[k]))), step)
        drift[k, 0:9], drift[k, 9:12] = T[1].T.reshape(9), T[2]
        drift[k, 12] = np.linalg.norm(drift[k, 9:12] - drift[k - 1, 9:12])
    return truth, drift


def true_edge(truth, a, i, j, weight=1.0, share=1.0):
    """The edge row (i, j) the true cameras give: node k's true correction scale is DRIFT_SCALE^-(share (k - a)) past the anchor."""
    li = -max(i - a, 0) * share * np.log(DRIFT_SCALE)
    lj = -max(j - a, 0) * share * np.log(DRIFT_SCALE)
    R, t = relative(truth[i, 0:9], truth[i, 9:12], li, truth[j, 0:9], truth[j, 9:12])
    row = np.zeros(EDGE_WORDS)
    row[0], row[1], row[2:11], row[11:14], row[14], row[15] = i, j, R.reshape(9), t, lj - li, weight
    return row


def graph_case(m, n_inner, seed=0, capacity=None, a=2):
    """A planted drift over m free nodes: (truth, table, edges, state, f).  The newest edge (a, f) is the truth; n_inner more true
    edges have both ends free."""
    f = a + m
    truth, drift = circuit(f + 1, a, capacity)
    rng = np.random.RandomState(seed)
    edges, state = new_edges(), new_state()
    n = 0
    for _ in range(n_inner):
        i = int(rng.randint(a + 1, f))
        edges[n] = true_edge(truth, a, i, int(rng.randint(i + 1, f + 1)), share=drift_share(f + 1))
        n += 1
    edges[n] = true_edge(truth, a, a, f, share=drift_share(f + 1))
    state[N_EDGES], state[LAST_FRAME], state[ACCEPTED], state[ANCHOR] = n + 1, f, 1, a
    return truth, drift, edges, state, f


def consistent_case(m=40, a=3):
    """graph_case whose only edge agrees with the drifted chain: the cost before is exactly 0."""
    truth, drift, edges, state, f = graph_case(m, 0, a=a)
    R, t = relative(drift[a, 0:9], drift[a, 9:12], 0.0, drift[f, 0:9], drift[f, 9:12])
    edges[0, 2:11], edges[0, 11:14], edges[0, 14] = R.reshape(9), t, 0.0
    return drift, edges, state, f


def transform_case(table, edges, sim):
    """The table and the edges under one similarity X -> s Q X + t of the world: Rw -> Rw Q^T, C -> s Q C + t, s -> s s, edge
    translations -> s t."""
    s, Q, t = sim
    out, ed = table.copy(), edges.copy()
    for k in range(table.shape[0]):
        out[k, 0:9] = (table[k, 0:9].reshape(3, 3) @ Q.T).reshape(9)
        out[k, 9:12] = s * (Q @ table[k, 9:12]) + t
        out[k, 12] = s * table[k, 12]
    ed[:, 11:14] = s * edges[:, 11:14]
    return out, ed


GRAPH_SIZES = ((1, 0), (2, 0), (2, 1), (3, 1), (63, 1), (64, 8), (65, 9), (1023, 0), (1025, 8))      # (free nodes, both-ends-free edges)
GRAPH_LARGE = (4095, 8)


def graph_difference(a, b):
    """The largest difference of two pose_graph results: (Rw, C, sigma)."""
    return tuple(float(np.abs(np.asarray(x, dtype=np.float64) - np.asarray(y, dtype=np.float64)).max()) for x, y in zip(a[:3], b[:3]))


def graph_way_difference(sizes=GRAPH_SIZES):
    """graph_difference between float64 and numpy.longdouble over the planted graphs of `sizes`, the largest per output."""
    worst = [0.0, 0.0, 0.0]
    for m, ni in sizes:
        _, table, edges, state, f = graph_case(m, ni)
        d = graph_difference(pose_graph(table, edges, state, f), pose_graph(table, edges, state, f, dt=np.longdouble))
        worst = [max(x, y) for x, y in zip(worst, d)]
    return tuple(worst)


def edge_case(name, seed=5):
    """Hand-made inputs of `edge`: dict(absolute, corr, xnew, n, last_frame, table, f, min_inliers, cooldown, weight, edges, state)."""
    rng = np.random.RandomState(seed)
    f, cap, n_rows = 40, 48, 64
    _, table = circuit(48, 3, 64)
    Rw, C = table[f, 0:9].reshape(3, 3), table[f, 9:12]
    sigma, Rc, tc = 0.93, _rot([1.0, -2.0, 0.5]), np.array([0.05, -0.02, 0.03])
    Rl, Cl = Rw @ Rc.T, sigma * (Rc @ C) + tc
    n = 30
    x = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1, 1, n), rng.uniform(3, 9, n)], 1)
    Xn = C + x @ Rw
    Xo = sigma * (Xn @ Rc.T) + tc
    corr, xnew = np.zeros((cap, N.CORR_WORDS)), np.zeros((cap, 4))
    corr[:n, 0:3], corr[:n, 3:5], corr[:n, 5], corr[:n, 6] = Xo, rng.uniform(0, 300, (n, 2)), rng.permutation(n_rows)[:n], 1.0
    xnew[:n, 0:3], xnew[:n, 3] = Xn, 1.0
    corr[4], xnew[4] = 0.0, 0.0                                   # a row the join refused
    xnew[7], xnew[9] = 0.0, 0.0                                   # inliers without a landmark
    mask = np.zeros(cap, dtype=np.uint8)
    mask[:n] = 1
    mask[[2, 11, 12]] = 0
    mask[n + 3] = 1                                               # past the rows: never read
    last = rng.randint(0, 6, n_rows).astype(np.int32)
    d = dict(absolute={"Rw": Rl, "C": Cl, "mask": mask, "status": 0}, corr=corr, xnew=xnew, n=(n, n - 1, n - 3), last_frame=last,
             table=table, f=f, min_inliers=12, cooldown=32, weight=1.0, edges=new_edges(), state=new_state())
    d["state"][REFUSED], d["state"][DROPPED] = 3, 1
    if name == "few_shared":
        keep = [k for k in range(n) if mask[k] and corr[k, 6] != 0.0 and xnew[k, 3] != 0.0][:7]
        for k in range(n):
            if k not in keep:
                xnew[k] = 0.0
    elif name == "negative_ratio":
        xnew[:n, 0:3] = C - x @ Rw
        xnew[[4, 7, 9]] = 0.0
    elif name == "nonfinite_ratio":
        xnew[:n, 0:3] = C
        xnew[[4, 7, 9]] = 0.0
    elif name == "status1":
        d["absolute"]["status"] = 1
    elif name == "nonfinite_pose":
        d["absolute"]["C"] = np.array([0.0, np.nan, 0.0])
    elif name == "few_inliers":
        mask[12:] = 0
    elif name == "anchor":
        last[int(corr[5, 5])] = f
    elif name == "cooldown":
        d["edges"][0] = true_edge(table, 3, 2, f - 3)
        d["state"][N_EDGES], d["state"][LAST_FRAME] = 1, f - 3
    elif name == "after_cooldown":
        d["edges"][0] = true_edge(table, 3, 2, f - 32)
        d["state"][N_EDGES], d["state"][LAST_FRAME] = 1, f - 32
    elif name == "full":
        d["edges"][:] = true_edge(table, 3, 1, 4)
        d["state"][N_EDGES], d["state"][LAST_FRAME] = MAX_EDGES, 4
    else:
        assert name == "accept", name
    return d


EDGE_CASES = {"accept": 0, "after_cooldown": 0, "status1": 1, "nonfinite_pose": 1, "few_inliers": 2, "few_shared": 3,
              "negative_ratio": 3, "nonfinite_ratio": 3, "anchor": 4, "cooldown": 5, "full": 6}       # name -> reason


def run_edge(d, dt=np.float64):
    return edge(d["absolute"], d["corr"], d["xnew"], d["n"], d["last_frame"], d["table"], d["f"], d["min_inliers"], d["cooldown"],
                d["weight"], d["edges"], d["state"], dt=dt)


def join_case(n_match, n_rows, seed, hand=False):
    """Inputs of `correspondences`: a map of n_rows rows (some with a non-finite X), n_match matches in ascending map row inside a
    table of more rows (the rest is garbage that must not be read as matches), frame points, and landmark rows of which some name no
    point, some name one point twice and some have a non-finite X.  hand: the first rows are the issue's hand-made cases."""
    from tests import world_ref as W
    rng = np.random.RandomState(seed)
    f, min_gap = 200, 32
    cap = n_match + 5
    n_pts = max(n_match, 4) + 3
    point_cap = n_pts + 2
    w = W.new_map(max(n_rows, 1) + 4, 16)
    w["state"][W.N_ROWS] = n_rows
    w["X"][:] = rng.randn(w["map_cap"], 3)
    w["last_frame"][:] = rng.randint(f - min_gap - 3, f - min_gap + 3, w["map_cap"])
    w["X"][rng.permutation(n_rows)[:max(1, n_rows // 50)], rng.randint(0, 3)] = np.inf
    match = np.zeros((cap, 3), dtype=np.float32)
    rows = np.sort(rng.permutation(n_rows)[:n_match])
    match[:n_match, 0], match[:n_match, 1], match[:n_match, 2] = rows, rng.permutation(n_pts)[:n_match], rng.uniform(0, 0.7, n_match)
    match[n_match:] = (0.0, 1.0, 0.1)                             # past n_match
    pts = rng.uniform(0, 300, (point_cap, 2))
    n_lm = n_pts + 6
    lms = np.zeros((n_lm + 2, 8))
    lms[:, 0], lms[:, 1:4], lms[:, 4] = np.arange(n_lm + 2), rng.randn(n_lm + 2, 3), 3
    lms[:, 7] = rng.randint(-1, n_pts, n_lm + 2)                  # -1: not in the newest frame; repeats: the lowest row wins
    lms[rng.permutation(n_lm)[:max(1, n_lm // 20)], 2] = np.nan
    if hand:
        assert n_match >= 6 and n_rows >= 6
        r = match[:6, 0].astype(np.int64)
        j = match[:6, 1].astype(np.int64)
        w["X"][r] = rng.randn(6, 3)
        w["last_frame"][r] = f - min_gap - 1
        w["last_frame"][r[0]] = f - min_gap                       # exactly at the gap: old
        w["last_frame"][r[1]] = f - min_gap + 1                   # one above: not old
        lms[:, 7][np.isin(lms[:, 7], j)] = -1
        lms[0, 7], lms[0, 1:4] = j[0], (1.0, 2.0, 3.0)
        lms[1, 7], lms[1, 1:4] = j[1], (1.5, 2.5, 3.5)
        # j[2]: a frame point without a landmark
        lms[2, 7], lms[2, 1:4] = j[3], (4.0, 5.0, 6.0)            # two rows name one point: the lowest wins
        lms[3, 7], lms[3, 1:4] = j[3], (7.0, 8.0, 9.0)
        lms[4, 7], lms[4, 1:4] = j[4], (1.0, np.inf, 0.0)         # a landmark with a non-finite X
        lms[5, 7], lms[5, 1:4] = j[5], (2.0, 2.0, 2.0)
        w["X"][r[5], 1] = np.nan                                   # a map row with a non-finite X
    return dict(w=w, match=match, n_match=n_match, pts_new=pts, count_new=n_pts, landmarks=lms, n_landmarks=n_lm, f=f, min_gap=min_gap)


def run_join(d):
    return correspondences(d["w"], d["match"], d["n_match"], d["pts_new"], d["count_new"], d["landmarks"], d["n_landmarks"], d["f"],
                           d["min_gap"])


def apply_case(name, seed=3):
    """Inputs of `apply`: dict(info, Rw, C, sigma, loop_state, f, chain_state, table, w)."""
    from tests import world_ref as W
    rng = np.random.RandomState(seed)
    a, f, capacity = 5, 20, 24
    truth, table = circuit(22, a, capacity)
    table[:, 14] = rng.randint(0, 32, capacity)                   # every combination of bits 0 to 4
    table[a + 1, 14], table[f, 14] = 31, 0
    Rw, C, sigma = truth[:, 0:9].copy(), truth[:, 9:12].copy(), np.ones(capacity)
    sigma[a + 1:f + 1] = DRIFT_SCALE ** -np.arange(1, f - a + 1)
    C[9] = C[8] + 1e-6                                            # a step below 1/64 of the row's s: s is kept
    C[11, 1] = np.inf                                             # not finite: s is kept, and its map rows are left alone
    st = np.zeros(P.STATE_WORDS)
    st[0], st[1], st[2:11], st[11:14] = f + 1, table[f, 12], table[f, 0:9], -(table[f, 0:9].reshape(3, 3) @ table[f, 9:12])
    w = W.new_map(40, 16)
    w["state"][W.N_ROWS] = 36
    w["X"][:] = rng.randn(40, 3) * 4
    w["last_frame"][:] = rng.randint(0, f + 1, 40)
    w["last_frame"][:8] = a, a + 1, f, f + 3, capacity + 5, 11, 9, a - 1      # at a, a + 1, f, past f, without a table row, non-finite
    w["last_frame"][36:] = f                                       # past n_rows
    loop_state = new_state()
    loop_state[ANCHOR], loop_state[ACCEPTED], loop_state[NONFINITE] = a, 1, 2
    info = np.zeros(INFO_WORDS)
    if name == "older_state":
        st[0] = f + 2                                             # the chain has moved on: the state is not touched
    elif name == "full_table":
        capacity = f + 1
        table, Rw, C, sigma = table[:capacity].copy(), Rw[:capacity].copy(), C[:capacity].copy(), sigma[:capacity].copy()
    elif name == "no_step":
        info[0] = 2.0
    else:
        assert name == "plain", name
    return dict(info=info, Rw=Rw, C=C, sigma=sigma, loop_state=loop_state, f=f, chain_state=st, table=table, w=w)


APPLY_CASES = ("plain", "older_state", "full_table", "no_step")


def run_apply(d):
    return apply(d["info"], d["Rw"], d["C"], d["sigma"], d["loop_state"], d["f"], d["chain_state"], d["table"], d["w"])


# As graph_way_difference() and the edge cases returned them when the fixtures were fixed (numpy.longdouble, 80-bit);
# tests/test_loop_cpu.py repeats the measurements.  The bounds are 16 times these.
GRAPH_WAY_DIFFERENCE = (6.1885405654160675e-12, 1.373559599393559e-11, 1.1585177261963508e-12)     # Rw, C, sigma over GRAPH_SIZES
EDGE_WAY_DIFFERENCE = 3.3306690738754696e-16                # the edge rows and candidate records of EDGE_CASES
GRAPH_BOUND = tuple(16.0 * x for x in GRAPH_WAY_DIFFERENCE)
EDGE_BOUND = 16.0 * EDGE_WAY_DIFFERENCE


# ---- a restated tracker with loop closure, and its closed circuit ---------------------------------------------------------------
CIRCUIT_FRAMES, CIRCUIT_LAP, CIRCUIT_RADIUS, CIRCUIT_CANDIDATES, CIRCUIT_NOISE = 26, 20, 2.0, 1470, 0.3
CIRCUIT_L, CIRCUIT_CAP, CIRCUIT_SEED0, CIRCUIT_GAP, CIRCUIT_MIN_INLIERS = 4, 256, 300, 12, 40
CIRCUIT_SEEDS = (1, 2, 3, 4)


def circuit_sequence(seed, noise=CIRCUIT_NOISE):
    """A camera that drives a closed circuit (a circle of CIRCUIT_LAP frames in the image plane's directions, looking ahead with a
    small wobble) and re-enters its first stretch for CIRCUIT_FRAMES - CIRCUIT_LAP more frames, on a slightly different path; about
    110 points per frame with `noise` pixels of error; points leave the image and return under new track ids.  world_ref's
    sequence layout (its `_finish` gives the sign descriptors and the matches)."""
    from tests import world_ref as W
    rng = np.random.RandomState(seed)
    k = P.intrinsics_of(0, False)
    Rf, tf, C = [], [], []
    for f in range(CIRCUIT_FRAMES):
        th = 2.0 * np.pi * f / CIRCUIT_LAP
        off = 0.0 if f < CIRCUIT_LAP else 0.08
        c = np.array([CIRCUIT_RADIUS * (1.0 - np.cos(th)) + off, CIRCUIT_RADIUS * np.sin(th) + 0.5 * off, 0.03 * (f % 3)])
        R = _rot(np.array([0.3, 1.5, -0.2]) * (c[0] / 2.7) + np.array([0.8, 0.0, 0.1]) * (c[1] / 2.7))      # the world is camera 0
        Rf.append(R), C.append(c), tf.append(-(R @ c))
    n_cand = CIRCUIT_CANDIDATES
    a = np.stack([rng.uniform(-300, 1000, n_cand), rng.uniform(-250, 490, n_cand)], axis=1)
    z = rng.uniform(3.0, 12.0, n_cand)
    X0 = np.stack([(a[:, 0] - k[2]) * z / k[0], (a[:, 1] - k[3]) * z / k[1], z], axis=1)
    pts, ids = [], []
    for f in range(CIRCUIT_FRAMES):
        Y = X0 @ Rf[f].T + tf[f]
        b = P._project(Y, k)
        seen = np.nonzero((Y[:, 2] > 1.0) & (b[:, 0] > 4) & (b[:, 0] < 316) & (b[:, 1] > 4) & (b[:, 1] < 236))[0]
        order = seen[rng.permutation(len(seen))]
        pts.append(np.ascontiguousarray(b[order] + noise * rng.randn(len(order), 2))), ids.append(order.astype(np.int64))
    pairs = []
    for f in range(1, CIRCUIT_FRAMES):
        Rs = Rf[f] @ Rf[f - 1].T
        ts = tf[f] - Rs @ tf[f - 1]
        pairs.append({"R": Rs, "t": ts / np.linalg.norm(ts), "length": float(np.linalg.norm(ts)), "intr": np.stack([k, k])})
    seq = {"pts": pts, "ids": ids, "intr": np.stack([k] * CIRCUIT_FRAMES), "pairs": pairs, "n_in": n_cand, "X0": X0,
           "centres": np.stack(C), "Rw": np.stack(Rf)}
    return W._finish(seq, 93 + seed)


def run_sequence(seq, max_length, point_cap, loop_mode, seed0, min_gap=32, loop_min_inliers=12, cooldown=32, iterations=10,
                 weight=1.0, world_cap=4096, tid_cap=1 << 16, min_inliers=16, thresh=N.THRESH, world_min_inliers=N.MIN_INLIERS,
                 way=P.WAY1):
    """world_ref.run_sequence(world_mode="observe") with loop closure: what a PointTracker(geometric_check="fundamental", intrinsics,
    world_map="observe", loop_closure=loop_mode) computes over the frames of seq.  dict(table, world (per frame the pose against the
    map), states (the map's), map, tracks, loop: per frame dict(n, pose, cand, state, info), edges, loop_state, landmarks: per
    frame the rows given to the insert)."""
    from tests import epipolar_ref as E
    from tests import landmarks_ref as LR
    from tests import tracks_ref as T
    from tests import world_ref as W
    dt = way[0]
    frames = len(seq["pts"])
    k = seq["intr"][0]
    tracks = T.Tracks(max_length)
    state = P.new_state(way)
    table = np.zeros((frames + 1, P.ROW_WORDS), dtype=dt)
    prev_pose = prev_match = None
    world = W.new_map(world_cap, tid_cap)
    edges, lstate = new_edges(), new_state()
    out = {"world": [], "states": [], "loop": [], "landmarks": []}
    mv, par, rep = LR.MIN_VIEWS, LR.MIN_PARALLAX_DEG, LR.MAX_REPROJ

    def words():
        w = np.zeros(P.STATE_WORDS, dtype=dt)
        w[0], w[1], w[2:11], w[11:14] = state["n_frames"], state["s"], np.asarray(state["Rw"], dtype=dt).reshape(9), state["tw"]
        return w

    def window_landmarks(f):
        cams = LR.map_window(f + 1, table, seq["intr"][:1], max_length, way=way)
        ring, first_slot = LR.ring_of(seq, max_length, point_cap, frames=f + 1)
        rows = LR.triangulate(tracks.ids, tracks.counts, ring, first_slot, cams, mv, LR.cos_of(par), rep, way=way)
        return LR.select(tracks.ids, tracks.tid, tracks.counts, point_cap, rows)
    for f in range(frames):
        n_pts = seq["pts"][f].shape[0]
        if f == 0:
            m4, match = np.zeros((0, 4)), np.zeros((0, 3), dtype=np.float32)
        else:
            match = seq["pairs"][f - 1]["match"]
            m4 = np.concatenate([seq["pts"][f - 1][match[:, 0].astype(np.int64)], seq["pts"][f][match[:, 1].astype(np.int64)]], axis=1)
        r = E.ransac(m4, seed0 + f)
        pose = P.two_view_pose(r["F"], r["mask"], r["n_inliers"], r["status"], m4, np.stack([k, k]), way=way)
        table[f], state = P.chain_step(prev_pose, pose, prev_match, match, 0 if prev_match is None else prev_match.shape[0],
                                       match.shape[0], state, point_cap, point_cap, way=way)
        prev_pose, prev_match = pose, match
        pts_new = np.zeros((point_cap, 2))
        pts_new[:n_pts] = seq["pts"][f]
        desc_new = np.zeros((point_cap, 256), dtype=np.float32)
        desc_new[:n_pts] = seq["desc"][f]
        mw = W.match_world(world["desc"], W.n_rows_of(world), desc_new, n_pts, W.NN_THRESH)
        corr, (n, nv) = W.correspondences(world, mw["match"], mw["n_match"], pts_new, n_pts)
        out["world"].append(N.ransac(corr, n, k, seed0 + f, thresh, world_min_inliers, way=way))
        keep = r["mask"] if (r["status"] == 0 and r["n_inliers"] >= min_inliers) else np.ones(match.shape[0], dtype=bool)
        T.update(tracks, n_pts, match[keep].astype(np.float64).T.reshape(3, -1))
        if f >= 1:
            lms = window_landmarks(f)
            if loop_mode is not None:
                lcorr, xnew, ln = correspondences(world, mw["match"], mw["n_match"], pts_new, n_pts, lms, lms.shape[0], f, min_gap)
                lres = N.ransac(lcorr, ln[0], k, seed0 + f, thresh, loop_min_inliers, way=way)
                edges, lstate, cand = edge(lres, lcorr, xnew, ln, world["last_frame"], table, f, loop_min_inliers, cooldown, weight,
                                           edges, lstate, dt=dt)
                Rw_o, C_o, sig, info = pose_graph(table, edges, lstate, f, iterations, dt=dt)
                if loop_mode == "apply":
                    w, table, X, bad = apply(info, Rw_o, C_o, sig, lstate, f, words(), table, world, dt=dt)
                    state = {"n_frames": state["n_frames"], "s": w[1], "Rw": w[2:11].reshape(3, 3).copy(), "tw": w[11:14].copy()}
                    world["X"][:] = X
                    lstate[NONFINITE] += bad
                    lms = window_landmarks(f)
                out["loop"].append({"n": ln, "pose": lres, "cand": cand, "state": lstate.copy(), "info": info})
            out["landmarks"].append(lms)
            W.insert(world, lms, lms.shape[0], desc_new, n_pts, np.asarray(table, dtype=np.float64), f + 1, W.PATIENCE)
        out["states"].append(world["state"].copy())
    out["table"], out["tracks"], out["map"] = np.asarray(table[:frames], dtype=np.float64), tracks, world
    out["edges"], out["loop_state"] = edges, lstate
    return out


def closures(run):
    """(frame, anchor, inliers) of the accepted edges of a run."""
    return [(int(x["cand"][0]), int(x["cand"][1]), int(x["cand"][2])) for x in run["loop"] if x["cand"][7] != 0.0]


@functools.lru_cache(maxsize=None)
def circuit_runs(seed):
    """(seq, {"observe", "apply"}): the restated tracker on the circuit of one seed, computed once, read-only."""
    seq = circuit_sequence(seed)
    run = lambda mode, **kw: run_sequence(seq, CIRCUIT_L, CIRCUIT_CAP, mode, CIRCUIT_SEED0, min_gap=CIRCUIT_GAP,
                                          loop_min_inliers=CIRCUIT_MIN_INLIERS, **kw)
    return seq, {"observe": run("observe"), "apply": run("apply")}


# The largest difference of the trajectory's centres between float64 and numpy.longdouble (80-bit) over the circuit of
# CIRCUIT_DEVICE_SEED under "apply", as measured when the sequence was fixed; tests/test_loop_cpu.py repeats the measurement.
CIRCUIT_DEVICE_SEED = 3
CIRCUIT_WAY_DIFFERENCE = 3.5894620609155936e-10
CIRCUIT_BOUND = 16.0 * CIRCUIT_WAY_DIFFERENCE
