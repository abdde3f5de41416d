"""numpy restatement of the windowed bundle adjustment (csrc/ba_kernels.hip.h): Levenberg-Marquardt over the
cameras of the retained frames of the newest consistent window (landmarks_ref.map_window) and the accepted rows of the N-view
triangulation (landmarks_ref.triangulate), by the Schur complement on the cameras, and the rule that writes the result back into
the trajectory (`apply`).  There is no reference counterpart, so this file is the specification the kernels are tested against.
Everything is fp64 in the parenthesisation written here, vectorised over the rows (the loops over the views and the pairs of
views are the kernel's); every function also runs in pose_ref.WAY2 (numpy.longdouble where that is wider than float64), which is
how the tolerance of the continuous outputs is measured (`way_difference`).  Sums over the rows run in the device's order:
block_sum's (csrc/geom_blocks.hip.h) inside a tile of 256 rows (`tile_sum`), the tiles ascending.  Also the fixtures: landmarks_ref's tables under
perturbed true cameras, two of its window scenarios, six noisy chains of pnp_ref.run_sequence."""
import functools
import math

import numpy as np

from tests import landmarks_ref as L
from tests import pnp_ref as PN
from tests import pose_ref as P

WAY1, WAY2 = P.WAY1, P.WAY2
CAM_WORDS = L.CAM_WORDS
INFO_WORDS = 8           # status, cost before, cost after, n_obs, rows used, accepted steps, refused V solves, final lambda
ADJUSTED, NOTHING, NO_STEP = 0, 1, 2
FLAG_ADJUSTED = 8
TILE = 256
LAMBDA0, LAMBDA_MIN, LAMBDA_MAX = 1e-4, 1e-12, 1e6
DONE_RELATIVE = 1e-10    # done: cur - new <= DONE_RELATIVE * cur ...
DONE_RESIDUAL = 1e-9     # ... or new <= 2 * n_obs * DONE_RESIDUAL ** 2
ITERATIONS = 10
MAX_ITERATIONS = 16


def _dot(p, q, rev=False):
    return P._dot(p, q, rev)


# ---- sums in the device's order ------------------------------------------------------------------------------------------------
def tile_sum(vals):
    """Sum over axis 0 (the rows; a row that takes no part holds zeros): per tile of 256 rows the xor butterfly inside each wave
    of 64 and the four wave partials in wave order (block_sum), then the tiles in ascending order."""
    vals = np.asarray(vals)
    n = vals.shape[0]
    tiles = max(1, -(-n // TILE))
    pad = np.zeros((tiles * TILE,) + vals.shape[1:], dtype=vals.dtype)
    pad[:n] = vals
    v = pad.reshape((tiles, TILE // 64, 64) + vals.shape[1:])
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, :, lanes ^ o]
    red = v[:, :, 0]
    acc = np.zeros(vals.shape[1:], dtype=vals.dtype)
    for t in range(tiles):
        s = red[t, 0]
        for w in range(1, TILE // 64):
            s = s + red[t, w]
        acc = acc + s
    return acc


# ---- the observations ----------------------------------------------------------------------------------------------------------
def observations(ids, counts, pts, first_slot, cams, status):
    """(used: L bool arrays [n_rows], pix: L arrays [n_rows, 2]) by section 26's id, count and clamp rules; rows whose status is
    not 0 have no observation."""
    ids = np.asarray(ids, dtype=np.int64)
    n_rows, Lw = ids.shape
    point_cap = pts.shape[1]
    counts = [min(max(int(v), 0), point_cap) for v in counts]
    first = [sum(counts[:c]) for c in range(Lw)]
    live = np.asarray(status) == 0
    used, pix = [], []
    for c in range(Lw):
        p = ids[:, c] - first[c]
        u = live & (ids[:, c] >= 0) & (cams[c, 16] != 0.0) & (p >= 0) & (p < counts[c])
        used.append(u)
        pix.append(pts[(first_slot + c) % Lw][np.where(u, p, 0)])
    return used, pix


def view(cam, X, px, rev=False):
    """One view of the points X (three arrays over the rows): dict(y2, r0, r1, p0 [3], p1 [3], j0 [6], j1 [6])."""
    q = (X[0] - cam[9], X[1] - cam[10], X[2] - cam[11])
    y0, y1, y2 = _dot(cam[0:3], q, rev), _dot(cam[3:6], q, rev), _dot(cam[6:9], q, rev)
    un, vn = y0 / y2, y1 / y2
    fa, fb = cam[12] / y2, cam[13] / y2
    r0, r1 = (cam[12] * un + cam[14]) - px[:, 0], (cam[13] * vn + cam[15]) - px[:, 1]
    p0 = [fa * (cam[k] - un * cam[6 + k]) for k in range(3)]
    p1 = [fb * (cam[3 + k] - vn * cam[6 + k]) for k in range(3)]
    j0 = [fa * (0.0 - un * y1), fa * (y2 + un * y0), fa * (0.0 - y1), 0.0 - p0[0], 0.0 - p0[1], 0.0 - p0[2]]
    j1 = [fb * ((0.0 - y2) - vn * y1), fb * (vn * y0), fb * y0, 0.0 - p1[0], 0.0 - p1[1], 0.0 - p1[2]]
    return {"y2": y2, "r0": r0, "r1": r1, "p0": p0, "p1": p1, "j0": j0, "j1": j1}


def cost_of(cams, X, used, pix, rev=False):
    """(cost: the sum of the squared residuals, per-row sums, per-row observation counts, front: every used y2 finite and > 0)."""
    dt = X[0].dtype
    ss = np.zeros(X[0].shape[0], dtype=dt)
    nv = np.zeros(X[0].shape[0], dtype=np.int64)
    front = True
    for c in range(len(used)):
        v = view(cams[c], X, pix[c], rev)
        ss = np.where(used[c], ss + (v["r0"] * v["r0"] + v["r1"] * v["r1"]), ss)
        nv += used[c]
        front = front and bool(np.all(~used[c] | (np.isfinite(v["y2"]) & (v["y2"] > 0.0))))
    return tile_sum(ss), ss, nv, front


# ---- the point blocks ----------------------------------------------------------------------------------------------------------
def point_blocks(views, used, lam, dt, rev):
    """Per row: the cofactors (c00, c01, c02, c11, c12, c22) and determinant of the damped V_r, g_r [3], z = V_r^-1 g_r, ok (the
    refusal rule of landmarks_ref._solve3)."""
    n = used[0].shape[0]
    zero = np.zeros(n, dtype=dt)
    h = [zero.copy() for _ in range(6)]
    g = [zero.copy() for _ in range(3)]
    for c in range(len(used)):
        v, u = views[c], used[c]
        p0, p1 = v["p0"], v["p1"]
        for k, (p, q) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
            h[k] = np.where(u, h[k] + (p0[p] * p0[q] + p1[p] * p1[q]), h[k])
        for k in range(3):
            g[k] = np.where(u, g[k] + (p0[k] * v["r0"] + p1[k] * v["r1"]), g[k])
    damp = dt(1.0) + lam
    a00, a01, a02, a11, a12, a22 = h[0] * damp, h[1], h[2], h[3] * damp, h[4], h[5] * damp
    c00, c01, c02 = a11 * a22 - a12 * a12, a02 * a12 - a01 * a22, a01 * a12 - a02 * a11
    c11, c12, c22 = a00 * a22 - a02 * a02, a01 * a02 - a00 * a12, a00 * a11 - a01 * a01
    det = _dot((a00, a01, a02), (c00, c01, c02), rev)
    cof = ((c00, c01, c02), (c01, c11, c12), (c02, c12, c22))
    z = [_dot(cof[k], g, rev) / det for k in range(3)]
    ok = np.isfinite(det) & (det > dt(L.DET_EPS) * ((a00 * a11) * a22)) & np.isfinite(z[0]) & np.isfinite(z[1]) & np.isfinite(z[2])
    return cof, det, g, z, ok


def _w_of(v):
    """W_rc [6][3] = j0 p0^T + j1 p1^T."""
    return [[v["j0"][a] * v["p0"][k] + v["j1"][a] * v["p1"][k] for k in range(3)] for a in range(6)]


def normal_equations(cams, X, used, pix, lam, way=WAY1):
    """The camera system before the gauge: dict(S [6L, 6L], lower triangle filled = damped U - sum W V^-1 W^T; rhs [6L]; cost; and
    what the back-substitution needs: W per view, the cofactors, det, g, ok per row)."""
    dt, rev = way
    Lw, n = len(used), X[0].shape[0]
    N = 6 * Lw
    zero = np.zeros(n, dtype=dt)
    views = [view(cams[c], X, pix[c], rev) for c in range(Lw)]
    cof, det, g, z, ok = point_blocks(views, used, lam, dt, rev)
    ss = zero.copy()
    for c in range(Lw):
        ss = np.where(used[c], ss + (views[c]["r0"] * views[c]["r0"] + views[c]["r1"] * views[c]["r1"]), ss)
    S = np.zeros((N, N), dtype=dt)
    rhs = np.zeros(N, dtype=dt)
    damp = dt(1.0) + lam
    Y = [None] * Lw
    W = [None] * Lw
    for c in range(Lw):
        act = used[c] & ok
        v = views[c]
        W[c] = _w_of(v)
        Y[c] = [[_dot(W[c][a], cof[k], rev) / det for k in range(3)] for a in range(6)]
        if not act.any():
            continue
        cols = [v["j0"][a] * v["j0"][b] + v["j1"][a] * v["j1"][b] for a in range(6) for b in range(a, 6)]
        cols += [v["j0"][a] * v["r0"] + v["j1"][a] * v["r1"] for a in range(6)]
        cols += [_dot(W[c][a], z, rev) for a in range(6)]
        s = tile_sum(np.stack([np.where(act, col, zero) for col in cols], axis=1))
        U = np.zeros((6, 6), dtype=dt)
        e = 0
        for a in range(6):
            for b in range(a, 6):
                U[b, a] = s[e] * damp if a == b else s[e]
                e += 1
        rhs[6 * c:6 * c + 6] = s[27:33] - s[21:27]
        for c2 in range(c + 1):
            both = act & used[c2]
            if not both.any():
                continue
            Ya = np.stack([np.stack(Y[c][a], axis=1) for a in range(6)], axis=1)          # [n, 6, 3]
            Wb = np.stack([np.stack(W[c2][b], axis=1) for b in range(6)], axis=1)         # [n, 6, 3]
            p = [Ya[:, :, None, k] * Wb[:, None, :, k] for k in range(3)]
            E = (p[2] + p[1]) + p[0] if rev else (p[0] + p[1]) + p[2]
            E = tile_sum(np.where(both[:, None, None], E, dt(0.0)))
            blk = (U - E) if c2 == c else (dt(0.0) - E)
            S[6 * c:6 * c + 6, 6 * c2:6 * c2 + 6] = np.tril(blk) if c2 == c else blk
    return {"S": S, "rhs": rhs, "cost": tile_sum(ss), "W": W, "cof": cof, "det": det, "g": g, "ok": ok}


# ---- the gauge and the solve ---------------------------------------------------------------------------------------------------
def gauge(cams):
    """(held [6L] bool, a, b, k*): all six parameters of every invalid view and of the first valid view a, and coordinate k* (the
    component of C_b - C_a of largest magnitude, the lowest on ties) of the centre of the last valid view b.  None when fewer
    than two views are valid."""
    Lw = cams.shape[0]
    valid = [c for c in range(Lw) if cams[c, 16] != 0.0]
    if len(valid) < 2:
        return None
    a, b = valid[0], valid[-1]
    d = np.abs(cams[b, 9:12] - cams[a, 9:12])
    ks = 0
    for k in (1, 2):
        if d[k] > d[ks]:
            ks = k
    held = np.ones(6 * Lw, dtype=bool)
    for c in valid[1:]:
        held[6 * c:6 * c + 6] = False
    held[6 * b + 3 + ks] = True
    return held, a, b, ks


def apply_gauge(S, rhs, held):
    """A held parameter: its row and column of S zeroed, its diagonal 1, its rhs 0 (the lower triangle is what is read)."""
    S, rhs = S.copy(), rhs.copy()
    for i in np.flatnonzero(held):
        S[i, :] = 0.0
        S[:, i] = 0.0
        S[i, i] = 1.0
        rhs[i] = 0.0
    return S, rhs


def cholesky_solve(S, rhs):
    """x of S x = rhs by Cholesky without pivoting on the lower triangle, right-looking: column k is scaled by its pivot's root,
    then taken out of every later column; the right-hand side rides along as one more column, and the back-substitution takes
    each solved unknown out of the earlier ones.  (x, ok): a pivot that is not finite or <= 0, or a result that is not finite,
    is a refusal."""
    A = np.array(S)
    y = np.array(rhs)
    N = A.shape[0]
    with np.errstate(all="ignore"):
        for k in range(N):
            d = A[k, k]
            if not (np.isfinite(d) and d > 0.0):
                return np.zeros(N, dtype=A.dtype), False
            r = np.sqrt(d)
            A[k, k] = r
            A[k + 1:, k] = A[k + 1:, k] / r
            y[k] = y[k] / r
            col = A[k + 1:, k]
            A[k + 1:, k + 1:] = A[k + 1:, k + 1:] - col[:, None] * col[None, :]
            y[k + 1:] = y[k + 1:] - col * y[k]
        for k in range(N - 1, -1, -1):
            y[k] = y[k] / A[k, k]
            y[:k] = y[:k] - A[k, :k] * y[k]
    return y, bool(np.all(np.isfinite(y)))


def candidate_cameras(cams, delta, held, rev=False):
    """Rw <- renormalised(Cay(w) Rw) (pnp_ref.cayley_update), C <- C + dC for every view that is not held whole; (cams, finite)."""
    out = cams.copy()
    dt = cams.dtype.type
    fin = True
    for c in range(cams.shape[0]):
        if held[6 * c:6 * c + 3].all():
            continue
        d = delta[6 * c:6 * c + 6]
        Rn, tn = PN.cayley_update(cams[c, 0:9], np.zeros(3, dtype=cams.dtype), [d[0], d[1], d[2], dt(0.0), dt(0.0), dt(0.0)], rev)
        Cn = cams[c, 9:12] + d[3:6]
        fin = fin and bool(np.all(np.isfinite(Rn)) and np.all(np.isfinite(tn)) and np.all(np.isfinite(Cn)))
        out[c, 0:9], out[c, 9:12] = Rn, Cn
    return out, fin


def back_substitute(ne, delta, used, X, way=WAY1):
    """X + dX, dX_r = V_r^-1 (-g_r - sum_c W_rc^T d_c); a refused row keeps its X."""
    dt, rev = way
    n = X[0].shape[0]
    t = [np.zeros(n, dtype=dt) for _ in range(3)]
    for c in range(len(used)):
        W, d = ne["W"][c], delta[6 * c:6 * c + 6]
        for k in range(3):
            s = W[0][k] * d[0] + W[1][k] * d[1]
            for a in range(2, 6):
                s = s + W[a][k] * d[a]
            t[k] = np.where(used[c] & ne["ok"], t[k] + s, t[k])
    b = [(0.0 - ne["g"][k]) - t[k] for k in range(3)]
    dX = [_dot(ne["cof"][k], b, rev) / ne["det"] for k in range(3)]
    return [np.where(ne["ok"], X[k] + dX[k], X[k]) for k in range(3)]


# ---- the loop ------------------------------------------------------------------------------------------------------------------
def adjust(ids, counts, pts, first_slot, cams, X, status, iterations=ITERATIONS, way=WAY1, trace=None):
    """ids [n_rows, L], counts [L], pts [L, point_cap, 2] (the ring), cams [L, CAM_WORDS] (landmarks_ref.map_window), X [n_rows, 3]
    and status [n_rows] of landmarks_ref.triangulate.  Returns dict(cams [L, CAM_WORDS], X [n_rows, 3], rms [n_rows], info
    [INFO_WORDS]).  trace: a list that receives one dict per iteration that ran."""
    dt, rev = way
    assert 1 <= int(iterations) <= MAX_ITERATIONS
    ids = np.asarray(ids, dtype=np.int64)
    n_rows, Lw = ids.shape
    pts = np.asarray(pts, dtype=dt)
    cams_in = np.asarray(cams, dtype=dt)
    cur_cams = np.zeros_like(cams_in)
    for c in range(Lw):
        if cams_in[c, 16] != 0.0:
            cur_cams[c] = cams_in[c]
    X_in = np.asarray(X, dtype=dt).reshape(n_rows, 3)
    status = np.asarray(status).reshape(n_rows)
    used, pix = observations(ids, counts, pts, first_slot, cur_cams, status)
    Xc = [X_in[:, k].copy() for k in range(3)]
    any_used = (status == 0)
    rows_used = int(any_used.sum())
    n_obs = int(sum(int(u.sum()) for u in used))
    n_valid = int((cur_cams[:, 16] != 0.0).sum())
    lam = dt(LAMBDA0)
    accepted, refused, done = 0, 0, False
    with np.errstate(all="ignore"):
        cost0, _, _, _ = cost_of(cur_cams, Xc, used, pix, rev)
        cost_cur = cost0
        g = gauge(cur_cams)
        if g is None or rows_used == 0 or 2 * n_obs < 6 * (n_valid - 1) - 1 + 3 * rows_used:
            state = NOTHING
        else:
            state = NO_STEP
            held = g[0]
            floor = dt(2.0) * dt(n_obs) * (dt(DONE_RESIDUAL) * dt(DONE_RESIDUAL))
            for it in range(int(iterations)):
                if done:
                    break
                ne = normal_equations(cur_cams, Xc, used, pix, lam, way)
                refused += int((any_used & ~ne["ok"]).sum())
                S, rhs = apply_gauge(ne["S"], ne["rhs"], held)
                delta, ok = cholesky_solve(S, rhs)
                rec = {"it": it, "lambda": lam, "cur": ne["cost"], "solved": ok, "S": S, "rhs": rhs, "delta": delta}
                accept = False
                if ok:
                    cand, ok = candidate_cameras(cur_cams, delta, held, rev)
                if ok:
                    Xn = back_substitute(ne, delta, used, Xc, way)
                    new, _, _, front = cost_of(cand, Xn, used, pix, rev)
                    accept = bool(np.isfinite(new)) and front and bool(new < ne["cost"])
                    rec.update(new=new, front=front)
                rec["accept"] = accept
                if accept:
                    cur_cams, Xc = cand, Xn
                    lam = max(lam / dt(10.0), dt(LAMBDA_MIN))
                    accepted += 1
                    state = ADJUSTED
                    done = bool(ne["cost"] - new <= dt(DONE_RELATIVE) * ne["cost"]) or bool(new <= floor)
                    cost_cur = new
                    rec.update(done=done, floor=floor)
                else:
                    lam = min(lam * dt(10.0), dt(LAMBDA_MAX))
                if trace is not None:
                    trace.append(rec)
        _, ss, nv, _ = cost_of(cur_cams, Xc, used, pix, rev)
        rms = np.where(nv > 0, np.sqrt(ss / (dt(2.0) * np.maximum(nv, 1).astype(dt))), dt(0.0))
    info = np.array([state, cost0, cost_cur, n_obs, rows_used, accepted, refused, lam], dtype=dt)
    return {"cams": cur_cams, "X": np.stack(Xc, axis=1) if n_rows else np.zeros((0, 3), dtype=dt), "rms": rms, "info": info}


# ---- the apply rule ------------------------------------------------------------------------------------------------------------
def apply(info, cams, state, table, L_window, n_frames=None, way=WAY1):
    """(state [STATE_WORDS], table [capacity, ROW_WORDS]) of one sequence after the adjusted cameras are written back (copies).
    Acts only under status 0.  Every valid view c other than the first valid one, with f = n - L + c inside the table: row f takes
    Rw and C, flag bit 3; s becomes |C_f - C_(f-1)| when view c - 1 is valid and the length is finite and above 1/64 of the row's
    s.  The state follows row n - 1 when that is its newest frame and the table is not full."""
    dt, rev = way
    state, table = np.array(state, dtype=dt), np.array(table, dtype=dt).reshape(-1, P.ROW_WORDS)
    cams = np.asarray(cams, dtype=dt)
    capacity = table.shape[0]
    if int(info[0]) != ADJUSTED:
        return state, table
    nf = state[0]
    count = int(nf) if 0.0 <= nf < 2147483647.0 else 0
    n = count if n_frames is None else int(n_frames)
    valid = [c for c in range(L_window) if cams[c, 16] != 0.0]
    for c in valid[1:]:
        f = n - L_window + c
        if not 0 <= f < capacity:
            continue
        row = table[f]
        row[0:12] = cams[c, 0:12]
        row[14] = dt(int(row[14]) | FLAG_ADJUSTED)
        if cams[c - 1, 16] != 0.0:
            d = cams[c, 9:12] - cams[c - 1, 9:12]
            with np.errstate(all="ignore"):
                length = np.sqrt(_dot(d, d, rev))
            if np.isfinite(length) and length > dt(PN.SCALE_FRACTION) * row[12]:
                row[12] = length
        if c == L_window - 1 and count == n and n < capacity:
            Rw, C = cams[c, 0:9], cams[c, 9:12]
            state[1], state[2:11] = row[12], Rw
            state[11:14] = [-_dot(Rw[3 * i:3 * i + 3], C, rev) for i in range(3)]
    return state, table


# ---- an independent way: the dense damped system ------------------------------------------------------------------------------
def dense_step(ids, counts, pts, first_slot, cams, X, status, lam=LAMBDA0):
    """One damped Gauss-Newton step by numpy.linalg.solve on the full system over the free camera parameters and every used
    point: (delta [6L] with zeros at the held parameters, dX [n_rows, 3])."""
    cams = np.asarray(cams, dtype=np.float64)
    X = np.asarray(X, dtype=np.float64)
    used, pix = observations(ids, counts, np.asarray(pts, dtype=np.float64), first_slot, cams, status)
    held = gauge(cams)[0]
    Lw, n = cams.shape[0], X.shape[0]
    rows = np.flatnonzero(np.asarray(status) == 0)
    col = {int(r): 6 * Lw + 3 * i for i, r in enumerate(rows)}
    J, res = [], []
    Xc = [X[:, k] for k in range(3)]
    for c in range(Lw):
        with np.errstate(all="ignore"):              # (the rows that do not see the view)
            v = view(cams[c], Xc, pix[c])
        for r in np.flatnonzero(used[c]):
            for jj, pp, rr in ((v["j0"], v["p0"], v["r0"]), (v["j1"], v["p1"], v["r1"])):
                line = np.zeros(6 * Lw + 3 * rows.size)
                line[6 * c:6 * c + 6] = [jj[a][r] if np.ndim(jj[a]) else jj[a] for a in range(6)]
                line[col[int(r)]:col[int(r)] + 3] = [pp[k][r] for k in range(3)]
                J.append(line)
                res.append(rr[r])
    J, res = np.array(J), np.array(res)
    free = np.concatenate([~held, np.ones(3 * rows.size, dtype=bool)])
    Jf = J[:, free]
    H = Jf.T @ Jf
    H[np.diag_indices_from(H)] *= 1.0 + lam
    step = np.linalg.solve(H, -(Jf.T @ res))
    full = np.zeros(J.shape[1])
    full[free] = step
    dX = np.zeros((n, 3))
    dX[rows] = full[6 * Lw:].reshape(-1, 3)
    return full[:6 * Lw], dX


# ---- fixtures ------------------------------------------------------------------------------------------------------------------
PERTURB_SEED = 3
# name -> another seed, where seed 3 leaves a comparison of the loop within a factor of 8 of its threshold (long16: its last step
# ended at 0.376 of the residual floor; seeds 4 to 6 accept 68 rows, not the 69 true tracks the table holds)
PERTURB_SEEDS = {"long16": 7}
FIXTURES = ("mixed48", "seq3", "seq5", "seq5_k", "seq5_late", "noisy5", "long16", "big")
NOISE_FREE = tuple(nm for nm in FIXTURES if nm != "noisy5")
SMALL_ROTATION = ("long16", "big")           # 0.05 degrees instead of 0.2
SCENARIOS = ("no_pose", "two_frames")
CHAIN_SEEDS = (41, 42, 43, 44, 45, 46)
CHAIN_L, CHAIN_POINT_CAP, CHAIN_SEED0 = 5, 96, 7
EXPECTED_ROWS = {"mixed48": 32, "seq3": 40, "seq5": 40, "seq5_k": 40, "seq5_late": 49, "noisy5": 40, "long16": 69, "big": 614}


def perturbed_cams(name):
    """The true cameras of a landmarks_ref fixture with every valid view but the first turned by a Cayley rotation of 0.2 (0.05)
    degrees about a random axis and its centre moved by N(0, 0.02 first baselines) per component; coordinate k* of the last view
    stays (the held coordinate), and mixed48 is turned only."""
    fx = L.fixture(name)
    cams = fx["cams"].copy()
    rng = np.random.RandomState(PERTURB_SEEDS.get(name, PERTURB_SEED))
    valid = [c for c in range(cams.shape[0]) if cams[c, 16] != 0.0]
    _, a, b, ks = gauge(cams)
    base = float(np.linalg.norm(cams[valid[1], 9:12] - cams[valid[0], 9:12]))
    deg = 0.05 if name in SMALL_ROTATION else 0.2
    for c in valid[1:]:
        axis = rng.randn(3)
        w = axis / np.linalg.norm(axis) * (2.0 * math.tan(math.radians(deg) / 2.0))
        shift = rng.randn(3) * (0.02 * base)
        Rn, _ = PN.cayley_update(cams[c, 0:9].copy(), np.zeros(3), [w[0], w[1], w[2], 0.0, 0.0, 0.0])
        cams[c, 0:9] = Rn
        if name != "mixed48":
            if c == b:
                shift[ks] = 0.0
            cams[c, 9:12] += shift
    return cams


@functools.lru_cache(maxsize=None)
def problem(name):
    """dict(ids, tid, tracks, counts, pts, first_slot, L, point_cap, cams, rows: landmarks_ref.triangulate under `cams` with the
    default thresholds, and for a fixture: point, X0, true_cams) of a fixture, a window scenario ("no_pose", "two_frames": the
    cameras of the restated chain) or a noisy chain ("chain41" ..: with seq, table, n_frames too).  Read-only."""
    if name in FIXTURES:
        fx = L.fixture(name)
        out = {k: fx[k] for k in ("ids", "tid", "tracks", "counts", "pts", "first_slot", "L", "point_cap", "point")}
        out.update(cams=perturbed_cams(name), true_cams=fx["cams"], X0=fx["seq"]["X0"])
    elif name in SCENARIOS:
        fx, n, table = L.scenario_inputs(name)
        out = {k: fx[k] for k in ("ids", "tid", "tracks", "counts", "pts", "first_slot", "L", "point_cap")}
        out.update(cams=L.map_window(n, table, fx["seq"]["intr"][:1], fx["L"]), table=table, n_frames=n)
    else:
        seed = int(name[len("chain"):])
        assert name.startswith("chain") and seed in CHAIN_SEEDS
        seq = L._scene(("side", seed, 5, 60, 8, 0.3, False))
        run = PN.run_sequence(seq, CHAIN_L, CHAIN_POINT_CAP, None, CHAIN_SEED0)
        frames = len(seq["pts"])
        table = np.zeros((frames + 3, P.ROW_WORDS))
        table[:frames] = run["table"]
        t = run["tracks"]
        pts, first_slot = L.ring_of(seq, CHAIN_L, CHAIN_POINT_CAP)
        out = {"ids": t.ids, "tid": t.tid, "tracks": t, "counts": list(t.counts), "pts": pts, "first_slot": first_slot, "L": CHAIN_L,
               "point_cap": CHAIN_POINT_CAP, "cams": L.map_window(frames, table, seq["intr"][:1], CHAIN_L), "table": table,
               "n_frames": frames, "seq": seq}
    out["rows"] = L.triangulate(out["ids"], out["counts"], out["pts"], out["first_slot"], out["cams"])
    return out


CHAINS = tuple("chain%d" % s for s in CHAIN_SEEDS)
COMPARED = FIXTURES + SCENARIOS + CHAINS            # what the device is compared on and the tolerance is measured on


def solve(name, iterations=ITERATIONS, way=WAY1, trace=None):
    pr = problem(name)
    return adjust(pr["ids"], pr["counts"], pr["pts"], pr["first_slot"], pr["cams"], pr["rows"]["X"], pr["rows"]["status"],
                  iterations, way, trace)


@functools.lru_cache(maxsize=None)
def solved(name, iterations=ITERATIONS, wide=False):
    """solve() once per (name, iterations, way): (result, trace).  Read-only."""
    trace = []
    return solve(name, iterations, WAY2 if wide else WAY1, trace), trace


def result_difference(a, b):
    """The largest difference of cams, X, rms and the two costs between two results, relative to max(1, |value|); the discrete
    words of info must agree."""
    assert [int(a["info"][k]) for k in (0, 3, 4, 5, 6)] == [int(b["info"][k]) for k in (0, 3, 4, 5, 6)], (a["info"], b["info"])
    worst = 0.0
    for x, y in ((a["cams"], b["cams"]), (a["X"], b["X"]), (a["rms"], b["rms"]), (a["info"][1:3], b["info"][1:3])):
        x, y = np.asarray(x, dtype=np.longdouble), np.asarray(y, dtype=np.longdouble)
        if x.size:
            worst = max(worst, float((np.abs(x - y) / np.maximum(1.0, np.abs(y))).max()))
    return worst


def way_difference(names=COMPARED, iterations=(ITERATIONS, 1)):
    return max(result_difference(solved(nm, it, False)[0], solved(nm, it, True)[0]) for nm in names for it in iterations)


def truth_error(name, res=None):
    """(largest |X - scene point| over the used true tracks, largest |C - true centre|, largest rms) of a noise-free fixture."""
    pr = problem(name)
    res = solved(name)[0] if res is None else res
    sel = (pr["point"] >= 0) & (np.asarray(pr["rows"]["status"]) == 0)
    X = np.asarray(res["X"], dtype=np.float64)
    cams = np.asarray(res["cams"], dtype=np.float64)
    return (float(np.abs(X[sel] - pr["X0"][pr["point"][sel]]).max()), float(np.abs(cams[:, 9:12] - pr["true_cams"][:, 9:12]).max()),
            float(np.asarray(res["rms"], dtype=np.float64).max()))


def chain_errors(name, res=None):
    """(centre error of the chain's table, centre error after the adjusted cameras are applied), in first baselines."""
    pr = problem(name)
    res = solved(name)[0] if res is None else res
    state = np.zeros(P.STATE_WORDS)
    state[0] = pr["n_frames"]
    _, table = apply(np.asarray(res["info"], dtype=np.float64), np.asarray(res["cams"], dtype=np.float64), state, pr["table"], pr["L"])
    n = pr["n_frames"]
    return PN.sequence_centre_error(pr["seq"], pr["table"][:n]), PN.sequence_centre_error(pr["seq"], table[:n])


# As way_difference(FIXTURES) (both iteration counts) and the maxima of truth_error(.) over NOISE_FREE returned them when the
# fixtures were fixed; tests/test_ba_cpu.py repeats the measurements.  The bounds are 16 times these.  The scenarios and the chains
# differ by at most 3.06e-13 between the two ways, inside the same tolerance.
WAY_DIFFERENCE = 8.96969673015724e-14         # (seq5_late after one iteration), numpy.longdouble (80-bit) as WAY2
TRUTH_ERROR_X = 1.3721793479248845e-08        # (long16: 16 views a fraction of a baseline apart)
TRUTH_ERROR_C = 4.497392458446825e-10
TRUTH_RMS = 5.180844152433846e-10
TOLERANCE = 16.0 * WAY_DIFFERENCE
TRUTH_BOUND_X = 16.0 * TRUTH_ERROR_X
TRUTH_BOUND_C = 16.0 * TRUTH_ERROR_C
TRUTH_BOUND_RMS = 16.0 * TRUTH_RMS
MARGIN = 8.0                                  # what decision_margins(FIXTURES) must reach; long16 missed it under seed 3 (2.66)


def unobserved_problem(name="seq5", view=2):
    """A fixture whose view `view` is valid but seen by no track: its 6 x 6 block of S is zero, the Cholesky pivot is refused and no
    step is ever accepted (status 2)."""
    pr = dict(problem(name))
    ids = pr["ids"].copy()
    ids[:, view] = -1
    pr["ids"] = ids
    pr["rows"] = L.triangulate(ids, pr["counts"], pr["pts"], pr["first_slot"], pr["cams"])
    return pr


def decision_margins(names=FIXTURES + CHAINS):
    """Over every iteration of the named problems that tried a step, in float64 and in the other way: the smallest factor by which
    a comparison of the loop clears its threshold - |cur - new| against DONE_RELATIVE * cur and new against the residual floor
    (either side), and |cur - new| against the difference of the two ways in that very quantity.  The two ways must have taken
    the same decisions."""
    worst = np.inf
    for nm in names:
        ta, tb = solved(nm, ITERATIONS, False)[1], solved(nm, ITERATIONS, True)[1]
        assert [(r["accept"], r.get("done")) for r in ta] == [(r["accept"], r.get("done")) for r in tb], nm
        n_obs = float(solved(nm)[0]["info"][3])
        floor = 2.0 * n_obs * DONE_RESIDUAL ** 2
        for ra, rb in zip(ta, tb):
            if "new" not in ra:
                continue
            cur, new = float(ra["cur"]), float(ra["new"])
            d, thr = cur - new, DONE_RELATIVE * cur
            by_floor = ra["accept"] and new <= floor
            for x, t in ((abs(d), thr), (new, floor)):
                if by_floor and t is thr:
                    continue                       # done by the residual floor: the relative rule decides nothing
                worst = min(worst, max(x / t, t / x) if x > 0.0 else np.inf)
            noise = abs(float((rb["cur"] - rb["new"]) - np.longdouble(d)))
            worst = min(worst, abs(d) / noise if noise > 0.0 else np.inf)
    return worst
