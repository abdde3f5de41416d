"""numpy restatement of the two-view pose (csrc/pose_kernels.hip.h): the essential matrix of a
fundamental matrix and the intrinsics, its singular vectors without a 3x3 SVD (the Jacobi sweeps of section 22 on E^T E),
the four (R, t) candidates, the cheirality count over the inliers, the per-row depths, the scale chain between consecutive
pairs and the trajectory rows.  There is no reference counterpart and no OpenCV here, so this file is the specification the
kernels are tested against.  Everything is fp64 in the parenthesisation written here; every function also runs in another
"way" (`WAY2`: numpy.longdouble where that is wider than float64, else the dot products and the chain sums in the reverse
order), which is how the tolerance of the continuous outputs is measured (`way_difference`, TOLERANCE below).
Also the synthetic sequences (a camera that rotates, translates and zooms past fixed points) and the fixtures of the tests."""
import functools

import numpy as np

from tests import epipolar_ref as E

MIN_FRONT = 8          # a pose needs that many inliers, and that many of them in front of both cameras
DET_EPS = 1e-12        # rays closer to parallel than det <= DET_EPS * (A11 * A22) give no depth
ROW_WORDS = 16         # trajectory row: Rw [9], C [3], s, n_shared, flags, ratio
STATE_WORDS = 16       # chain state: n_frames, s, Rw [9], tw [3], 2 spare
FLAG_NO_POSE, FLAG_SCALE_CARRIED = 1, 2

WIDE = bool(np.finfo(np.longdouble).eps < np.finfo(np.float64).eps)
WAY1 = (np.float64, False)
WAY2 = (np.longdouble, False) if WIDE else (np.float64, True)


def _dot(p, q, rev=False):
    """(p0*q0 + p1*q1) + p2*q2; rev: the same three products added from the other end."""
    if rev:
        return (p[2] * q[2] + p[1] * q[1]) + p[0] * q[0]
    return (p[0] * q[0] + p[1] * q[1]) + p[2] * q[2]


def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], dtype=a.dtype)


def _usable(v):
    return bool(np.isfinite(v) and v > 0.0)


def jacobi3(G, dt=np.float64):
    """epipolar_ref.jacobi3 in the number format dt (bit-identical to it for float64: tests/test_pose_cpu.py)."""
    G = np.array(G, dtype=dt).reshape(3, 3)
    V = np.eye(3, dtype=dt)
    one, two = dt(1.0), dt(2.0)
    with np.errstate(all="ignore"):
        for _ in range(E.JACOBI_SWEEPS):
            for (p, q) in ((0, 1), (0, 2), (1, 2)):
                gpq = G[p, q]
                if gpq == 0.0:
                    continue
                r = 3 - p - q
                theta = (G[q, q] - G[p, p]) / (two * gpq)
                t = one / (abs(theta) + np.sqrt(theta * theta + one))
                if theta < 0.0:
                    t = -t
                c = one / np.sqrt(t * t + one)
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
    return np.array([G[0, 0], G[1, 1], G[2, 2]], dtype=dt), V


def essential(F, intr, way=WAY1):
    """E0 = K2^T F K1 in two stages, divided by its Frobenius norm: [9], or None (status 1).  intr: [2][4] rows
    (fx, fy, cx, cy) of view 1 and view 2."""
    dt, _ = way
    F = np.asarray(F, dtype=dt).reshape(9)
    (fx1, fy1, cx1, cy1), (fx2, fy2, cx2, cy2) = np.asarray(intr, dtype=dt).reshape(2, 4)
    with np.errstate(all="ignore"):
        B = np.zeros(9, dtype=dt)
        for r in range(3):
            B[3 * r] = F[3 * r] * fx1
            B[3 * r + 1] = F[3 * r + 1] * fy1
            B[3 * r + 2] = (F[3 * r] * cx1 + F[3 * r + 1] * cy1) + F[3 * r + 2]
        E0 = np.zeros(9, dtype=dt)
        for c in range(3):
            E0[c] = fx2 * B[c]
            E0[3 + c] = fy2 * B[3 + c]
            E0[6 + c] = (cx2 * B[c] + cy2 * B[3 + c]) + B[6 + c]
        ss = dt(0.0)
        for k in range(9):
            ss = ss + E0[k] * E0[k]
        nrm = np.sqrt(ss)
        if not _usable(nrm):
            return None
        return E0 / nrm


def decompose(E0, way=WAY1):
    """(U [3,3], V [3,3]) with columns u0 u1 u2 / v0 v1 v2 as the rules build them, or None (status 1)."""
    dt, rev = way
    E0 = np.asarray(E0, dtype=dt).reshape(3, 3)
    with np.errstate(all="ignore"):
        G = np.zeros((3, 3), dtype=dt)
        for i in range(3):
            for j in range(3):
                G[i, j] = _dot(E0[:, i], E0[:, j], rev)
        d, Vj = jacobi3(G, dt)
        k0 = 0
        for j in (1, 2):
            if d[j] > d[k0]:
                k0 = j
        rest = [j for j in range(3) if j != k0]
        k1 = rest[1] if d[rest[1]] > d[rest[0]] else rest[0]
        v0, v1 = Vj[:, k0].copy(), Vj[:, k1].copy()
        v2 = _cross(v0, v1)
        w = np.array([_dot(E0[r], v0, rev) for r in range(3)], dtype=dt)
        n0 = np.sqrt(_dot(w, w, rev))
        if not _usable(n0):
            return None
        u0 = w / n0
        w = np.array([_dot(E0[r], v1, rev) for r in range(3)], dtype=dt)
        w = w - _dot(w, u0, rev) * u0
        n1 = np.sqrt(_dot(w, w, rev))
        if not _usable(n1):
            return None
        u1 = w / n1
        u2 = _cross(u0, u1)
    return np.stack([u0, u1, u2], axis=1), np.stack([v0, v1, v2], axis=1)


def candidates(U, V):
    """(E [3,3], Ra, Rb, u2): E = u0 v0^T + u1 v1^T, Ra = U W V^T, Rb = U W^T V^T written out."""
    u0, u1, u2 = U[:, 0], U[:, 1], U[:, 2]
    v0, v1, v2 = V[:, 0], V[:, 1], V[:, 2]
    Em, Ra, Rb = (np.zeros((3, 3), dtype=U.dtype) for _ in range(3))
    for r in range(3):
        for c in range(3):
            Em[r, c] = u0[r] * v0[c] + u1[r] * v1[c]
            Ra[r, c] = (u1[r] * v0[c] - u0[r] * v1[c]) + u2[r] * v2[c]
            Rb[r, c] = (u0[r] * v1[c] - u1[r] * v0[c]) + u2[r] * v2[c]
    return Em, Ra, Rb, u2.copy()


def rays(m, intr, way=WAY1):
    """x1 [n,3], x2 [n,3] of matches m [n,4] (ax, ay, bx, by)."""
    dt, _ = way
    m = np.asarray(m, dtype=dt).reshape(-1, 4)
    (fx1, fy1, cx1, cy1), (fx2, fy2, cx2, cy2) = np.asarray(intr, dtype=dt).reshape(2, 4)
    one = np.ones(m.shape[0], dtype=dt)
    with np.errstate(all="ignore"):
        return (np.stack([(m[:, 0] - cx1) / fx1, (m[:, 1] - cy1) / fy1, one], axis=1),
                np.stack([(m[:, 2] - cx2) / fx2, (m[:, 3] - cy2) / fy2, one], axis=1))


def depths(R, t, x1, x2, way=WAY1):
    """(z1 [n], z2 [n], front [n]) of the rays under candidate (R, t): the least-squares meeting point of z1 R x1 + t and z2 x2."""
    dt, rev = way
    with np.errstate(all="ignore"):
        d1 = [_dot(R[r], x1.T, rev) for r in range(3)]
        d2 = [x2[:, 0], x2[:, 1], x2[:, 2]]
        A11, A22, A12 = _dot(d1, d1, rev), _dot(d2, d2, rev), _dot(d1, d2, rev)
        b1, b2 = -_dot(d1, t, rev), _dot(d2, t, rev)
        det = A11 * A22 - A12 * A12
        z1 = (b1 * A22 + A12 * b2) / det
        z2 = (A11 * b2 + A12 * b1) / det
        front = (det > dt(DET_EPS) * (A11 * A22)) & np.isfinite(z1) & np.isfinite(z2) & (z1 > 0.0) & (z2 > 0.0)
    return z1, z2, front


def two_view_pose(F, mask, n_inliers, status_in, m, intr, way=WAY1):
    """The pose of one pair.  F [9] / [3,3], mask [n] over the match rows m [n,4], n_inliers and status of the epipolar check,
    intr [2][4].  Returns dict(R [3,3], t [3], E [3,3], cand, counts [4], n_front, status, front [n] bool, depth [n,2],
    X [n,3]) in the number format of `way`."""
    dt, _ = way
    m = np.asarray(m, dtype=np.float64).reshape(-1, 4)
    n = m.shape[0]
    mask = np.asarray(mask).astype(bool).reshape(-1)[:n]
    out = {"R": np.eye(3, dtype=dt), "t": np.zeros(3, dtype=dt), "E": np.zeros((3, 3), dtype=dt), "cand": -1,
           "counts": np.zeros(4, dtype=np.int64), "n_front": 0, "status": 1, "front": np.zeros(n, dtype=bool),
           "depth": np.zeros((n, 2), dtype=dt), "X": np.zeros((n, 3), dtype=dt)}
    if int(status_in) != 0 or int(n_inliers) < MIN_FRONT:
        return out
    E0 = essential(F, intr, way)
    UV = decompose(E0, way) if E0 is not None else None
    if UV is None:
        return out
    Em, Ra, Rb, u2 = candidates(*UV)
    x1, x2 = rays(m, intr, way)
    cands = ((Ra, u2), (Ra, -u2), (Rb, u2), (Rb, -u2))
    res = [depths(R, t, x1, x2, way) for R, t in cands]
    counts = np.array([int((f & mask).sum()) for _, _, f in res], dtype=np.int64)
    win = 0
    for c in (1, 2, 3):
        if counts[c] > counts[win]:
            win = c
    z1, z2, front = res[win]
    front = front & mask
    zero = dt(0.0)
    out.update(R=cands[win][0], t=cands[win][1], E=Em, cand=win, counts=counts, n_front=int(counts[win]),
               status=2 if (counts[win] < MIN_FRONT or 2 * counts[win] < int(n_inliers)) else 0, front=front,
               depth=np.stack([np.where(front, z1, zero), np.where(front, z2, zero)], axis=1),
               X=np.where(front[:, None], z1[:, None] * x1, zero))
    return out


def _indices(match, n_match, cap):
    """(i [n], j [n]) of match rows (i, j, d), clamped as section 22 clamps them."""
    n = min(max(int(n_match), 0), match.shape[0])
    return (np.clip(match[:n, 0].astype(np.int64), 0, cap - 1), np.clip(match[:n, 1].astype(np.int64), 0, cap - 1))


def new_state(way=WAY1):
    dt, _ = way
    return {"n_frames": 0, "s": dt(1.0), "Rw": np.eye(3, dtype=dt), "tw": np.zeros(3, dtype=dt)}


def chain_step(prev, cur, match_prev, match_cur, n_match_prev, n_match_cur, state, cap_prev, cap_cur, way=WAY1):
    """One frame of the scale chain and the trajectory.  prev / cur: two_view_pose dicts of pair A = (f-1, f) (None: there is no
    such pair) and B = (f, f+1); match rows [.,3] (i, j, d) of both.  Returns (row [ROW_WORDS], the new state)."""
    dt, rev = way
    shared_prev, shared_cur = [], []
    if prev is not None:
        _, jA = _indices(match_prev, n_match_prev, cap_prev)
        zprev = {}
        for k in range(jA.shape[0]):
            if prev["front"][k] and int(jA[k]) not in zprev:       # the lowest row wins
                zprev[int(jA[k])] = prev["depth"][k, 1]
        iB, _ = _indices(match_cur, n_match_cur, cap_cur)
        for k in range(iB.shape[0]):
            if cur["front"][k] and int(iB[k]) in zprev:
                shared_prev.append(zprev[int(iB[k])])
                shared_cur.append(cur["depth"][k, 0])
    n_shared = len(shared_cur)
    sa, sb = dt(0.0), dt(0.0)
    for k in (range(n_shared - 1, -1, -1) if rev else range(n_shared)):
        sa = sa + dt(shared_prev[k])
        sb = sb + dt(shared_cur[k])
    with np.errstate(all="ignore"):
        ratio = sa / sb if n_shared > 0 else dt(0.0)
    ok = (prev is not None and prev["status"] == 0 and cur["status"] == 0 and n_shared >= MIN_FRONT and _usable(ratio))
    s = state["s"] * ratio if ok else state["s"]
    posed = cur["status"] == 0
    R = np.asarray(cur["R"], dtype=dt) if posed else np.eye(3, dtype=dt)
    t = np.asarray(cur["t"], dtype=dt) if posed else np.zeros(3, dtype=dt)
    Rw0, tw0 = state["Rw"], state["tw"]
    Rw, tw = np.zeros((3, 3), dtype=dt), np.zeros(3, dtype=dt)
    for r in range(3):
        for c in range(3):
            Rw[r, c] = _dot(R[r], Rw0[:, c], rev)
        tw[r] = _dot(R[r], tw0, rev) + s * t[r]
    C = np.array([-_dot(Rw[:, c], tw, rev) for c in range(3)], dtype=dt)
    flags = (0 if posed else FLAG_NO_POSE) | (0 if ok else FLAG_SCALE_CARRIED)
    row = np.concatenate([Rw.reshape(9), C, [s, dt(n_shared), dt(flags), ratio]]).astype(dt)
    return row, {"n_frames": state["n_frames"] + 1, "s": s, "Rw": Rw, "tw": tw}


def state_words(state):
    """The chain state as the device keeps it: float64 [STATE_WORDS]."""
    out = np.zeros(STATE_WORDS)
    out[0], out[1] = state["n_frames"], state["s"]
    out[2:11], out[11:14] = np.asarray(state["Rw"], dtype=np.float64).reshape(9), state["tw"]
    return out


# ---- synthetic sequences -------------------------------------------------------------------------------------------------
# The camera of frame f sees X_f = R_f X_0 + t_f; between frames it rotates by a few degrees, translates by a step of varying
# length and, with zoom, changes its focal length and principal point, so the two views of a pair have unequal intrinsics.
MOTIONS = {                      # rotation vector of a step in degrees, direction of its translation
    "side": ((1.0, 7.0, -2.0), (1.0, 0.2, 0.3)),
    "forward": ((0.5, -1.5, 1.0), (0.05, 0.03, -1.0)),      # the epipole lies inside the image
    "backward": ((-2.0, 3.0, 1.0), (0.2, -0.1, 1.0)),
}


def _rodrigues(deg):
    w = np.deg2rad(np.asarray(deg, dtype=np.float64))
    th = np.linalg.norm(w)
    k = w / th
    Kx = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(th) * Kx + (1.0 - np.cos(th)) * (Kx @ Kx)


def intrinsics_of(frame, zoom):
    """(fx, fy, cx, cy) of a frame."""
    if not zoom:
        return np.array([E.FOCAL, E.FOCAL, E.WIDTH / 2, E.HEIGHT / 2])
    return np.array([E.FOCAL * (1.0 + 0.06 * frame), E.FOCAL * (1.0 + 0.05 * frame), E.WIDTH / 2 + 2.0 * frame, E.HEIGHT / 2 - 1.5 * frame])


def k_matrix(intr):
    fx, fy, cx, cy = intr
    return np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])


def _project(X, intr):
    return np.stack([intr[0] * X[:, 0] / X[:, 2] + intr[2], intr[1] * X[:, 1] / X[:, 2] + intr[3]], axis=1)


def make_sequence(seed, frames, n_in, n_out, noise=0.0, motion="side", zoom=True):
    """`frames` views of n_in fixed points at depth 3 to 12 that stay visible, plus n_out stray points per frame whose matches are
    wrong: at least E.MARGIN px from both epipolar lines of their pair.  Returns dict(pts: per frame [N,2] rows in an order of
    its own, ids: per frame the point of each row, intr [frames,4], centres [frames,3] (world = camera 0), pairs: per pair
    dict(m [n,4], match [n,3] float32 rows (i, j, d) in ascending i, truth [n], R, t (unit), length, F, intr [2,4]))."""
    rng = np.random.RandomState(seed)
    rot, direction = MOTIONS[motion]
    direction = np.asarray(direction) / np.linalg.norm(direction)
    Rf, tf = [np.eye(3)], [np.zeros(3)]
    steps = []
    for f in range(1, frames):
        Rs = _rodrigues(np.asarray(rot) * (0.8 + 0.4 * rng.rand()))
        ts = direction * (0.3 + 0.25 * rng.rand())
        steps.append((Rs, ts))
        Rf.append(Rs @ Rf[-1])
        tf.append(Rs @ tf[-1] + ts)
    intr = np.stack([intrinsics_of(f, zoom) for f in range(frames)])
    N = n_in + n_out
    X0 = np.zeros((0, 3))
    while X0.shape[0] < n_in:
        a = np.stack([rng.uniform(8, E.WIDTH - 8, 4 * n_in + 8), rng.uniform(8, E.HEIGHT - 8, 4 * n_in + 8)], axis=1)
        z = rng.uniform(3.0, 12.0, a.shape[0])
        X = np.stack([(a[:, 0] - intr[0, 2]) * z / intr[0, 0], (a[:, 1] - intr[0, 3]) * z / intr[0, 1], z], axis=1)
        ok = np.ones(X.shape[0], dtype=bool)
        for f in range(frames):
            Y = X @ Rf[f].T + tf[f]
            b = _project(Y, intr[f])
            ok &= (Y[:, 2] > 1.0) & (b[:, 0] > 4) & (b[:, 0] < E.WIDTH - 4) & (b[:, 1] > 4) & (b[:, 1] < E.HEIGHT - 4)
        X0 = np.concatenate([X0, X[ok]])
    X0 = X0[:n_in]
    by_id = []                                   # per frame: the pixel of every point id (true points first, strays behind)
    pairs = []
    for f in range(frames):
        px = _project(X0 @ Rf[f].T + tf[f], intr[f])
        if noise > 0.0:
            px = px + noise * rng.randn(n_in, 2)
        stray = np.stack([rng.uniform(8, E.WIDTH - 8, n_out), rng.uniform(8, E.HEIGHT - 8, n_out)], axis=1)
        if f > 0:
            Rs, ts = steps[f - 1]
            tx = np.array([[0.0, -ts[2], ts[1]], [ts[2], 0.0, -ts[0]], [-ts[1], ts[0], 0.0]])
            F = np.linalg.inv(k_matrix(intr[f])).T @ tx @ Rs @ np.linalg.inv(k_matrix(intr[f - 1]))
            a = by_id[f - 1][n_in:]
            for k in range(n_out):
                while True:
                    b = np.stack([rng.uniform(8, E.WIDTH - 8, 32), rng.uniform(8, E.HEIGHT - 8, 32)], axis=1)
                    d1, d2 = E.line_dist(F, np.repeat(a[k:k + 1], 32, axis=0), b)
                    good = np.nonzero((d1 >= E.MARGIN) & (d2 >= E.MARGIN))[0]
                    if good.size:
                        stray[k] = b[good[0]]
                        break
            pairs.append({"R": Rs, "t": ts / np.linalg.norm(ts), "length": float(np.linalg.norm(ts)), "F": F,
                          "intr": np.stack([intr[f - 1], intr[f]])})
        by_id.append(np.concatenate([px, stray]))
    ids = [rng.permutation(N) for _ in range(frames)]
    pts = [np.ascontiguousarray(by_id[f][ids[f]]) for f in range(frames)]
    for f in range(1, frames):
        row_prev, row_cur = np.argsort(ids[f - 1]), np.argsort(ids[f])      # row of every point id
        order = ids[f - 1]                                                   # ascending i: the ids in the previous frame's row order
        match = np.zeros((N, 3), dtype=np.float32)
        match[:, 0] = np.arange(N)
        match[:, 1] = row_cur[order]
        match[:, 2] = rng.rand(N).astype(np.float32)
        assert np.array_equal(row_prev[order], np.arange(N))
        pairs[f - 1].update(match=match, truth=order < n_in,
                            m=np.concatenate([pts[f - 1], pts[f][row_cur[order]]], axis=1).astype(np.float64))
    centres = np.stack([-(Rf[f].T @ tf[f]) for f in range(frames)])
    return {"pts": pts, "ids": ids, "intr": intr, "centres": centres, "pairs": pairs, "n_in": n_in}


def angle_deg(a, b):
    """Angle between two vectors (atan2 of |a x b| and a . b) or between two rotations (from |a - b|_F = 2 sqrt(2) sin(angle / 2)),
    in degrees; both forms stay accurate near zero, where arccos does not."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.ndim == 2:
        return float(np.degrees(2.0 * np.arcsin(min(1.0, np.linalg.norm(a - b) / (2.0 * np.sqrt(2.0))))))
    return float(np.degrees(np.arctan2(np.linalg.norm(np.cross(a, b)), a @ b)))


# ---- fixtures ------------------------------------------------------------------------------------------------------------
# name -> (scene seed, frames, inliers, outliers, noise px, motion, zoom, RANSAC seed of pair 0; pair k uses seed + k).  The seeds
# were searched with the restatements so that on the noise-free fixtures every pair's RANSAC mask equals the truth and every
# inlier lies in front of both cameras; tests/test_pose_cpu.py asserts both before anything else.
CASES = {
    "mixed48": (0, 2, 32, 16, 0.0, "side", True, 200),
    "eight": (1, 2, 8, 0, 0.0, "side", True, 201),
    "eight_k": (1, 2, 8, 0, 0.0, "side", False, 201),       # "eight" seen by two equal cameras (per-pair intrinsics)
    "five": (2, 2, 5, 0, 0.0, "side", True, 202),
    "empty": (3, 2, 0, 0, 0.0, "side", True, 203),
    "n257": (4, 2, 200, 57, 0.0, "side", True, 204),
    "n4096": (5, 2, 3000, 1096, 0.0, "side", True, 205),
    "noisy": (6, 2, 150, 100, 0.3, "side", True, 206),
    "forward": (7, 2, 60, 0, 0.0, "forward", True, 207),
    "backward": (8, 2, 60, 0, 0.0, "backward", True, 208),
    "equal_k": (9, 2, 60, 0, 0.0, "side", False, 209),
    "seq3": (10, 3, 40, 8, 0.0, "side", True, 210),
    "seq5": (17, 5, 40, 8, 0.0, "side", True, 220),
    "seq5_k": (30, 5, 40, 8, 0.0, "side", False, 230),      # one camera throughout: what a tracker with one set of intrinsics sees
}
NOISE_FREE = tuple(k for k, v in CASES.items() if v[4] == 0.0 and v[2] >= 8)
COMPARED = ("mixed48", "eight", "n257", "n4096", "noisy", "seq5")      # the fixtures the device results are compared on


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(seq = make_sequence(...), ransac: per pair epipolar_ref.ransac, pose / pose2: per pair two_view_pose in WAY1 / WAY2,
    rows / rows2, state / state2: the chain over the sequence in both ways); computed once and shared: treat it as read-only."""
    scene_seed, frames, n_in, n_out, noise, motion, zoom, seed = CASES[name]
    seq = make_sequence(scene_seed, frames, n_in, n_out, noise=noise, motion=motion, zoom=zoom)
    out = {"seq": seq, "ransac": [], "pose": [], "pose2": [], "seeds": []}
    for k, pr in enumerate(seq["pairs"]):
        r = E.ransac(pr["m"], seed + k)
        out["ransac"].append(r)
        out["seeds"].append(seed + k)
        for key, way in (("pose", WAY1), ("pose2", WAY2)):
            out[key].append(two_view_pose(r["F"], r["mask"], r["n_inliers"], r["status"], pr["m"], pr["intr"], way))
    for pose, rows, st, way in (("pose", "rows", "state", WAY1), ("pose2", "rows2", "state2", WAY2)):
        out[rows], out[st] = run_chain(out[pose], [pr["match"] for pr in seq["pairs"]], way)
    return out


def run_chain(poses, matches, way=WAY1, cap=None):
    """The chain over consecutive pairs: (rows [len(poses), ROW_WORDS], final state)."""
    dt, _ = way
    state = new_state(way)
    rows = np.zeros((len(poses), ROW_WORDS), dtype=dt)
    for k, cur in enumerate(poses):
        prev = poses[k - 1] if k > 0 else None
        mp = matches[k - 1] if k > 0 else None
        rows[k], state = chain_step(prev, cur, mp, matches[k], mp.shape[0] if k > 0 else 0, matches[k].shape[0], state,
                                    cap or (mp.shape[0] if k > 0 else 1), cap or matches[k].shape[0], way)
    return rows, state


POSE_KEYS = ("R", "t", "E")


def way_difference(names=COMPARED):
    """The largest difference of the continuous outputs between WAY1 and WAY2 over the named fixtures (depth and X relative to
    max(1, |value|)); the discrete outputs must agree."""
    worst = 0.0
    for nm in names:
        c = case(nm)
        for a, b in zip(c["pose"], c["pose2"]):
            assert a["status"] == b["status"] and a["cand"] == b["cand"] and np.array_equal(a["counts"], b["counts"])
            assert np.array_equal(a["front"], b["front"])
            for k in POSE_KEYS:
                worst = max(worst, float(np.abs(a[k] - b[k]).max()))
            for k in ("depth", "X"):
                if a[k].size:
                    worst = max(worst, float((np.abs(a[k] - b[k]) / np.maximum(1.0, np.abs(b[k]))).max()))
        ra, rb = c["rows"], c["rows2"]
        assert np.array_equal(ra[:, 13:15], rb[:, 13:15])                 # n_shared, flags
        if ra.size:
            worst = max(worst, float(np.abs(ra - rb).max()))
    return worst


# The largest error of the restatement against the truth on the noise-free fixtures (rotation angle, angle of t, in degrees) and
# the largest WAY1 / WAY2 difference over COMPARED, as truth_error(NOISE_FREE) and way_difference(COMPARED) returned them when
# the fixtures were fixed; tests/test_pose_cpu.py repeats the measurements.  The bounds are 16 times these.
TRUTH_ERROR_DEG = 3.7806594530038714e-08     # (the forward-motion fixture; the others stay below 1e-10)
CENTRE_ERROR = 7.567280135845067e-13          # centre_error(): the chained centres of seq3 / seq5 against the true ones
WAY_DIFFERENCE = 7.10441598877202e-13         # (the noisy fixture), measured with numpy.longdouble (80-bit) as WAY2
TRUTH_BOUND_DEG = 16.0 * TRUTH_ERROR_DEG
CENTRE_BOUND = 16.0 * CENTRE_ERROR
TOLERANCE = 16.0 * WAY_DIFFERENCE


def truth_error(names=NOISE_FREE):
    """The largest angle (degrees) between the restatement's R and the true rotation and between its t and the true direction."""
    worst = 0.0
    for nm in names:
        c = case(nm)
        for pose, pr in zip(c["pose"], c["seq"]["pairs"]):
            worst = max(worst, angle_deg(pose["R"], pr["R"]), angle_deg(pose["t"], pr["t"]))
    return worst


def scaled_centres(rows):
    """The centres of trajectory rows with the first one's length as the unit: [frames - 1, 3]."""
    C = np.asarray(rows, dtype=np.float64)[:, 9:12]
    return C / np.linalg.norm(C[0])


def centre_error(names=("seq3", "seq5")):
    """The largest difference between the chained centres and the true ones, both scaled to a first baseline of 1."""
    worst = 0.0
    for nm in names:
        c = case(nm)
        worst = max(worst, float(np.abs(scaled_centres(c["rows"]) - c["seq"]["centres"][1:] / np.linalg.norm(c["seq"]["centres"][1])).max()))
    return worst
