"""numpy restatement of the homography pose and the model selection (csrc/pose_h_kernels.hip.h): the
camera motion a homography implies (a plane seen twice, or a camera that only rotates), the decision between the fundamental
matrix and the homography of a pair, and the fixtures of the tests.  There is no reference counterpart, so this file is the
specification the kernels are tested against.  Everything is fp64 in the parenthesisation written here; every function also runs
in another "way" (pose_ref.WAY2), which is how the tolerance of the continuous outputs is measured (way_difference, TOLERANCE).
The depths of a row come from pose_ref.depths: F frames and H frames share one estimator."""
import functools

import numpy as np

from tests import epipolar_ref as E
from tests import eval_restatement as ER
from tests import pose_ref as P

WAY1, WAY2 = P.WAY1, P.WAY2
MIN_FRONT = P.MIN_FRONT
ROTATION_EPS, NORMAL_MARGIN, MODEL_RATIO = 0.02, 0.01, 0.40      # the defaults of the operators
CHI2_H, CHI2_F = 5.99, 3.84                                      # chi-square 95 % at one pixel: 2 and 1 degrees of freedom
_dot, _cross, _usable = P._dot, P._cross, P._usable


def normalised_h(H, intr, way=WAY1):
    """Hn = K2^-1 H K1 in two stages: [3,3]."""
    dt, _ = way
    H = np.asarray(H, dtype=dt).reshape(9)
    (fx1, fy1, cx1, cy1), (fx2, fy2, cx2, cy2) = np.asarray(intr, dtype=dt).reshape(2, 4)
    B, Hn = np.zeros(9, dtype=dt), np.zeros(9, dtype=dt)
    with np.errstate(all="ignore"):
        for r in range(3):
            B[3 * r] = H[3 * r] * fx1
            B[3 * r + 1] = H[3 * r + 1] * fy1
            B[3 * r + 2] = (H[3 * r] * cx1 + H[3 * r + 1] * cy1) + H[3 * r + 2]
        for c in range(3):
            Hn[c] = (B[c] - cx2 * B[6 + c]) / fx2
            Hn[3 + c] = (B[3 + c] - cy2 * B[6 + c]) / fy2
            Hn[6 + c] = B[6 + c]
    return Hn.reshape(3, 3)


def _apply(M, x, rev):
    """M x for rows x [n,3]: three arrays [n]."""
    return [_dot(M[r], x.T, rev) for r in range(3)]


def spectrum(Hn, way=WAY1):
    """(Hn / sqrt(w2), w1 / w2, w3 / w2, v1, v2, v3) of the signed Hn, or None (status 1): the Jacobi sweeps on Hn^T Hn, the
    eigenvalues in descending order (the lowest index on ties), v3 flipped so that det [v1 v2 v3] = +1; a negative w3 (rounding
    of a singular matrix) counts as 0."""
    dt, rev = way
    with np.errstate(all="ignore"):
        G = np.zeros((3, 3), dtype=dt)
        for i in range(3):
            for j in range(3):
                G[i, j] = _dot(Hn[:, i], Hn[:, j], rev)
        d, V = P.jacobi3(G, dt)
        k0 = 0
        for j in (1, 2):
            if d[j] > d[k0]:
                k0 = j
        rest = [j for j in range(3) if j != k0]
        k1, k2 = (rest[1], rest[0]) if d[rest[1]] > d[rest[0]] else (rest[0], rest[1])
        v1, v2, v3 = V[:, k0].copy(), V[:, k1].copy(), V[:, k2].copy()
        if _dot(_cross(v1, v2), v3, rev) < 0.0:
            v3 = -v3
        w1, w2, w3 = d[k0], d[k1], d[k2]
        if not (np.isfinite(w1) and np.isfinite(w3) and _usable(w2)):
            return None
        s2 = np.sqrt(w2)
        Hs = Hn / s2
        w1, w3 = w1 / w2, w3 / w2
        if not w3 > 0.0:
            w3 = dt(0.0)
        if not (np.all(np.isfinite(Hs)) and np.isfinite(w1)):
            return None
    return Hs, w1, w3, v1, v2, v3


def orthonormal(M, way=WAY1):
    """Row 0 normalised, row 1 made orthogonal to it and normalised, row 2 their cross product."""
    _, rev = way
    with np.errstate(all="ignore"):
        r0 = M[0] / np.sqrt(_dot(M[0], M[0], rev))
        w = M[1] - _dot(M[1], r0, rev) * r0
        r1 = w / np.sqrt(_dot(w, w, rev))
    return np.stack([r0, r1, _cross(r0, r1)])


def plane_candidates(Hs, w1, w3, v1, v2, v3, way=WAY1):
    """The four (R, N, T) of a normalised plane homography, T = t / d not yet of unit length."""
    dt, rev = way
    with np.errstate(all="ignore"):
        p, q, r = np.sqrt(dt(1.0) - w3), np.sqrt(w1 - dt(1.0)), np.sqrt(w1 - w3)
        out = []
        for sg in (1.0, -1.0):
            u = np.array([(p * v1[k] + q * v3[k]) / r if sg > 0 else (p * v1[k] - q * v3[k]) / r for k in range(3)], dtype=dt)
            N = _cross(v2, u)
            hv = np.array([_dot(Hs[k], v2, rev) for k in range(3)], dtype=dt)
            hu = np.array([_dot(Hs[k], u, rev) for k in range(3)], dtype=dt)
            hw = _cross(hv, hu)
            R = np.zeros((3, 3), dtype=dt)
            for a in range(3):
                for b in range(3):
                    R[a, b] = (hv[a] * v2[b] + hu[a] * u[b]) + hw[a] * N[b]
            T = np.array([_dot(Hs[k] - R[k], N, rev) for k in range(3)], dtype=dt)
            out += [(R, N, T), (R, -N, -T)]
    return out


def homography_pose(H, mask, n_inliers, status_in, m, intr, prior=None, rotation_eps=ROTATION_EPS, normal_margin=NORMAL_MARGIN,
                    way=WAY1):
    """The pose of one pair from its homography.  H [9] / [3,3] (view 1 pixels to view 2 pixels), mask [n] over the match rows
    m [n,4], n_inliers and status of the homography RANSAC, intr [2][4], prior [2,3] or None.  Returns dict(R, t, cand, counts,
    n_front, status, front, depth, X as pose_ref.two_view_pose; model 0 / 1 / 2, normal [3], normals2 [2,3]; and for the conditions
    of the fixtures: spread = sqrt(w1) - sqrt(w3), alive [4], prior_scores [4] or None, min_side = the smallest |N . a| that took
    part in a count)."""
    dt, rev = way
    m = np.asarray(m, dtype=np.float64).reshape(-1, 4)
    n = m.shape[0]
    mask = np.asarray(mask).astype(bool).reshape(-1)[:n]
    zero = dt(0.0)
    out = {"R": np.eye(3, dtype=dt), "t": np.zeros(3, dtype=dt), "cand": -1, "counts": np.zeros(4, dtype=np.int64), "n_front": 0,
           "status": 1, "front": np.zeros(n, dtype=bool), "depth": np.zeros((n, 2), dtype=dt), "X": np.zeros((n, 3), dtype=dt),
           "model": 0, "normal": np.zeros(3, dtype=dt), "normals2": np.zeros((2, 3), dtype=dt), "spread": None,
           "alive": np.zeros(4, dtype=bool), "prior_scores": None, "min_side": np.inf}
    if int(status_in) != 0 or int(n_inliers) < MIN_FRONT:
        return out
    Hn = normalised_h(H, intr, way)
    x1, x2 = P.rays(m, intr, way)
    with np.errstate(all="ignore"):
        ha = _apply(Hn, x1, rev)
        pos = int(((_dot([x2[:, 0], x2[:, 1], x2[:, 2]], ha, rev) > 0.0) & mask).sum())
    if 2 * pos < int(n_inliers):
        Hn = -Hn
    sp = spectrum(Hn, way)
    if sp is None:
        return out
    Hs, w1, w3, v1, v2, v3 = sp
    spread = np.sqrt(w1) - np.sqrt(w3)
    out["spread"] = float(spread)
    pri = np.zeros((2, 3), dtype=dt) if prior is None else np.asarray(prior, dtype=dt).reshape(2, 3)
    have = [bool(pri[k, 0] != 0.0 or pri[k, 1] != 0.0 or pri[k, 2] != 0.0) for k in range(2)]
    if spread <= dt(rotation_eps):
        R = orthonormal(Hs, way)
        if not np.all(np.isfinite(R)):
            return out
        n2 = np.zeros((2, 3), dtype=dt)
        for k in range(2):
            if have[k]:
                n2[k] = [_dot(R[r], pri[k], rev) for r in range(3)]
        out.update(R=R, status=0, model=2, normals2=n2)
        return out
    cands = plane_candidates(Hs, w1, w3, v1, v2, v3, way)
    with np.errstate(all="ignore"):
        units = []
        for R, N, T in cands:
            tn = np.sqrt(_dot(T, T, rev))
            units.append(T / tn)
            if not (_usable(tn) and np.all(np.isfinite(R)) and np.all(np.isfinite(N))):
                return out
    res, counts = [], np.zeros(4, dtype=np.int64)
    for c, (R, N, T) in enumerate(cands):
        z1, z2, front = P.depths(R, units[c], x1, x2, way)
        side = _dot(N, x1.T, rev)
        if mask.any():
            out["min_side"] = min(out["min_side"], float(np.abs(side[mask]).min()))
        front = front & mask & (side > 0.0)
        res.append((z1, z2, front))
        counts[c] = int(front.sum())
    alive = np.array([counts[c] >= MIN_FRONT and 2 * counts[c] >= int(n_inliers) for c in range(4)])
    n_alive = int(alive.sum())
    status = 2
    if n_alive == 0:
        win = 0
        for c in (1, 2, 3):
            if counts[c] > counts[win]:
                win = c
    elif n_alive == 1:
        win, status = int(np.nonzero(alive)[0][0]), 0
    else:
        win = -1
        if have[0] or have[1]:
            sc = np.full(4, -np.inf, dtype=dt)
            for c in range(4):
                for k in range(2):
                    if have[k]:
                        sc[c] = max(sc[c], _dot(cands[c][1], pri[k], rev))
            out["prior_scores"] = sc.astype(np.float64)
            best = -1
            for c in range(4):
                if alive[c] and (best < 0 or sc[c] > sc[best]):
                    best = c
            second = -1
            for c in range(4):
                if alive[c] and c != best and (second < 0 or sc[c] > sc[second]):
                    second = c
            if sc[best] - sc[second] >= dt(normal_margin):
                win, status = best, 0
        if win < 0:
            for c in range(4):
                if alive[c] and (win < 0 or cands[c][1][2] > cands[win][1][2]):
                    win = c
    R, N, _ = cands[win]
    z1, z2, front = res[win]
    n2, k = np.zeros((2, 3), dtype=dt), 0
    for c in range(4):
        if alive[c] and k < 2:
            n2[k] = [_dot(cands[c][0][r], cands[c][1], rev) for r in range(3)]
            k += 1
    out.update(R=R, t=units[win], cand=win, counts=counts, n_front=int(counts[win]), status=status, front=front, model=1,
               normal=N, normals2=n2, alive=alive,
               depth=np.stack([np.where(front, z1, zero), np.where(front, z2, zero)], axis=1),
               X=np.where(front[:, None], z1[:, None] * x1, zero))
    return out


def _rho(d2, limit):
    with np.errstate(all="ignore"):
        return np.where(d2 < limit, d2.dtype.type(CHI2_H) - d2, d2.dtype.type(0.0))


def model_scores(F, H, m, way=WAY1):
    """(S_H, S_F) of the match rows m [n,4]: the sums in block_sum's order (WAY1) or ascending in the wide format."""
    dt, rev = way
    m = np.asarray(m, dtype=dt).reshape(-1, 4)
    h = np.asarray(H, dtype=dt).reshape(9)
    f = np.asarray(F, dtype=dt).reshape(9)
    ax, ay, bx, by = (m[:, k] for k in range(4))
    one = np.ones(m.shape[0], dtype=dt)
    with np.errstate(all="ignore"):
        A = np.array([h[4] * h[8] - h[5] * h[7], h[2] * h[7] - h[1] * h[8], h[1] * h[5] - h[2] * h[4],
                      h[5] * h[6] - h[3] * h[8], h[0] * h[8] - h[2] * h[6], h[2] * h[3] - h[0] * h[5],
                      h[3] * h[7] - h[4] * h[6], h[1] * h[6] - h[0] * h[7], h[0] * h[4] - h[1] * h[3]], dtype=dt)
        det = _dot(h[0:3], [A[0], A[3], A[6]], rev)

        def transfer(M, x, y, u0, v0):
            w = _dot(M[6:9], [x, y, one], rev)
            du = _dot(M[0:3], [x, y, one], rev) / w - u0
            dv = _dot(M[3:6], [x, y, one], rev) / w - v0
            return du * du + dv * dv

        th = _rho(transfer(h, ax, ay, bx, by), dt(CHI2_H)) + _rho(transfer(A, bx, by, ax, ay), dt(CHI2_H))
        if not (np.isfinite(det) and det != 0.0):
            th = np.zeros(m.shape[0], dtype=dt)
        l2 = [_dot(f[3 * r:3 * r + 3], [ax, ay, one], rev) for r in range(3)]
        l1 = [_dot([f[c], f[3 + c], f[6 + c]], [bx, by, one], rev) for c in range(3)]
        e = _dot([bx, by, one], l2, rev)
        ee = e * e
        tf = _rho(ee / (l2[0] * l2[0] + l2[1] * l2[1]), dt(CHI2_F)) + _rho(ee / (l1[0] * l1[0] + l1[1] * l1[1]), dt(CHI2_F))
    if dt is np.float64 and not rev:
        idx = np.arange(m.shape[0])
        return float(E.block_sum(th, idx)), float(E.block_sum(tf, idx))
    sh, sf = dt(0.0), dt(0.0)
    for k in range(m.shape[0]):
        sh, sf = sh + th[k], sf + tf[k]
    return sh, sf


def model_select(F, f_status, H, h_status, m, model_ratio=MODEL_RATIO, way=WAY1):
    """dict(scores [2] = (S_H, S_F), use_h, ratio = S_H / (S_H + S_F) or None)."""
    dt, _ = way
    sh, sf = model_scores(F, H, m, way)
    use_h = int(h_status) == 0 and (int(f_status) != 0 or bool(sh >= dt(model_ratio) * (sh + sf)))
    return {"scores": np.array([sh, sf], dtype=dt), "use_h": int(use_h), "ratio": float(sh / (sh + sf)) if sh + sf > 0 else None}


# ---- synthetic sequences: pose_ref.make_sequence with the points on a plane and steps that may only rotate -------------------
PLANE_N0 = np.array([0.15, -0.25, 1.0]) / np.linalg.norm([0.15, -0.25, 1.0])      # the plane N0 . X = PLANE_D0 in camera 0's frame
PLANE_D0 = 6.0
MOTIONS = dict(P.MOTIONS, up=((6.0, 1.0, 2.0), (0.2, -1.0, 0.3)))                   # "up": another direction, another second pose
ROTATE_DEG = (2.0, -6.0, 1.5)                                                      # the step "rotate": no translation


def make_sequence(seed, steps, n_in, n_out, noise=0.0, zoom=True, planar=True, base=1.0):
    """len(steps) + 1 views; steps: names of pose_ref.MOTIONS or "rotate".  The layout of pose_ref.make_sequence's result, and per
    pair also H (the true homography, H[2,2] = 1; planar scenes and rotations), N and d (the plane in the first camera's frame)
    and t = 0, length = 0 for a rotation.  base scales the baselines.  Stray matches lie E.MARGIN px from the transferred point
    and, where there is a baseline, from both epipolar lines."""
    rng = np.random.RandomState(seed)
    frames = len(steps) + 1
    Rf, tf, moves = [np.eye(3)], [np.zeros(3)], []
    for name in steps:
        if name == "rotate":
            Rs, ts = P._rodrigues(np.asarray(ROTATE_DEG) * (0.8 + 0.4 * rng.rand())), np.zeros(3)
        else:
            rot, direction = MOTIONS[name]
            Rs = P._rodrigues(np.asarray(rot) * (0.8 + 0.4 * rng.rand()))
            ts = np.asarray(direction) / np.linalg.norm(direction) * (0.3 + 0.25 * rng.rand()) * base
        moves.append((Rs, ts))
        Rf.append(Rs @ Rf[-1])
        tf.append(Rs @ tf[-1] + ts)
    intr = np.stack([P.intrinsics_of(f, zoom) for f in range(frames)])
    N = n_in + n_out
    X0 = np.zeros((0, 3))
    for _ in range(64):                 # (a scene whose points cannot stay visible is an error, not a loop)
        if X0.shape[0] >= n_in:
            break
        a = np.stack([rng.uniform(8, E.WIDTH - 8, 4 * n_in + 8), rng.uniform(8, E.HEIGHT - 8, 4 * n_in + 8)], axis=1)
        ray = np.stack([(a[:, 0] - intr[0, 2]) / intr[0, 0], (a[:, 1] - intr[0, 3]) / intr[0, 1], np.ones(a.shape[0])], axis=1)
        z = PLANE_D0 / (ray @ PLANE_N0) if planar else rng.uniform(3.0, 12.0, a.shape[0])
        X = ray * z[:, None]
        ok = z > 1.0
        for f in range(frames):
            Y = X @ Rf[f].T + tf[f]
            b = P._project(Y, intr[f])
            ok &= (Y[:, 2] > 1.0) & (b[:, 0] > 4) & (b[:, 0] < E.WIDTH - 4) & (b[:, 1] > 4) & (b[:, 1] < E.HEIGHT - 4)
        X0 = np.concatenate([X0, X[ok]])
    assert X0.shape[0] >= n_in, "the points do not stay visible under these steps"
    X0 = X0[:n_in]
    by_id, pairs = [], []
    for f in range(frames):
        px = P._project(X0 @ Rf[f].T + tf[f], intr[f])
        if noise > 0.0:
            px = px + noise * rng.randn(n_in, 2)
        stray = np.stack([rng.uniform(8, E.WIDTH - 8, n_out), rng.uniform(8, E.HEIGHT - 8, n_out)], axis=1)
        if f > 0:
            Rs, ts = moves[f - 1]
            K1i, K2 = np.linalg.inv(P.k_matrix(intr[f - 1])), P.k_matrix(intr[f])
            Np = Rf[f - 1] @ PLANE_N0
            dp = PLANE_D0 + Np @ tf[f - 1]
            length = float(np.linalg.norm(ts))
            H = F = None
            if planar or length == 0.0:
                H = K2 @ (Rs + np.outer(ts, Np) / dp) @ K1i
                H = H / H[2, 2]
            if length > 0.0:
                tx = np.array([[0.0, -ts[2], ts[1]], [ts[2], 0.0, -ts[0]], [-ts[1], ts[0], 0.0]])
                F = np.linalg.inv(K2).T @ tx @ Rs @ K1i
            a = by_id[f - 1][n_in:]
            for k in range(n_out):
                while True:
                    b = np.stack([rng.uniform(8, E.WIDTH - 8, 32), rng.uniform(8, E.HEIGHT - 8, 32)], axis=1)
                    good = np.ones(32, dtype=bool)
                    if F is not None:
                        d1, d2 = E.line_dist(F, np.repeat(a[k:k + 1], 32, axis=0), b)
                        good &= (d1 >= E.MARGIN) & (d2 >= E.MARGIN)
                    if H is not None:
                        q = H @ np.array([a[k, 0], a[k, 1], 1.0])
                        good &= np.linalg.norm(b - q[:2] / q[2], axis=1) >= E.MARGIN
                    if good.any():
                        stray[k] = b[np.nonzero(good)[0][0]]
                        break
            pairs.append({"R": Rs, "t": ts / length if length > 0.0 else np.zeros(3), "length": length, "F": F, "H": H,
                          "N": Np, "d": float(dp), "intr": np.stack([intr[f - 1], intr[f]])})
        by_id.append(np.concatenate([px, stray]))
    ids = [rng.permutation(N) for _ in range(frames)]
    pts = [np.ascontiguousarray(by_id[f][ids[f]]) for f in range(frames)]
    for f in range(1, frames):
        row_cur = np.argsort(ids[f])
        order = ids[f - 1]
        match = np.zeros((N, 3), dtype=np.float32)
        match[:, 0] = np.arange(N)
        match[:, 1] = row_cur[order]
        match[:, 2] = rng.rand(N).astype(np.float32)
        pairs[f - 1].update(match=match, truth=order < n_in,
                            m=np.concatenate([pts[f - 1], pts[f][row_cur[order]]], axis=1).astype(np.float64))
    centres = np.stack([-(Rf[f].T @ tf[f]) for f in range(frames)])
    return {"pts": pts, "ids": ids, "intr": intr, "centres": centres, "pairs": pairs, "n_in": n_in, "Rf": Rf}


# ---- fixtures ------------------------------------------------------------------------------------------------------------
# Scenes: name -> (seed, steps, inliers, outliers, noise px, zoom, planar, baseline scale).
SCENES = {
    "plane48": (40, ("side",), 32, 16, 0.0, True, True, 1.0),
    "plane48b": (41, ("backward",), 32, 16, 0.0, True, True, 1.0),
    "plane_k": (42, ("side",), 40, 8, 0.0, False, True, 1.0),
    "empty": (43, ("side",), 0, 0, 0.0, True, True, 1.0),
    "three": (44, ("side",), 3, 0, 0.0, True, True, 1.0),
    "seven": (45, ("side",), 7, 0, 0.0, True, True, 1.0),
    "eight": (101, ("side",), 8, 0, 0.0, True, True, 1.0),
    "eleven": (116, ("side",), 11, 0, 0.0, True, True, 1.0),         # one candidate alive: counts (7, 4, 0, 11)
    "n257": (47, ("side",), 200, 57, 0.0, True, True, 1.0),
    "n4096": (48, ("side",), 3000, 1096, 0.0, True, True, 1.0),
    "noisy": (49, ("side",), 150, 100, 0.3, True, True, 1.0),
    "rotate": (50, ("rotate",), 40, 8, 0.0, True, False, 1.0),
    "small": (51, ("side",), 40, 8, 0.0, True, True, 0.05),           # a baseline near the rotation threshold
    "solid": (52, ("side",), 32, 16, 0.0, True, False, 1.0),         # not planar: the fundamental matrix wins
    "planar5": (53, ("side", "up", "side", "up"), 40, 8, 0.0, False, True, 1.0),    # the trackers' planar sequence, one camera
    "srs": (54, ("side", "rotate", "side"), 40, 8, 0.0, False, False, 1.0),      # side - rotate in place - side, one camera
}


@functools.lru_cache(maxsize=None)
def scene(name):
    seed, steps, n_in, n_out, noise, zoom, planar, base = SCENES[name]
    return make_sequence(seed, steps, n_in, n_out, noise=noise, zoom=zoom, planar=planar, base=base)


def _truth_inputs(pr):
    """The inputs of both operators for a pair whose models are the scene's own: H and F of the truth, the true rows as both masks."""
    n = pr["m"].shape[0]
    mask = pr["truth"].copy() if n else np.zeros(0, dtype=bool)
    return {"H": pr["H"] if pr["H"] is not None else np.eye(3), "h_mask": mask, "h_n": int(mask.sum()), "h_status": 0,
            "F": pr["F"] if pr["F"] is not None else np.zeros((3, 3)), "f_mask": mask.copy(), "f_n": int(mask.sum()),
            "f_status": 0 if pr["F"] is not None else 1}


# Cases: name -> (scene, pair, changes).  A change names an input and what to do with it.
CASES = {
    "plane48": ("plane48", 0, {}),
    "plane48b": ("plane48b", 0, {}),
    "plane_k": ("plane_k", 0, {}),
    "empty": ("empty", 0, {}),
    "three": ("three", 0, {}),
    "seven": ("seven", 0, {}),
    "eight": ("eight", 0, {}),
    "one_alive": ("eleven", 0, {}),
    "n257": ("n257", 0, {}),
    "n4096": ("n4096", 0, {}),
    "noisy": ("noisy", 0, {}),
    "negative": ("plane48", 0, {"negate_h": True}),
    "no_model": ("plane48", 0, {"h_status": 1}),
    "salted": ("plane48", 0, {"salt": 6}),
    "prior_true": ("plane48", 0, {"prior": "true"}),
    "prior_other": ("plane48", 0, {"prior": "other"}),
    "prior_tie": ("plane48", 0, {"prior": "tie"}),
    "rotate": ("rotate", 0, {}),
    "rotate_prior": ("rotate", 0, {"prior": "fixed"}),
    "small_in": ("small", 0, {"eps_factor": 1.0 / 0.7}),       # rotation_eps = spread / 0.7: inside
    "small_out": ("small", 0, {"eps_factor": 1.0 / 1.5}),      # rotation_eps = spread / 1.5: outside
    "singular": ("plane48", 0, {"singular_h": True}),
    "no_f": ("plane48", 0, {"f_status": 1}),
    "solid": ("solid", 0, {"fit_h": 300}),
}
POSE_COMPARED = tuple(CASES)
FOUR = ("plane48", "eight", "seven", "empty")          # n_match = (48, 8, 7, 0): one call, shared intrinsics
FOUR_K = ("plane48", "plane_k", "three", "rotate")     # ... with a pair of other intrinsics and a rotation among them


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(m, match, intr, H, h_mask, h_n, h_status, F, f_mask, f_n, f_status, prior, rotation_eps, pair = the scene's pair,
    pose / pose2 = homography_pose in both ways, select / select2 = model_select in both ways); read-only."""
    sc, k, ch = CASES[name]
    pr = scene(sc)["pairs"][k]
    c = dict(_truth_inputs(pr), m=pr["m"], match=pr["match"], intr=pr["intr"], pair=pr, prior=None, rotation_eps=ROTATION_EPS)
    if "fit_h" in ch:                                   # a homography fitted to points that do not lie on a plane
        r = ER.ransac(pr["m"], ch["fit_h"])
        c.update(H=r["H"], h_mask=r["mask"], h_n=int(r["mask"].sum()), h_status=r["status"])
    if ch.get("negate_h"):
        c["H"] = -c["H"]
    if ch.get("singular_h"):
        H = c["H"].copy()
        H[1] = H[0]
        c["H"] = H
    for key in ("h_status", "f_status"):
        if key in ch:
            c[key] = ch[key]
    if "salt" in ch:                                    # the first stray rows enter the mask
        mask = c["h_mask"].copy()
        mask[np.nonzero(~pr["truth"])[0][:ch["salt"]]] = True
        c.update(h_mask=mask, h_n=int(mask.sum()))
    free = homography_pose(c["H"], c["h_mask"], c["h_n"], c["h_status"], c["m"], c["intr"])
    if "eps_factor" in ch:
        c["rotation_eps"] = free["spread"] * ch["eps_factor"]
    if "prior" in ch:
        if ch["prior"] == "fixed":
            c["prior"] = np.array([[0.0, 0.6, 0.8], [0.0, 0.0, 0.0]])
        else:
            assert int(free["alive"].sum()) == 2, name
            a, b = (plane_candidates(*spectrum(_signed(c), WAY1))[i][1] for i in np.nonzero(free["alive"])[0])
            true_first = np.linalg.norm(a - pr["N"]) < np.linalg.norm(b - pr["N"])
            good, other = (a, b) if true_first else (b, a)
            if ch["prior"] == "true":
                c["prior"] = np.stack([good, np.zeros(3)])
            elif ch["prior"] == "other":
                c["prior"] = np.stack([np.zeros(3), other])
            else:
                c["prior"] = np.stack([(a + b) / np.linalg.norm(a + b), np.zeros(3)])
    for key, way in (("pose", WAY1), ("pose2", WAY2)):
        c[key] = homography_pose(c["H"], c["h_mask"], c["h_n"], c["h_status"], c["m"], c["intr"], c["prior"], c["rotation_eps"],
                                 NORMAL_MARGIN, way)
    for key, way in (("select", WAY1), ("select2", WAY2)):
        c[key] = model_select(c["F"], c["f_status"], c["H"], c["h_status"], c["m"], MODEL_RATIO, way)
    return c


def _signed(c):
    """The Hn of a case with the sign rule applied (float64)."""
    Hn = normalised_h(c["H"], c["intr"])
    x1, x2 = P.rays(c["m"], c["intr"])
    s = _dot([x2[:, 0], x2[:, 1], x2[:, 2]], _apply(Hn, x1, False))
    return -Hn if 2 * int(((s > 0.0) & c["h_mask"]).sum()) < c["h_n"] else Hn


CONT_KEYS = ("R", "t", "normal", "normals2")


def way_difference(names=POSE_COMPARED):
    """The largest difference of the continuous outputs between WAY1 and WAY2 over the named cases (depth, X and the scores
    relative to max(1, |value|)); the discrete outputs must agree."""
    worst = 0.0
    for nm in names:
        c = case(nm)
        a, b = c["pose"], c["pose2"]
        for k in ("status", "cand", "model", "n_front"):
            assert a[k] == b[k], (nm, k)
        assert np.array_equal(a["counts"], b["counts"]) and np.array_equal(a["front"], b["front"]), nm
        for k in CONT_KEYS:
            worst = max(worst, float(np.abs(a[k] - b[k]).max()))
        for k in ("depth", "X"):
            if a[k].size:
                worst = max(worst, float((np.abs(a[k] - b[k]) / np.maximum(1.0, np.abs(b[k]))).max()))
        sa, sb = c["select"], c["select2"]
        assert sa["use_h"] == sb["use_h"], nm
        worst = max(worst, float((np.abs(sa["scores"] - sb["scores"]) / np.maximum(1.0, np.abs(sb["scores"]))).max()))
    return worst


def truth_error(names=("one_alive", "prior_true", "rotate")):
    """The largest error of the restatement on noise-free cases whose status is 0: (angle of R, angle of t, angle of the normal)
    in degrees."""
    worst = [0.0, 0.0, 0.0]
    for nm in names:
        c = case(nm)
        pose, pr = c["pose"], c["pair"]
        assert pose["status"] == 0, nm
        worst[0] = max(worst[0], P.angle_deg(pose["R"], pr["R"]))
        if pose["model"] == 1:
            worst[1] = max(worst[1], P.angle_deg(pose["t"], pr["t"]))
            worst[2] = max(worst[2], P.angle_deg(pose["normal"], pr["N"]))
    return tuple(worst)


# ---- the sequences of the tracker tests, through the restatements --------------------------------------------------------
SEQ_SEED = 400        # the check seed of the first pair of "planar5" and "srs"; pair k uses SEQ_SEED + k


def auto_frame(m, intr, seed, prior, h_key="H"):
    """One frame of geometric_check="auto" in numpy: both RANSACs, the F pose, the selection, the H pose over it.  Returns
    dict(pose = the pose that enters the chain, model, select, f = epipolar_ref.ransac, h = eval_restatement.ransac)."""
    f, h = E.ransac(m, seed), ER.ransac(m, seed)
    pose = P.two_view_pose(f["F"], f["mask"], f["n_inliers"], f["status"], m, intr)
    Hm = h[h_key] if h["status"] == 0 else h["H"]
    sel = model_select(f["F"], f["status"], Hm, h["status"], m)
    model = 0
    if sel["use_h"]:
        pose = homography_pose(Hm, h["mask"], int(h["mask"].sum()), h["status"], m, intr, prior)
        model = pose["model"]
    return {"pose": pose, "model": model, "select": sel, "f": f, "h": h}


@functools.lru_cache(maxsize=None)
def auto_sequence(name, h_key="H"):
    """A scene through auto_frame and pose_ref.run_chain: dict(frames: per pair auto_frame's dict, rows [pairs, ROW_WORDS]).
    h_key "H_lanes": the homography refitted with its sums in the device's order (eval_restatement.ransac)."""
    seq = scene(name)
    frames, prior = [], None
    for k, pr in enumerate(seq["pairs"]):
        fr = auto_frame(pr["m"], pr["intr"], SEQ_SEED + k, prior, h_key)
        prior = fr["pose"]["normals2"] if fr["model"] else None
        frames.append(fr)
    rows, _ = P.run_chain([fr["pose"] for fr in frames], [pr["match"] for pr in seq["pairs"]])
    return {"frames": frames, "rows": rows}


def planar_truth():
    """The true centres of frames 2 .. 4 of "planar5" in the frame of camera 1, the first baseline after it as the unit: the first
    planar pair has no prior and stays ambiguous (status 2: no pose, the centre repeats), so the trajectory starts at frame 1."""
    seq = scene("planar5")
    C = np.stack([seq["Rf"][1] @ (seq["centres"][f] - seq["centres"][1]) for f in (2, 3, 4)])
    return C / np.linalg.norm(C[0])


def planar_centres(rows):
    """The same from trajectory rows [4, ROW_WORDS] of the sequence (row k: pair k)."""
    C = np.asarray(rows, dtype=np.float64)[1:4, 9:12]
    return C / np.linalg.norm(C[0])


def planar_centre_error():
    """The largest difference between planar_centres of the restatement's chain and planar_truth, over the two refits of the
    homography."""
    return max(float(np.abs(planar_centres(auto_sequence("planar5", k)["rows"]) - planar_truth()).max()) for k in ("H", "H_lanes"))


# What the measurements returned when the fixtures were fixed; tests/test_pose_h_cpu.py repeats them.  The bounds are 16 times these.
WAY_DIFFERENCE = 5.966249991814023e-10        # ("prior_other": the depths under the pose a wrong prior selects), numpy.longdouble (80-bit) as WAY2
TRUTH_ERROR_DEG = (4.5137690904840274e-14, 8.443668854897707e-13, 2.5000252329381497e-13)      # R, t, normal
TRUTH_BOUND_DEG = 16.0 * max(TRUTH_ERROR_DEG)
TOLERANCE = 16.0 * WAY_DIFFERENCE
PLANAR_CENTRE_ERROR = 2.0650148258027912e-14      # planar_centre_error(): the chained centres of "planar5" against the true ones
PLANAR_CENTRE_BOUND = 16.0 * PLANAR_CENTRE_ERROR
