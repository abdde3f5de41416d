"""numpy restatement of the landmark kernels (csrc/landmark_kernels.hip.h): the cameras of the retained
frames inside the newest consistent window (`map_window`), the N-view triangulation of every track row (`triangulate`: unit rays,
parallax, midpoint, four Gauss-Newton steps on the pixel reprojection error, cheirality, rms) and the stable selection of the
accepted rows (`select`).  There is no reference counterpart and no OpenCV here, so this file is the specification the kernels
are tested against.  Everything is fp64 in the parenthesisation written here, vectorised over the rows (the loop over the views is
the kernel's); every function also runs in another "way" (pose_ref.WAY2: numpy.longdouble where that is wider than float64, else
the dot products and the sums over the views in the reverse order), which is how the tolerance of the continuous outputs is
measured (`way_difference`).  Also the fixtures: pose_ref.make_sequence's scenes with their true cameras, a slow-moving 16-frame
scene of its own, and the track tables tracks_ref builds from their matches."""
import functools
import math

import numpy as np

from tests import epipolar_ref as E
from tests import pose_ref as P
from tests import tracks_ref as T

CAM_WORDS = 20         # Rw [9], C [3], fx, fy, cx, cy, valid, 3 spare
LANDMARK_WORDS = 8     # track id, X, Y, Z, n_views, rms, cos_parallax, index of the point in the newest frame or -1
GN_STEPS = 4
DET_EPS = 1e-12
OK, FEW_VIEWS, DEGENERATE, BEHIND, REPROJ = 0, 1, 2, 3, 4
WAY1, WAY2 = P.WAY1, P.WAY2
MIN_VIEWS, MIN_PARALLAX_DEG, MAX_REPROJ = 2, 1.0, 2.0      # the defaults of the public interface


def cos_of(deg):
    """What the host passes for min_parallax_deg."""
    return math.cos(math.radians(float(deg)))


def _dot(p, q, rev=False):
    return P._dot(p, q, rev)


# ---- map_window ----------------------------------------------------------------------------------------------------------------
def window_start(flags, n, L, capacity):
    """The start w of the newest consistent window of n frames, walked down no further than the oldest retained frame.  flags: the
    flag word of every table row; a row the table does not hold carries both bits."""
    def flag(f):
        return int(flags[f]) if 0 <= f < capacity else 3
    w = n - 1
    while w > max(n - L, 0):
        if (flag(w) & 1) or (w + 1 <= n - 1 and (flag(w + 1) & 2)):
            break
        w -= 1
    return w


def map_window(n_frames, table, intr, L, way=WAY1):
    """cams [L, CAM_WORDS] of the L retained frames.  table [capacity, pose_ref.ROW_WORDS], intr [1, 4] or [L, 4]."""
    dt, _ = way
    table = np.asarray(table, dtype=dt).reshape(-1, P.ROW_WORDS)
    intr = np.asarray(intr, dtype=dt).reshape(-1, 4)
    capacity, n = table.shape[0], int(n_frames)
    w = window_start(table[:, 14], n, L, capacity)
    cams = np.zeros((L, CAM_WORDS), dtype=dt)
    for c in range(L):
        f = n - L + c
        k = intr[0 if intr.shape[0] == 1 else c]
        if 0 <= f < capacity and f >= w and np.isfinite(k[0]) and np.isfinite(k[1]) and k[0] > 0.0 and k[1] > 0.0:
            cams[c, :12], cams[c, 12:16], cams[c, 16] = table[f, :12], k, 1.0
    return cams


# ---- triangulate ---------------------------------------------------------------------------------------------------------------
def _solve3(a, b, dt, rev):
    """x = A^-1 b of symmetric 3x3 systems by cofactors.  a = (a00, a01, a02, a11, a12, a22), b = (b0, b1, b2), arrays over the
    rows.  Returns (x [3], ok)."""
    a00, a01, a02, a11, a12, a22 = a
    with np.errstate(all="ignore"):
        c00, c01, c02 = a11 * a22 - a12 * a12, a02 * a12 - a01 * a22, a01 * a12 - a02 * a11
        c11, c12, c22 = a00 * a22 - a02 * a02, a01 * a02 - a00 * a12, a00 * a11 - a01 * a01
        det = _dot((a00, a01, a02), (c00, c01, c02), rev)
        x = [_dot((c00, c01, c02), b, rev) / det, _dot((c01, c11, c12), b, rev) / det, _dot((c02, c12, c22), b, rev) / det]
        ok = np.isfinite(det) & (det > dt(DET_EPS) * ((a00 * a11) * a22)) & np.isfinite(x[0]) & np.isfinite(x[1]) & np.isfinite(x[2])
    return x, ok


def _view(cam, X, px, rev):
    """y2, u, v, r0, r1 of the points X [3] (arrays over the rows) in camera record cam against the pixels px [., 2]."""
    q = (X[0] - cam[9], X[1] - cam[10], X[2] - cam[11])
    y0, y1, y2 = _dot(cam[0:3], q, rev), _dot(cam[3:6], q, rev), _dot(cam[6:9], q, rev)
    u, v = y0 / y2, y1 / y2
    return y2, u, v, (cam[12] * u + cam[14]) - px[:, 0], (cam[13] * v + cam[15]) - px[:, 1]


def triangulate(ids, counts, pts, first_slot, cams, min_views=MIN_VIEWS, cos_min_parallax=None, max_reproj=MAX_REPROJ, way=WAY1):
    """ids [n_rows, L] of a track table, counts [L] of its retained frames, pts [L, point_cap, 2] the ring (retained frame c in slot
    (first_slot + c) % L), cams [L, CAM_WORDS].  Returns dict(X [n_rows, 3], n_views, rms, cos_parallax, status, last_step: the
    length of the fourth Gauss-Newton step)."""
    dt, rev = way
    if cos_min_parallax is None:
        cos_min_parallax = cos_of(MIN_PARALLAX_DEG)
    ids = np.asarray(ids, dtype=np.int64)
    n_rows, L = ids.shape
    pts = np.asarray(pts, dtype=dt)
    point_cap = pts.shape[1]
    cams = np.asarray(cams, dtype=dt)
    counts = [min(max(int(v), 0), point_cap) for v in counts]
    first = [sum(counts[:c]) for c in range(L)]
    order = range(L - 1, -1, -1) if rev else range(L)
    zero = np.zeros(n_rows, dtype=dt)
    used, pix = [], []
    for c in range(L):
        p = ids[:, c] - first[c]
        u = (ids[:, c] >= 0) & (cams[c, 16] != 0.0) & (p >= 0) & (p < counts[c])
        used.append(u)
        pix.append(pts[(first_slot + c) % L][np.where(u, p, 0)])
    n_views = np.sum(used, axis=0).astype(np.int64) if L else np.zeros(n_rows, dtype=np.int64)
    with np.errstate(all="ignore"):
        # the rays and the midpoint system
        rays = [None] * L
        a = [zero.copy() for _ in range(6)]
        b = [zero.copy() for _ in range(3)]
        for c in order:
            cam, u = cams[c], used[c]
            x0, x1 = (pix[c][:, 0] - cam[14]) / cam[12], (pix[c][:, 1] - cam[15]) / cam[13]
            one = np.ones(n_rows, dtype=dt)
            e = [_dot((cam[k], cam[3 + k], cam[6 + k]), (x0, x1, one), rev) for k in range(3)]
            nrm = np.sqrt(_dot(e, e, rev))
            d = [e[0] / nrm, e[1] / nrm, e[2] / nrm]
            rays[c] = d
            m00, m11, m22 = 1.0 - d[0] * d[0], 1.0 - d[1] * d[1], 1.0 - d[2] * d[2]
            m01, m02, m12 = 0.0 - d[0] * d[1], 0.0 - d[0] * d[2], 0.0 - d[1] * d[2]
            C = (cam[9], cam[10], cam[11])
            for k, term in enumerate((m00, m01, m02, m11, m12, m22)):
                a[k] = np.where(u, a[k] + term, a[k])
            for k, row in enumerate(((m00, m01, m02), (m01, m11, m12), (m02, m12, m22))):
                b[k] = np.where(u, b[k] + _dot(row, C, rev), b[k])
        # parallax
        cosp = np.full(n_rows, np.inf, dtype=dt)
        for i in range(L):
            for j in range(i + 1, L):
                v = _dot(rays[i], rays[j], rev)
                cosp = np.where(used[i] & used[j] & (v < cosp), v, cosp)
        degenerate = cosp > dt(cos_min_parallax)
        X, ok = _solve3(a, b, dt, rev)
        degenerate |= ~ok
        behind = np.zeros(n_rows, dtype=bool)
        for c in range(L):
            cam = cams[c]
            z = _dot(cam[6:9], (X[0] - cam[9], X[1] - cam[10], X[2] - cam[11]), rev)
            behind |= used[c] & ~(np.isfinite(z) & (z > 0.0))
        # Gauss-Newton
        step_len = zero.copy()
        for _ in range(GN_STEPS):
            h = [zero.copy() for _ in range(6)]
            g = [zero.copy() for _ in range(3)]
            for c in order:
                cam, u = cams[c], used[c]
                y2, uu, vv, r0, r1 = _view(cam, X, pix[c], rev)
                fa, fb = cam[12] / y2, cam[13] / y2
                j0 = [fa * (cam[k] - uu * cam[6 + k]) for k in range(3)]
                j1 = [fb * (cam[3 + k] - vv * cam[6 + k]) for k in range(3)]
                for k, (p, q) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
                    h[k] = np.where(u, h[k] + (j0[p] * j0[q] + j1[p] * j1[q]), h[k])
                for k in range(3):
                    g[k] = np.where(u, g[k] + (j0[k] * r0 + j1[k] * r1), g[k])
            s, ok = _solve3(h, g, dt, rev)
            degenerate |= ~ok
            X = [X[0] - s[0], X[1] - s[1], X[2] - s[2]]
            step_len = np.sqrt(_dot(s, s, rev))
        # residuals and cheirality of the result
        ss = zero.copy()
        for c in order:
            y2, _, _, r0, r1 = _view(cams[c], X, pix[c], rev)
            behind |= used[c] & ~(np.isfinite(y2) & (y2 > 0.0))
            ss = np.where(used[c], ss + (r0 * r0 + r1 * r1), ss)
        rms = np.sqrt(ss / (2.0 * n_views.astype(dt)))
        few = n_views < int(min_views)
        status = np.where(few, FEW_VIEWS, np.where(degenerate, DEGENERATE, np.where(behind, BEHIND,
                          np.where(rms > dt(max_reproj), REPROJ, OK)))).astype(np.int64)
        x_ok = np.isfinite(X[0]) & np.isfinite(X[1]) & np.isfinite(X[2]) & ~few
        Xo = np.stack([np.where(x_ok, X[k], zero) for k in range(3)], axis=1) if n_rows else np.zeros((0, 3), dtype=dt)
        return {"X": Xo, "n_views": n_views, "rms": np.where(np.isfinite(rms) & ~few, rms, zero),
                "cos_parallax": np.where(np.isfinite(cosp) & ~few, cosp, zero), "status": status,
                "last_step": np.where(few, zero, step_len)}


ROW_KEYS = ("X", "n_views", "rms", "cos_parallax", "status")


def select(ids, tid, counts, point_cap, rows):
    """The status-0 rows in table order: [M, LANDMARK_WORDS]."""
    ids = np.asarray(ids, dtype=np.int64)
    L = ids.shape[1]
    counts = [min(max(int(v), 0), point_cap) for v in counts]
    first = sum(counts[:L - 1])
    keep = np.flatnonzero(rows["status"] == OK)
    p = ids[keep, L - 1] - first
    newest = np.where((ids[keep, L - 1] >= 0) & (p >= 0) & (p < counts[L - 1]), p, -1)
    dt = rows["X"].dtype
    return np.concatenate([np.asarray(tid)[keep, None].astype(dt), rows["X"][keep], rows["n_views"][keep, None].astype(dt),
                           rows["rms"][keep, None], rows["cos_parallax"][keep, None], newest[:, None].astype(dt)], axis=1)


# ---- an independent way: plain numpy midpoint + Gauss-Newton (numpy.linalg.solve, matrix products) -----------------------------
def plain_triangulate(obs):
    """obs: list of (Rw [3,3], C [3], (fx, fy, cx, cy), pixel [2]).  Returns (X, rms px, last step, parallax degrees, min depth)."""
    A, b, rays = np.zeros((3, 3)), np.zeros(3), []
    for Rw, C, k, px in obs:
        d = Rw.T @ np.array([(px[0] - k[2]) / k[0], (px[1] - k[3]) / k[1], 1.0])
        d /= np.linalg.norm(d)
        rays.append(d)
        M = np.eye(3) - np.outer(d, d)
        A += M
        b += M @ C
    X = np.linalg.solve(A, b)
    cosp = min(float(rays[i] @ rays[j]) for i in range(len(rays)) for j in range(i + 1, len(rays)))
    step = np.zeros(3)
    for _ in range(GN_STEPS):
        J, r = [], []
        for Rw, C, k, px in obs:
            y = Rw @ (X - C)
            r += [k[0] * y[0] / y[2] + k[2] - px[0], k[1] * y[1] / y[2] + k[3] - px[1]]
            J += [k[0] / y[2] * (Rw[0] - y[0] / y[2] * Rw[2]), k[1] / y[2] * (Rw[1] - y[1] / y[2] * Rw[2])]
        J, r = np.array(J), np.array(r)
        step = np.linalg.solve(J.T @ J, J.T @ r)
        X = X - step
    r, zmin = [], np.inf
    for Rw, C, k, px in obs:
        y = Rw @ (X - C)
        r += [k[0] * y[0] / y[2] + k[2] - px[0], k[1] * y[1] / y[2] + k[3] - px[1]]
        zmin = min(zmin, y[2])
    return (X, float(np.sqrt(np.sum(np.square(r)) / len(r))), float(np.linalg.norm(step)),
            float(np.degrees(np.arccos(min(1.0, cosp)))), float(zmin))


# ---- scenes --------------------------------------------------------------------------------------------------------------------
def true_poses(seq):
    """(Rw [frames,3,3], C [frames,3]) by chaining each pair's R and t * length; world = camera 0."""
    Rw, tw = [np.eye(3)], [np.zeros(3)]
    for pr in seq["pairs"]:
        Rw.append(pr["R"] @ Rw[-1])
        tw.append(pr["R"] @ tw[-1] + pr["t"] * pr["length"])
    return np.stack(Rw), np.stack([-(R.T @ t) for R, t in zip(Rw, tw)])


def scene_points(scene_seed, frames, n_in, motion, zoom):
    """The fixed points X0 [n_in, 3] of pose_ref.make_sequence(scene_seed, frames, n_in, ...): its random draws replayed (the
    steps' two draws per frame, then the candidate loop).  Fixture builders check the replay by projecting the result."""
    rng = np.random.RandomState(scene_seed)
    rot, direction = P.MOTIONS[motion]
    direction = np.asarray(direction) / np.linalg.norm(direction)
    Rf, tf = [np.eye(3)], [np.zeros(3)]
    for f in range(1, frames):
        Rs = P._rodrigues(np.asarray(rot) * (0.8 + 0.4 * rng.rand()))
        ts = direction * (0.3 + 0.25 * rng.rand())
        Rf.append(Rs @ Rf[-1])
        tf.append(Rs @ tf[-1] + ts)
    intr = np.stack([P.intrinsics_of(f, zoom) for f in range(frames)])
    X0 = np.zeros((0, 3))
    while X0.shape[0] < n_in:
        a = np.stack([rng.uniform(8, E.WIDTH - 8, 4 * n_in + 8), rng.uniform(8, E.HEIGHT - 8, 4 * n_in + 8)], axis=1)
        z = rng.uniform(3.0, 12.0, a.shape[0])
        X = np.stack([(a[:, 0] - intr[0, 2]) * z / intr[0, 0], (a[:, 1] - intr[0, 3]) * z / intr[0, 1], z], axis=1)
        ok = np.ones(X.shape[0], dtype=bool)
        for f in range(frames):
            Y = X @ Rf[f].T + tf[f]
            b = P._project(Y, intr[f])
            ok &= (Y[:, 2] > 1.0) & (b[:, 0] > 4) & (b[:, 0] < E.WIDTH - 4) & (b[:, 1] > 4) & (b[:, 1] < E.HEIGHT - 4)
        X0 = np.concatenate([X0, X[ok]])
    return X0[:n_in]


def make_slow_sequence(seed, frames, n_in, n_out, noise=0.0):
    """A scene in make_sequence's format whose camera moves in small steps (0.9 to 1.5 degrees, 0.12 to 0.2 sideways, one camera
    throughout), so that n_in points stay visible over many frames; n_out stray points per frame are uniform pixels matched
    to one another (wrong matches, no margin promised).  Adds "X0": the points."""
    rng = np.random.RandomState(seed)
    direction = np.array([1.0, 0.15, 0.1]) / np.linalg.norm([1.0, 0.15, 0.1])
    Rf, tf, pairs = [np.eye(3)], [np.zeros(3)], []
    intr1 = P.intrinsics_of(0, False)
    for f in range(1, frames):
        Rs = P._rodrigues(np.array([0.2, 1.2, -0.3]) * (0.75 + 0.5 * rng.rand()))
        ts = direction * (0.12 + 0.08 * rng.rand())
        Rf.append(Rs @ Rf[-1])
        tf.append(Rs @ tf[-1] + ts)
        pairs.append({"R": Rs, "t": ts / np.linalg.norm(ts), "length": float(np.linalg.norm(ts)), "intr": np.stack([intr1, intr1])})
    X0 = np.zeros((0, 3))
    while X0.shape[0] < n_in:
        a = np.stack([rng.uniform(8, E.WIDTH - 8, 4 * n_in + 8), rng.uniform(8, E.HEIGHT - 8, 4 * n_in + 8)], axis=1)
        z = rng.uniform(3.0, 12.0, a.shape[0])
        X = np.stack([(a[:, 0] - intr1[2]) * z / intr1[0], (a[:, 1] - intr1[3]) * z / intr1[1], z], axis=1)
        ok = np.ones(X.shape[0], dtype=bool)
        for f in range(frames):
            Y = X @ Rf[f].T + tf[f]
            b = P._project(Y, intr1)
            ok &= (Y[:, 2] > 1.0) & (b[:, 0] > 4) & (b[:, 0] < E.WIDTH - 4) & (b[:, 1] > 4) & (b[:, 1] < E.HEIGHT - 4)
        X0 = np.concatenate([X0, X[ok]])
    X0 = X0[:n_in]
    N = n_in + n_out
    by_id = []
    for f in range(frames):
        px = P._project(X0 @ Rf[f].T + tf[f], intr1)
        if noise > 0.0:
            px = px + noise * rng.randn(n_in, 2)
        stray = np.stack([rng.uniform(8, E.WIDTH - 8, n_out), rng.uniform(8, E.HEIGHT - 8, n_out)], axis=1)
        by_id.append(np.concatenate([px, stray]))
    ids = [rng.permutation(N) for _ in range(frames)]
    pts = [np.ascontiguousarray(by_id[f][ids[f]]) for f in range(frames)]
    for f in range(1, frames):
        row_cur = np.argsort(ids[f])
        order = ids[f - 1]
        match = np.zeros((N, 3), dtype=np.float32)
        match[:, 0], match[:, 1], match[:, 2] = np.arange(N), row_cur[order], rng.rand(N).astype(np.float32)
        pairs[f - 1].update(match=match, truth=order < n_in)
    return {"pts": pts, "ids": ids, "intr": np.stack([intr1] * frames), "pairs": pairs, "n_in": n_in, "X0": X0,
            "centres": np.stack([-(Rf[f].T @ tf[f]) for f in range(frames)])}


# ---- fixtures ------------------------------------------------------------------------------------------------------------------
# name -> (scene, L, point_cap, share of the matches dropped (tracks that end, tracks that start late), seed of the drops).
# scene: a pose_ref.CASES name, or ("slow", seed, frames, n_in, n_out, noise) / ("side", seed, frames, n_in, n_out, noise, zoom).
FIXTURES = {
    "mixed48": ("mixed48", 2, 64, 0.0, 0),
    "n257": ("n257", 2, 320, 0.0, 0),
    "seq3": ("seq3", 3, 48, 0.0, 0),
    "seq5": ("seq5", 5, 64, 0.0, 0),                                  # a camera that zooms: per-frame intrinsics
    "seq5_k": ("seq5_k", 5, 64, 0.0, 0),
    "seq5_late": ("seq5_k", 5, 64, 0.15, 5),                          # tracks that end early and tracks that start late
    "seq5_short": ("seq5_k", 3, 64, 0.0, 0),                          # L below the number of frames: the oldest frames have left
    "forward": ("forward", 2, 64, 0.0, 0),
    "backward": ("backward", 2, 64, 0.0, 0),
    "noisy5": (("side", 41, 5, 40, 8, 0.3, False), 5, 64, 0.0, 0),
    "long16": (("slow", 50, 16, 40, 4, 0.0), 16, 48, 0.05, 6),
    "big": (("slow", 52, 6, 650, 50, 0.0), 5, 704, 0.55, 7),          # more than 2048 rows: tiles and compaction cross workgroups
}
SIDE_NOISE_FREE = ("mixed48", "n257", "seq3", "seq5", "seq5_k")       # the fixtures of the issue's parallax table
SHORT_TRACKS = ("seq5_late", "seq5_short", "long16", "big")           # noise-free too; tracks of two close views lack parallax
COMPARED = ("mixed48", "seq3", "seq5", "seq5_k", "seq5_late", "noisy5", "long16", "big")   # what the device is compared on


def _scene(spec):
    if isinstance(spec, str):
        scene_seed, frames, n_in, n_out, noise, motion, zoom, _ = P.CASES[spec]
        seq = dict(P.case(spec)["seq"])
        seq["X0"] = scene_points(scene_seed, frames, n_in, motion, zoom)
    elif spec[0] == "side":
        _, seed, frames, n_in, n_out, noise, zoom = spec
        seq = dict(P.make_sequence(seed, frames, n_in, n_out, noise=noise, motion="side", zoom=zoom))
        seq["X0"] = scene_points(seed, frames, n_in, "side", zoom)
    else:
        _, seed, frames, n_in, n_out, noise = spec
        seq = make_slow_sequence(seed, frames, n_in, n_out, noise)
    seq["noise"] = noise
    return seq


def build_tracks(seq, L, frames=None, drop=0.0, drop_seed=0):
    """The table tracks_ref keeps after the first `frames` frames of seq, fed the sequence's matches (a share `drop` of them
    left out)."""
    frames = len(seq["pts"]) if frames is None else frames
    rng = np.random.RandomState(1000 + drop_seed)
    t = T.Tracks(L)
    for f in range(frames):
        n = seq["pts"][f].shape[0]
        if f == 0:
            m = np.zeros((3, 0))
        else:
            m = seq["pairs"][f - 1]["match"].astype(np.float64)
            if drop > 0.0:
                m = m[rng.rand(m.shape[0]) >= drop]
            m = m.T
        T.update(t, n, m)
    return t


def ring_of(seq, L, point_cap, frames=None):
    """(pts [L, point_cap, 2] with frame f in slot f % L, first_slot) after `frames` frames."""
    frames = len(seq["pts"]) if frames is None else frames
    pts = np.zeros((L, point_cap, 2))
    for f in range(max(0, frames - L), frames):
        pts[f % L, :seq["pts"][f].shape[0]] = seq["pts"][f]
    return pts, frames % L


def true_cams(seq, L, frames=None):
    """Camera records of the retained frames from the true poses; retained frames before the first are zero records."""
    frames = len(seq["pts"]) if frames is None else frames
    Rw, C = true_poses(seq)
    cams = np.zeros((L, CAM_WORDS))
    for c in range(L):
        f = frames - L + c
        if f >= 0:
            cams[c, :9], cams[c, 9:12], cams[c, 12:16], cams[c, 16] = Rw[f].reshape(9), C[f], seq["intr"][f], 1.0
    return cams


def row_points(seq, t, L, frames=None):
    """Per table row: the scene point its observations belong to (-1: a stray or a mixture) and the list of (frame, row of the
    point in its frame)."""
    frames = len(seq["pts"]) if frames is None else frames
    first = np.concatenate([[0], np.cumsum(t.counts)])[:L]
    point = np.full(t.ids.shape[0], -1, dtype=np.int64)
    obs = []
    for r in range(t.ids.shape[0]):
        o = [(frames - L + c, int(t.ids[r, c] - first[c])) for c in range(L) if t.ids[r, c] >= 0]
        who = {int(seq["ids"][f][p]) for f, p in o}
        if len(who) == 1 and min(who) < seq["n_in"]:
            point[r] = min(who)
        obs.append(o)
    return point, obs


@functools.lru_cache(maxsize=None)
def fixture(name):
    """dict(seq, L, point_cap, tracks (tracks_ref.Tracks), ids, tid, counts, pts, first_slot, cams (true), point, obs, rows / rows2:
    triangulate in WAY1 / WAY2 under the true cameras with the default thresholds); computed once: treat it as read-only."""
    spec, L, point_cap, drop, drop_seed = FIXTURES[name]
    seq = _scene(spec)
    frames = len(seq["pts"])
    Rw, C = true_poses(seq)
    if seq["noise"] == 0.0:                      # the replayed / generated points project onto the sequence's true points
        for f in range(frames):
            px = P._project((seq["X0"] - C[f]) @ Rw[f].T, seq["intr"][f])
            order = np.argsort(seq["ids"][f])[:seq["n_in"]]
            assert np.abs(px - seq["pts"][f][order]).max() < 1e-9, (name, f)
    t = build_tracks(seq, L, drop=drop, drop_seed=drop_seed)
    pts, first_slot = ring_of(seq, L, point_cap)
    cams = true_cams(seq, L)
    point, obs = row_points(seq, t, L)
    out = {"seq": seq, "L": L, "point_cap": point_cap, "tracks": t, "ids": t.ids, "tid": t.tid, "counts": list(t.counts), "pts": pts,
           "first_slot": first_slot, "cams": cams, "point": point, "obs": obs, "frames": frames}
    out["rows"] = triangulate(t.ids, t.counts, pts, first_slot, cams, way=WAY1)
    out["rows2"] = triangulate(t.ids, t.counts, pts, first_slot, cams, way=WAY2)
    return out


def rows_difference(a, b):
    """The largest difference of X, rms, cos_parallax between two results, relative to max(1, |value|); the discrete outputs must
    agree."""
    assert np.array_equal(a["status"], b["status"]) and np.array_equal(a["n_views"], b["n_views"])
    worst = 0.0
    for k in ("X", "rms", "cos_parallax"):
        if a[k].size:
            x, y = np.asarray(a[k], dtype=np.longdouble), np.asarray(b[k], dtype=np.longdouble)
            worst = max(worst, float((np.abs(x - y) / np.maximum(1.0, np.abs(y))).max()))
    return worst


def way_difference(names=COMPARED):
    """The largest WAY1 / WAY2 difference of the continuous outputs over the named fixtures (true cameras) and over the chain
    scenarios of seq5_k (the cameras of the restated chain)."""
    worst = max(rows_difference(fixture(nm)["rows"], fixture(nm)["rows2"]) for nm in names)
    for sc in WINDOW_SCENARIOS:
        a, b = (scenario_rows(sc, w) for w in (WAY1, WAY2))
        worst = max(worst, rows_difference(a, b))
    return worst


def truth_error(name, rows=None):
    """The largest |X - scene point| over the accepted true tracks of a fixture (true cameras)."""
    fx = fixture(name)
    rows = fx["rows"] if rows is None else rows
    sel = (fx["point"] >= 0) & (np.asarray(rows["status"]) == OK)
    assert sel.any()
    return float(np.abs(np.asarray(rows["X"], dtype=np.float64)[sel] - fx["seq"]["X0"][fx["point"][sel]]).max())


# ---- the window scenarios (the cameras of seq5_k from the restated chain's rows) -------------------------------------------------
WINDOW_SCENARIOS = ("plain", "no_pose", "carried", "full", "two_frames")


def chain_table(poses, matches, capacity):
    """The trajectory table a tracker keeps: row 0 is the first frame (no pair: identity, both flag bits), row f the chain's row of
    pair f - 1; cut to `capacity` rows."""
    rows, _ = P.run_chain(poses, matches)
    first = np.zeros((1, P.ROW_WORDS))
    first[0, [0, 4, 8]] = 1.0
    first[0, 12], first[0, 14] = 1.0, 3.0
    table = np.concatenate([first, rows.astype(np.float64)])
    out = np.zeros((capacity, P.ROW_WORDS))
    out[:min(capacity, table.shape[0])] = table[:capacity]
    return out


@functools.lru_cache(maxsize=None)
def window_scenario(name):
    """(n_frames, table [capacity, ROW_WORDS], expected valid flags of the 5 retained frames) for the table of fixture seq5_k
    (two_frames: for the table after its first two frames)."""
    c = P.case("seq5_k")
    seq = c["seq"]
    matches = [pr["match"] for pr in seq["pairs"]]
    poses = list(c["pose"])
    if name == "plain":
        return 5, chain_table(poses, matches, 8), (1, 1, 1, 1, 1)
    if name == "no_pose":            # the pose of frame 2 replaced by identity: it anchors what follows, not what precedes
        r = c["ransac"][1]
        poses[1] = P.two_view_pose(r["F"], np.zeros_like(r["mask"]), 0, 1, seq["pairs"][1]["m"], seq["pairs"][1]["intr"])
        table = chain_table(poses, matches, 8)
        assert list(table[:5, 14]) == [3, 2, 3, 2, 0]
        return 5, table, (0, 0, 1, 1, 1)
    if name == "carried":            # frame 2's scale carried (the flag alone is edited): it joins frame 1 only
        table = chain_table(poses, matches, 8)
        table[2, 14] = 2.0
        return 5, table, (0, 1, 1, 1, 1)
    if name == "full":               # a table of 3 rows after 5 frames: the newest frame's row does not exist
        return 5, chain_table(poses, matches, 3), (0, 0, 0, 0, 0)
    assert name == "two_frames"
    return 2, chain_table(poses[:1], matches[:1], 8), (0, 0, 0, 1, 1)


def scenario_inputs(name):
    """(fixture-like dict of the track table the scenario belongs to, n_frames, table)."""
    n, table, _ = window_scenario(name)
    fx = fixture("seq5_k")
    if name != "two_frames":
        return fx, n, table
    t = build_tracks(fx["seq"], fx["L"], frames=2)
    pts, first_slot = ring_of(fx["seq"], fx["L"], fx["point_cap"], frames=2)
    return {"seq": fx["seq"], "L": fx["L"], "point_cap": fx["point_cap"], "tracks": t, "ids": t.ids, "tid": t.tid,
            "counts": list(t.counts), "pts": pts, "first_slot": first_slot}, n, table


def scenario_rows(name, way=WAY1):
    """triangulate under the cameras map_window gives for a window scenario."""
    fx, n, table = scenario_inputs(name)
    cams = map_window(n, table, fx["seq"]["intr"][:1], fx["L"], way)
    return triangulate(fx["ids"], fx["counts"], fx["pts"], fx["first_slot"], cams, way=way)


def chain_truth_error(rows=None, name="plain"):
    """The largest |X - scene point| over the accepted true tracks of seq5_k under the cameras of the restated chain, both in
    units of the first baseline (the chain's unit)."""
    fx, n, _ = scenario_inputs(name)
    rows = scenario_rows(name) if rows is None else rows
    point = row_points(fx["seq"], fx["tracks"], fx["L"], frames=n)[0]
    sel = (point >= 0) & (np.asarray(rows["status"]) == OK)
    assert sel.any()
    want = fx["seq"]["X0"][point[sel]] / fx["seq"]["pairs"][0]["length"]
    return float(np.abs(np.asarray(rows["X"], dtype=np.float64)[sel] - want).max())


# As way_difference(), max(truth_error(.)) over SIDE_NOISE_FREE + SHORT_TRACKS and chain_truth_error() returned them when the
# fixtures were fixed; tests/test_landmarks_cpu.py repeats the measurements.  The bounds are 16 times these.
WAY_DIFFERENCE = 5.8641168041342e-12          # (a stray track of fixture big), numpy.longdouble (80-bit) as WAY2
TRUTH_ERROR = 8.881784197001252e-14
CHAIN_TRUTH_ERROR = 2.3661073100811336e-12
TOLERANCE = 16.0 * WAY_DIFFERENCE
TRUTH_BOUND = 16.0 * TRUTH_ERROR
CHAIN_TRUTH_BOUND = 16.0 * CHAIN_TRUTH_ERROR
