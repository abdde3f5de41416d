"""numpy restatement of the world map (csrc/world_kernels.hip.h): the landmark store and its anchor rule
(`new_map`, `insert`), the matcher of a frame's descriptors against the map (`match_world`), the join of its matches with the map's
points (`correspondences`) and the repair of the newest trajectory row from the pose found against the map (`repair`).  There is no
reference counterpart, so this file is the specification the kernels are tested against.  The repair is pnp_ref.repair's rule with
another firing condition; the matcher follows readout_ref.match_two_way's arithmetic (the exact dot product rounded to fp32, 2 - 2
clip and the root in fp32, first index on ties) and flags the rows whose decision may hang on the fp32 summation order.  On rows
whose entries all are +-2^e for one e (sign descriptors) every partial sum is a multiple of 2^2e below 2^(2e+8): exact in fp32 in
any order, so nothing is flagged and the matches are exact.  Also a restated tracker with the map (`run_sequence`) and its two
sequences: a blackout and a revisit."""
import functools

import numpy as np

from tests import landmarks_ref as L
from tests import pnp_ref as N
from tests import pose_ref as P
from tests import readout_ref as R

F32 = np.float32
STATE_WORDS = 8        # n_rows, anchored, lost_frames, streak, dropped (full), dropped (tid), appended, updated
N_ROWS, ANCHORED, LOST, STREAK, DROP_FULL, DROP_TID, APPENDED, UPDATED = range(8)
MAX_ROWS = 65536
FLAG_WORLD = 16
PATIENCE = 30
WAY1, WAY2 = P.WAY1, P.WAY2


# ---- the store -------------------------------------------------------------------------------------------------------------------
def new_map(map_cap, tid_cap=1 << 22):
    """An empty map: zeroed arrays (zeroed memory is an empty map)."""
    assert 1 <= map_cap <= MAX_ROWS and tid_cap >= 1
    return {"X": np.zeros((map_cap, 3)), "desc": np.zeros((map_cap, 256), F32), "tid": np.zeros(map_cap, np.int32),
            "n_views": np.zeros(map_cap, np.int32), "first_frame": np.zeros(map_cap, np.int32),
            "last_frame": np.zeros(map_cap, np.int32), "rms": np.zeros(map_cap), "slot_of_tid": np.zeros(tid_cap, np.int32),
            "state": np.zeros(STATE_WORDS, np.int32), "map_cap": map_cap, "tid_cap": tid_cap}


def copy_map(w):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in w.items()}


def n_rows_of(w):
    return min(max(int(w["state"][N_ROWS]), 0), w["map_cap"])


def lookup(w, t):
    """The slot of track t, or -1."""
    if not 0 <= t < w["tid_cap"]:
        return -1
    s = int(w["slot_of_tid"][t])
    return s if 0 <= s < n_rows_of(w) and int(w["tid"][s]) == t else -1


def anchor(w, flags, patience=PATIENCE):
    """The anchor rule on the map's state from the newest trajectory row's flag word (None: no such row, which counts as flagged).
    Returns anchored'.  In place."""
    st = w["state"]
    n_rows, anchored, lost, streak = n_rows_of(w), bool(st[ANCHORED]), int(st[LOST]), int(st[STREAK])
    ok = flags is not None and 0.0 <= flags < 2147483647.0 and (int(flags) & 3) == 0
    anch = ok and (n_rows == 0 or anchored or streak >= 2)
    if n_rows > 0 and not anch:
        lost += 1
        if lost > patience:
            n_rows, lost, streak = 0, 0, 0
            st[DROP_FULL] = st[DROP_TID] = 0
    else:
        lost = 0
    st[N_ROWS], st[ANCHORED], st[LOST], st[STREAK], st[APPENDED], st[UPDATED] = n_rows, int(anch), lost, streak, 0, 0
    return anch


def insert(w, landmarks, n_landmarks, desc_new, count_new, table, n_frames, patience=PATIENCE):
    """One frame's landmark rows into the map, in place (and returned).  landmarks [row_cap, LANDMARK_WORDS] of landmarks_ref.select
    for the window ending at the newest frame, desc_new [point_cap, 256] and count_new of that frame, table [capacity, ROW_WORDS],
    n_frames the frames seen so far."""
    landmarks = np.asarray(landmarks, dtype=np.float64).reshape(-1, L.LANDMARK_WORDS)
    table = np.asarray(table, dtype=np.float64).reshape(-1, P.ROW_WORDS)
    desc_new = np.asarray(desc_new, dtype=F32)
    flags = table[n_frames - 1, 14] if 1 <= n_frames <= table.shape[0] else None
    if not anchor(w, flags, patience):
        return w
    st = w["state"]
    n0 = n_rows_of(w)
    count = min(max(int(count_new), 0), desc_new.shape[0])
    nl = min(max(int(n_landmarks), 0), landmarks.shape[0])
    n_new = n_upd = n_over = 0
    for r in range(nl):
        t, p = landmarks[r, 0], landmarks[r, 7]
        if not (np.all(np.isfinite(landmarks[r, 1:4])) and np.isfinite(p) and 0.0 <= p < count and np.isfinite(t) and t >= 0.0):
            continue
        if not t < w["tid_cap"]:
            n_over += 1
            continue
        t, p = int(t), int(p)
        s = int(w["slot_of_tid"][t])
        found = 0 <= s < n0 and int(w["tid"][s]) == t
        if not found:
            s = n0 + n_new
            n_new += 1
            if s >= w["map_cap"]:
                continue
            w["tid"][s], w["first_frame"][s], w["slot_of_tid"][t] = t, n_frames - 1, s
        else:
            n_upd += 1
        w["X"][s], w["n_views"][s], w["rms"][s], w["last_frame"][s] = landmarks[r, 1:4], int(landmarks[r, 4]), landmarks[r, 5], n_frames - 1
        w["desc"][s] = desc_new[p]
    appended = min(n_new, w["map_cap"] - n0)
    st[N_ROWS] = n0 + appended
    st[DROP_FULL] += n_new - appended
    st[DROP_TID] += n_over
    st[APPENDED], st[UPDATED] = appended, n_upd
    return w


def map_rows(w):
    """(rows [n_rows, 8] = (tid, X, Y, Z, n_views, rms, first_frame, last_frame), descriptors [n_rows, 256])"""
    n = n_rows_of(w)
    rows = np.column_stack([w["tid"][:n], w["X"][:n], w["n_views"][:n], w["rms"][:n], w["first_frame"][:n], w["last_frame"][:n]])
    return rows.astype(np.float64).reshape(n, 8), w["desc"][:n].copy()


# ---- the matcher -----------------------------------------------------------------------------------------------------------------
def _sign_rows(d):
    """True when every entry of d is +-2^e for one e (or d is empty): its dot products are exact in fp32 in any order."""
    a = np.abs(np.asarray(d, np.float64))
    if a.size == 0:
        return True
    m, e = np.frexp(a.flat[0])
    return bool(m == 0.5 and np.all(a == a.flat[0]) and a.shape[-1] <= 256 and e > -60)


def sign_descriptors(seed, n, dim=256):
    """n rows of +-1/16 (unit rows for dim = 256)."""
    rng = np.random.RandomState(seed)
    return (rng.randint(0, 2, (n, dim)).astype(F32) * F32(2) - F32(1)) / F32(np.sqrt(dim))


def match_world(desc_map, n_rows, desc2, count2, thr):
    """nn_match_two_way of the map's first n_rows rows against the frame's first count2 rows (float32 data): dict(match [cap, 3]
    float32 rows (map row, frame row, d) in ascending map row, zero past n_match; n_match; amb_rows [n_rows] bool: the decision on
    that map row may hang on the fp32 summation order (its best and another distance, exact copies of the best aside, are closer
    than their error bounds add up to, the same for the column it picks, or its best distance is that close to thr))."""
    desc_map, desc2 = np.asarray(desc_map, F32), np.asarray(desc2, F32)
    cap = desc2.shape[0]
    n1, n2 = min(max(int(n_rows), 0), desc_map.shape[0]), min(max(int(count2), 0), cap)
    out = {"match": np.zeros((cap, 3), F32), "n_match": 0, "amb_rows": np.zeros(n1, bool)}
    if n1 == 0 or n2 == 0:
        return out
    exact = _sign_rows(desc_map[:n1]) and _sign_rows(desc2[:n2]) and abs(desc_map[0, 0]) == abs(desc2[0, 0])
    if exact:          # (an fp32 product is as exact as any other here, and a 65 536 x 4 096 one fits in memory)
        dot32 = desc_map[:n1] @ desc2[:n2].T
    else:
        a, b = desc_map[:n1].astype(np.float64), desc2[:n2].astype(np.float64)
        dot = a @ b.T
        dot32 = dot.astype(F32)
    d32 = np.sqrt(F32(2) - F32(2) * np.clip(dot32, F32(-1), F32(1)))
    assert d32.dtype == F32
    rb, cb = d32.argmin(axis=1), d32.argmin(axis=0)
    thr32 = F32(thr)
    ar = np.arange(n1)
    keep = (d32[ar, rb] < thr32) & (cb[rb] == ar)
    k = int(keep.sum())
    out["match"][:k, 0], out["match"][:k, 1], out["match"][:k, 2] = ar[keep], rb[keep], d32[ar, rb][keep]
    out["n_match"] = k
    if exact:
        return out
    # the error bound of readout_ref.match_distances, vectorised
    dc = a.shape[1] * R.EPS * (np.abs(a) @ np.abs(b).T)
    d2_ = 2.0 - 2.0 * np.clip(dot, -1.0, 1.0)
    d = np.sqrt(d2_)
    slack = 2 * dc + 2.0 ** -23
    delta = np.maximum(d - np.sqrt(np.maximum(d2_ - slack, 0.0)), np.sqrt(d2_ + slack) - d) + 2.0 ** -23 * d
    del dc, d2_, slack
    lo, hi = d - delta, d + delta

    def ambiguous(lo_, hi_, best, copies):
        other = copies[None, :] != copies[best][:, None]
        return np.where(other, lo_, np.inf).min(axis=1) <= hi_[np.arange(len(best)), best]
    row_amb = ambiguous(lo, hi, rb, R._first_of_equals(desc2[:n2]))
    col_amb = ambiguous(lo.T, hi.T, cb, R._first_of_equals(desc_map[:n1]))
    near_thr = np.abs(d[ar, rb] - float(thr32)) <= delta[ar, rb]
    out["amb_rows"] = row_amb | col_amb[rb] | near_thr
    return out


# ---- the join ----------------------------------------------------------------------------------------------------------------
def correspondences(w, match, n_match, pts_new, count_new):
    """Correspondence rows [cap, CORR_WORDS] = (X, Y, Z, px, py, map row, valid, 0) aligned with the match rows, and (n, n_valid)."""
    match, pts_new = np.asarray(match), np.asarray(pts_new, dtype=np.float64)
    cap = match.shape[0]
    n_rows, count = n_rows_of(w), min(max(int(count_new), 0), pts_new.shape[0])
    n = min(max(int(n_match), 0), cap)
    out = np.zeros((cap, N.CORR_WORDS))
    n_valid = 0
    for k in range(n):
        fi, fj = float(match[k, 0]), float(match[k, 1])
        if not (0.0 <= fi < n_rows and 0.0 <= fj < count):
            continue
        i, j = int(fi), int(fj)
        row = [w["X"][i, 0], w["X"][i, 1], w["X"][i, 2], pts_new[j, 0], pts_new[j, 1]]
        if not all(np.isfinite(row)):
            continue
        out[k, :5], out[k, 5], out[k, 6] = row, i, 1.0
        n_valid += 1
    return out, (n, n_valid)


# ---- the repair ------------------------------------------------------------------------------------------------------------------
def repair(w, absolute, state, table, way=WAY1):
    """pnp_ref.repair's rule with the world's firing condition: (state [STATE_WORDS], table [capacity, ROW_WORDS]) of one sequence
    (copies); the map's streak is updated in place.  Fires on row n - 1 (1 <= n < capacity rows) when the pose has status 0 and is
    finite and either the row carries flag bit 0 or 1 or the map is lost (rows, not anchored)."""
    dt, rev = way
    state, table = np.array(state, dtype=dt), np.array(table, dtype=dt).reshape(-1, P.ROW_WORDS)
    capacity = table.shape[0]
    nf = state[0]
    n = int(nf) if 0.0 <= nf < 2147483647.0 else 0
    lost = n_rows_of(w) > 0 and int(w["state"][ANCHORED]) == 0
    fire = 1 <= n < capacity and int(absolute["status"]) == 0
    if fire:
        row = table[n - 1]
        flags = int(row[14])
        Rw, C = np.asarray(absolute["Rw"], dtype=dt).reshape(9), np.asarray(absolute["C"], dtype=dt).reshape(3)
        fire = bool(np.all(np.isfinite(Rw)) and np.all(np.isfinite(C))) and bool((flags & 3) or lost)
    if not fire:
        w["state"][STREAK] = 0
        return state, table
    tw = np.array([-N._dot(Rw[3 * i:3 * i + 3], C, rev) for i in range(3)], dtype=dt)
    s, keep = state[1], flags & 2
    if n >= 2:
        d = C - table[n - 2, 9:12]
        with np.errstate(all="ignore"):
            length = np.sqrt(N._dot(d, d, rev))
        if np.isfinite(length) and length > dt(N.SCALE_FRACTION) * s:
            s, keep = length, 0
    row[0:9], row[9:12], row[12], row[14] = Rw, C, s, dt(keep | N.FLAG_ABSOLUTE | FLAG_WORLD)
    state[1], state[2:11], state[11:14] = s, Rw, tw
    w["state"][STREAK] += 1
    return state, table


# ---- sequences: a blackout and a revisit -------------------------------------------------------------------------------------------
NN_THRESH = 0.7
BLACKOUT = (50, 10, 40, 4)         # landmarks_ref's slow camera: seed, frames, points; the frame that has no points
BLACKOUT_L, REVISIT_L = 5, 4
REVISIT = (7, 13, 420)             # seed, frames (out 0..6, back 7..12), candidate points


def _finish(seq, desc_seed):
    """Sign descriptors per scene point, and every pair's matches as the matcher finds them from these: equal descriptors at
    distance 0, in ascending row of the previous frame (unequal sign rows lie near sqrt(2): never below NN_THRESH)."""
    n_ids = max([int(i.max()) + 1 for i in seq["ids"] if len(i)] + [1])
    by_id = sign_descriptors(desc_seed, n_ids)
    seq["desc"] = [by_id[i] for i in seq["ids"]]
    for f in range(1, len(seq["pts"])):
        row_cur = {int(p): r for r, p in enumerate(seq["ids"][f])}
        rows = [(i, row_cur[int(p)], 0.0) for i, p in enumerate(seq["ids"][f - 1]) if int(p) in row_cur]
        match = np.array(rows, dtype=np.float32).reshape(-1, 3)
        seq["pairs"][f - 1].update(match=match, truth=np.ones(match.shape[0], dtype=bool))
    return seq


def blackout_sequence():
    """landmarks_ref's slow camera, noise-free, no strays; frame BLACKOUT[3] has no points, so the pairs on both sides of it have
    no matches.  Refuses (AssertionError) unless at least 12 scene points seen before the blackout are seen in the two frames
    after it."""
    seed, frames, n_in, dark = BLACKOUT
    seq = L.make_slow_sequence(seed, frames, n_in, 0)
    seq["pts"][dark], seq["ids"][dark] = np.zeros((0, 2)), np.zeros(0, dtype=np.int64)
    seq["dark"] = dark
    before = set(np.concatenate(seq["ids"][:dark]).tolist())
    assert min(len(before & set(seq["ids"][f].tolist())) for f in (dark + 1, dark + 2)) >= 12
    return _finish(seq, 91)


def revisit_sequence():
    """A camera that moves sideways out (frames 0..6) and comes back (7..12) on a slightly different path, noise-free: points
    leave the image and return after more than REVISIT_L frames, under new track ids."""
    seed, frames, n_cand = REVISIT
    rng = np.random.RandomState(seed)
    k = P.intrinsics_of(0, False)
    half = frames // 2
    Rf, tf, C = [], [], []
    for f in range(frames):
        x = 0.45 * f if f <= half else 0.45 * (frames - 1 - f) + 0.2
        c = np.array([x, 0.04 * f, 0.02 * (f % 3)])
        R = P._rodrigues(np.array([0.3, 1.5, -0.2]) * (x / 2.7)) if f else np.eye(3)      # the world is camera 0
        Rf.append(R), C.append(c), tf.append(-(R @ c))
    a = np.stack([rng.uniform(-300, 900, n_cand), rng.uniform(8, 232, n_cand)], axis=1)
    z = rng.uniform(3.0, 12.0, n_cand)
    X0 = np.stack([(a[:, 0] - k[2]) * z / k[0], (a[:, 1] - k[3]) * z / k[1], z], axis=1)
    pts, ids = [], []
    for f in range(frames):
        Y = X0 @ Rf[f].T + tf[f]
        b = P._project(Y, k)
        seen = np.nonzero((Y[:, 2] > 1.0) & (b[:, 0] > 4) & (b[:, 0] < 316) & (b[:, 1] > 4) & (b[:, 1] < 236))[0]
        order = seen[rng.permutation(len(seen))]
        pts.append(np.ascontiguousarray(b[order])), ids.append(order.astype(np.int64))
    pairs = []
    for f in range(1, frames):
        Rs = Rf[f] @ Rf[f - 1].T
        ts = tf[f] - Rs @ tf[f - 1]
        pairs.append({"R": Rs, "t": ts / np.linalg.norm(ts), "length": float(np.linalg.norm(ts)), "intr": np.stack([k, k])})
    seq = {"pts": pts, "ids": ids, "intr": np.stack([k] * frames), "pairs": pairs, "n_in": n_cand, "X0": X0, "centres": np.stack(C),
           "Rw": np.stack(Rf)}
    return _finish(seq, 92)


def run_sequence(seq, max_length, point_cap, world_mode, seed0, absolute_mode=None, world_cap=4096, tid_cap=1 << 16,
                 patience=PATIENCE, min_inliers=16, thresh=N.THRESH, abs_min_inliers=N.MIN_INLIERS,
                 landmark_params=(L.MIN_VIEWS, L.MIN_PARALLAX_DEG, L.MAX_REPROJ), way=WAY1):
    """pnp_ref.run_sequence with the world map: what a PointTracker(geometric_check="fundamental", intrinsics=one camera,
    absolute_pose=absolute_mode, world_map=world_mode) computes over the frames of seq.  dict(table [frames, ROW_WORDS], world: per
    frame the ransac dict against the map, world_corr: per frame (corr, n, n_valid), world_match, states: per frame the map's state
    after the insert, map: the map at the end, maps_last_frame: per frame the map's last_frame column before the frame, tracks)."""
    from tests import epipolar_ref as E
    from tests import tracks_ref as T
    dt = way[0]
    frames = len(seq["pts"])
    k = seq["intr"][0]
    tracks = T.Tracks(max_length)
    state = P.new_state(way)
    table = np.zeros((frames + 1, P.ROW_WORDS), dtype=dt)
    prev_pose = prev_match = lms = None
    world = new_map(world_cap, tid_cap)
    out = {"world": [], "world_corr": [], "world_match": [], "states": [], "maps_last_frame": [], "absolute": []}
    mv, par, rep = landmark_params

    def put_back(w):
        return {"n_frames": state["n_frames"], "s": w[1], "Rw": w[2:11].reshape(3, 3).copy(), "tw": w[11:14].copy()}

    def words():
        w = np.zeros(P.STATE_WORDS, dtype=dt)
        w[0], w[1], w[2:11], w[11:14] = state["n_frames"], state["s"], np.asarray(state["Rw"], dtype=dt).reshape(9), state["tw"]
        return w
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
        res = None
        if absolute_mode is not None and lms is not None:
            padded = np.zeros((point_cap, 3), dtype=np.float32)
            padded[:match.shape[0]] = match
            corr, (n, nv) = N.join(lms, lms.shape[0], padded, match.shape[0], pts_new)
            res = N.ransac(corr, n, k, seed0 + f, thresh, abs_min_inliers, way=way)
            if absolute_mode == "repair":
                w, table = N.repair(res, words(), table, way=way)
                state = put_back(w)
        out["absolute"].append(res)
        desc_new = np.zeros((point_cap, 256), dtype=F32)
        desc_new[:n_pts] = seq["desc"][f]
        out["maps_last_frame"].append(world["last_frame"][:n_rows_of(world)].copy())
        if world_mode is not None:
            mw = match_world(world["desc"], n_rows_of(world), desc_new, n_pts, NN_THRESH)
            corr, (n, nv) = correspondences(world, mw["match"], mw["n_match"], pts_new, n_pts)
            wres = N.ransac(corr, n, k, seed0 + f, thresh, abs_min_inliers, way=way)
            if world_mode == "relocalise":
                w, table = repair(world, wres, words(), table, way=way)
                state = put_back(w)
            out["world"].append(wres), out["world_corr"].append((corr, n, nv)), out["world_match"].append(mw)
        keep = r["mask"] if (r["status"] == 0 and r["n_inliers"] >= min_inliers) else np.ones(match.shape[0], dtype=bool)
        T.update(tracks, n_pts, match[keep].astype(np.float64).T.reshape(3, -1))
        if f >= 1:
            cams = L.map_window(f + 1, table, seq["intr"][:1], max_length, way=way)
            ring, first_slot = L.ring_of(seq, max_length, point_cap, frames=f + 1)
            rows = L.triangulate(tracks.ids, tracks.counts, ring, first_slot, cams, mv, L.cos_of(par), rep, way=way)
            lms = L.select(tracks.ids, tracks.tid, tracks.counts, point_cap, rows)
            if world_mode is not None:
                insert(world, lms, lms.shape[0], desc_new, n_pts, np.asarray(table, dtype=np.float64), f + 1, patience)
        out["states"].append(world["state"].copy())
    out["table"], out["tracks"], out["map"] = np.asarray(table[:frames], dtype=np.float64), tracks, world
    return out


def centre_errors(seq, table):
    """Per frame 1..: the largest difference between the table's centre and the true one, both in first baselines."""
    unit = np.linalg.norm(seq["centres"][1] - seq["centres"][0])
    want = (seq["centres"][:table.shape[0]] - seq["centres"][0]) / unit
    got = np.asarray(table, dtype=np.float64)[:, 9:12]
    got = got / np.linalg.norm(got[1])
    return np.abs(got - want).max(axis=1)


def way_difference(seq, max_length, point_cap, world_mode, seed0, **kw):
    """The largest difference of the centres of run_sequence (the trajectory's and the world poses') between float64 and
    pose_ref.WAY2."""
    a = run_sequence(seq, max_length, point_cap, world_mode, seed0, **kw)
    b = run_sequence(seq, max_length, point_cap, world_mode, seed0, way=WAY2, **kw)
    worst = float(np.abs(a["table"][:, 9:12] - b["table"][:, 9:12]).max())
    for x, y in zip(a["world"], b["world"]):
        assert x["status"] == y["status"]
        worst = max(worst, float(np.abs(np.asarray(x["C"], dtype=np.float64) - np.asarray(y["C"], dtype=np.float64)).max()))
    return worst


# As way_difference() returned them when the sequences were fixed (numpy.longdouble, 80-bit, as WAY2); tests/test_world_cpu.py
# repeats the measurements.  The bounds are 16 times these, in units of the trajectory (first baselines).
BLACKOUT_SEED0, REVISIT_SEED0 = 100, 200
BLACKOUT_CAP, REVISIT_CAP = 48, 256
BLACKOUT_WAY_DIFFERENCE = 1.4583889651476056e-12
REVISIT_WAY_DIFFERENCE = 8.526512829121202e-14
BLACKOUT_BOUND = 16.0 * BLACKOUT_WAY_DIFFERENCE
REVISIT_BOUND = 16.0 * REVISIT_WAY_DIFFERENCE


@functools.lru_cache(maxsize=None)
def blackout_runs():
    """(seq, {"repair": pnp_ref's repair alone, "observe", "relocalise"}): computed once, read-only."""
    seq = blackout_sequence()
    run = lambda mode, **kw: run_sequence(seq, BLACKOUT_L, BLACKOUT_CAP, mode, BLACKOUT_SEED0, **kw)
    return seq, {"repair": run(None, absolute_mode="repair"), "observe": run("observe"), "relocalise": run("relocalise"),
                 "plain": run(None)}


@functools.lru_cache(maxsize=None)
def revisit_runs():
    """(seq, {"plain", "observe", "relocalise"}): computed once, read-only."""
    seq = revisit_sequence()
    run = lambda mode: run_sequence(seq, REVISIT_L, REVISIT_CAP, mode, REVISIT_SEED0)
    return seq, {"plain": run(None), "observe": run("observe"), "relocalise": run("relocalise")}


def old_inliers(run, f, max_length):
    """How many inliers of frame f's world pose are map rows last seen before frame f + 1 - max_length."""
    w = run["world"][f]
    corr, n, _ = run["world_corr"][f]
    rows = corr[:n][np.asarray(w["mask"][:n], dtype=bool), 5].astype(np.int64)
    return int((run["maps_last_frame"][f][rows] < f + 1 - max_length).sum())


def world_centre_error(seq, run, f):
    """Frame f's world pose against the true camera: the centre in first baselines, the rotation's largest entry difference."""
    unit = np.linalg.norm(seq["centres"][1] - seq["centres"][0])
    C = np.asarray(run["world"][f]["C"], dtype=np.float64) / np.linalg.norm(run["table"][1, 9:12])
    return float(np.abs(C - (seq["centres"][f] - seq["centres"][0]) / unit).max())
