"""numpy restatement of the world map's upkeep (csrc/world_upkeep_kernels.hip.h): `upkeep` merges the row
pair of a scene point that returned under a new track id, culls rows that never matured, evicts the rows of smallest key when the
map nears its capacity, and compacts the store.  There is no reference counterpart, so this file is the specification the kernels
are tested against.  The store, its lookup and its insert are tests/world_ref.py's; the one floating-point decision, the
reprojection gate of the merge, is pnp_ref.view in float64, and `upkeep` flags a merge decision that lies within 1e-9 (relative)
of a threshold as ambiguous.  Also the restated tracker with upkeep (`run_sequence`) and a second sequence beside world_ref's
revisit: a long run, on which a map without upkeep fills up and forgets the present."""
import functools

import numpy as np

from tests import landmarks_ref as L
from tests import pnp_ref as N
from tests import pose_ref as P
from tests import world_ref as W

REPORT_WORDS = 8       # rows before, merged, culled, evicted, rows after, eviction fired, rows wanted but protected, skipped
BEFORE, MERGED, CULLED, EVICTED, AFTER, FIRED, PROTECTED, SKIPPED = range(8)
AMBIGUOUS = 1e-9
COLUMNS = ("X", "desc", "tid", "n_views", "first_frame", "last_frame", "rms")
OFF = dict(merge=False, cull_age=-1, high_water=-1)      # every phase disabled


def owners(landmarks, n_landmarks, count, tid_cap):
    """{frame point: the lowest landmark row that passes the insert's test and names it}"""
    landmarks = np.asarray(landmarks, dtype=np.float64).reshape(-1, L.LANDMARK_WORDS)
    nl = min(max(int(n_landmarks), 0), landmarks.shape[0])
    own = {}
    for q in range(nl):
        t, p = landmarks[q, 0], landmarks[q, 7]
        if (np.all(np.isfinite(landmarks[q, 1:4])) and np.isfinite(p) and 0.0 <= p < count and np.isfinite(t) and 0.0 <= t < tid_cap
                and int(p) not in own):
            own[int(p)] = q
    return own


def evict_key(n_views, last_frame, slot):
    """Fewest views first, then the oldest, then the higher slot: compared as tuples (or as the 56-bit integer of the kernel)."""
    return (min(max(int(n_views), 0), 255), max(int(last_frame), 0), 65535 - int(slot))


def upkeep(w, match, n_match, landmarks, n_landmarks, pts_new, count_new, table, n_frames, k, merge=True, merge_thresh=2.0,
           cull_age=-1, cull_min_views=3, high_water=-1, low_water=0):
    """One call on the map w (world_ref.new_map's dict), in place.  match [cap, 3] rows (map row, frame point, d) of
    world_ref.match_world before the insert, landmarks / n_landmarks / count_new / table / n_frames as given to world_ref.insert,
    pts_new [point_cap, >= 2], k = (fx, fy, cx, cy).  Returns (report int32 [REPORT_WORDS], info) with info = dict(pairs: the merged
    (r, r') in match order, ambiguous: a merge decision lay within AMBIGUOUS of a threshold, dead: the mark of every row before the
    compaction (0 alive, 1 merged, 2 culled, 3 evicted))."""
    match = np.asarray(match)
    landmarks = np.asarray(landmarks, dtype=np.float64).reshape(-1, L.LANDMARK_WORDS)
    pts_new = np.asarray(pts_new, dtype=np.float64)
    table = np.asarray(table, dtype=np.float64).reshape(-1, P.ROW_WORDS)
    k = np.asarray(k, dtype=np.float64).reshape(4)
    assert high_water < 0 or 0 <= low_water <= high_water <= w["map_cap"]
    n0, f = W.n_rows_of(w), int(n_frames) - 1
    report = np.zeros(REPORT_WORDS, np.int32)
    report[BEFORE] = report[AFTER] = n0
    info = {"pairs": [], "ambiguous": False, "dead": np.zeros(n0, np.int32)}
    if not (int(w["state"][W.ANCHORED]) == 1 and n0 > 0 and 1 <= n_frames <= table.shape[0]):
        report[SKIPPED] = 1
        return report, info
    dead = info["dead"]
    last = w["last_frame"]
    # a. merge: every decision on the map as the insert left it, then the rows
    if merge:
        count = min(max(int(count_new), 0), pts_new.shape[0])
        own = owners(landmarks, n_landmarks, count, w["tid_cap"])
        Rw, C = table[f, 0:9], table[f, 9:12]
        t2 = float(merge_thresh) * float(merge_thresh)
        for m in range(min(max(int(n_match), 0), match.shape[0])):
            fi, fj = float(match[m, 0]), float(match[m, 1])
            if not (0.0 <= fi < n0 and 0.0 <= fj < count) or int(fj) not in own:
                continue
            r, p = int(fi), int(fj)
            r2 = W.lookup(w, int(landmarks[own[p], 0]))
            if r2 < 0 or r2 == r or not last[r] < f or last[r2] != f:
                continue
            with np.errstate(all="ignore"):
                e, front = N.view(Rw, C, w["X"][r], pts_new[p], k)
                q = w["X"][r] - C
                depth = (Rw[6] * q[0] + Rw[7] * q[1]) + Rw[8] * q[2]
            if abs(e - t2) <= AMBIGUOUS * t2 or abs(depth) <= AMBIGUOUS * float(np.abs(q).max()):
                info["ambiguous"] = True
            if bool(front) and e <= t2:
                info["pairs"].append((r, r2))
        rows = [x for pair in info["pairs"] for x in pair]
        assert len(set(rows)) == len(rows), "merging pairs share a row: the match rows are not one-to-one"
        for r, r2 in info["pairs"]:
            keep, die = min(r, r2), max(r, r2)
            first = min(int(w["first_frame"][r]), int(w["first_frame"][r2]))
            if keep == r:
                for c in ("X", "desc", "tid", "n_views", "rms"):
                    w[c][r] = w[c][r2]
                last[r] = f
                w["slot_of_tid"][int(w["tid"][r])] = r
            w["first_frame"][keep] = first
            dead[die] = 1
    # b. cull
    if cull_age >= 0:
        for i in range(n0):
            if dead[i] == 0 and last[i] < f - cull_age and w["n_views"][i] < cull_min_views:
                dead[i] = 2
    # c. evict
    alive = int((dead == 0).sum())
    if high_water >= 0 and alive > high_water:
        cand = sorted((evict_key(w["n_views"][i], last[i], i), i) for i in range(n0) if dead[i] == 0 and last[i] != f)
        want = alive - low_water
        n_evict = min(want, len(cand))
        for _, i in cand[:n_evict]:
            dead[i] = 3
        report[EVICTED], report[FIRED], report[PROTECTED] = n_evict, 1, want - n_evict
    # d. compact: survivors keep their order
    report[MERGED], report[CULLED] = int((dead == 1).sum()), int((dead == 2).sum())
    keep = np.nonzero(dead == 0)[0]
    n1 = len(keep)
    report[AFTER] = n1
    if n1 != n0:
        for c in COLUMNS:
            w[c][:n1] = w[c][keep]
        for d in range(int(np.nonzero(dead != 0)[0][0]), n1):
            t = int(w["tid"][d])
            if 0 <= t < w["tid_cap"]:
                w["slot_of_tid"][t] = d
        w["state"][W.N_ROWS] = n1
    return report, info


# ---- the restated tracker with upkeep ------------------------------------------------------------------------------------------
def upkeep_options(max_length, world_cap, thresh=N.THRESH, world_upkeep="on", world_merge=True, world_merge_thresh=None,
                   world_cull_age=None, world_cull_min_views=3, world_high_water=None, world_low_water=None):
    """PointTracker's options as the keyword arguments of `upkeep` (None: no upkeep), with the tracker's defaults."""
    if world_upkeep is None:
        return None
    return dict(merge=bool(world_merge), merge_thresh=thresh if world_merge_thresh is None else world_merge_thresh,
                cull_age=max_length if world_cull_age is None else world_cull_age, cull_min_views=world_cull_min_views,
                high_water=world_cap - world_cap // 16 if world_high_water is None else world_high_water,
                low_water=world_cap - world_cap // 8 if world_low_water is None else world_low_water)


def run_sequence(seq, max_length, point_cap, world_mode, seed0, upkeep_params=None, world_cap=4096, tid_cap=1 << 16,
                 patience=W.PATIENCE, min_inliers=16, thresh=N.THRESH, abs_min_inliers=N.MIN_INLIERS,
                 landmark_params=(L.MIN_VIEWS, L.MIN_PARALLAX_DEG, L.MAX_REPROJ), way=W.WAY1):
    """world_ref.run_sequence (without absolute_pose) followed, after every insert, by `upkeep` with the keyword arguments
    upkeep_params (None: no call, which is world_ref.run_sequence): what PointTracker(world_map=world_mode, world_upkeep="on")
    computes.  world_ref.run_sequence's dict plus reports: per frame the report (None where the tracker makes no call), merged: per
    frame the merged pairs as (scene point of r, scene point of r'), ambiguous: any merge decision was, maps: per frame the live
    map rows and descriptors after the frame (world_ref.map_rows)."""
    from tests import epipolar_ref as E
    from tests import tracks_ref as T
    dt = way[0]
    frames = len(seq["pts"])
    k = seq["intr"][0]
    tracks = T.Tracks(max_length)
    state = P.new_state(way)
    table = np.zeros((frames + 1, P.ROW_WORDS), dtype=dt)
    prev_pose = prev_match = None
    world = W.new_map(world_cap, tid_cap)
    scene = {}                      # track id -> scene point, from the newest observation of every inserted landmark
    out = {"world": [], "world_corr": [], "world_match": [], "states": [], "maps_last_frame": [], "reports": [], "merged": [],
           "ambiguous": False, "maps": []}
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
        desc_new = np.zeros((point_cap, 256), dtype=W.F32)
        desc_new[:n_pts] = seq["desc"][f]
        out["maps_last_frame"].append(world["last_frame"][:W.n_rows_of(world)].copy())
        mw = W.match_world(world["desc"], W.n_rows_of(world), desc_new, n_pts, W.NN_THRESH)
        corr, (n, nv) = W.correspondences(world, mw["match"], mw["n_match"], pts_new, n_pts)
        wres = N.ransac(corr, n, k, seed0 + f, thresh, abs_min_inliers, way=way)
        if world_mode == "relocalise":
            w, table = W.repair(world, wres, words(), table, way=way)
            state = put_back(w)
        out["world"].append(wres), out["world_corr"].append((corr, n, nv)), out["world_match"].append(mw)
        keep = r["mask"] if (r["status"] == 0 and r["n_inliers"] >= min_inliers) else np.ones(match.shape[0], dtype=bool)
        T.update(tracks, n_pts, match[keep].astype(np.float64).T.reshape(3, -1))
        report, merged = None, []
        if f >= 1:
            cams = L.map_window(f + 1, table, seq["intr"][:1], max_length, way=way)
            ring, first_slot = L.ring_of(seq, max_length, point_cap, frames=f + 1)
            rows = L.triangulate(tracks.ids, tracks.counts, ring, first_slot, cams, mv, L.cos_of(par), rep, way=way)
            lms = L.select(tracks.ids, tracks.tid, tracks.counts, point_cap, rows)
            table64 = np.asarray(table, dtype=np.float64)
            W.insert(world, lms, lms.shape[0], desc_new, n_pts, table64, f + 1, patience)
            for q in range(lms.shape[0]):
                if 0.0 <= lms[q, 7] < n_pts:
                    scene[int(lms[q, 0])] = int(seq["ids"][f][int(lms[q, 7])])
            if upkeep_params is not None:
                tids = world["tid"].copy()
                report, info = upkeep(world, mw["match"], mw["n_match"], lms, lms.shape[0], pts_new, n_pts, table64, f + 1, k,
                                      **upkeep_params)
                merged = [(scene.get(int(tids[a]), -1), scene.get(int(tids[b]), -2)) for a, b in info["pairs"]]
                out["ambiguous"] = out["ambiguous"] or info["ambiguous"]
        out["reports"].append(report), out["merged"].append(merged)
        out["states"].append(world["state"].copy()), out["maps"].append(W.map_rows(world))
    out["table"], out["tracks"], out["map"] = np.asarray(table[:frames], dtype=np.float64), tracks, world
    return out


# ---- the long run: a camera that translates steadily past a long strip of points ---------------------------------------------------
LONG_RUN = (11, 36, 400, 1.2)      # seed, frames, candidate points, the step of the camera along x per frame
LONG_RUN_L, LONG_RUN_CAP, LONG_RUN_WORLD_CAP, LONG_RUN_SEED0 = 4, 96, 256, 300
# As world_ref.way_difference() returned it on the long run when the sequence was fixed (numpy.longdouble, 80-bit);
# tests/test_world_upkeep_cpu.py repeats the measurement.  The bound is 16 times that, as world_ref's are.
LONG_RUN_WAY_DIFFERENCE = 1.1368683772161603e-13
LONG_RUN_BOUND = 16.0 * LONG_RUN_WAY_DIFFERENCE
LONG_RUN_LATE = 4                  # the last frames, by which a map that stopped growing has lost sight of the camera


def long_run_sequence():
    """A camera that moves sideways at a constant step (no rotation beyond a slow yaw), noise-free, over a strip of points many
    image widths long: every frame brings points no earlier frame saw, and none returns."""
    seed, frames, n_cand, step = LONG_RUN
    rng = np.random.RandomState(seed)
    k = P.intrinsics_of(0, False)
    Rf, tf, C = [], [], []
    for f in range(frames):
        c = np.array([step * f, 0.03 * f, 0.02 * (f % 3)])
        R = P._rodrigues(np.array([0.0, 0.004, 0.0]) * f) if f else np.eye(3)      # the world is camera 0
        Rf.append(R), C.append(c), tf.append(-(R @ c))
    z = rng.uniform(4.0, 12.0, n_cand)
    x = rng.uniform(-2.0, step * frames + 6.0, n_cand)
    v = rng.uniform(8, 232, n_cand)
    X0 = np.stack([x, (v - k[3]) * z / k[1], z], axis=1)
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
    assert max(len(i) for i in ids) <= LONG_RUN_CAP
    return W._finish(seq, 93)


@functools.lru_cache(maxsize=None)
def revisit_runs():
    """(seq, {"plain": world_ref's "observe" run, "off": upkeep with every phase disabled, "on": the tracker's defaults}) on
    world_ref's revisit: computed once, read-only."""
    seq = W.revisit_sequence()
    run = lambda prm: run_sequence(seq, W.REVISIT_L, W.REVISIT_CAP, "observe", W.REVISIT_SEED0, upkeep_params=prm)
    return seq, {"plain": run(None), "off": run(OFF), "on": run(upkeep_options(W.REVISIT_L, 4096))}


@functools.lru_cache(maxsize=None)
def long_runs():
    """(seq, {"plain", "on"}) on the long run with a map of LONG_RUN_WORLD_CAP rows: computed once, read-only."""
    seq = long_run_sequence()
    run = lambda prm: run_sequence(seq, LONG_RUN_L, LONG_RUN_CAP, "observe", LONG_RUN_SEED0, upkeep_params=prm,
                                   world_cap=LONG_RUN_WORLD_CAP)
    return seq, {"plain": run(None), "on": run(upkeep_options(LONG_RUN_L, LONG_RUN_WORLD_CAP))}
