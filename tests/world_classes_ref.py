"""numpy restatement of the world map's classes (csrc/world_class_kernels.hip.h and the CLASSES instance of
world_match_kernel): the class vote per track (`vote`, `decode`), the map read out as a labelled point cloud (`world_classes`), the
map matcher restricted to pairs of one known, kept class (`match_world_classes`), and world_ref.run_sequence with the votes and the
class-aware matcher (`run_sequence`) on the revisit with planted aliases (`alias_sequence`).  There is no reference counterpart, so
this file is the specification.  It imports world_ref and changes nothing in it.  The matcher is stated for sign descriptors only
(world_ref.sign_descriptors: every dot product exact in fp32 in any order), so every comparison against it is ==."""
import functools

import numpy as np

from tests import landmarks_ref as L
from tests import pnp_ref as N
from tests import pose_ref as P
from tests import world_ref as W

F32 = np.float32
CLASS_NONE = 255
VOTE_MAX = 255
FULL_MASK = (0xFFFFFFFF,) * 8


# ---- the votes -------------------------------------------------------------------------------------------------------------------
def new_votes(tid_cap):
    """uint16 [tid_cap]: the low byte the class, the high byte the vote count; zero = no class yet"""
    return np.zeros(tid_cap, np.uint16)


def vote_step(v, c):
    """One Boyer-Moore step of the entry v with an observation of class c != CLASS_NONE."""
    n, have = int(v) >> 8, int(v) & 255
    if n == 0:
        return (1 << 8) | c
    if have == c:
        return (min(n + 1, VOTE_MAX) << 8) | c
    return ((n - 1) << 8) | have


def vote(votes, landmarks, n_landmarks, cls_new, count_new):
    """One frame's votes, in place (and returned).  landmarks [row_cap, LANDMARK_WORDS]: word 0 the track id t, word 7 the
    newest-frame index p; cls_new uint8 [point_cap].  A row takes part iff 0 <= p < count, 0 <= t < tid_cap and cls_new[p] !=
    CLASS_NONE: world_ref.insert's test without X."""
    landmarks = np.asarray(landmarks, dtype=np.float64).reshape(-1, L.LANDMARK_WORDS)
    cls_new = np.asarray(cls_new, dtype=np.uint8)
    count = min(max(int(count_new), 0), cls_new.shape[0])
    nl = min(max(int(n_landmarks), 0), landmarks.shape[0])
    seen = set()
    for r in range(nl):
        t, p = landmarks[r, 0], landmarks[r, 7]
        if not (np.isfinite(p) and 0.0 <= p < count and np.isfinite(t) and 0.0 <= t < votes.shape[0]):
            continue
        c = int(cls_new[int(p)])
        if c == CLASS_NONE:
            continue
        assert int(t) not in seen, "track ids must be unique within a call"
        seen.add(int(t))
        votes[int(t)] = vote_step(votes[int(t)], c)
    return votes


def decode(v):
    """The class an entry (or an array of entries) stands for: CLASS_NONE without votes."""
    v = np.asarray(v, dtype=np.uint16)
    return np.where((v >> 8) > 0, v & 255, CLASS_NONE).astype(np.uint8)


def class_of_tracks(votes, tids):
    """decode(votes[tids]); a track id outside [0, tid_cap) has no class"""
    tids = np.asarray(tids, dtype=np.int64)
    ok = (tids >= 0) & (tids < votes.shape[0])
    out = np.full(tids.shape, CLASS_NONE, np.uint8)
    out[ok] = decode(votes[tids[ok]])
    return out


def world_classes(w, votes):
    """uint8 [map_cap]: the class of every map row's track below n_rows, CLASS_NONE past it"""
    out = np.full(w["map_cap"], CLASS_NONE, np.uint8)
    n = W.n_rows_of(w)
    out[:n] = class_of_tracks(votes, w["tid"][:n])
    return out


map_classes = world_classes       # (run_sequence has an option of that name)


# ---- the matcher -----------------------------------------------------------------------------------------------------------------
def kept(classes, mask=FULL_MASK):
    """bool: the class is known and its bit of the eight 32-bit words `mask` (lib.class_mask's layout) is set"""
    c = np.asarray(classes, dtype=np.int64)
    words = np.asarray([int(m) for m in mask], dtype=np.uint64)
    return (c != CLASS_NONE) & (((words[c >> 5] >> (c & 31).astype(np.uint64)) & np.uint64(1)) == 1)


def match_world_classes(desc_map, n_rows, cls_map, desc2, cls2, count2, thr, mask=FULL_MASK):
    """world_ref.match_world with one more condition: (i, j) is a candidate iff cls_map[i] == cls2[j], cls_map[i] != CLASS_NONE and
    the mask keeps cls_map[i]; any other pair takes part in neither arg-min, a row or a column without a candidate gives no match.
    cls_map [>= n_rows]: the decoded class of every map row.  Sign descriptors only.  dict(match [cap, 3], n_match)."""
    desc_map, desc2 = np.asarray(desc_map, F32), np.asarray(desc2, F32)
    cap = desc2.shape[0]
    n1, n2 = min(max(int(n_rows), 0), desc_map.shape[0]), min(max(int(count2), 0), cap)
    out = {"match": np.zeros((cap, 3), F32), "n_match": 0}
    if n1 == 0 or n2 == 0:
        return out
    assert W._sign_rows(desc_map[:n1]) and W._sign_rows(desc2[:n2]) and abs(desc_map[0, 0]) == abs(desc2[0, 0])
    cm, c2 = np.asarray(cls_map, np.uint8)[:n1], np.asarray(cls2, np.uint8)[:n2]
    dot32 = desc_map[:n1] @ desc2[:n2].T
    d32 = np.sqrt(F32(2) - F32(2) * np.clip(dot32, F32(-1), F32(1)))
    assert d32.dtype == F32
    cand = (cm[:, None] == c2[None, :]) & kept(cm, mask)[:, None]
    d = np.where(cand, d32, F32(np.inf))
    rb, cb = d.argmin(axis=1), d.argmin(axis=0)          # (the first index on ties; a line without a candidate is all inf)
    ar = np.arange(n1)
    keep = cand[ar, rb] & (d[ar, rb] < F32(thr)) & (cb[rb] == ar)
    k = int(keep.sum())
    out["match"][:k, 0], out["match"][:k, 1], out["match"][:k, 2] = ar[keep], rb[keep], d32[ar, rb][keep]
    out["n_match"] = k
    return out


# ---- the revisit with classes and aliases ----------------------------------------------------------------------------------------
N_CLASSES = 3
ALIAS_PAIRS = 4


def alias_sequence():
    """world_ref.revisit_sequence with a class per scene point (id % N_CLASSES; every 17th point unknown) and planted aliases: pairs
    of scene points (b, a) of different classes where a carries b's descriptor.  No frame of a is a frame of b or next to one, so the
    two never meet in a frame pair (the sequence's own matches stay those of its identities), and b has become a landmark before a
    first appears, so b's map row is the older one: the plain map matcher joins a's point with b's row by the first-index rule.  dict: the sequence plus
    "cls": per frame uint8 [n], "cls_of": per scene point, "aliases": [(b, a)]."""
    seq = dict(W.revisit_sequence())
    frames = len(seq["pts"])
    n_ids = seq["n_in"]
    vis = [set() for _ in range(n_ids)]
    for f in range(frames):
        for p in seq["ids"][f]:
            vis[int(p)].add(f)
    cls_of = (np.arange(n_ids) % N_CLASSES).astype(np.uint8)
    cls_of[::17] = CLASS_NONE
    aliases, used = [], set()
    for b in range(n_ids):
        if len(aliases) == ALIAS_PAIRS:
            break
        # b: of a known class, seen in its first three frames in a row (it becomes a landmark there)
        first = min(vis[b]) if vis[b] else 0
        if b in used or cls_of[b] == CLASS_NONE or not {first, first + 1, first + 2} <= vis[b]:
            continue
        for a in range(n_ids):
            if a in used or a == b or cls_of[a] in (CLASS_NONE, cls_of[b]) or len(vis[a]) < 3:
                continue
            # a first appears two frames or more after b's third, and no frame of a is a frame of b or next to one
            if min(vis[a]) >= first + 4 and all(abs(fa - fb) >= 2 for fa in vis[a] for fb in vis[b]):
                aliases.append((b, a))
                used.update((a, b))
                break
    assert len(aliases) == ALIAS_PAIRS, aliases
    desc = [np.array(d, dtype=F32, copy=True) for d in seq["desc"]]
    for b, a in aliases:
        src = next(desc[f][list(seq["ids"][f]).index(b)] for f in sorted(vis[b]))
        for f in vis[a]:
            desc[f][list(seq["ids"][f]).index(a)] = src
    seq["desc"] = desc
    seq["cls"] = [cls_of[np.asarray(i, dtype=np.int64)] for i in seq["ids"]]
    seq["cls_of"], seq["aliases"] = cls_of, aliases
    return seq


def run_sequence(seq, max_length, point_cap, seed0, world_classes=None, mask=FULL_MASK, world_cap=4096, tid_cap=1 << 16,
                 patience=W.PATIENCE, min_inliers=16, thresh=N.THRESH, abs_min_inliers=N.MIN_INLIERS,
                 landmark_params=(L.MIN_VIEWS, L.MIN_PARALLAX_DEG, L.MAX_REPROJ)):
    """world_ref.run_sequence(world_mode="observe") with the classes: what a PointTracker(geometric_check="fundamental", intrinsics,
    world_map="observe", world_classes=world_classes) computes over the frames of seq (seq["cls"]: the class of every point).
    world_classes None: the plain run; "observe": the votes are kept beside the insert; "match": the frame is matched against the
    map by match_world_classes under `mask`.  world_ref.run_sequence's keys, plus votes: the votes at the end, classes: per frame
    world_classes() after the frame, scene_of_tid: the scene point whose observation first carried each track id, wrong_joins: the
    match rows (frame, map row, frame row) that join a frame point with the map row of another scene point."""
    from tests import epipolar_ref as E
    from tests import tracks_ref as T
    way = W.WAY1
    dt = way[0]
    frames = len(seq["pts"])
    k = seq["intr"][0]
    tracks = T.Tracks(max_length)
    state = P.new_state(way)
    table = np.zeros((frames + 1, P.ROW_WORDS), dtype=dt)
    prev_pose = prev_match = None
    world = W.new_map(world_cap, tid_cap)
    votes = new_votes(tid_cap)
    out = {"world": [], "world_corr": [], "world_match": [], "states": [], "classes": [], "wrong_joins": []}
    scene_of_tid = {}
    mv, par, rep = landmark_params
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
        desc_new = np.zeros((point_cap, 256), dtype=F32)
        desc_new[:n_pts] = seq["desc"][f]
        cls_new = np.full(point_cap, CLASS_NONE, np.uint8)
        cls_new[:n_pts] = seq["cls"][f]
        n_rows = W.n_rows_of(world)
        if world_classes == "match":
            mw = match_world_classes(world["desc"], n_rows, map_classes(world, votes), desc_new, cls_new, n_pts, W.NN_THRESH, mask)
        else:
            mw = W.match_world(world["desc"], n_rows, desc_new, n_pts, W.NN_THRESH)
        for i, j, _ in mw["match"][:mw["n_match"]]:
            if scene_of_tid[int(world["tid"][int(i)])] != int(seq["ids"][f][int(j)]):
                out["wrong_joins"].append((f, int(i), int(j)))
        corr, (n, nv) = W.correspondences(world, mw["match"], mw["n_match"], pts_new, n_pts)
        wres = N.ransac(corr, n, k, seed0 + f, thresh, abs_min_inliers, way=way)
        out["world"].append(wres), out["world_corr"].append((corr, n, nv)), out["world_match"].append(mw)
        keep = r["mask"] if (r["status"] == 0 and r["n_inliers"] >= min_inliers) else np.ones(match.shape[0], dtype=bool)
        T.update(tracks, n_pts, match[keep].astype(np.float64).T.reshape(3, -1))
        if f >= 1:
            cams = L.map_window(f + 1, table, seq["intr"][:1], max_length, way=way)
            ring, first_slot = L.ring_of(seq, max_length, point_cap, frames=f + 1)
            rows = L.triangulate(tracks.ids, tracks.counts, ring, first_slot, cams, mv, L.cos_of(par), rep, way=way)
            lms = L.select(tracks.ids, tracks.tid, tracks.counts, point_cap, rows)
            W.insert(world, lms, lms.shape[0], desc_new, n_pts, np.asarray(table, dtype=np.float64), f + 1, patience)
            for row in lms:
                if 0 <= row[7] < n_pts:
                    scene_of_tid.setdefault(int(row[0]), int(seq["ids"][f][int(row[7])]))
            if world_classes is not None:
                vote(votes, lms, lms.shape[0], cls_new, n_pts)
        out["states"].append(world["state"].copy())
        out["classes"].append(map_classes(world, votes))
    out["table"], out["tracks"], out["map"], out["votes"] = np.asarray(table[:frames], dtype=np.float64), tracks, world, votes
    out["scene_of_tid"] = scene_of_tid
    return out


ALIAS_L, ALIAS_CAP, ALIAS_SEED0 = W.REVISIT_L, W.REVISIT_CAP, W.REVISIT_SEED0
ALIAS_DROP = (2,)            # the class the "match-drop" run keeps out of the map matcher


def mask_of(keep=None, drop=None, n_classes=N_CLASSES):
    """lib.class_mask, restated: eight 32-bit words, bit c of word c // 32 = class c is kept"""
    ids = set(keep) if keep is not None else set(range(n_classes)) - set(drop)
    words = [0] * 8
    for c in ids:
        words[c >> 5] |= 1 << (c & 31)
    return tuple(words)


@functools.lru_cache(maxsize=None)
def alias_runs():
    """(seq, {"plain", "observe", "match", "match-drop"}): computed once, read-only."""
    seq = alias_sequence()
    run = lambda mode, **kw: run_sequence(seq, ALIAS_L, ALIAS_CAP, ALIAS_SEED0, mode, **kw)
    return seq, {"plain": run(None), "observe": run("observe"), "match": run("match"),
                 "match-drop": run("match", mask=mask_of(drop=ALIAS_DROP))}
