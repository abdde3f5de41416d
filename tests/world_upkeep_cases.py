"""Inputs of the world map's upkeep (tests/world_upkeep_ref.py) shared by tests/test_world_upkeep_cpu.py and
tests/test_gpu_world_upkeep.py: hand-made maps, one per rule of each phase, and random maps with planted merges, culls and an
eviction at a given row count.  A case is a dict of world_upkeep_ref.upkeep's arguments: world (world_ref.new_map's dict), match,
n_match, landmarks, n_landmarks, pts_new, count_new, table, n_frames, k and params (the keyword arguments)."""
import numpy as np

from tests import landmarks_ref as L
from tests import pose_ref as P
from tests import world_ref as W

F = 9                  # the newest frame of every case
THRESH = 2.0
K = np.array([300.0, 300.0, 160.0, 120.0])
POINT_CAP, ROW_CAP, CAPACITY = 8, 12, 12
NO_PHASE = dict(merge=False, merge_thresh=THRESH, cull_age=-1, cull_min_views=3, high_water=-1, low_water=0)


def camera():
    """(Rw [9], C [3]) of frame F: a camera that is neither at the origin nor axis-aligned."""
    R = P._rodrigues(np.array([0.05, -0.2, 0.03]))
    return R.reshape(9), np.array([0.4, -0.1, 0.2])


def project(X):
    Rw, C = camera()
    Y = Rw.reshape(3, 3) @ (np.asarray(X, dtype=np.float64) - C)
    return np.array([K[0] * (Y[0] / Y[2]) + K[2], K[1] * (Y[1] / Y[2]) + K[3]])


def pose_table(capacity=CAPACITY, frame=F):
    table = np.zeros((capacity, P.ROW_WORDS))
    if frame < capacity:
        table[frame, 0:9], table[frame, 9:12] = camera()
    return table


def base_map(n_rows, map_cap, tid_cap=64, seed=0, last=None, views=None):
    """A map of n_rows rows in front of frame F's camera: track ids 10 + 2 slot, random descriptors, every row anchored."""
    rng = np.random.RandomState(seed)
    w = W.new_map(map_cap, tid_cap)
    Rw, C = camera()
    for i in range(n_rows):
        Y = np.array([rng.uniform(-1.5, 1.5), rng.uniform(-1.0, 1.0), rng.uniform(3.0, 9.0)])
        w["X"][i] = Rw.reshape(3, 3).T @ Y + C
    w["desc"][:n_rows] = rng.standard_normal((n_rows, 256)).astype(np.float32)
    w["tid"][:n_rows] = 10 + 2 * np.arange(n_rows)
    w["n_views"][:n_rows] = 4 if views is None else views
    w["first_frame"][:n_rows] = rng.randint(0, 3, n_rows)
    w["last_frame"][:n_rows] = F - 2 if last is None else last
    w["rms"][:n_rows] = rng.uniform(0.0, 0.5, n_rows)
    w["slot_of_tid"][w["tid"][:n_rows]] = np.arange(n_rows)
    w["state"][W.N_ROWS], w["state"][W.ANCHORED] = n_rows, 1
    return w


def _case(world, params, match=(), landmarks=(), pts=(), n_frames=F + 1, table=None):
    m = np.zeros((POINT_CAP, 3), np.float32)
    m[:len(match)] = np.asarray(match, np.float32).reshape(-1, 3)
    lm = np.zeros((ROW_CAP, L.LANDMARK_WORDS))
    lm[:len(landmarks)] = np.asarray(landmarks, np.float64).reshape(-1, L.LANDMARK_WORDS)
    p = np.zeros((POINT_CAP, 2))
    p[:len(pts)] = np.asarray(pts, np.float64).reshape(-1, 2)
    return dict(world=world, match=m, n_match=len(match), landmarks=lm, n_landmarks=len(landmarks), pts_new=p, count_new=len(pts),
                table=pose_table() if table is None else table, n_frames=n_frames, k=K.copy(), params=dict(NO_PHASE, **params))


def _merge_case(old, new, offset=(THRESH / 2, 0.0), edit=None, lm_edit=None):
    """Map row `old` was last seen at F - 3; row `new` was written by this frame's insert for the track of landmark row 1, whose
    newest observation is frame point 2; the frame's match rows name (old, 2).  The point lies `offset` pixels from X[old]'s
    reprojection.  edit(world), lm_edit(landmark rows): what a refusal case changes."""
    w = base_map(6, 8, last=F - 3)
    w["last_frame"][new], w["n_views"][new], w["first_frame"][new] = F, 2, F - 1
    w["first_frame"][old] = 1
    lms = np.zeros((3, L.LANDMARK_WORDS))
    for q, slot in enumerate((3, new, 5)):      # rows 0 and 2 belong to other tracks: row 0 has no point in the frame
        lms[q] = [w["tid"][slot], *w["X"][slot], w["n_views"][slot], w["rms"][slot], 0.9, (-1, 2, 0)[q]]
    w["last_frame"][5] = F
    pts = np.zeros((4, 2))
    pts[0], pts[1], pts[3] = project(w["X"][5]), (10.0, 10.0), (300.0, 200.0)
    pts[2] = project(w["X"][old]) + np.asarray(offset)
    if edit is not None:
        edit(w)
    if lm_edit is not None:
        lm_edit(lms)
    return _case(w, dict(merge=True), match=[(old, 2, 0.25)], landmarks=lms, pts=pts)


def _behind(w):
    Rw, C = camera()
    w["X"][1] = Rw.reshape(3, 3).T @ np.array([0.2, 0.1, -4.0]) + C


def _stale_slot(w):
    w["slot_of_tid"][w["tid"][4]] = 7      # past n_rows: the returning track is not in the map (a full map dropped it)


def _lm(word, value):
    def edit(lms):
        lms[1, word] = value
    return edit


def _evict_case(n_rows, high, low, protected=(), views=None, last=None, map_cap=None):
    w = base_map(n_rows, map_cap or n_rows + 2, views=views, last=last)
    for i in protected:
        w["last_frame"][i] = F
    return _case(w, dict(high_water=high, low_water=low))


def _mixed():
    """Every phase at once: a merge that keeps the old slot, two culled rows, an eviction that wants one row more than it may take."""
    c = _merge_case(1, 4)
    w = c["world"]
    w["n_views"][0], w["last_frame"][0] = 2, F - 5
    w["n_views"][2], w["last_frame"][2] = 1, 0
    c["params"].update(cull_age=3, cull_min_views=3, high_water=2, low_water=0)
    return c


HAND_MADE = {
    # merge
    "merge_survivor_is_r": lambda: _merge_case(1, 4),
    "merge_survivor_is_r2": lambda: _merge_case(4, 1),
    "merge_half_thresh": lambda: _merge_case(1, 4, offset=(0.6 * THRESH / 2, -0.8 * THRESH / 2)),
    "merge_refused_twice_thresh": lambda: _merge_case(1, 4, offset=(0.0, 2 * THRESH)),
    "merge_refused_no_slot": lambda: _merge_case(1, 4, edit=_stale_slot),
    "merge_refused_same_row": lambda: _merge_case(4, 4),
    "merge_refused_r_written": lambda: _merge_case(1, 4, edit=lambda w: w["last_frame"].__setitem__(1, F)),
    "merge_refused_r2_old": lambda: _merge_case(1, 4, edit=lambda w: w["last_frame"].__setitem__(4, F - 1)),
    "merge_refused_behind": lambda: _merge_case(1, 4, edit=_behind),
    "merge_refused_landmark_not_finite": lambda: _merge_case(1, 4, lm_edit=_lm(2, np.inf)),
    "merge_refused_landmark_tid": lambda: _merge_case(1, 4, lm_edit=_lm(0, 64.0)),
    "merge_off": lambda: dict(_merge_case(1, 4), params=dict(NO_PHASE)),
    # cull: rows 0..3 at the age boundary and one frame older, with too few views and with enough
    "cull_age_boundary": lambda: _case(base_map(5, 8, last=[F - 3, F - 4, F - 4, F - 9, F], views=[2, 2, 3, 2, 1]),
                                       dict(cull_age=3, cull_min_views=3)),
    "cull_views_boundary": lambda: _case(base_map(4, 4, last=0, views=[2, 3, 4, 0]), dict(cull_age=0, cull_min_views=3)),
    "cull_age_zero": lambda: _case(base_map(3, 8, last=[F, F - 1, F - 2], views=1), dict(cull_age=0, cull_min_views=2)),
    # evict
    "evict_at_high_water": lambda: _evict_case(6, 6, 2),
    "evict_above_high_water": lambda: _evict_case(7, 6, 4, views=[5, 2, 9, 2, 3, 300, 2], last=[1, 4, 1, 2, 0, 0, F - 1]),
    "evict_none_unprotected": lambda: _evict_case(5, 3, 1, protected=range(5)),
    "evict_all_unprotected": lambda: _evict_case(7, 5, 1, protected=(0, 3, 6)),
    "evict_ties_by_slot": lambda: _evict_case(8, 7, 5, views=3, last=4, map_cap=8),
    "evict_to_empty": lambda: _evict_case(4, 0, 0),
    # compact and the call's conditions
    "nothing_dies": lambda: _case(base_map(6, 8), dict(merge=True, cull_age=3, high_water=7, low_water=6)),
    "everything_dies": lambda: _case(base_map(6, 6, last=1, views=1), dict(cull_age=2, cull_min_views=2)),
    "mixed": _mixed,
    "not_anchored": lambda: _case(base_map(6, 8, last=0, views=1), dict(merge=True, cull_age=0, high_water=0)),   # (see hand_made)
    "no_rows": lambda: _case(base_map(0, 8), dict(cull_age=0, high_water=0)),
    "no_table_row": lambda: _case(base_map(6, 8, last=0, views=1), dict(cull_age=0), n_frames=CAPACITY + 1),
}


def hand_made(name):
    c = HAND_MADE[name]()
    if name == "not_anchored":
        c["world"]["state"][W.ANCHORED] = 0
    return c


def random_case(seed, n_rows, map_cap, n_merge=None, dying=0.1, point_cap=None):
    """A map of n_rows rows at frame F = 40: about a tenth of the rows were written by this frame's insert, min(n_merge, ...) of
    them return an older row's scene point (half within THRESH / 2 of its reprojection, half about 2 THRESH away), a share `dying`
    of the older rows has two views and an age past cull_age, and the eviction takes a sixteenth of what is left."""
    rng = np.random.RandomState(seed)
    f = 40
    Rw, C = camera()
    R = Rw.reshape(3, 3)
    w = W.new_map(map_cap, tid_cap=1 << 17)
    Y = np.stack([rng.uniform(-1.5, 1.5, n_rows), rng.uniform(-1.0, 1.0, n_rows), rng.uniform(3.0, 9.0, n_rows)], axis=1)
    w["X"][:n_rows] = Y @ R + C
    w["desc"][:n_rows] = rng.standard_normal((n_rows, 256)).astype(np.float32)
    tids = rng.permutation(1 << 17)[:n_rows].astype(np.int32)
    new = rng.rand(n_rows) < 0.1
    if n_rows <= 2:
        new[:] = False
    last = np.where(new, f, rng.randint(f - 12, f, n_rows))
    views = rng.randint(3, 9, n_rows)
    weak = ~new & (rng.rand(n_rows) < dying)
    views[weak], last[weak] = 2, rng.randint(0, f - 12, int(weak.sum()))
    w["tid"][:n_rows], w["n_views"][:n_rows], w["last_frame"][:n_rows] = tids, views, last
    w["first_frame"][:n_rows] = np.minimum(last, rng.randint(0, f, n_rows))
    w["rms"][:n_rows] = rng.uniform(0.0, 0.5, n_rows)
    w["slot_of_tid"][tids] = np.arange(n_rows)
    w["state"][W.N_ROWS], w["state"][W.ANCHORED] = n_rows, 1
    new_rows, old_rows = np.nonzero(new)[0], np.nonzero(~new)[0]
    point_cap = point_cap or int(min(max(len(new_rows), 4), 4096))
    n_pts = min(len(new_rows), point_cap)
    n_merge = min(n_pts, len(old_rows), 64 if n_merge is None else n_merge)
    olds = np.sort(rng.choice(old_rows, n_merge, replace=False)) if n_merge else np.zeros(0, np.int64)
    points = rng.permutation(n_pts)
    pts = np.stack([rng.uniform(4, 316, point_cap), rng.uniform(4, 236, point_cap)], axis=1)
    lms = np.zeros((max(n_pts, 1), L.LANDMARK_WORDS))
    for q in range(n_pts):          # landmark row q is the track of map row new_rows[q], seen at frame point points[q]
        s = new_rows[q]
        lms[q] = [tids[s], *w["X"][s], views[s], w["rms"][s], 0.9, points[q]]
    match = np.zeros((point_cap, 3), np.float32)
    for m, r in enumerate(olds):    # ascending map row; match row m names the point of landmark row m
        Yr = R @ (w["X"][r] - C)
        b = np.array([K[0] * Yr[0] / Yr[2] + K[2], K[1] * Yr[1] / Yr[2] + K[3]])
        pts[points[m]] = b + (np.array([0.3, -0.4]) * THRESH if m % 2 == 0 else np.array([2 * THRESH, 0.5]))
        match[m] = (r, points[m], 0.0)
    table = np.zeros((f + 2, P.ROW_WORDS))
    table[f, 0:9], table[f, 9:12] = Rw, C
    alive = n_rows - int(weak.sum()) - (n_merge + 1) // 2
    low = max(alive - max(alive // 16, 1), 0)
    params = dict(merge=True, merge_thresh=THRESH, cull_age=12, cull_min_views=3, high_water=min(max(alive - 1, 0), map_cap),
                  low_water=min(low, max(alive - 1, 0)))
    return dict(world=w, match=match, n_match=n_merge, landmarks=lms, n_landmarks=n_pts, pts_new=pts, count_new=n_pts, table=table,
                n_frames=f + 1, k=K.copy(), params=params)


def run_ref(case):
    """world_upkeep_ref.upkeep on a copy of the case's map: (the map after the call, report, info)."""
    from tests import world_upkeep_ref as U
    w = W.copy_map(case["world"])
    report, info = U.upkeep(w, case["match"], case["n_match"], case["landmarks"], case["n_landmarks"], case["pts_new"], case["count_new"],
                            case["table"], case["n_frames"], case["k"], **case["params"])
    return w, report, info
