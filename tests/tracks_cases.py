"""Generated sequences for the track operators and the launches built from them: what
tests/test_tracks_cases_cpu.py shows to be what it claims and tests/test_gpu_tracks_exact.py runs on the device.

A sequence is, per frame, a point count, a set of mutual matches against the previous frame (no i and no j twice) in shuffled row
order, and fp64 scores with all their mantissa bits; column 2 of the float32 rows holds the rounded score, so the two score paths
of ssp_op_track_update give different bits.  The expected tables come from tests/tracks_ref.py.  Four rules of
csrc/track_kernels.hip.h are not in tracks_ref (the reference has no capacities): they are restated here, each beside the header's
sentence, in `clamped_update` and `track_points_expected`.  Nothing in this file needs a device."""
import functools

import numpy as np

from tests import tracks_ref as TR

BLOCK = 1024            # TRACK_BLOCK
MAX_LENGTH = 16         # SSP_TRACK_MAX_LENGTH

# name -> max_length, point_cap, seed, points per frame, share of the previous frame's points that continue
CASES = {
    # three blocks of new points; shares 0, 1 (every point of the previous frame matched) and 0.6
    "blocks": dict(L=3, point_cap=2304, seed=4101, counts=(1023, 1024, 1025, 2048, 2049, 0, 2304, 1, 2304),
                   keep=(0, 1, 0.6, 0.6, 0.6, 0, 0, 1, 0.6)),
    # no match for L frames of point_cap points: the table holds exactly row_cap rows; then a frame that prunes
    "full2": dict(L=2, point_cap=1100, seed=4102, counts=(1100, 1100, 1100, 700), keep=(0, 0, 0, 0.5)),
    "full3": dict(L=3, point_cap=1100, seed=4103, counts=(1100, 1100, 1100, 1100, 700), keep=(0, 0, 0, 0, 0.5)),
    # rows live 16 columns and the shift drops real ids
    "long": dict(L=MAX_LENGTH, point_cap=1025, seed=4104,
                 counts=(700, 1025, 881, 1024, 733, 990, 1025, 812, 768, 1001, 700, 955, 1023, 846, 1025, 790, 917, 1024, 705, 1025),
                 keep=(0,) + (0.8,) * 19),
    # the empty frame cuts every track
    "short": dict(L=2, point_cap=300, seed=4105, counts=(300, 0, 300, 300), keep=(0, 0, 0, 0.7)),
    # the sequence the decoy launches are built on (`launches(..., decoys=True)`)
    "decoys": dict(L=3, point_cap=300, seed=4106, counts=(200, 250, 220, 260, 300, 240, 0, 230, 210), keep=(0, 0.6, 0.7, 0.5, 0.6, 0.6, 0, 0, 0.6)),
}
DECOY_OVER, DECOY_UNDER = 4, 6   # frames of "decoys" whose n_match and n_points are point_cap + 7 / -3


@functools.lru_cache(maxsize=None)
def sequence(name):
    """[(n, match float64 [3, K])] of case `name`: rows (i, j, score) of the mutual matches, shuffled."""
    c = CASES[name]
    rs = np.random.RandomState(c["seed"])
    frames, prev = [], 0
    for n, keep in zip(c["counts"], c["keep"]):
        k = min(int(round(keep * prev)), n)
        m = np.stack([rs.permutation(prev)[:k].astype(np.float64), rs.permutation(n)[:k].astype(np.float64),
                      rs.uniform(0.05, 0.5, k) * (1.0 + rs.uniform(-1e-9, 1e-9, k))])
        frames.append((n, m[:, rs.permutation(k)]))
        prev = n
    return frames


def launches(name, point_cap=None, decoys=False):
    """One dict per frame: rows float32 [point_cap, 3], s64 float64 [point_cap], n_match, n_points (python ints) and `used`, the
    number of rows the kernel may read.  Rows past n_match hold i = j = -1 and NaN scores or, with decoys, valid-looking mutual matches
    of points no true match uses.  With decoys the rows before n_match also hold four matches outside their frames (i = -1, i = n_prev,
    j = n_new, j = point_cap), and frame DECOY_OVER / DECOY_UNDER gives both counts as point_cap + 7 / -3."""
    c = CASES[name]
    cap = c["point_cap"] if point_cap is None else point_cap
    assert cap >= c["point_cap"]
    rs = np.random.RandomState(c["seed"] + 1)
    out, prev = [], 0
    for f, (n, m) in enumerate(sequence(name)):
        k = m.shape[1]
        rows, s64 = np.full((cap, 3), -1.0, np.float32), np.full(cap, np.nan)   # (i = j = -1: a row that is no match)
        body = m
        if decoys:
            bad = np.array([[-1, 0, 0.1], [prev, 1, 0.2], [0, n, 0.3], [1, cap, 0.4]]).T
            body = np.concatenate([m, bad], axis=1)[:, rs.permutation(k + 4)]
            free_i, free_j = np.setdiff1d(np.arange(prev), m[0]), np.setdiff1d(np.arange(n), m[1])
            d = min(len(free_i), len(free_j), cap - k - 4)
            tail = np.stack([rs.permutation(free_i)[:d].astype(np.float64), rs.permutation(free_j)[:d].astype(np.float64),
                             rs.uniform(0.05, 0.5, d)])
            body = np.concatenate([body, tail], axis=1)
        used = k + (4 if decoys else 0)
        rows[:body.shape[1]] = body.T
        s64[:body.shape[1]] = body[2]
        n_match, n_points = used, n
        if decoys and f == DECOY_OVER:
            assert n == cap                         # the clamp gives the frame's true count; every row of the capacity is read
            n_match = n_points = cap + 7
            used = cap
        if decoys and f == DECOY_UNDER:
            assert n == 0
            n_match = n_points = -3
            used = 0
        out.append(dict(rows=rows, s64=s64, n_match=n_match, n_points=n_points, used=used))
        prev = n
    return out


def clamped_update(t, rows, s64, n_match, n_points, point_cap, row_cap):
    """tracks_ref.update behind the capacities of csrc/track_kernels.hip.h.  rows: [., 3] (i, j, distance); s64: the fp64 distances
    that replace column 2, or None.  Changes nothing when nothing needs clamping."""
    # "Every count a kernel reads from the device is clamped to its capacity first."
    n_new = min(max(int(n_points), 0), point_cap)
    nm = min(max(int(n_match), 0), point_cap)
    t.counts = [min(max(int(c), 0), point_cap) for c in t.counts]
    if t.ids.shape[0] > row_cap:
        t.ids, t.tid, t.score = t.ids[:row_cap], t.tid[:row_cap], t.score[:row_cap]
    # "match: [.][3] float rows (i, j, distance) ... with n_match rows": rows past n_match are not matches
    r = np.asarray(rows, np.float64)[:nm]
    i, j = np.trunc(r[:, 0]).astype(np.int64), np.trunc(r[:, 1]).astype(np.int64)
    d = r[:, 2] if s64 is None else np.asarray(s64, np.float64)[:nm]
    # track_match_kernel: "if (i < 0 || i >= t.n_prev || j < 0 || j >= n_new) return;": a match outside its frames is ignored
    ok = (i >= 0) & (i < t.counts[-1]) & (j >= 0) & (j < n_new)
    TR.update(t, n_new, np.stack([i[ok].astype(np.float64), j[ok].astype(np.float64), d[ok]]))
    # track_scatter_kernel: "if (keep && pos < row_cap)" and "state_out[1] = t.track_count + (rows - kept_old)": a row that does not
    # fit is dropped, and the track count advances all the same
    if t.ids.shape[0] > row_cap:
        t.ids, t.tid, t.score = t.ids[:row_cap], t.tid[:row_cap], t.score[:row_cap]
    return t


def state_of(t):
    return np.array([t.ids.shape[0], t.track_count] + list(t.counts), dtype=np.int32)


def snapshot(t):
    c = TR.Tracks(t.L)
    c.ids, c.tid, c.score, c.counts, c.track_count = t.ids.copy(), t.tid.copy(), t.score.copy(), list(t.counts), t.track_count
    return c


def select(t, min_length):
    """op_track_select: min_length == 0 is every row (track_row_selected), otherwise tracks_ref.get_tracks."""
    return t.matrix() if min_length == 0 else TR.get_tracks(t, min_length)


def min_lengths(L):
    return (0, 1, 2, L, L + 1)


@functools.lru_cache(maxsize=None)
def expected(name, decoys=False, score64=True):
    """[tracks_ref.Tracks] after every frame of the case's launches at its own capacity."""
    c = CASES[name]
    t, out = TR.Tracks(c["L"]), []
    for la in launches(name, decoys=decoys):
        clamped_update(t, la["rows"], la["s64"] if score64 else None, la["n_match"], la["n_points"], c["point_cap"], c["L"] * c["point_cap"])
        out.append(snapshot(t))
    return out


def edge_classes(before, after, row_cap):
    """What one update reached of the device's layout (blocks of BLOCK old rows, then blocks of BLOCK new points): `new_blocks`: the
    new-point blocks in which a new row starts; `gap`: the largest base - kept_old over those blocks, base being the output position
    at which the block starts; `old_lost`: the old blocks that lose a row; `old_held`: the old blocks that held one; `full`:
    n_rows == row_cap after the update."""
    alive = np.isin(before.tid, after.tid)
    fresh = after.tid >= before.track_count
    first_new = sum(after.counts[:-1])
    j = np.sort(after.ids[fresh, -1] - first_new)
    assert len(j) == after.track_count - before.track_count or after.ids.shape[0] == row_cap
    blocks = sorted(set((j // BLOCK).tolist()))
    gap = max([int((j < b * BLOCK).sum()) for b in blocks] + [0])
    return dict(new_blocks=blocks, gap=gap, old_lost=sorted(set((np.flatnonzero(~alive) // BLOCK).tolist())),
                old_held=sorted(set((np.arange(len(alive)) // BLOCK).tolist())), full=after.ids.shape[0] == row_cap)


# ---- hand-made tables: the clamps of track_counts and of the scatter at a table that cannot hold its rows -----------------------
def overfull():
    """(table before, device state, launch, point_cap, row_cap): L = 2, every row of the capacity alive because each point of the
    previous frame is named by two rows (no sequence gives that), and a state vector above every capacity; 25 unmatched points
    arrive.  All 25 rows are dropped, the track count advances by 25."""
    L, cap = 2, 40
    t = TR.Tracks(L)
    t.ids = np.stack([np.full(L * cap, -1), cap + np.arange(L * cap) % cap], axis=1).astype(np.int64)
    t.tid = 100 + 3 * np.arange(L * cap, dtype=np.int64)
    t.score = 0.25 + np.arange(L * cap) / 1024.0
    t.counts, t.track_count = [cap, cap], 1000
    state = np.array([L * cap + 5, 1000, cap + 9, cap + 7], dtype=np.int32)
    rows = np.full((cap, 3), -1.0, np.float32)
    return t, state, dict(rows=rows, s64=np.full(cap, np.nan), n_match=0, n_points=25, used=0), cap, L * cap


def negative_state():
    """As overfull, with a state vector below zero everywhere: the table reads as empty (the rows it holds are not rows)."""
    t, _, la, cap, row_cap = overfull()
    empty = TR.Tracks(2)
    empty.track_count = 7
    return t, empty, np.array([-2, 7, -5, -1], dtype=np.int32), la, cap, row_cap


# ---- op_track_points ---------------------------------------------------------------------------------------------------------
def ring(name, first_slot, point_cap=None):
    """float64 [L, point_cap, 2]: seeded coordinates, every slot filled to the capacity (a kernel that read past a frame's count
    would return a number, not NaN); retained frame c lives in slot (first_slot + c) % L."""
    c = CASES[name]
    cap = c["point_cap"] if point_cap is None else point_cap
    return np.random.RandomState(c["seed"] + 2 + first_slot).uniform(0.0, 640.0, (c["L"], cap, 2))


def track_points_expected(tracks, pts_ring, counts, first_slot, point_cap):
    """track_points_kernel: "xy [track_cap][L][2]: NaN where the id is -1 or does not name a point of its frame"."""
    L = pts_ring.shape[0]
    out = np.full((tracks.shape[0], L, 2), np.nan)
    off = 0
    for c in range(L):
        cnt = min(max(int(counts[c]), 0), point_cap)
        idv = tracks[:, 2 + c]
        ok = (idv >= 0.0) & (idv < 2147483647.0)
        k = np.where(ok, np.trunc(idv), 0).astype(np.int64) - off
        ok &= (k >= 0) & (k < cnt)
        out[ok, c] = pts_ring[(first_slot + c) % L, k[ok]]
        off += cnt
    return out


def edited_tracks(t):
    """The table's matrix with ids changed by hand so that they name no point of their frame: at its count, past it, below its first
    id, a negative id other than -1, and one no int32 holds.  Returns (matrix, the [row, column] pairs edited)."""
    m = t.matrix()
    L = t.L
    off = np.concatenate([[0], np.cumsum(t.counts)])
    assert m.shape[0] >= 8
    edits = []
    for r, (c, v) in enumerate(((L - 1, off[L]), (L - 1, off[L] + 5), (L - 2, off[L - 1]), (L - 1, off[L - 1] - 1), (0, -2.0), (1, -7.5),
                                (L - 1, 2147483648.0), (0, float(off[1])))):
        m[r, 2 + c] = float(v)
        edits.append((r, c))
    return m, edits
