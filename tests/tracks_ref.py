"""Numpy restatement of the track bookkeeping rules of DESIGN.md section 17 (PointTracker.update / get_tracks), written from
the rules: integer id columns, an fp64 score column, one dictionary lookup per match.  The tests and bench_tracks.py use it
where the reference is not at hand; tests/test_tracks_cpu.py pins it to the tables the reference itself produced
(tests/golden/g19_tracks.npz)."""
import numpy as np

NO_SCORE = 9999.0


class Tracks:
    """The table of a tracker of `max_length` frames: ids int64 [M, L], tid int64 [M], score float64 [M], the point counts
    of the L retained frames (oldest first) and the running track count."""

    def __init__(self, max_length):
        self.L = int(max_length)
        self.ids = np.zeros((0, self.L), np.int64)
        self.tid = np.zeros(0, np.int64)
        self.score = np.zeros(0, np.float64)
        self.counts = [0] * self.L
        self.track_count = 0

    def matrix(self):
        """float64 [M, 2 + L] rows (track id, score, ids): the layout of the reference's `tracks`."""
        return np.concatenate([self.tid[:, None].astype(np.float64), self.score[:, None], self.ids.astype(np.float64)], axis=1)


def update(t, n_points, matches):
    """One frame of n_points points; matches: [3, K] (index in the previous frame, index in the new frame, distance)."""
    L = t.L
    remove_size = t.counts[0]
    t.counts = t.counts[1:] + [int(n_points)]
    first_prev = sum(t.counts[:L - 2])            # id of point 0 of the previous frame
    first_new = first_prev + t.counts[L - 2]      # id of point 0 of the new frame
    ids = np.maximum(t.ids[:, 1:] - remove_size, -1)
    ids = np.concatenate([ids, np.full((ids.shape[0], 1), -1, np.int64)], axis=1)
    row_of_id = {int(v): r for r, v in enumerate(ids[:, L - 2]) if v >= 0}
    matched = np.zeros(int(n_points), bool)
    for i, j, d in np.asarray(matches, np.float64).T:
        r = row_of_id.get(int(i) + first_prev)
        if r is None:
            continue
        ids[r, L - 1] = int(j) + first_new
        matched[int(j)] = True
        if t.score[r] == NO_SCORE:
            t.score[r] = d
        else:
            frac = 1.0 / (float(np.count_nonzero(ids[r] != -1)) - 1.0)
            t.score[r] = (1.0 - frac) * t.score[r] + frac * d
    fresh = np.flatnonzero(~matched)
    new_ids = np.full((len(fresh), L), -1, np.int64)
    new_ids[:, L - 1] = fresh + first_new
    ids = np.concatenate([ids, new_ids])
    tid = np.concatenate([t.tid, t.track_count + np.arange(len(fresh), dtype=np.int64)])
    score = np.concatenate([t.score, np.full(len(fresh), NO_SCORE)])
    t.track_count += len(fresh)
    alive = (ids >= 0).any(axis=1)
    t.ids, t.tid, t.score = ids[alive], tid[alive], score[alive]
    return t


def get_tracks(t, min_length):
    if min_length < 1:
        raise ValueError("'min_length' too small.")
    keep = ((t.ids != -1).sum(axis=1) >= min_length) & (t.ids[:, t.L - 1] != -1)
    return t.matrix()[keep]


def track_points(tracks, all_pts):
    """[M, L, 2] coordinates of a tracks matrix [M, 2 + L] in the retained frames all_pts (list of [>= 2, N] arrays, oldest
    first); NaN where the id is -1."""
    L = len(all_pts)
    out = np.full((tracks.shape[0], L, 2), np.nan)
    first = 0
    for c, p in enumerate(all_pts):
        col = tracks[:, 2 + c].astype(np.int64)
        has = col != -1
        out[has, c] = np.asarray(p)[:2, col[has] - first].T
        first += p.shape[1]
    return out
