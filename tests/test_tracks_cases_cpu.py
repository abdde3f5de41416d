"""The generated track sequences (tests/tracks_cases.py) are what they claim, without a GPU: every case
prints and asserts the edge classes of the device layout it reaches, the decoy launches hold what they say, the hand-made tables
do overflow, and the clamping wrapper changes nothing on the recorded G19 sequences."""
import numpy as np
import pytest

from tests import golden_util as G
from tests import tracks_cases as TC
from tests import tracks_ref as TR
from tests.golden_tracks import GET_TRACKS_M, SEQUENCES


def _classes(name, **kw):
    c = TC.CASES[name]
    row_cap = c["L"] * c["point_cap"]
    before, per_frame = TR.Tracks(c["L"]), []
    for t in TC.expected(name, **kw):
        per_frame.append(TC.edge_classes(before, t, row_cap))
        before = t
    return per_frame


def _summary(name, per_frame):
    new_blocks = sorted(set(b for e in per_frame for b in e["new_blocks"]))
    lost = sorted(set(b for e in per_frame for b in e["old_lost"]))
    held = sorted(set(b for e in per_frame for b in e["old_held"]))
    most = max(per_frame, key=lambda e: len(e["old_lost"]))
    s = dict(new_blocks=new_blocks, gap=max(e["gap"] for e in per_frame), old_lost=lost, old_held=held,
             full=[f for f, e in enumerate(per_frame) if e["full"]], old_lost_at_once=most["old_lost"])
    print("%-7s new rows start in new-point blocks %s; largest kept_old != base gap %d; n_rows == row_cap at frames %s; old blocks "
          "that lose a row %s of the blocks that held one %s (at once: %s)"
          % (name, s["new_blocks"], s["gap"], s["full"], s["old_lost"], s["old_held"], s["old_lost_at_once"]))
    return s


def test_sequences_are_mutual_and_shuffled():
    for name, c in TC.CASES.items():
        prev = 0
        for (n, m), want in zip(TC.sequence(name), c["counts"]):
            assert n == want and m.shape[0] == 3
            i, j = m[0].astype(int), m[1].astype(int)
            assert len(set(i)) == len(i) and len(set(j)) == len(j)                  # mutual: no i and no j twice
            assert (i >= 0).all() and (i < max(prev, 1)).all() and (j >= 0).all() and (j < max(n, 1)).all()
            if len(i) > 8:
                assert (np.diff(i) < 0).any() and (np.diff(j) < 0).any()            # shuffled row order
                assert (m[2].astype(np.float32).astype(np.float64) != m[2]).all()   # the float32 column is another number
            prev = n
        assert len(TC.sequence(name)) == len(c["counts"]) == len(c["keep"])


def test_blocks_reaches_every_new_point_block_and_prunes_old_blocks():
    per_frame = _classes("blocks")
    s = _summary("blocks", per_frame)
    assert TC.CASES["blocks"]["point_cap"] == 3 * TC.BLOCK - 768 and -(-TC.CASES["blocks"]["point_cap"] // TC.BLOCK) == 3
    assert s["new_blocks"] == [0, 1, 2]                    # a new row starts in the second and in the third new-point block
    assert s["gap"] >= 2 * TC.BLOCK                        # kept_old != base, by two whole blocks of new rows
    first = min(f for f, e in enumerate(per_frame) if e["gap"] > 0)
    assert per_frame[first]["new_blocks"] == [0, 1] and first == 3
    # Rows die where the oldest retained frame's rows stand: a prefix of the table of at most 2049 rows here (no frame older than
    # the last three has 2304 points), so old blocks 0, 1 and 2 are every old block in which a row can be pruned.  All three lose
    # rows at once (frame 7), and at frame 6 the first two lose some rows and keep others, with live rows behind them.
    assert s["old_lost"] == [0, 1, 2] and s["old_lost_at_once"] == [0, 1, 2]
    assert per_frame[6]["old_lost"] == [0, 1] and per_frame[6]["old_held"] == [0, 1, 2]
    assert s["old_held"] == [0, 1, 2, 3, 4]
    shares = set(TC.CASES["blocks"]["keep"])
    assert shares == {0, 1, 0.6}
    assert TC.sequence("blocks")[1][1].shape[1] == 1023    # share 1: every point of the previous frame continues


@pytest.mark.parametrize("name", ["full2", "full3"])
def test_full_fills_the_table_and_then_prunes(name):
    c = TC.CASES[name]
    per_frame = _classes(name)
    s = _summary(name, per_frame)
    ts = TC.expected(name)
    assert s["full"] == [c["L"] - 1, c["L"]] and ts[c["L"] - 1].ids.shape[0] == c["L"] * c["point_cap"]
    assert ts[-1].ids.shape[0] < ts[-2].ids.shape[0] and per_frame[-1]["old_lost"]   # the last frame prunes
    assert s["new_blocks"] == [0, 1] and s["gap"] == TC.BLOCK


def test_long_rows_live_sixteen_columns():
    c = TC.CASES["long"]
    s = _summary("long", _classes("long"))
    ts = TC.expected("long")
    assert c["L"] == TC.MAX_LENGTH == 16 and len(ts) == 20 and min(c["counts"]) == 700 and max(c["counts"]) == c["point_cap"] == 1025
    assert ((ts[-1].ids != -1).sum(axis=1) == 16).any()        # a track seen in all 16 retained frames
    assert (ts[-1].ids < -1).sum() == 0 and ts[-1].track_count > ts[-1].ids.shape[0]
    assert s["new_blocks"] == [0, 1] and s["old_lost"] and len(s["old_held"]) >= 3


def test_short_empty_frame_cuts_every_track():
    ts = TC.expected("short")
    _summary("short", _classes("short"))
    assert [t.ids.shape[0] for t in ts[:3]] == [300, 300, 300] and list(ts[1].counts) == [300, 0]
    assert TC.select(ts[1], 1).shape[0] == 0 and TC.select(ts[2], 2).shape[0] == 0 and TC.select(ts[3], 2).shape[0] == 210
    assert ts[2].tid.min() == 300                              # frame 0's tracks are gone, none continued


def test_decoy_launches_hold_what_they_claim():
    c = TC.CASES["decoys"]
    cap = c["point_cap"]
    plain, dec = TC.launches("decoys"), TC.launches("decoys", decoys=True)
    _summary("decoys", _classes("decoys", decoys=True))
    prev = 0
    for f, (a, b) in enumerate(zip(plain, dec)):
        n = c["counts"][f]
        head = b["rows"][:a["used"] + 4].astype(np.float64)
        for bad in ([-1, 0], [prev, 1], [0, n], [1, cap]):                          # the four matches outside their frames
            assert (head[:, :2] == bad).all(axis=1).sum() == 1, (f, bad)
        tail = b["rows"][a["used"] + 4:].astype(int)
        tail = tail[tail[:, 0] >= 0]
        if f not in (0, TC.DECOY_UNDER, TC.DECOY_UNDER + 1):
            assert len(tail) > 0
        every = np.concatenate([TC.sequence("decoys")[f][1][:2].T.astype(int), tail[:, :2]])
        assert len(set(every[:, 0])) == len(every) == len(set(every[:, 1]))        # valid-looking: mutual with the true matches
        assert (tail[:, 0] < prev).all() and (tail[:, 1] < n).all()
        prev = n
    assert (dec[TC.DECOY_OVER]["n_match"], dec[TC.DECOY_OVER]["n_points"]) == (cap + 7, cap + 7)
    assert (dec[TC.DECOY_UNDER]["n_match"], dec[TC.DECOY_UNDER]["n_points"]) == (-3, -3)
    # the decoys change the expected tables only where the clamp turns them into matches (frame DECOY_OVER reads every row)
    for f, (a, b) in enumerate(zip(TC.expected("decoys"), TC.expected("decoys", decoys=True))):
        same = np.array_equal(a.matrix(), b.matrix())
        assert same == (f < TC.DECOY_OVER), f
    assert not np.array_equal(TC.expected("decoys", decoys=True, score64=False)[-1].score, TC.expected("decoys", decoys=True)[-1].score)


def test_hand_made_tables_overflow_and_clamp():
    t, state, la, cap, row_cap = TC.overfull()
    before = TC.snapshot(t)
    TC.clamped_update(t, la["rows"], la["s64"], la["n_match"], la["n_points"], cap, row_cap)
    assert t.ids.shape[0] == row_cap == 80 and t.track_count == before.track_count + 25      # 25 rows dropped, all counted
    assert np.array_equal(t.tid, before.tid) and (t.ids[:, 0] >= 0).all() and list(t.counts) == [cap, 25]
    assert (state[[0, 2, 3]] > [row_cap, cap, cap]).all()
    _, empty, state, la, cap, row_cap = TC.negative_state()
    TC.clamped_update(empty, la["rows"], la["s64"], la["n_match"], la["n_points"], cap, row_cap)
    assert list(TC.state_of(empty)) == [25, 32, 0, 25] and (state[[0, 2, 3]] < 0).all()


def test_track_points_restatement_and_the_edited_matrix():
    for name in ("blocks", "short"):
        c = TC.CASES[name]
        t = TC.expected(name)[-1]
        for first in range(c["L"]):
            ring = TC.ring(name, first)
            all_pts = [ring[(first + k) % c["L"], :t.counts[k]].T for k in range(c["L"])]
            want = TR.track_points(t.matrix(), all_pts)
            assert np.array_equal(TC.track_points_expected(t.matrix(), ring, t.counts, first, c["point_cap"]), want, equal_nan=True)
        m, edits = TC.edited_tracks(t)
        xy = TC.track_points_expected(m, ring, t.counts, first, c["point_cap"])
        for r, col in edits:
            assert np.isnan(xy[r, col]).all() and m[r, 2 + col] != -1.0


@pytest.mark.parametrize("name", sorted(SEQUENCES))
def test_wrapper_changes_nothing_on_the_recorded_sequences(name):
    """tracks_ref through clamped_update, at the capacity the GPU test gives the recorded sequences, still gives the golden tables."""
    g19 = G.load("g19_tracks.npz")
    spec = SEQUENCES[name]
    L, cap = spec["max_length"], max(spec["counts"])
    t = TR.Tracks(L)
    for f, n in enumerate(spec["counts"]):
        key = "%s/%d/" % (name, f)
        m = g19[key + "matches"]
        rows = np.full((cap, 3), -1.0)
        rows[:m.shape[1]] = m.T
        TC.clamped_update(t, rows, None, m.shape[1], n, cap, L * cap)
        assert np.array_equal(t.matrix(), g19[key + "tracks"]), key
        assert list(TC.state_of(t)) == [g19[key + "tracks"].shape[0], int(g19[key + "track_count"])] + ([0] * L + list(spec["counts"][:f + 1]))[-L:]
        for q in GET_TRACKS_M(L):
            assert np.array_equal(TC.select(t, q), g19[key + "gt%d" % q]), (key, q)
