"""The numpy restatement of the world map (tests/world_ref.py) checked on its own: the store through
hand-made cases, the anchor state machine over flag sequences, the repair rule (every case of section 27 and the world's own), the
matcher on sign descriptors (exact, with ties) and against readout_ref.match_two_way on random unit rows, and the restated tracker
on a blackout ("relocalise" against the truth) and on a revisit ("observe")."""
import numpy as np
import pytest

from tests import landmarks_ref as LR
from tests import pnp_ref as N
from tests import pose_ref as P
from tests import readout_ref as R
from tests import world_ref as W


def _lm(rows):
    out = np.zeros((len(rows), LR.LANDMARK_WORDS))
    for r, (t, p, x) in enumerate(rows):
        out[r] = [t, x, x + 0.5, x + 1.5, 3 + r % 4, 0.125 * r, 0.9, p]
    return out


def _table(flags):
    t = np.zeros((len(flags) + 1, P.ROW_WORDS))
    t[:len(flags), 14] = flags
    return t


CLEAN3 = [1, 1, 0]          # rows 0 and 1 always carry flag bits: the first insertion is frame 2 at the earliest


# ---- insert --------------------------------------------------------------------------------------------------------------------
def test_insert_append_update_stable_order():
    w = W.new_map(16, 64)
    desc = W.sign_descriptors(1, 8)
    W.insert(w, _lm([(5, 0, 1.0), (9, 3, 2.0), (2, 7, 3.0)]), 3, desc, 8, _table(CLEAN3), 3)
    assert w["state"].tolist() == [3, 1, 0, 0, 0, 0, 3, 0]
    assert w["tid"][:3].tolist() == [5, 9, 2]                      # landmark order, not track order
    assert [W.lookup(w, t) for t in (5, 9, 2, 3)] == [0, 1, 2, -1]
    assert np.array_equal(w["desc"][:3], desc[[0, 3, 7]]) and np.array_equal(w["X"][1], [2.0, 2.5, 3.5])
    assert w["first_frame"][:3].tolist() == [2, 2, 2] and w["last_frame"][:3].tolist() == [2, 2, 2]
    desc2 = W.sign_descriptors(2, 8)
    W.insert(w, _lm([(9, 1, 7.0), (11, 2, 8.0), (5, 5, 9.0)]), 3, desc2, 8, _table(CLEAN3 + [0]), 4)
    assert w["state"].tolist() == [4, 1, 0, 0, 0, 0, 1, 2]
    assert w["tid"][:4].tolist() == [5, 9, 2, 11]
    assert np.array_equal(w["desc"][:4], np.stack([desc2[5], desc2[1], desc[7], desc2[2]]))      # newest wins: a copy
    assert w["X"][:4, 0].tolist() == [9.0, 7.0, 3.0, 8.0]
    assert w["first_frame"][:4].tolist() == [2, 2, 2, 3] and w["last_frame"][:4].tolist() == [3, 3, 2, 3]
    assert w["n_views"][:2].tolist() == [5, 3] and w["rms"][:2].tolist() == [0.25, 0.0]


def test_insert_skips_and_drops():
    w = W.new_map(4, 16)
    desc = W.sign_descriptors(3, 8)
    lm = _lm([(5, -1, 1.0), (6, 8, 2.0), (7, 7, 3.0), (8, np.nan, 4.0), (9, 0, np.inf), (16, 1, 1.0), (400, 2, 1.0), (-2, 3, 1.0)])
    W.insert(w, lm, 8, desc, 8, _table(CLEAN3), 3)                 # p = -1, p = count, p NaN, X inf, tid >= tid_cap (twice), tid < 0
    assert w["state"].tolist() == [1, 1, 0, 0, 0, 2, 1, 0] and w["tid"][0] == 7
    W.insert(w, _lm([(t, t, float(t)) for t in range(6)]), 6, desc, 5, _table(CLEAN3 + [0]), 4)     # count 5: tid 5 has p = 5
    assert w["state"].tolist() == [4, 1, 0, 0, 2, 2, 3, 0]         # 5 new rows for 3 slots: two dropped and counted
    assert w["tid"].tolist() == [7, 0, 1, 2]
    assert W.lookup(w, 3) == -1 and W.lookup(w, 4) == -1
    W.insert(w, _lm([(3, 0, 1.0), (1, 1, 5.0)]), 2, desc, 8, _table(CLEAN3 + [0, 0]), 5)
    assert w["state"].tolist() == [4, 1, 0, 0, 3, 2, 0, 1] and w["X"][2, 0] == 5.0
    W.insert(w, lm, 1, desc, 8, _table(CLEAN3 + [0, 0, 0]), 6)     # n_landmarks = 1: the other rows are not read
    assert w["state"].tolist() == [4, 1, 0, 0, 3, 2, 0, 0]


def test_insert_stale_slot_after_clear():
    w = W.new_map(8, 32)
    desc = W.sign_descriptors(4, 8)
    W.insert(w, _lm([(5, 0, 1.0), (9, 3, 2.0)]), 2, desc, 8, _table(CLEAN3), 3)
    w["state"][W.N_ROWS] = 0                                       # cleared without a memset: slot_of_tid[9] still says 1
    W.insert(w, _lm([(9, 1, 4.0)]), 1, desc, 8, _table(CLEAN3 + [0]), 4)
    assert w["state"][W.N_ROWS] == 1 and w["tid"][0] == 9 and W.lookup(w, 9) == 0 and W.lookup(w, 5) == -1
    W.insert(w, _lm([(5, 2, 6.0)]), 1, desc, 8, _table(CLEAN3 + [0, 0]), 5)     # slot_of_tid[5] = 0 is stale: tid[0] == 9
    assert w["tid"][:2].tolist() == [9, 5] and w["state"][W.APPENDED] == 1 and w["state"][W.UPDATED] == 0


# ---- the anchor state machine ------------------------------------------------------------------------------------------------------
def _run_flags(flags, repaired=(), rows=1, patience=3):
    """state after each frame: (n_rows, anchored, lost, streak); repaired: the frames whose row the world repair wrote"""
    w = W.new_map(8, 8)
    w["state"][W.N_ROWS] = rows
    w["state"][W.ANCHORED] = 1 if rows else 0
    out = []
    for f, flag in enumerate(flags):
        w["state"][W.STREAK] = w["state"][W.STREAK] + 1 if f in repaired else 0     # (what repair() leaves)
        W.anchor(w, flag, patience)
        if w["state"][W.ANCHORED] and w["state"][W.N_ROWS] == 0:
            w["state"][W.N_ROWS] = 1                                # (the insertion)
        out.append(tuple(int(v) for v in w["state"][:4]))
    return out


def test_anchor_adoption_and_loss():
    assert _run_flags([1, 3, 0, 0], rows=0) == [(0, 0, 0, 0), (0, 0, 0, 0), (1, 1, 0, 0), (1, 1, 0, 0)]
    assert _run_flags([0, 2, 0, 0]) == [(1, 1, 0, 0), (1, 0, 1, 0), (1, 0, 2, 0), (1, 0, 3, 0)]      # a flagged row loses the anchor
    assert _run_flags([None, 0], rows=0) == [(0, 0, 0, 0), (1, 1, 0, 0)]                             # no such row counts as flagged
    assert _run_flags([4, 8, 16 | 4], rows=1) == [(1, 1, 0, 0)] * 3                                   # bits 2, 3, 4 do not matter


def test_anchor_needs_two_repaired_rows():
    got = _run_flags([1, 20, 0, 0], repaired=(1,))                  # one repaired row, then chained rows: never anchored again
    assert [g[1] for g in got] == [0, 0, 0, 0] and got[1][3] == 1 and got[2][3] == 0
    got = _run_flags([1, 20, 20, 0], repaired=(1, 2))
    assert [g[1] for g in got] == [0, 0, 1, 1] and got[2] == (1, 1, 0, 2)
    got = _run_flags([1, 20, 22, 20, 20], repaired=(1, 2, 3, 4))    # a repaired row that kept bit 1 is not ok
    assert [g[1] for g in got] == [0, 0, 0, 1, 1]


def test_anchor_patience_and_observe():
    got = _run_flags([1, 0, 0, 0, 0, 0], patience=3)                # "observe": no repair, so only patience brings the anchor back
    assert got == [(1, 0, 1, 0), (1, 0, 2, 0), (1, 0, 3, 0), (0, 0, 0, 0), (1, 1, 0, 0), (1, 1, 0, 0)]
    got = _run_flags([1, 1, 1, 1, 1, 0], patience=0)
    assert got[0] == (0, 0, 0, 0) and got[-1] == (1, 1, 0, 0)
    w = W.new_map(8, 8)
    w["state"][:] = [5, 0, 3, 1, 7, 9, 2, 2]
    W.anchor(w, 1, 3)                                               # the clear zeroes the counters
    assert w["state"].tolist() == [0, 0, 0, 0, 0, 0, 0, 0]


# ---- the repair ------------------------------------------------------------------------------------------------------------------
def _repair_inputs(flag, n=4, status=0, anchored=1, rows=10, streak=0):
    rng = np.random.RandomState(3)
    table = np.zeros((6, P.ROW_WORDS))
    for f in range(4):
        table[f, 0:9], table[f, 9:12], table[f, 12] = np.eye(3).reshape(9), rng.rand(3) * 0.1 * f, 0.1
    table[n - 1, 14] = flag
    st = np.zeros(P.STATE_WORDS)
    st[0], st[1], st[2:11] = n, 0.1, np.eye(3).reshape(9)
    w = W.new_map(16, 16)
    w["state"][:4] = [rows, anchored, 0, streak]
    a = {"Rw": P._rodrigues(np.array([3.0, -2.0, 1.0])), "C": np.array([0.3, -0.1, 0.05]), "status": status}
    return w, a, st, table


@pytest.mark.parametrize("flag", [1, 2, 3, 1 | 8])
def test_repair_is_section_27_on_flagged_rows(flag):
    """Where section 27's rule fires, the world's writes the same numbers and adds bit 4."""
    w, a, st, table = _repair_inputs(flag)
    s27, t27 = N.repair(a, st, table)
    s29, t29 = W.repair(w, a, st, table)
    assert np.array_equal(s27, s29)
    t27[3, 14] += W.FLAG_WORLD
    assert np.array_equal(t27, t29) and int(t29[3, 14]) == (N.FLAG_ABSOLUTE | W.FLAG_WORLD)
    assert w["state"][W.STREAK] == 1


def test_repair_short_step_keeps_scale_and_bit_1():
    w, a, st, table = _repair_inputs(2)
    a["C"] = table[2, 9:12] + 1e-4
    s29, t29 = W.repair(w, a, st, table)
    assert s29[1] == 0.1 and int(t29[3, 14]) == (2 | N.FLAG_ABSOLUTE | W.FLAG_WORLD)


def test_repair_firing_condition():
    w, a, st, table = _repair_inputs(0, streak=3)                   # clean row, anchored map: nothing written, streak zeroed
    s, t = W.repair(w, a, st, table)
    assert np.array_equal(s, st) and np.array_equal(t, table) and w["state"][W.STREAK] == 0
    w, a, st, table = _repair_inputs(0, anchored=0, streak=1)       # clean row rewritten while lost
    s, t = W.repair(w, a, st, table)
    assert int(t[3, 14]) == (N.FLAG_ABSOLUTE | W.FLAG_WORLD) and np.array_equal(t[3, 9:12], a["C"]) and w["state"][W.STREAK] == 2
    assert s[1] == np.sqrt(np.sum((a["C"] - table[2, 9:12]) ** 2)) or abs(s[1] - np.linalg.norm(a["C"] - table[2, 9:12])) < 1e-15
    w, a, st, table = _repair_inputs(0, anchored=0, rows=0)         # an empty map is not lost
    s, t = W.repair(w, a, st, table)
    assert np.array_equal(t, table)
    w, a, st, table = _repair_inputs(1, status=1, streak=2)         # nothing written under status 1
    s, t = W.repair(w, a, st, table)
    assert np.array_equal(s, st) and np.array_equal(t, table) and w["state"][W.STREAK] == 0
    w, a, st, table = _repair_inputs(1)
    a["Rw"][0, 0] = np.inf
    s, t = W.repair(w, a, st, table)
    assert np.array_equal(t, table)
    w, a, st, table = _repair_inputs(1)
    st[0] = 6                                                      # a full table is left alone
    s, t = W.repair(w, a, st, table)
    assert np.array_equal(t, table) and w["state"][W.STREAK] == 0
    w, a, st, table = _repair_inputs(1, n=1)                        # the first row: no previous centre, s is kept
    s, t = W.repair(w, a, st, table)
    assert s[1] == 0.1 and int(t[0, 14]) == (N.FLAG_ABSOLUTE | W.FLAG_WORLD)


# ---- the join ----------------------------------------------------------------------------------------------------------------
def test_correspondences():
    w = W.new_map(8, 8)
    w["X"][:4] = np.arange(12.0).reshape(4, 3)
    w["X"][2, 1] = np.nan
    w["state"][W.N_ROWS] = 4
    match = np.array([[0, 1, .1], [1, 5, .2], [2, 0, .3], [4, 2, .4], [3, 2, .5], [3, 3, .6]], np.float32)
    pts = np.arange(12.0).reshape(6, 2) + 100
    corr, (n, nv) = W.correspondences(w, match, 5, pts, 5)
    assert (n, nv) == (5, 2)                                        # frame point 5 >= count, NaN landmark, map row 4 >= n_rows, past n_match
    assert corr[0].tolist() == [0, 1, 2, 102, 103, 0, 1, 0] and corr[4].tolist() == [9, 10, 11, 104, 105, 3, 1, 0]
    assert not corr[[1, 2, 3, 5]].any()


# ---- the matcher -----------------------------------------------------------------------------------------------------------------
def test_matcher_sign_descriptors_exact_with_ties():
    n1, n2 = 2000, 800
    d1, d2 = W.sign_descriptors(1, n1), W.sign_descriptors(2, n2)
    d2[:100] = d1[200:300]
    d1[650] = d1[210]                                               # a later copy of a matched map row: the first index wins
    d2[290] = d2[20]                                                # and a later copy of a matched frame row
    res = W.match_world(d1, n1, d2, n2, 0.7)
    assert not res["amb_rows"].any()
    # in exact integers: 256 dot = 2 (agreeing signs) - 256
    s1, s2 = (d1 > 0).astype(np.int64), (d2 > 0).astype(np.int64)
    agree = s1 @ s2.T + (1 - s1) @ (1 - s2).T
    dot = (2 * agree - 256) / 256.0
    d32 = np.sqrt(np.float32(2) - np.float32(2) * dot.astype(np.float32))
    ties = int(((d32 == d32.min(axis=1, keepdims=True)).sum(axis=1) > 1).sum() + ((d32 == d32.min(axis=0, keepdims=True)).sum(axis=0) > 1).sum())
    print("%d rows and columns whose minimum is tied" % ties)
    assert ties >= 200, ties
    rb, cb = d32.argmin(axis=1), d32.argmin(axis=0)
    want = [(i, rb[i], d32[i, rb[i]]) for i in range(n1) if d32[i, rb[i]] < np.float32(0.7) and cb[rb[i]] == i]
    assert res["n_match"] == len(want) >= 100
    assert np.array_equal(res["match"][:len(want)], np.array(want, np.float32))
    rows = res["match"][:len(want), 0].astype(int).tolist()
    assert 210 in rows and 650 not in rows and 220 in rows
    assert res["match"][rows.index(220), 1] == 20
    assert not res["match"][len(want):].any()


def test_matcher_counts_and_empty_sides():
    d1, d2 = W.sign_descriptors(1, 40), W.sign_descriptors(2, 30)
    d2[:10] = d1[:10]
    d2[25] = d1[30]
    assert W.match_world(d1, 0, d2, 30, 0.7)["n_match"] == 0 and W.match_world(d1, 40, d2, 0, 0.7)["n_match"] == 0
    assert W.match_world(d1, 40, d2, 20, 0.7)["n_match"] == 10      # frame row 25 is past the count
    assert W.match_world(d1, 30, d2, 30, 0.7)["n_match"] == 10      # map row 30 is past n_rows
    assert W.match_world(d1, 40, d2, 30, 0.7)["n_match"] == 11
    assert W.match_world(d1, 99, d2, 99, 0.7)["n_match"] == 11      # counts are clamped


MATCH_SEED = 5


def test_matcher_against_two_way_restatement():
    """8 229 x 1 131 random unit rows with planted noisy correspondences against readout_ref.match_two_way: the rows this
    restatement does not flag as ambiguous agree; no planted correspondence is flagged; at most 1 % of the rows are."""
    n1, n2, k = 8229, 1131, 500
    rng = np.random.RandomState(MATCH_SEED)
    d1 = rng.randn(n1, 256).astype(np.float32)
    d1 /= np.linalg.norm(d1, axis=1, keepdims=True)
    d2 = rng.randn(n2, 256).astype(np.float32)
    planted = rng.permutation(n1)[:k]
    d2[:k] = d1[planted] + 0.03 * rng.randn(k, 256).astype(np.float32)
    d2 /= np.linalg.norm(d2, axis=1, keepdims=True)
    res = W.match_world(d1, n1, d2, n2, 0.7)
    ref = R.match_two_way(d1, d2, 0.7)
    amb = res["amb_rows"]
    print("flagged %d of %d rows (%.3f %%), %d matches" % (amb.sum(), n1, 100.0 * amb.mean(), res["n_match"]))
    assert not amb[planted].any()
    assert amb.mean() <= 0.01
    got = {(int(i), int(j)) for i, j, _ in res["match"][:res["n_match"]] if not amb[int(i)]}
    want = {(i, j) for i, j in ref["matches"] if not amb[i]}
    assert got == want and len(got) >= k
    assert {(int(p), c) for c, p in enumerate(planted)} <= got


# ---- the blackout ----------------------------------------------------------------------------------------------------------------
def test_blackout_relocalises():
    """Measured (float64 against numpy.longdouble): centres differ by 1.46e-12 first baselines at most, so the bound is 2.33e-11;
    the relocalised centres are within 6.9e-12 of the truth, the ones of absolute_pose="repair" alone 0.5 to 2.3 off."""
    seq, runs = W.blackout_runs()
    dark, frames = seq["dark"], len(seq["pts"])
    assert frames >= 9 and W.BLACKOUT_L == 5 and seq["pts"][dark].shape[0] == 0
    # preconditions: the map is seen again, and section 27's repair alone does not survive the blackout
    before = runs["observe"]["states"][dark - 1]
    assert before[W.N_ROWS] >= 12 and before[W.ANCHORED] == 1
    for f in (dark + 1, dark + 2):
        assert runs["observe"]["world_corr"][f][2] >= 12, f
    err_repair = W.centre_errors(seq, runs["repair"]["table"])
    print("repair alone: centre errors %s" % ["%.2e" % e for e in err_repair])
    assert err_repair[dark + 1:].min() >= 1000.0 * W.BLACKOUT_BOUND
    measured = W.way_difference(seq, W.BLACKOUT_L, W.BLACKOUT_CAP, "relocalise", W.BLACKOUT_SEED0)
    print("float64 against WAY2: %.3e (recorded %.3e, bound %.3e)" % (measured, W.BLACKOUT_WAY_DIFFERENCE, W.BLACKOUT_BOUND))
    assert measured <= W.BLACKOUT_BOUND
    rel = runs["relocalise"]
    err = W.centre_errors(seq, rel["table"])
    print("relocalise: centre errors %s, flags %s" % (["%.2e" % e for e in err], rel["table"][:, 14].tolist()))
    assert err[dark + 1:].max() <= W.BLACKOUT_BOUND and err[:dark].max() <= W.BLACKOUT_BOUND
    for f in (dark + 1, dark + 2):
        assert int(rel["table"][f, 14]) & W.FLAG_WORLD and int(rel["table"][f, 14]) & N.FLAG_ABSOLUTE
    assert [int(s[W.ANCHORED]) for s in rel["states"]][dark:dark + 4] == [0, 0, 1, 1]
    assert rel["states"][dark + 2][W.STREAK] == 2 and rel["states"][-1][W.LOST] == 0
    # observing never repairs: the map stays lost (patience is far away) and nothing old changes
    obs = runs["observe"]
    assert [int(s[W.ANCHORED]) for s in obs["states"]][dark:] == [0] * (frames - dark)
    assert np.array_equal(obs["table"], runs["plain"]["table"])


# ---- the revisit -----------------------------------------------------------------------------------------------------------------
def test_revisit_observed():
    """Measured: 8.53e-14 between float64 and numpy.longdouble, so the bound is 1.36e-12; the world poses of the return frames
    are within 8.2e-14 first baselines of the true centres."""
    seq, runs = W.revisit_runs()
    obs, plain = runs["observe"], runs["plain"]
    frames, Lm = len(seq["pts"]), W.REVISIT_L
    measured = W.way_difference(seq, Lm, W.REVISIT_CAP, "observe", W.REVISIT_SEED0)
    print("float64 against WAY2: %.3e (recorded %.3e, bound %.3e)" % (measured, W.REVISIT_WAY_DIFFERENCE, W.REVISIT_BOUND))
    assert measured <= W.REVISIT_BOUND
    back = range(frames - 3, frames)                                   # the return frames
    for f in back:
        w = obs["world"][f]
        old, err = W.old_inliers(obs, f, Lm), W.world_centre_error(seq, obs, f)
        rot = float(np.abs(np.asarray(w["Rw"], dtype=np.float64) - seq["Rw"][f]).max())
        print("frame %d: status %d, %d inliers, %d of them last seen before frame %d, centre %.2e, rotation %.2e"
              % (f, w["status"], w["n_inliers"], old, f + 1 - Lm, err, rot))
        assert w["status"] == 0 and old >= 6
        assert err <= W.REVISIT_BOUND and rot <= W.REVISIT_BOUND
    # points return under new track ids: the map holds two rows for them
    rows, desc = W.map_rows(obs["map"])
    assert len({d.tobytes() for d in desc}) < len(desc)
    # observing changes nothing old
    assert np.array_equal(obs["table"], plain["table"])
    assert np.array_equal(obs["tracks"].ids, plain["tracks"].ids) and np.array_equal(obs["tracks"].tid, plain["tracks"].tid)
