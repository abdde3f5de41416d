"""World map classes on the CPU: the rules of tests/world_classes_ref.py checked by hand - the vote's
sequences, what it skips, the masked matcher on a 3 x 3 case and on aliased structure (equal descriptors, different classes: the
tie rule makes the plain matcher's wrong answer deterministic, and it is asserted, not assumed) - and the restated tracker on the
revisit with planted aliases: joins of different scene points counted by the sequence's own identities."""
import re
import os

import numpy as np

from tests import landmarks_ref as LR
from tests import world_classes_ref as WC
from tests import world_ref as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = WC.CLASS_NONE


def _entry(cls, n):
    return (n << 8) | cls


def _run(seq, v=0):
    out = []
    for c in seq:
        v = WC.vote_step(v, c)
        out.append(v)
    return out


# ---- the vote --------------------------------------------------------------------------------------------------------------------
def test_vote_sequences_by_hand():
    assert WC.decode(0) == NONE
    assert _run([7]) == [_entry(7, 1)] and WC.decode(_entry(7, 1)) == 7                       # the first vote
    up = _run([7] * 300)
    assert up[253] == _entry(7, 254) and up[254] == up[299] == _entry(7, 255)                # agreement saturates at 255
    down = _run([9, 9, 9], _entry(7, 3))
    assert down == [_entry(7, 2), _entry(7, 1), _entry(7, 0)]                                # disagreement: the class byte is kept
    assert list(WC.decode(down)) == [7, 7, NONE]                                             # ... and at 0 votes it reads as none
    assert _run([9], down[-1]) == [_entry(9, 1)]                                             # a new class is adopted after 0
    assert _run([3], _entry(5, 255)) == [_entry(5, 254)]
    a, b = 4, 6
    flicker = _run([a, b, a, a])
    assert flicker == [_entry(a, 1), _entry(a, 0), _entry(a, 1), _entry(a, 2)] and WC.decode(flicker[-1]) == a


def _landmarks(rows):
    lm = np.zeros((len(rows), LR.LANDMARK_WORDS))
    for r, (t, p) in enumerate(rows):
        lm[r, 0], lm[r, 7] = t, p
        lm[r, 1:4] = np.nan                                                                  # X plays no part in the vote
    return lm


def test_vote_skips_what_the_insert_skips():
    tid_cap, count = 8, 3
    cls_new = np.array([2, NONE, 5, 7], np.uint8)                                            # (row 3 lies past the count)
    lm = _landmarks([(0, 0), (1, 1), (2, -1), (3, 3), (8, 0), (4, 2), (5, np.nan), (np.nan, 0), (-1, 0), (6, 2)])
    votes = WC.vote(WC.new_votes(tid_cap), lm, 9, cls_new, count)                            # (the tenth row lies past n_landmarks)
    want = np.zeros(tid_cap, np.uint16)
    want[0], want[4] = _entry(2, 1), _entry(5, 1)
    assert np.array_equal(votes, want)
    assert list(WC.decode(votes)) == [2, NONE, NONE, NONE, 5, NONE, NONE, NONE]
    WC.vote(votes, lm, 10, cls_new, 4)                                                       # now rows (3, 3) and (6, 2) vote too
    want[0], want[4], want[3], want[6] = _entry(2, 2), _entry(5, 2), _entry(7, 1), _entry(5, 1)
    assert np.array_equal(votes, want)


def test_read_out():
    w = W.new_map(6, 8)
    w["tid"][:4] = [3, 0, 7, 5]
    w["state"][W.N_ROWS] = 3
    votes = WC.new_votes(8)
    votes[3], votes[0], votes[7], votes[5] = _entry(9, 2), _entry(4, 0), _entry(1, 1), _entry(2, 9)
    assert list(WC.world_classes(w, votes)) == [9, NONE, 1, NONE, NONE, NONE]


# ---- the masked matcher ----------------------------------------------------------------------------------------------------------
def _rows(m):
    return [tuple(r) for r in m["match"][:m["n_match"], :2].astype(int).tolist()]


def test_masked_matcher_3x3_by_hand():
    d = W.sign_descriptors(1, 3)
    d1, d2 = d.copy(), d[[1, 2, 0]].copy()                     # frame row j is map row (j + 1) % 3
    plain = W.match_world(d1, 3, d2, 3, 0.7)
    assert _rows(plain) == [(0, 2), (1, 0), (2, 1)]
    same = WC.match_world_classes(d1, 3, [4, 4, 4], d2, [4, 4, 4], 3, 0.7)
    assert _rows(same) == _rows(plain) and np.array_equal(same["match"], plain["match"])
    # map classes (4, 5, 4); frame classes (5, 4, 4): (0, 2) 4 == 4 stays, (1, 0) 5 == 5 stays, (2, 1) 4 == 4 stays
    assert _rows(WC.match_world_classes(d1, 3, [4, 5, 4], d2, [5, 4, 4], 3, 0.7)) == [(0, 2), (1, 0), (2, 1)]
    # frame classes (4, 4, 4): map row 1 (class 5) has no candidate; its frame row 0 finds nothing below the threshold
    assert _rows(WC.match_world_classes(d1, 3, [4, 5, 4], d2, [4, 4, 4], 3, 0.7)) == [(0, 2), (2, 1)]
    # class 5 outside the mask, class 4 kept
    only4 = WC.mask_of(keep=(4,), n_classes=8)
    assert _rows(WC.match_world_classes(d1, 3, [4, 5, 4], d2, [5, 4, 4], 3, 0.7, only4)) == [(0, 2), (2, 1)]
    # an unknown map class matches nothing, not even an unknown frame class
    assert _rows(WC.match_world_classes(d1, 3, [NONE, 5, 4], d2, [5, 4, NONE], 3, 0.7)) == [(1, 0), (2, 1)]
    # a column that loses every candidate: frame row 1 is of class 6, which no map row has
    assert _rows(WC.match_world_classes(d1, 3, [4, 4, 4], d2, [4, 6, 4], 3, 0.7)) == [(0, 2), (1, 0)]
    assert WC.match_world_classes(d1, 3, [1, 1, 1], d2, [2, 2, 2], 3, 0.7)["n_match"] == 0
    assert WC.match_world_classes(d1, 0, [], d2, [2, 2, 2], 3, 0.7)["n_match"] == 0


def _aliased(n1, b, a, j=2, n2=5):
    d1, d2 = W.sign_descriptors(3, n1), W.sign_descriptors(4, n2)
    d1[a] = d1[b]
    d2[j] = d1[b]
    c1, c2 = np.full(n1, 1, np.uint8), np.full(n2, 1, np.uint8)
    c1[a], c2[j] = 2, 2                                        # b keeps class 1; a and the frame row carry class 2
    return d1, c1, d2, c2


def test_aliased_structure_is_decided_by_the_tie_rule():
    for n1, b, a in ((40, 5, 17), (200, 100, 130)):            # the same strip; different strips (a >= 128 > b)
        assert b < a
        d1, c1, d2, c2 = _aliased(n1, b, a)
        assert np.array_equal(d1[a], d1[b]) and c1[a] != c1[b] and c2[2] == c1[a]
        assert _rows(W.match_world(d1, n1, d2, 5, 0.7)) == [(b, 2)]                           # the first index: the wrong row
        assert _rows(WC.match_world_classes(d1, n1, c1, d2, c2, 5, 0.7)) == [(a, 2)]
        assert _rows(WC.match_world_classes(d1, n1, c1, d2, c2, 5, 0.7, WC.mask_of(drop=(2,)))) == []
        c1[a] = NONE
        assert _rows(WC.match_world_classes(d1, n1, c1, d2, c2, 5, 0.7)) == []


# ---- the restated tracker ---------------------------------------------------------------------------------------------------------
def test_restated_tracker_on_the_revisit_with_aliases():
    seq, runs = WC.alias_runs()
    plain, observe, match, drop = runs["plain"], runs["observe"], runs["match"], runs["match-drop"]
    print("aliases (b, a):", seq["aliases"])
    for name, run in runs.items():
        print("%-10s wrong joins %2d, matches per frame %s, map rows %d" % (name, len(run["wrong_joins"]),
                                                                           [m["n_match"] for m in run["world_match"]],
                                                                           int(run["states"][-1][W.N_ROWS])))
    assert len(plain["wrong_joins"]) >= 1
    assert len(match["wrong_joins"]) == 0 and len(drop["wrong_joins"]) == 0
    assert sum(m["n_match"] for m in match["world_match"]) > 500                             # (it still matches)
    # every wrong join of the plain run joins a planted a with its b's row
    pairs = {(b, a) for b, a in seq["aliases"]}
    for f, i, j in plain["wrong_joins"]:
        assert any(int(seq["ids"][f][j]) == a for _, a in pairs), (f, i, j)
    # observing changes no old output
    for f in range(len(seq["pts"])):
        assert np.array_equal(plain["world_match"][f]["match"], observe["world_match"][f]["match"])
        assert np.array_equal(plain["states"][f], observe["states"][f])
        for k in ("Rw", "C", "status", "n_inliers"):
            assert np.array_equal(np.asarray(plain["world"][f][k]), np.asarray(observe["world"][f][k])), (f, k)
    assert np.array_equal(plain["table"], observe["table"])
    for k in ("X", "desc", "tid", "n_views", "first_frame", "last_frame", "rms", "slot_of_tid", "state"):
        assert np.array_equal(plain["map"][k], observe["map"][k]), k
    assert not plain["votes"].any() and observe["votes"].any()
    # the votes are those of the scene points: every voted track reads its scene point's class
    cls = observe["classes"][-1][:int(observe["states"][-1][W.N_ROWS])]
    tids = observe["map"]["tid"][:len(cls)]
    want = np.array([seq["cls_of"][observe["scene_of_tid"][int(t)]] for t in tids], np.uint8)
    assert np.array_equal(cls, want)
    assert set(np.unique(cls)) == {0, 1, 2, NONE}
    # the dropped class matches nothing
    for f, m in enumerate(drop["world_match"]):
        cols = m["match"][:m["n_match"], 1].astype(int)
        assert not np.isin(seq["cls"][f][cols], WC.ALIAS_DROP).any()


def test_new_exports_are_declared_and_listed():
    from semantic_superpoint_amd import lib
    with open(os.path.join(ROOT, "include", "ssp_hip.h")) as f:
        header = f.read()
    for name in ("ssp_op_track_class_votes", "ssp_op_world_classes", "ssp_match_world_classes"):
        assert re.search(r"\b%s\(" % name, header) and name in lib.EXPORTS and name in lib.SIGNATURES
    assert lib.CLASS_NONE == NONE and WC.mask_of(drop=(2,)) == lib.class_mask(drop=(2,), n_classes=WC.N_CLASSES)
    assert lib.WORLD_SPEC[1].keys() == {"X", "desc", "tid", "n_views", "first_frame", "last_frame", "rms", "slot_of_tid", "state"}
