"""The world map's upkeep, on the CPU: tests/world_upkeep_ref.py, the specification of
csrc/world_upkeep_kernels.hip.h, on the hand-made cases of tests/world_upkeep_cases.py (one per rule of each phase) and on two
sequences under the restated tracker: world_ref's revisit, where upkeep merges the rows of returning points, and a long run on which
a map without upkeep fills up and loses the camera."""
import numpy as np
import pytest

from tests import world_ref as W
from tests import world_upkeep_cases as K
from tests import world_upkeep_ref as U

F = K.F


def run(name):
    case = K.hand_made(name)
    w, report, info = K.run_ref(case)
    return case, w, report, info


def test_no_hand_made_case_is_ambiguous():
    """A condition of the fixtures: no merge decision lies within 1e-9 (relative) of its threshold, so == is owed on the device."""
    for name in K.HAND_MADE:
        assert not K.run_ref(K.hand_made(name))[2]["ambiguous"], name
    for seed, n in enumerate((1, 63, 64, 65, 1024, 1025)):
        assert not K.run_ref(K.random_case(seed, n, n + 3))[2]["ambiguous"]


@pytest.mark.parametrize("name,old,new", [("merge_survivor_is_r", 1, 4), ("merge_survivor_is_r2", 4, 1), ("merge_half_thresh", 1, 4)])
def test_merge(name, old, new):
    case, w, report, info = run(name)
    w0 = case["world"]
    assert info["pairs"] == [(old, new)] and report.tolist() == [6, 1, 0, 0, 5, 0, 0, 0]
    s, t_new, t_old = min(old, new), int(w0["tid"][new]), int(w0["tid"][old])
    assert W.lookup(w, t_new) == s and W.lookup(w, t_old) == -1          # the stale entry of the dead track fails the lookup
    for c in ("X", "desc", "tid", "n_views", "rms"):
        assert np.array_equal(w[c][s], w0[c][new]), c
    assert w["last_frame"][s] == F and w["first_frame"][s] == 1 == min(w0["first_frame"][old], w0["first_frame"][new])
    # the other rows keep their order: row 5 moved to slot 4 and its track follows
    others = [i for i in range(6) if i not in (old, new)]
    kept = sorted(others + [s])
    for c in U.COLUMNS:
        for d, i in enumerate(kept):
            if i != s:
                assert np.array_equal(w[c][d], w0[c][i]), (c, d, i)
    for d, i in enumerate(kept):
        if i != s:
            assert W.lookup(w, int(w0["tid"][i])) == d


@pytest.mark.parametrize("name", [n for n in K.HAND_MADE if n.startswith("merge_refused") or n == "merge_off"])
def test_merge_refused(name):
    """One case per condition: r' not in the map, r' == r, the insert wrote r, r' not written by it, X[r] behind the camera, a
    reprojection error of twice the threshold, a landmark row the insert would have left out, and merging switched off."""
    case, w, report, info = run(name)
    assert info["pairs"] == [] and report.tolist() == [6, 0, 0, 0, 6, 0, 0, 0]
    for c in W.new_map(1, 1):
        assert np.array_equal(w[c], case["world"][c]), c


def test_merge_gate_distances():
    """The two merge cases lie about thresh / 2 and 2 thresh from the reprojection, far from the threshold."""
    for name, want in (("merge_survivor_is_r", K.THRESH / 2), ("merge_half_thresh", K.THRESH / 2), ("merge_refused_twice_thresh", 2 * K.THRESH)):
        case = K.hand_made(name)
        d = np.linalg.norm(case["pts_new"][2] - K.project(case["world"]["X"][1]))
        assert abs(d - want) < 1e-9, (name, d)


def test_cull_boundaries():
    case, w, report, info = run("cull_age_boundary")      # cull_age 3: F - 3 is kept, F - 4 dies unless it has 3 views
    assert info["dead"].tolist() == [0, 2, 0, 2, 0] and report.tolist() == [5, 0, 2, 0, 3, 0, 0, 0]
    assert w["tid"][:3].tolist() == case["world"]["tid"][[0, 2, 4]].tolist()
    case, w, report, info = run("cull_views_boundary")    # cull_min_views 3: 2 dies, 3 stays
    assert info["dead"].tolist() == [2, 0, 0, 2] and report[U.AFTER] == 2
    case, w, report, info = run("cull_age_zero")
    assert info["dead"].tolist() == [0, 2, 2]


def test_evict():
    _, _, report, info = run("evict_at_high_water")
    assert report.tolist() == [6, 0, 0, 0, 6, 0, 0, 0] and not info["dead"].any()
    case, w, report, info = run("evict_above_high_water")     # 7 > 6: 7 - 4 = 3 rows, fewest views first, then the oldest
    assert report.tolist() == [7, 0, 0, 3, 4, 1, 0, 0] and info["dead"].tolist() == [0, 3, 0, 3, 0, 0, 3]
    _, _, report, info = run("evict_none_unprotected")        # k = 0: fired, nothing to take
    assert report.tolist() == [5, 0, 0, 0, 5, 1, 4, 0]
    _, _, report, info = run("evict_all_unprotected")         # wants 6, may take 4
    assert report.tolist() == [7, 0, 0, 4, 3, 1, 2, 0] and info["dead"].tolist() == [0, 3, 3, 0, 3, 3, 0]
    _, _, report, info = run("evict_ties_by_slot")            # equal views and age: the higher slots go
    assert report.tolist() == [8, 0, 0, 3, 5, 1, 0, 0] and info["dead"].tolist() == [0, 0, 0, 0, 0, 3, 3, 3]
    _, w, report, _ = run("evict_to_empty")
    assert report.tolist() == [4, 0, 0, 4, 0, 1, 0, 0] and w["state"][W.N_ROWS] == 0
    assert U.evict_key(300, -1, 7) == (255, 0, 65528) and U.evict_key(2, 5, 1) < U.evict_key(2, 5, 0) < U.evict_key(2, 6, 9)


def test_compact():
    case, w, report, _ = run("nothing_dies")
    assert report.tolist() == [6, 0, 0, 0, 6, 0, 0, 0]
    for c in W.new_map(1, 1):                 # identity, slot_of_tid and the state included
        assert np.array_equal(w[c], case["world"][c]), c
    case, w, report, _ = run("everything_dies")
    assert report.tolist() == [6, 0, 6, 0, 0, 0, 0, 0] and w["state"].tolist() == [0, 1, 0, 0, 0, 0, 0, 0]
    assert all(W.lookup(w, int(t)) == -1 for t in case["world"]["tid"][:6])
    case, w, report, info = run("mixed")
    assert report.tolist() == [6, 1, 2, 1, 2, 1, 2, 0] and info["dead"].tolist() == [2, 0, 2, 3, 1, 0]
    w0 = case["world"]
    assert W.lookup(w, int(w0["tid"][4])) == 0 and W.lookup(w, int(w0["tid"][5])) == 1
    assert all(W.lookup(w, int(w0["tid"][i])) == -1 for i in (0, 1, 2, 3))
    assert np.array_equal(w["desc"][0], w0["desc"][4]) and np.array_equal(w["desc"][1], w0["desc"][5])


@pytest.mark.parametrize("name", ["not_anchored", "no_rows", "no_table_row"])
def test_skipped_call(name):
    case, w, report, _ = run(name)
    n = W.n_rows_of(case["world"])
    assert report.tolist() == [n, 0, 0, 0, n, 0, 0, 1]
    for c in W.new_map(1, 1):
        assert np.array_equal(w[c], case["world"][c]), c


def test_random_cases_do_what_they_plant():
    for seed, n in enumerate((65, 1025)):
        case = K.random_case(seed, n, n + 7)
        w, report, info = K.run_ref(case)
        assert report[U.MERGED] == (case["n_match"] + 1) // 2 > 0 and report[U.CULLED] > 0 and report[U.FIRED] == 1
        assert report[U.EVICTED] > 0 and report[U.AFTER] == n - report[1:4].sum() == W.n_rows_of(w)
        for d in range(W.n_rows_of(w)):
            assert W.lookup(w, int(w["tid"][d])) == d


# ---- sequences ------------------------------------------------------------------------------------------------------------------
def test_revisit_merges_returning_points():
    seq, runs = U.revisit_runs()
    plain, off, on = runs["plain"], runs["off"], runs["on"]
    assert not on["ambiguous"]
    merged = [p for frame in on["merged"] for p in frame]
    assert len(merged) >= 10 and all(a == b >= 0 for a, b in merged)          # every pair is one scene point
    assert W.n_rows_of(on["map"]) < W.n_rows_of(plain["map"]) - 10
    for f in (10, 11, 12):
        assert on["world"][f]["status"] == 0
        assert W.world_centre_error(seq, on, f) <= W.REVISIT_BOUND
    # disabled phases change nothing: the map, the poses, the trajectory
    assert np.array_equal(off["table"], plain["table"])
    for c in W.new_map(1, 1):
        assert np.array_equal(off["map"][c], plain["map"][c]), c
    assert all(r is None or r.tolist() == [r[0], 0, 0, 0, r[0], 0, 0, int(r[7])] for r in off["reports"])
    # observing the map never feeds the trajectory, with or without upkeep
    assert np.array_equal(on["table"], plain["table"])
    rows, _ = W.map_rows(on["map"])
    assert len(set(rows[:, 0].tolist())) == len(rows)


def test_long_run_needs_upkeep():
    seq, runs = U.long_runs()
    plain, on = runs["plain"], runs["on"]
    frames = len(seq["pts"])
    late = range(frames - U.LONG_RUN_LATE, frames)
    distinct = len(set(t for m in on["maps"] for t in m[0][:, 0].tolist()))      # (nothing is dropped there: see below)
    assert distinct > U.LONG_RUN_WORLD_CAP
    # without upkeep the full map drops every new landmark and the late frames find no pose against it
    assert plain["states"][-1][W.DROP_FULL] > 0 and plain["states"][-1][W.N_ROWS] == U.LONG_RUN_WORLD_CAP
    assert all(plain["world"][f]["status"] != 0 for f in late)
    # with upkeep nothing is ever dropped and every late frame has its pose
    assert all(s[W.DROP_FULL] == 0 for s in on["states"])
    assert all(on["world"][f]["status"] == 0 for f in late)
    assert sum(int(r[U.EVICTED]) for r in on["reports"] if r is not None) > 0
    assert max(int(s[W.N_ROWS]) for s in on["states"]) <= U.LONG_RUN_WORLD_CAP - U.LONG_RUN_WORLD_CAP // 16 + max(int(s[W.APPENDED]) for s in on["states"])
    assert not on["ambiguous"] and np.array_equal(on["table"], plain["table"])      # observing never feeds the trajectory


def test_long_run_bound_is_the_measured_one():
    """The bound the device trackers are held to on the long run: 16 times the float64 / long double difference, measured here."""
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip("numpy.longdouble is float64 here: nothing to measure against")
    seq, _ = U.long_runs()
    d = W.way_difference(seq, U.LONG_RUN_L, U.LONG_RUN_CAP, "observe", U.LONG_RUN_SEED0, world_cap=U.LONG_RUN_WORLD_CAP)
    assert d == U.LONG_RUN_WAY_DIFFERENCE and U.LONG_RUN_BOUND == 16.0 * d
