"""The numpy restatement of the homography pose and the model selection (tests/pose_h_ref.py) against the
truth of its noise-free scenes, its two ways against each other, and the conditions the fixtures must keep so that no decision
of a compared case hangs on the last bits.  No GPU."""
import numpy as np
import pytest

from tests import pose_h_ref as H
from tests import pose_ref as P


def test_restatement_finds_the_truth():
    """Measured: R 4.5e-14, t 8.4e-13, normal 2.5e-13 degrees (TRUTH_ERROR_DEG); the bound is 16 times the largest."""
    err = H.truth_error()
    print("truth error (R, t, normal) in degrees:", err)
    assert max(err) <= H.TRUTH_BOUND_DEG
    for nm in ("one_alive", "prior_true"):
        c = H.case(nm)
        assert c["pose"]["model"] == 1 and c["pose"]["status"] == 0
        assert np.abs(np.linalg.det(c["pose"]["R"].astype(np.float64)) - 1.0) < 1e-12
    c = H.case("rotate")
    assert c["pose"]["model"] == 2 and c["pose"]["cand"] == -1 and not c["pose"]["t"].any() and not c["pose"]["front"].any()


@pytest.mark.parametrize("name", ("plane48", "plane48b", "plane_k", "eight", "n257", "n4096"))
def test_true_pose_is_among_the_alive_candidates(name):
    """A plane seen twice has two poses; without a prior the frame is ambiguous (status 2) but the true one is alive."""
    c = H.case(name)
    cands = H.plane_candidates(*H.spectrum(H._signed(c)))
    pr = c["pair"]
    best = min(P.angle_deg(cands[k][0], pr["R"]) + P.angle_deg(cands[k][1], pr["N"]) for k in np.nonzero(c["pose"]["alive"])[0])
    print(name, "closest alive candidate: %.3e degrees" % best)
    assert best <= H.TRUTH_BOUND_DEG and c["pose"]["model"] == 1


def test_two_ways_agree():
    """Measured: 5.97e-10 (WAY_DIFFERENCE, the case "prior_other"); every other case stays below 8e-11."""
    d = H.way_difference()
    print("way difference %.3e (recorded %.3e, tolerance %.3e)" % (d, H.WAY_DIFFERENCE, H.TOLERANCE))
    if P.WIDE:
        assert d <= 2.0 * H.WAY_DIFFERENCE
    assert d <= H.TOLERANCE


def test_expected_decisions():
    want = {"plane48": (1, 2), "one_alive": (1, 0), "prior_true": (1, 0), "prior_other": (1, 0), "prior_tie": (1, 2), "rotate": (2, 0),
            "rotate_prior": (2, 0), "small_in": (2, 0), "small_out": (1, 2), "no_model": (0, 1), "seven": (0, 1), "three": (0, 1),
            "empty": (0, 1), "eight": (1, 2), "negative": (1, 2), "salted": (1, 2)}
    for nm, (model, status) in want.items():
        p = H.case(nm)["pose"]
        assert (p["model"], p["status"]) == (model, status), nm
    assert H.case("prior_true")["pose"]["cand"] != H.case("prior_other")["pose"]["cand"]
    assert int(H.case("one_alive")["pose"]["alive"].sum()) == 1 and int(H.case("plane48")["pose"]["alive"].sum()) == 2
    for k in ("R", "t", "normal", "depth"):                       # the sign of H does not matter
        assert np.array_equal(H.case("negative")["pose"][k], H.case("plane48")["pose"][k]), k
    assert np.any(H.case("rotate_prior")["pose"]["normals2"][0]) and not np.any(H.case("rotate_prior")["pose"]["normals2"][1])
    use = {nm: H.case(nm)["select"]["use_h"] for nm in H.CASES}
    assert use["plane48"] == 1 and use["solid"] == 0 and use["singular"] == 0 and use["no_f"] == 1 and use["no_model"] == 0
    assert use["rotate"] == 1 and use["noisy"] == 1
    assert H.case("singular")["select"]["scores"][0] == 0.0


@pytest.mark.parametrize("name", tuple(H.CASES))
def test_conditions_on_the_fixtures(name):
    """The margins of the issue: no compared case is near a decision."""
    c = H.case(name)
    p, s = c["pose"], c["select"]
    if s["ratio"] is not None and c["h_status"] == 0 and c["f_status"] == 0:
        assert abs(s["ratio"] - H.MODEL_RATIO) >= 0.05, s["ratio"]
    if p["spread"] is not None:
        assert abs(p["spread"] - c["rotation_eps"]) >= c["rotation_eps"] / 4, p["spread"]
    if p["model"] == 1:
        alive, dead = p["counts"][p["alive"]], p["counts"][~p["alive"]]
        if alive.size and dead.size:
            assert alive.min() - dead.max() >= 4, p["counts"]
        assert p["min_side"] >= 1e-9
        if p["prior_scores"] is not None and int(p["alive"].sum()) >= 2:
            sc = np.sort(p["prior_scores"][p["alive"]])[::-1]
            assert sc[0] - sc[1] >= 0.05 or sc[0] - sc[1] <= 1e-12, sc


def _sequence_conditions(fr):
    p, sel = fr["pose"], fr["select"]
    if fr["f"]["status"] == 0 and fr["h"]["status"] == 0:
        assert abs(sel["ratio"] - H.MODEL_RATIO) >= 0.05, sel["ratio"]
    if fr["model"]:
        assert abs(p["spread"] - H.ROTATION_EPS) >= H.ROTATION_EPS / 4
    if fr["model"] == 1:
        alive, dead = p["counts"][p["alive"]], p["counts"][~p["alive"]]
        assert alive.min() - dead.max() >= 4 and p["min_side"] >= 1e-9
        if p["prior_scores"] is not None and int(p["alive"].sum()) >= 2:
            sc = np.sort(p["prior_scores"][p["alive"]])[::-1]
            assert sc[0] - sc[1] >= 0.05, sc


@pytest.mark.parametrize("h_key", ("H", "H_lanes"))
def test_planar_sequence_through_the_restatements(h_key):
    """The trackers' planar sequence in numpy: every frame obeys the homography; the first has no prior and stays ambiguous (no
    pose, the centre repeats), the later ones are decided by the transported normals with status 0 and the true rotation.
    Measured: the chained centres from frame 1 on are the true ones to 2.07e-14 (PLANAR_CENTRE_ERROR)."""
    a, seq = H.auto_sequence("planar5", h_key), H.scene("planar5")
    assert [fr["model"] for fr in a["frames"]] == [1, 1, 1, 1]
    assert [fr["pose"]["status"] for fr in a["frames"]] == [2, 0, 0, 0]
    assert list(a["rows"][:, 14]) == [3, 2, 0, 0]
    for fr, pr in zip(a["frames"], seq["pairs"]):
        _sequence_conditions(fr)
        if fr["pose"]["status"] == 0:
            assert P.angle_deg(fr["pose"]["R"], pr["R"]) <= 1e-9 and P.angle_deg(fr["pose"]["normal"], pr["N"]) <= 1e-9
    err = H.planar_centre_error()
    print("planar centre error %.3e (recorded %.3e)" % (err, H.PLANAR_CENTRE_ERROR))
    assert err <= H.PLANAR_CENTRE_BOUND


def test_rotation_in_the_middle_through_the_restatements():
    """Side - rotate in place - side: F, rotation, F; the middle row keeps the true rotation, repeats the centre, carries the scale."""
    a, seq = H.auto_sequence("srs"), H.scene("srs")
    assert [fr["model"] for fr in a["frames"]] == [0, 2, 0]
    for fr in a["frames"]:
        _sequence_conditions(fr)
    rows = a["rows"]
    assert list(rows[:, 14]) == [2, 2, 2] and np.abs(rows[1, 9:12] - rows[0, 9:12]).max() <= 1e-14      # (recomputed from R Rw and R tw: equal up to rounding)
    assert P.angle_deg(rows[1, :9].reshape(3, 3), seq["Rf"][2]) <= 1e-9


def test_solid_sequence_keeps_the_fundamental_matrix():
    """pose_ref's seq5_k, the trackers' scene that is not planar: the best homography scores far below model_ratio on every pair."""
    c = P.case("seq5_k")
    for k, pr in enumerate(c["seq"]["pairs"]):
        fr = H.auto_frame(pr["m"], pr["intr"], c["seeds"][k], None)
        print("pair %d: ratio %.3f" % (k, fr["select"]["ratio"]))
        assert fr["model"] == 0 and fr["select"]["ratio"] <= H.MODEL_RATIO - 0.05
