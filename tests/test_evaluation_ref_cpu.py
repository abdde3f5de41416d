"""CPU: the restatement of the evaluation kernels (tests/evaluation_ref.py, tests/eval_restatement.py) against the G16 record and
against counts worked out by hand, the conditions under which the GPU comparison is exact (tests/evaluation_cases.py), the LDS
boundaries of the launchers, and the mutants that show the cases have teeth."""
import os
import re

import numpy as np
import pytest

from tests import eval_restatement as ER
from tests import evaluation_cases as C
from tests import evaluation_ref as R
from tests.golden_evaluation import CASES, EMPTY_CASE, case_pair

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G16 = os.path.join(ROOT, "tests", "golden", "g16_evaluation.npz")


def _call(name):
    return next(c for c in C.repeat_calls() if c["name"] == name)


def _row(name, pair=0):
    c = _call(name)
    return [float(v) for v in c["expect"][pair, :7]]


def test_restatement_reproduces_g16_record():
    f = np.load(G16)
    worst = np.inf
    for k, case in enumerate(CASES + [EMPTY_CASE]):
        d = case_pair(case)[0]
        H = d["homography"]
        N1, N2, c1, c2, s1, s2, unw, margin = R.repeatability(d["prob"], d["warped_prob"], H, np.linalg.inv(H), 240, 320, 1000, 3.0)
        rep = (c1 + c2) / (N1 + N2) if c1 + c2 > 0 else 0
        loc = s1 / (c1 + c2) + s2 / (c1 + c2) if c1 + c2 > 0 else -1
        assert rep == f["rep"][k], case[0]
        assert abs(loc - f["loc_err"][k]) <= 1e-12, case[0]
        assert unw == f["n_unwarped"][k], case[0]
        worst = min(worst, margin)
    print("G16: smallest decision margin %.3g px" % worst)
    assert worst >= C.MARGIN


def test_hand_computed_thresholds():
    """threshold_pair: the warped side-1 points a = (5,5) (20,5) (35,5) (5,25) (25,25), side 2 b = (5,5) (23,5) (38,9) (5,29)
    (45,30).  Row minima: 0, 3 (b1), 5 (b2: 3-4-5), 4 (b3), and a4 is > 20 from every b; column minima the same, b4 > 20 from
    every a.  So thresh 3: counts 2 / 2, sums 0 + 3; one ulp below 3: 1 / 1, sum 0; thresh 5: 4 / 4, sums 0 + 3 + 5 + 4 = 12; one
    ulp below 5: 3 / 3, sums 7; thresh 0: the coincident pair alone.  Matching-score count: (x, y) -> (u, v) = (y - 2, x - 1) kept
    when u <= 52 and v <= 36: b0 (3, 4), b1 (3, 22), b3 (27, 4) stay, b2 (v = 37) and b4 (v = 44) go: 3."""
    assert _row("thresh_3") == [5, 5, 2, 2, 3, 3, 3]
    assert _row("thresh_3_below") == [5, 5, 1, 1, 0, 0, 3]
    assert _row("thresh_5") == [5, 5, 4, 4, 12, 12, 3]
    assert _row("thresh_5_below") == [5, 5, 3, 3, 7, 7, 3]
    assert _row("thresh_0") == [5, 5, 1, 1, 0, 0, 3]


def test_hand_computed_borders_and_truncation():
    """border_pair at 12x16 under the identity.  Side 1: (0,5) (15,5) (4,0) (4,11) are inside; (16,5) (x = W), (4,12) (y = H)
    and (-1,3) are not: N1 = 4.  Side 2 has the same seven and (-0.5, 3.25), (3.25, -0.75) (outside), (11.625, 2.5) (inside, 4.2 px
    from (15,5), further from the rest): N2 = 5.  The four shared points coincide: counts 4 / 4, sums 0.
    Matching-score count, (u, v) = (trunc y, trunc x) kept when u <= 15 and v <= 11: (0,5) (4,0) (4,11) (4,12) stay, (15,5) (16,5)
    (v > 11) and (-1,3) (v < 0) go; (-0.5, 3.25) -> (3, -0 = 0) stays, (3.25, -0.75) -> (-0 = 0, 3) stays, (11.625, 2.5) -> (2, 11)
    stays: 7.  Rounding instead would give (2, 12), (-1, 3): 5.
    side1_outside: every side-1 point has x < 0, so N1 = 0 and neither side can repeat."""
    assert _row("geometry_12x16", 0) == [4, 5, 4, 4, 0, 0, 7]
    r = _row("geometry_12x16", 1)
    assert r[:6] == [0, 9, 0, 0, 0, 0]


def test_hand_computed_ties_and_horizon():
    """tie_pair: one confidence on all 12 rows a side, keep_k = 6: the lower index wins, rows 0..5, each 1 px from its partner:
    counts 6 / 6, sums 6.  The same with -0.0 on rows 0..5 and +0.0 on rows 6..11: the zeros tie.
    horizon_pair: the points on the horizon have u = inf or v = NaN and are outside, like the points behind it (u < 0)."""
    assert _row("ties_straddle", 0) == [6, 6, 6, 6, 6, 6, 10]
    assert _row("ties_straddle", 1) == [6, 6, 6, 6, 6, 6, 10]
    c = _call("horizon_48x64")
    u, v = R.warp(c["H"][0], c["pts1"][0, :2, 0], c["pts1"][0, :2, 1])
    assert np.isinf(u[0]) and np.isinf(v[0]) and np.isinf(u[1]) and np.isnan(v[1])
    u2, _ = R.warp(c["H_inv"][0], c["pts2"][0, 2, 0], c["pts2"][0, 2, 1])
    assert np.isinf(u2)
    x = c["pts1"][0, :40, 0]
    assert np.sum(x < 32) >= 10 and np.sum(x > 32) >= 10          # the horizon passes through the cloud
    assert 0 < c["expect"][0, 0] < np.sum(x < 32)


def test_tie_rule_is_irrelevant_when_ties_lie_inside_the_kept_set():
    c = _call("ties_3levels")
    conf = c["pts1"][0, :30, 2]
    assert len(set(conf)) == 3 and c["keep_k"] == np.sum(conf >= 0.5) < 30
    a, _ = R.repeatability_call(c)
    b, _ = R.repeatability_call(c, "ties_high")
    assert a[:, :4].tolist() == b[:, :4].tolist() and a[0, 6] == b[0, 6]
    np.testing.assert_allclose(a[:, 4:6], b[:, 4:6], rtol=1e-14)     # the same terms in another order


def test_large_keep_k_case_equals_itself_at_cap_n():
    a, b = _call("k2048_cap4096"), _call("k2048_cap2500")
    assert a["keep_k"] == 2048 and a["cap"] == 4096 and b["cap"] == 2500 == a["n1"][0]
    assert np.array_equal(a["expect"], b["expect"]) and a["expect"][0, 0] == 2048 == a["expect"][0, 1]
    lds = ((a["cap"] + 1) & ~1) * 8 + 2 * 2048 * 16
    assert lds == 96 * 1024


def test_repeatability_cases_cover_the_issue_and_are_decided():
    calls = C.repeat_calls()
    worst = min(float(c["margins"].min()) for c in calls)
    for c in calls:
        print("%-24s seed %5d  %dx%d cap %4d stride %d keep_k %4d thresh %.17g  margin %.3g px"
              % (c["name"], c["seed"], c["height"], c["width"], c["cap"], c["pair_stride"], c["keep_k"], c["thresh"], c["margins"].min()))
    print("repeatability: %d launches, %d pairs, smallest decision margin %.3g px, ambiguous decisions: 0"
          % (len(calls), sum(c["n_pairs"] for c in calls), worst))
    assert worst >= C.MARGIN
    assert {(c["height"], c["width"]) for c in calls} == {(12, 16), (37, 53), (48, 64), (240, 320)}
    assert {c["pair_stride"] for c in calls} == {1, 2, 3}
    counts = {int(min(c["n1"][p * c["pair_stride"]], c["cap"])) for c in calls for p in range(c["n_pairs"])}
    assert {0, 1, 255, 256, 257} <= counts
    assert any(c["n1"][p * c["pair_stride"]] > c["cap"] for c in calls for p in range(c["n_pairs"]))
    assert {1, 7, 19, 20, 21, 2048} <= {c["keep_k"] for c in calls} and any(c["keep_k"] >= c["cap"] for c in calls)
    assert {0.0, 3.0, 5.0, np.nextafter(3.0, 0), np.nextafter(5.0, 0)} <= {c["thresh"] for c in calls}


def test_ransac_cases_are_decided_in_both_summation_orders():
    spread = {}
    for name in C.RANSAC_SPECS:
        p = C.ransac_problem(name)
        ref, m = p["ref"], p["m"]
        n = m.shape[0]
        if n < 4:
            assert ref["status"] == 1
            continue
        assert ref["status"] == 0 and p["gap"] >= C.RESID_BAND, name
        # the winner and its inlier set are formed before any sum: the refits in both orders must leave every match on its side
        for key in ("H", "H_lanes"):
            assert np.array_equal(ER.resid2(ref[key].reshape(1, 9), m)[0] <= 9.0, ER.resid2(ref["H_best"].reshape(1, 9), m)[0] <= 9.0), name
        s = float(np.abs(ref["H"] - ref["H_lanes"]).max() / np.abs(ref["H"]).max())
        fam = C.family_of(n)
        spread[fam] = max(spread.get(fam, 0.0), s)
        a, b = ref["ap"], ER.average_precision_counting(ref["mask"], p["dist"])
        print("%-18s seed %5d n %4d inliers %4d winner %4d  gap to 9: %.3g  H spread %.3g  ap %.17g (counting form %+.3g)"
              % (name, p["seed"], n, ref["mask"].sum(), ref["best"], p["gap"], s, a, b - a))
        assert abs(a - b) <= (ref["mask"].sum() + 2) * 2.0 ** -52
    print("RANSAC: ambiguous decisions: 0; spread of the refit between the two summation orders:", spread)
    assert C.ransac_problem("ap_all_inliers")["ref"]["mask"].all()
    p = C.ransac_problem("ap_outliers_first")
    assert np.array_equal(p["ref"]["mask"], ~p["outliers"]) and p["dist"][p["outliers"]].max() < p["dist"][~p["outliers"]].min()
    p = C.ransac_problem("ap_3levels")
    assert len(set(p["dist"])) == 3 and len(set(p["dist"][p["ref"]["mask"]])) == 3 and len(set(p["dist"][~p["ref"]["mask"]])) == 3
    # the sampler at 5 matches: most draws repeat an index already taken, some hypotheses spend all their draws
    draws = [ER.sample(C.ransac_problem("n5_clean")["seed"], h, 5) for h in range(ER.HYPOTHESES)]
    assert all(d is not None and len(set(d)) == 4 for d in draws)


def test_lane_order_sum_is_a_reordering():
    rng = np.random.default_rng(3)
    t = rng.standard_normal((300, 3))
    idx = np.sort(rng.permutation(700)[:300])
    s = ER.lane_sum(t, idx)
    np.testing.assert_allclose(s, t.sum(0), rtol=0, atol=300 * 2.0 ** -52 * np.abs(t).sum(0).max())
    assert np.array_equal(ER.lane_sum(np.arange(130.0), np.arange(130)), 8385.0)   # integers: exact in every order


def test_lds_boundaries_of_the_launchers():
    """eval_ransac_kernel stages cap * (sizeof(double4) + 5) = 37 cap bytes; it needs more than the 64 KiB a kernel gets without
    asking from cap 1772 and leaves LDS for global memory from cap 3322 (EVAL_LDS_MAX); the caps of the GPU test sit on both."""
    src = open(os.path.join(ROOT, "semantic-superpoint_amd", "csrc", "ops_host.hip.h")).read()
    m = re.search(r"#define EVAL_LDS_MAX \((\d+) \* 1024\)", src)
    lds_max = int(m.group(1)) * 1024
    assert "const size_t small = (size_t)cap * (sizeof(float) + 1);" in src
    assert "const bool use_lds = (size_t)cap * sizeof(double4) + small <= EVAL_LDS_MAX;" in src
    per = 32 + 4 + 1
    assert per * 3321 <= lds_max < per * 3322
    assert per * 1771 <= 64 * 1024 < per * 1772
    assert {1771, 1772, 3321, 3322, 4096} <= set(C.CAPS)
    keep_max = int(re.search(r"#define EVAL_KEEP_MAX (\d+)", src).group(1))
    assert keep_max == 2048 and 4096 * 8 + 2 * keep_max * 16 <= lds_max


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_mutant_changes_an_integer_output(mutant):
    hit = []
    for c in C.repeat_calls():
        if c["cap"] > 300:
            continue
        out, _ = R.repeatability_call(c, mutant)
        cols = [0, 1, 2, 3, 6]
        if not np.array_equal(out[:, cols], c["expect"][:, cols]):
            hit.append(c["name"])
    print(mutant, "caught by", hit)
    assert hit
