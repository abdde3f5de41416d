"""The numpy restatement of the landmark kernels (tests/landmarks_ref.py) against itself, against plain
numpy and against the truth; no GPU.  The first test asserts the conditions every other test, here and on the GPU, rests on."""
import os
import re

import numpy as np
import pytest

from tests import landmarks_ref as R
from tests import pose_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ssp_landmark_workspace_bytes", "ssp_map_window", "ssp_op_triangulate_tracks", "ssp_op_landmarks_select")
# the smallest parallax of a true track, in degrees, as the fixtures were fixed (plain numpy under the true cameras)
PARALLAX_DEG = {"seq3": 3.15, "seq5": 6.80, "seq5_k": 5.80, "mixed48": 2.01, "n257": 1.62}


def _plain(fx, r):
    Rw, C = R.true_poses(fx["seq"])
    return R.plain_triangulate([(Rw[f], C[f], fx["seq"]["intr"][f], fx["seq"]["pts"][f][p]) for f, p in fx["obs"][r]])


def test_conditions_the_other_tests_rest_on():
    for name in R.SIDE_NOISE_FREE:
        fx = R.fixture(name)
        rows, true = fx["rows"], fx["point"] >= 0
        assert true.sum() == fx["seq"]["n_in"] and (~true).any()
        # plain numpy midpoint + Gauss-Newton: parallax, convergence, residual
        plain = [_plain(fx, r) for r in np.flatnonzero(true)]
        par = min(p[3] for p in plain)
        print("%s: smallest parallax %.2f degrees, largest rms %.2e px, largest last step %.2e"
              % (name, par, max(p[1] for p in plain), max(p[2] for p in plain)))
        assert abs(par - PARALLAX_DEG[name]) < 0.005 and par > R.MIN_PARALLAX_DEG
        assert max(p[1] for p in plain) < 4e-14 and max(p[2] for p in plain) < 1e-13 and min(p[4] for p in plain) > 0.0
        # the restatement: every true track accepted and converged, no stray accepted
        assert (rows["status"][true] == R.OK).all() and (rows["status"][~true] != R.OK).all(), name
        assert rows["rms"][true].max() < 4e-14 and rows["last_step"][true].max() < 1e-13, name
        for r in np.flatnonzero(~true):                       # strays: far above the threshold, not near it
            assert len(fx["obs"][r]) < 2 or _plain(fx, r)[1] > 2.0 * R.MAX_REPROJ or rows["status"][r] in (R.DEGENERATE, R.BEHIND)
    for name in R.SHORT_TRACKS:                               # true tracks lack views or parallax at worst; no stray is accepted
        fx = R.fixture(name)
        rows, true = fx["rows"], fx["point"] >= 0
        assert np.isin(rows["status"][true], (R.OK, R.FEW_VIEWS, R.DEGENERATE)).all() and (rows["status"][~true] != R.OK).all(), name
        ok = true & (rows["status"] == R.OK)
        # (hundreds of tracks instead of 40, down to 1 degree of parallax: the residual stays below two ulps of a pixel coordinate,
        # ulp(256 .. 511) = 5.7e-14, and a residual r moves the point by r * depth / (focal * sin(parallax)): 1.14e-13 * 12 /
        # (300 * sin(1 degree)) = 2.6e-13)
        assert ok.sum() >= 40 and rows["rms"][ok].max() < 1.14e-13 and rows["last_step"][ok].max() < 2.6e-13, name
    fx = R.fixture("noisy5")
    rows, true = fx["rows"], fx["point"] >= 0
    print("noisy5: largest rms of a true track %.3f px, largest fourth step %.2e" % (rows["rms"][true].max(), rows["last_step"][true].max()))
    assert (rows["status"][true] == R.OK).all() and (rows["status"][~true] != R.OK).all()
    assert 0.3 < rows["rms"][true].max() < 0.4 and rows["last_step"][true].max() < 1e-11
    for name, smallest in (("forward", 0.04), ("backward", 0.09)):        # the fixtures for status 2, not for acceptance
        fx = R.fixture(name)
        par = np.degrees(np.arccos(np.minimum(1.0, fx["rows"]["cos_parallax"])))
        assert abs(par.min() - smallest) < 0.005 and (fx["rows"]["status"] == R.DEGENERATE).sum() >= 20
        assert ((fx["rows"]["status"] == R.DEGENERATE) == (par < R.MIN_PARALLAX_DEG)).all()


def test_symbols_declared_and_exported():
    from semantic_superpoint_amd import lib
    with open(os.path.join(ROOT, "include", "ssp_hip.h")) as f:
        hdr = f.read()
    for n in NEW:
        assert re.search(r"\b%s\(" % n, hdr), n
        assert n in lib.EXPORTS, n
    for n in ("op_map_window", "op_triangulate_tracks", "op_landmarks_select", "landmarks_to_numpy", "landmark_buffers"):
        assert callable(getattr(lib, n))
    assert re.search(r"#define SSP_CAM_WORDS %d\b" % lib.CAM_WORDS, hdr) and lib.CAM_WORDS == R.CAM_WORDS
    assert re.search(r"#define SSP_LANDMARK_WORDS %d\b" % lib.LANDMARK_WORDS, hdr) and lib.LANDMARK_WORDS == R.LANDMARK_WORDS
    for n, v in (("FEW_VIEWS", R.FEW_VIEWS), ("DEGENERATE", R.DEGENERATE), ("BEHIND", R.BEHIND), ("REPROJ", R.REPROJ)):
        assert re.search(r"#define SSP_LANDMARK_%s %d\b" % (n, v), hdr) and getattr(lib, "LANDMARK_" + n) == v
    assert lib.LANDMARK_OK == R.OK == 0
    from semantic_superpoint_amd.export import PointTracker, SequenceTracker
    for cls in (PointTracker, SequenceTracker):
        for n in ("landmarks", "landmarks_device", "landmark_rows_device"):
            assert callable(getattr(cls, n))


def test_the_two_ways_agree_and_the_tolerance_is_the_measured_one():
    worst = R.way_difference()
    print("largest WAY1 / WAY2 difference over %s and the window scenarios: %.3e (recorded %.3e; longdouble is %s)"
          % (", ".join(R.COMPARED), worst, R.WAY_DIFFERENCE, "wider" if P.WIDE else "no wider"))
    if P.WIDE:
        assert worst == pytest.approx(R.WAY_DIFFERENCE, rel=0.05)
    assert worst <= R.TOLERANCE
    for name in ("n257", "seq5_short", "forward", "backward"):           # not compared on the device: the discrete outputs agree
        R.rows_difference(R.fixture(name)["rows"], R.fixture(name)["rows2"])


def test_against_the_truth():
    worst = max(R.truth_error(name) for name in R.SIDE_NOISE_FREE + R.SHORT_TRACKS)
    print("largest |X - scene point| over the accepted true tracks: %.3e (recorded %.3e)" % (worst, R.TRUTH_ERROR))
    assert worst == pytest.approx(R.TRUTH_ERROR, rel=0.05) and worst <= R.TRUTH_BOUND
    chain = R.chain_truth_error()
    print("the same under the cameras of the restated chain of seq5_k, in first baselines: %.3e (recorded %.3e)" % (chain, R.CHAIN_TRUTH_ERROR))
    assert chain == pytest.approx(R.CHAIN_TRUTH_ERROR, rel=0.05)


def test_closed_form_solve_against_numpy():
    rng = np.random.RandomState(3)
    for _ in range(50):
        J = rng.randn(8, 3) * rng.uniform(0.1, 100.0, 3)
        A, b = J.T @ J, rng.randn(3) * 10.0
        a = tuple(np.array([v]) for v in (A[0, 0], A[0, 1], A[0, 2], A[1, 1], A[1, 2], A[2, 2]))
        for way in (R.WAY1, R.WAY2):
            x, ok = R._solve3(tuple(v.astype(way[0]) for v in a), tuple(np.array([v], dtype=way[0]) for v in b), way[0], way[1])
            want = np.linalg.solve(A, b)
            assert ok[0] and np.abs(np.array([float(v[0]) for v in x]) - want).max() <= 1e-9 * np.linalg.cond(A) * np.abs(want).max()
    # singular, almost singular and non-finite systems are refused
    one, zero = np.array([1.0]), np.array([0.0])
    assert not R._solve3((one, one, one, one, one, one), (one, one, one), np.float64, False)[1][0]
    assert not R._solve3((one, one, zero, np.array([1.0 + 1e-13]), zero, one), (one, one, one), np.float64, False)[1][0]
    assert R._solve3((one, one, zero, np.array([1.0 + 1e-11]), zero, one), (one, one, one), np.float64, False)[1][0]
    assert not R._solve3((one, zero, zero, one, zero, np.array([np.nan])), (one, one, one), np.float64, False)[1][0]
    # the restated triangulation against the plain one on a fixture with 3 to 5 views per track
    fx = R.fixture("seq5_late")
    for r in np.flatnonzero((fx["point"] >= 0) & (fx["rows"]["status"] == R.OK)):
        X, rms, _, par, _ = _plain(fx, r)
        assert np.abs(X - fx["rows"]["X"][r]).max() < 1e-10 and abs(rms - fx["rows"]["rms"][r]) < 1e-12
        assert abs(np.cos(np.radians(par)) - fx["rows"]["cos_parallax"][r]) < 1e-12


def test_window_rule():
    for name in R.WINDOW_SCENARIOS:
        fx, n, table = R.scenario_inputs(name)
        _, _, valid = R.window_scenario(name)
        cams = R.map_window(n, table, fx["seq"]["intr"][:1], fx["L"])
        assert tuple(int(v) for v in cams[:, 16]) == valid, name
        for c in range(fx["L"]):
            f = n - fx["L"] + c
            if valid[c]:
                assert np.array_equal(cams[c, :12], table[f, :12]) and np.array_equal(cams[c, 12:16], fx["seq"]["intr"][0])
            else:
                assert not cams[c].any()
        rows = R.scenario_rows(name)
        true = R.row_points(fx["seq"], fx["tracks"], fx["L"], frames=n)[0] >= 0
        if name == "full":
            assert (rows["status"] == R.FEW_VIEWS).all() and not rows["X"].any() and not rows["n_views"].any()
        else:
            # the chain's cameras are the true ones up to the global scale, to the 1e-12 of section 24: every true track is accepted
            assert (rows["status"][true] == R.OK).all() and (rows["status"][~true] != R.OK).all(), name
            assert (rows["n_views"][true] == sum(valid)).all() and rows["rms"][true].max() < 1e-8
    # rows 0 and 1 alone: a window of two; frame 2 joins only if its scale was chained
    flags = [3, 2, 2, 0]
    assert R.window_start(flags, 2, 5, 8) == 0 and R.window_start(flags, 3, 5, 8) == 1 and R.window_start(flags, 4, 5, 8) == 1
    assert R.window_start([3, 2, 0, 0], 4, 5, 8) == 0 and R.window_start([3, 2, 0, 0], 4, 2, 8) == 2
    assert R.window_start([3, 3, 0, 0], 4, 5, 8) == 1 and R.window_start([3, 2, 0, 1], 4, 5, 8) == 3
    # per-frame intrinsics: a frame whose focal length is not finite and positive is no view
    fx, n, table = R.scenario_inputs("plain")
    intr = np.repeat(fx["seq"]["intr"][:1], 5, axis=0)
    intr[1, 0], intr[3, 1] = 0.0, np.inf
    assert list(R.map_window(n, table, intr, 5)[:, 16]) == [1, 0, 1, 0, 1]


def test_status_precedence_and_thresholds():
    fx = R.fixture("seq5_late")
    args = (fx["ids"], fx["counts"], fx["pts"], fx["first_slot"], fx["cams"])
    base = fx["rows"]
    assert {R.OK, R.FEW_VIEWS, R.BEHIND} <= set(np.unique(base["status"]).tolist())
    # min_views above a track's length: status 1 and nothing else written, whatever the other tests would say
    for mv in (3, 5, 6):
        rows = R.triangulate(*args, min_views=mv)
        few = base["n_views"] < mv
        assert few.any() and (rows["status"][few] == R.FEW_VIEWS).all() and np.array_equal(rows["status"][~few], base["status"][~few])
        assert not rows["X"][few].any() and not rows["rms"][few].any() and not rows["cos_parallax"][few].any()
        assert np.array_equal(rows["n_views"], base["n_views"])
    assert (R.triangulate(*args, min_views=6)["status"] == R.FEW_VIEWS).all()
    # a parallax threshold above every track's: status 2 wins over 3 and 4, and X / rms / cos_parallax stay written
    rows = R.triangulate(*args, cos_min_parallax=R.cos_of(150.0))
    seen = base["n_views"] >= 2
    assert (rows["status"][seen] == R.DEGENERATE).all() and (base["status"][seen] >= R.BEHIND).any()
    for k in ("X", "rms", "cos_parallax"):
        assert np.array_equal(rows[k], base[k])
    # a reprojection threshold of zero: status 4 where it was 0 (unless the residual is exactly zero), 3 stays 3
    rows = R.triangulate(*args, max_reproj=0.0)
    was_ok = base["status"] == R.OK
    assert np.array_equal(rows["status"][was_ok], np.where(base["rms"][was_ok] > 0.0, R.REPROJ, R.OK)) and (rows["status"] == R.REPROJ).sum() > 30
    assert np.array_equal(rows["status"][~was_ok], base["status"][~was_ok])
    # a point behind a camera: the mirror image of a true track's pixels about the principal point in one view
    fx3 = R.fixture("seq3")
    r = int(np.flatnonzero(fx3["point"] >= 0)[0])
    cams = fx3["cams"].copy()
    cams[:, 9:12] = -cams[:, 9:12]                                      # every centre mirrored: the rays now meet behind the cameras
    rows = R.triangulate(fx3["ids"][r:r + 1], fx3["counts"], fx3["pts"], fx3["first_slot"], cams)
    assert rows["status"][0] == R.BEHIND and rows["X"][0].any() and rows["rms"][0] > 0.0
    assert R.triangulate(fx3["ids"][r:r + 1], fx3["counts"], fx3["pts"], fx3["first_slot"], cams,
                         cos_min_parallax=R.cos_of(150.0))["status"][0] == R.DEGENERATE


def test_an_id_outside_its_frame_is_ignored():
    fx = R.fixture("seq3")
    ids = fx["ids"].copy()
    r = int(np.flatnonzero(fx["point"] >= 0)[0])
    total = sum(fx["counts"])
    ids[r, 1] = total + 5                                              # past the frame's points (it names one of a later frame)
    ids[r + 1, 0] = fx["counts"][0] + 2                                # names a point of the NEXT frame
    rows = R.triangulate(ids, fx["counts"], fx["pts"], fx["first_slot"], fx["cams"])
    assert rows["n_views"][r] == 2 and rows["n_views"][r + 1] == 2 and rows["status"][r] == R.OK
    counts = list(fx["counts"])
    counts[2] -= 1                                                     # the last point of the newest frame is no longer one
    rows = R.triangulate(fx["ids"], counts, fx["pts"], fx["first_slot"], fx["cams"])
    gone = fx["ids"][:, 2] == total - 1
    assert gone.sum() == 1 and rows["n_views"][gone][0] == 2 and (rows["n_views"][~gone] == 3).all()
    lm = R.select(fx["ids"], fx["tid"], counts, fx["point_cap"], rows)
    assert (lm[:, 7] == -1).sum() == (1 if rows["status"][gone][0] == R.OK else 0)


def test_select_is_stable_and_carries_the_newest_index():
    fx = R.fixture("seq5_late")
    rows = fx["rows"]
    lm = R.select(fx["ids"], fx["tid"], fx["counts"], fx["point_cap"], rows)
    keep = np.flatnonzero(rows["status"] == R.OK)
    assert lm.shape == (keep.size, R.LANDMARK_WORDS) and np.array_equal(lm[:, 0], fx["tid"][keep]) and (np.diff(keep) > 0).all()
    assert np.array_equal(lm[:, 1:4], rows["X"][keep]) and np.array_equal(lm[:, 4], rows["n_views"][keep])
    first_new = sum(fx["counts"][:-1])
    has = fx["ids"][keep, -1] >= 0
    assert has.any() and (~has).any()                                   # tracks that ended before the newest frame carry -1
    assert np.array_equal(lm[has, 7], fx["ids"][keep, -1][has] - first_new) and (lm[~has, 7] == -1).all()
    # the newest index names the observation itself
    seq, f = fx["seq"], fx["frames"] - 1
    for row, k in zip(lm[has], keep[has]):
        assert fx["obs"][k][-1] == (f, int(row[7]))
