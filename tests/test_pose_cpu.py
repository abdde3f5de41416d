"""The rules of the two-view pose as tests/pose_ref.py restates them: the fixtures first (on the
noise-free ones the RANSAC mask is the truth and every inlier lies in front of both cameras, so the status-2 rule is a
condition the fixtures themselves satisfy), the SVD-free decomposition against numpy.linalg.svd, the cheirality test on the
four kinds of motion, the status rules, the scale chain, and the measured bounds: pose_ref.TRUTH_BOUND_DEG (16 times the
restatement's own error against the truth) and pose_ref.TOLERANCE (16 times the difference between its two ways)."""
import numpy as np
import pytest

from tests import epipolar_ref as E
from tests import pose_ref as P


@pytest.mark.parametrize("name", P.NOISE_FREE)
def test_fixtures_mask_is_truth_and_every_inlier_in_front(name):
    c = P.case(name)
    assert len(c["pose"]) == P.CASES[name][1] - 1
    for r, pose, pr in zip(c["ransac"], c["pose"], c["seq"]["pairs"]):
        assert r["status"] == 0 and np.array_equal(r["mask"], pr["truth"]), name
        assert pose["status"] == 0 and pose["n_front"] == r["n_inliers"] == int(pr["truth"].sum()), name
        assert np.array_equal(pose["front"], pr["truth"])
        assert sorted(pose["counts"]) == [0, 0, 0, r["n_inliers"]]        # exactly one candidate takes every inlier
        # outliers keep their distance from both epipolar lines
        d1, d2 = E.line_dist(pr["F"], pr["m"][~pr["truth"], :2], pr["m"][~pr["truth"], 2:])
        assert d1.size == 0 or min(d1.min(), d2.min()) >= E.MARGIN


def test_fixture_sizes_and_motions():
    assert [P.case(nm)["seq"]["pairs"][0]["m"].shape[0] for nm in ("mixed48", "eight", "five", "empty", "n257", "n4096", "noisy")] == \
        [48, 8, 5, 0, 257, 4096, 250]
    pr = P.case("forward")["seq"]["pairs"][0]
    e = P.k_matrix(pr["intr"][1]) @ pr["t"]                                # the epipole of view 2: inside the image
    assert 0 < e[0] / e[2] < E.WIDTH and 0 < e[1] / e[2] < E.HEIGHT
    assert P.case("backward")["seq"]["pairs"][0]["t"][2] > 0.9 and pr["t"][2] < -0.9
    k = P.case("mixed48")["seq"]["pairs"][0]["intr"]
    assert k[0, 0] != k[1, 0] and k[0, 2] != k[1, 2]                       # different focal lengths in the two views
    k = P.case("equal_k")["seq"]["pairs"][0]["intr"]
    assert np.array_equal(k[0], k[1])


def test_jacobi_is_section_22s():
    rng = np.random.RandomState(0)
    for _ in range(20):
        A = rng.randn(3, 3)
        d0, V0 = E.jacobi3(A.T @ A)
        d1, V1 = P.jacobi3(A.T @ A)
        assert np.array_equal(d0, d1) and np.array_equal(V0, V1)           # bit for bit


@pytest.mark.parametrize("name", ("mixed48", "forward", "backward", "equal_k", "noisy", "n257"))
def test_decomposition_against_numpy_svd(name):
    c = P.case(name)
    pr, r = c["seq"]["pairs"][0], c["ransac"][0]
    E0 = P.essential(r["F"], pr["intr"])
    assert abs(np.linalg.norm(E0) - 1.0) < 1e-15
    U, V = P.decompose(E0)
    Em, Ra, Rb, u2 = P.candidates(U, V)
    eye = np.eye(3)
    for M in (U, V, Ra, Rb):
        assert np.abs(M.T @ M - eye).max() < 1e-14 and abs(np.linalg.det(M) - 1.0) < 1e-14, name   # proper rotations
    assert np.abs(np.linalg.svd(Em, compute_uv=False) - np.array([1.0, 1.0, 0.0])).max() < 1e-14
    # E is E0 with its singular values replaced by (1, 1, 0): numpy's U diag(1, 1, 0) V^T
    Un, sn, Vtn = np.linalg.svd(E0.reshape(3, 3))
    want = Un @ np.diag([1.0, 1.0, 0.0]) @ Vtn
    # an exact essential matrix has two equal singular values: the SVD's plane basis is then free, the product is not
    slack = 1e-12 if name != "noisy" else 2.0 * (sn[0] - sn[1]) / sn[1] + 1e-12
    assert np.abs(Em - want).max() < slack, (name, np.abs(Em - want).max(), sn)
    W = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    assert np.abs(Ra - U @ W @ V.T).max() < 1e-15 and np.abs(Rb - U @ W.T @ V.T).max() < 1e-15
    assert np.array_equal(c["pose"][0]["E"], Em)


@pytest.mark.parametrize("name", P.NOISE_FREE)
def test_pose_against_truth(name):
    c = P.case(name)
    for pose, pr in zip(c["pose"], c["seq"]["pairs"]):
        dR, dt = P.angle_deg(pose["R"], pr["R"]), P.angle_deg(pose["t"], pr["t"])
        print("%s: rotation off by %.3e deg, t by %.3e deg (bound %.3e)" % (name, dR, dt, P.TRUTH_BOUND_DEG))
        assert dR <= P.TRUTH_BOUND_DEG and dt <= P.TRUTH_BOUND_DEG
        assert abs(np.linalg.norm(pose["t"]) - 1.0) < 1e-15
        # depths with the baseline as the unit: the true depths over the true baseline
        z = pose["depth"][pose["front"]]
        X1 = pose["X"][pose["front"]]
        X2 = X1 @ pr["R"].T + pr["t"]
        assert np.abs(X2[:, 2] - z[:, 1]).max() < 1e-6 * max(1.0, np.abs(z).max()), name
        assert z.min() * pr["length"] > 1.0 and z.max() * pr["length"] < 14.0


def test_measured_bounds():
    t, cen, w = P.truth_error(), P.centre_error(), P.way_difference()
    print("truth error %.17g deg, centre error %.17g, way difference %.17g (longdouble wider: %s)" % (t, cen, w, P.WIDE))
    assert 0.0 < t <= P.TRUTH_BOUND_DEG and 0.0 < cen <= P.CENTRE_BOUND and 0.0 < w <= P.TOLERANCE
    assert P.TOLERANCE == 16.0 * P.WAY_DIFFERENCE and P.TRUTH_BOUND_DEG == 16.0 * P.TRUTH_ERROR_DEG


def test_noisy_fixture_is_compared_with_the_restatement_only():
    c = P.case("noisy")
    a, b = c["pose"][0], c["pose2"][0]
    assert a["status"] == b["status"] == 0 and a["cand"] == b["cand"] and np.array_equal(a["front"], b["front"])
    assert a["n_front"] == c["ransac"][0]["n_inliers"]
    for k in P.POSE_KEYS:
        assert np.abs(a[k] - b[k]).max() <= P.TOLERANCE
    pr = c["seq"]["pairs"][0]
    assert P.angle_deg(a["R"], pr["R"]) < 2.0           # the noise floor of a short baseline, not the arithmetic's


@pytest.mark.parametrize("n", (0, 5, 7))
def test_too_few_inliers_is_no_pose(n):
    pr = P.case("equal_k")["seq"]["pairs"][0]
    m = pr["m"][pr["truth"]][:n]
    o = P.two_view_pose(pr["F"], np.ones(n, dtype=bool), n, 0, m, pr["intr"])
    assert o["status"] == 1 and o["cand"] == -1 and o["n_front"] == 0 and not o["counts"].any()
    assert np.array_equal(o["R"], np.eye(3)) and not o["t"].any() and not o["E"].any()
    assert not o["front"].any() and not o["depth"].any() and not o["X"].any()


def test_input_status_and_degenerate_matrices_are_no_pose():
    pr = P.case("equal_k")["seq"]["pairs"][0]
    m, n = pr["m"], pr["m"].shape[0]
    ones = np.ones(n, dtype=bool)
    assert P.two_view_pose(pr["F"], ones, n, 0, m, pr["intr"])["status"] == 0
    assert P.two_view_pose(pr["F"], ones, n, 1, m, pr["intr"])["status"] == 1
    assert P.two_view_pose(np.zeros(9), ones, n, 0, m, pr["intr"])["status"] == 1            # zero norm
    assert P.two_view_pose(np.full(9, np.nan), ones, n, 0, m, pr["intr"])["status"] == 1
    rank1 = np.outer([1.0, 2.0, 3.0], [0.0, 0.0, 1.0]).reshape(9)                            # E0 v1 = 0: no second singular vector
    assert P.two_view_pose(rank1, ones, n, 0, m, np.array([[1.0, 1.0, 0.0, 0.0]] * 2))["status"] == 1


def salted_scene():
    """20 true matches of the forward-motion pair, 15 points behind both cameras and 15 in front of the first and behind the
    second: all 50 satisfy the epipolar constraint, no candidate puts half of them in front."""
    pr = P.case("forward")["seq"]["pairs"][0]
    rng = np.random.RandomState(5)
    K1, K2 = P.k_matrix(pr["intr"][0]), P.k_matrix(pr["intr"][1])
    t = pr["t"] * pr["length"]
    m = [pr["m"][pr["truth"]][:20]]
    for lo, hi in ((-6.0, -3.0), (0.05, 0.2)):
        X1 = np.stack([rng.uniform(-0.3, 0.3, 15), rng.uniform(-0.3, 0.3, 15), rng.uniform(lo, hi, 15)], axis=1)
        X2 = X1 @ pr["R"].T + t
        assert (X2[:, 2] < 0).all()
        a, b = X1 @ K1.T, X2 @ K2.T
        m.append(np.concatenate([a[:, :2] / a[:, 2:], b[:, :2] / b[:, 2:]], axis=1))
    return pr, np.concatenate(m)


def test_salted_mask_is_ambiguous_and_the_winner_is_still_reported():
    pr, m = salted_scene()
    d2, _ = E.sampson2(pr["F"].reshape(1, 9) / np.linalg.norm(pr["F"]), m)
    assert d2.max() < 1e-12                                      # all 50 rows fit F
    o = P.two_view_pose(pr["F"], np.ones(50, dtype=bool), 50, 0, m, pr["intr"])
    assert o["status"] == 2 and o["n_front"] == 20 and sorted(o["counts"]) == [0, 15, 15, 20]
    assert np.array_equal(o["front"], np.arange(50) < 20) and not o["depth"][20:].any()
    assert P.angle_deg(o["R"], pr["R"]) < 1e-6 and P.angle_deg(o["t"], pr["t"]) < 1e-6
    # fewer than 8 in front is ambiguous as well, however few the inliers
    mask = np.zeros(50, dtype=bool)
    mask[:7] = mask[20:23] = True
    o = P.two_view_pose(pr["F"], mask, 10, 0, m, pr["intr"])
    assert o["status"] == 2 and o["n_front"] == 7 and o["cand"] >= 0


@pytest.mark.parametrize("name", ("seq3", "seq5"))
def test_chain_reproduces_the_true_centres_up_to_scale(name):
    c = P.case(name)
    rows, seq = c["rows"], c["seq"]
    frames = P.CASES[name][1]
    assert rows.shape == (frames - 1, P.ROW_WORDS) and c["state"]["n_frames"] == frames - 1
    assert rows[0, 12] == 1.0 and rows[0, 14] == P.FLAG_SCALE_CARRIED and rows[0, 13] == 0       # the first pair has s = 1
    assert (rows[1:, 14] == 0).all() and (rows[1:, 13] == seq["n_in"]).all()
    want = seq["centres"][1:] / np.linalg.norm(seq["centres"][1])
    err = np.abs(P.scaled_centres(rows) - want).max()
    print("%s: centres off by %.3e (bound %.3e)" % (name, err, P.CENTRE_BOUND))
    assert err <= P.CENTRE_BOUND
    lengths = np.array([pr["length"] for pr in seq["pairs"]])
    assert np.abs(rows[:, 12] - lengths / lengths[0]).max() < 1e-9                                # s is the baseline over the first
    for f in range(frames - 1):                                                                   # Rw against the true world rotation
        Rt = np.eye(3)
        for pr in seq["pairs"][:f + 1]:
            Rt = pr["R"] @ Rt
        assert P.angle_deg(rows[f, :9].reshape(3, 3), Rt) < 1e-6


def test_chain_status_and_shared_point_rules():
    c = P.case("seq5")
    poses, matches = list(c["pose"]), [pr["match"] for pr in c["seq"]["pairs"]]
    n = matches[0].shape[0]
    none = P.two_view_pose(np.zeros(9), np.zeros(n, dtype=bool), 0, 1, c["seq"]["pairs"][1]["m"], c["seq"]["pairs"][1]["intr"])
    rows, _ = P.run_chain([poses[0], none, poses[2], poses[3]], matches)
    assert list(rows[:, 14]) == [2, 3, 2, 0]                  # no pose in the middle: bit 0; the scale is carried until two poses meet
    assert np.array_equal(rows[1, :12], rows[0, :12])         # the centre (and Rw) repeat
    assert rows[1, 12] == rows[0, 12] == rows[2, 12] == 1.0 and rows[3, 12] == rows[3, 15] != 1.0
    # fewer than 8 shared points: pair 1 keeps only 5 of the rows whose points pair 0 saw in front
    few = dict(poses[1])
    keep = np.nonzero(few["front"])[0][:5]
    few["front"] = np.zeros(n, dtype=bool)
    few["front"][keep] = True
    rows, _ = P.run_chain([poses[0], few, poses[2]], matches[:3])
    assert rows[1, 13] == 5 and rows[1, 14] == P.FLAG_SCALE_CARRIED and rows[1, 12] == 1.0 and rows[1, 15] > 0


def test_chain_duplicate_j_lowest_row_wins():
    c = P.case("seq3")
    a, b = dict(c["pose"][0]), c["pose"][1]
    ma, mb = c["seq"]["pairs"][0]["match"].copy(), c["seq"]["pairs"][1]["match"]
    fr = np.nonzero(a["front"])[0]
    lo, hi = int(fr[3]), int(fr[10])
    ma[hi, 1] = ma[lo, 1]                                        # two rows of A name the same point of frame f
    a["depth"] = a["depth"].copy()
    a["depth"][hi, 1] = 1000.0                                   # the higher row's depth must not be used
    st = P.new_state()
    row, _ = P.chain_step(a, b, ma, mb, ma.shape[0], mb.shape[0], st, ma.shape[0], mb.shape[0])
    ref, _ = P.chain_step(c["pose"][0], b, c["seq"]["pairs"][0]["match"], mb, ma.shape[0], mb.shape[0], st, ma.shape[0], mb.shape[0])
    assert row[13] == ref[13] - 1 and row[15] < 2.0              # the point row `hi` named is no longer shared
    a["depth"][lo, 1] = 1000.0
    row2, _ = P.chain_step(a, b, ma, mb, ma.shape[0], mb.shape[0], st, ma.shape[0], mb.shape[0])
    assert row2[15] > 2.0                                        # ... and the lower row's is
