"""The numpy restatement of the absolute pose from landmarks (tests/pnp_ref.py) against the truth, against
numpy's own root finder and solver, and against itself in another number format.  No GPU.

Masks first: on every noise-free fixture (the salted ones included) the restatement's mask equals the truth; the seeds were
searched until it did.  The measured figures (pnp_ref.WAY_DIFFERENCE, TRUTH_ERROR, SEQUENCE_CENTRE_ERROR) are repeated here; the
bounds the device tests use are 16 times them."""
import numpy as np
import pytest

from tests import epipolar_ref as E
from tests import landmarks_ref as L
from tests import pose_ref as P
from tests import pnp_ref as R


def test_masks_equal_the_truth_on_every_noise_free_fixture():
    for name in R.NOISE_FREE:
        c = R.case(name)
        r = c["res"] if name != "four" else R.ransac(c["corr"], c["n"], c["k"], c["seed"], min_inliers=4)
        assert r["status"] == 0, name
        assert np.array_equal(r["mask"], c["truth"]), name            # no true row dropped, no salted row kept
        assert r["n_inliers"] == int(c["truth"].sum()) and r["n_inliers"] >= r["score"], name
    for name in ("n257", "n4096", "salted", "planar"):                # the salt, the rows behind the camera, the invalid rows
        c = R.case(name)
        assert 0.25 * c["n"] < (~c["truth"]).sum() < 0.4 * c["n"] and (c["corr"][:, 6] == 0.0).sum() >= 2, name
    c = R.case("planar")
    X = c["corr"][c["truth"], :3]
    assert np.linalg.svd(X - X.mean(axis=0), compute_uv=False)[2] < 1e-9      # a plane: P3P does not need depth variety
    c = R.case("noisy")
    assert c["res"]["status"] == 0 and 0.2 < float(c["res"]["rms"]) < 0.4 and c["res"]["n_inliers"] == c["n"]


def test_quartic_roots_agree_with_numpy_and_hit_the_true_pose():
    B = 2000
    X, px, k, Rw, C = R.random_samples(5, B)
    g, roots, valid = R.sample_quartics(X, px, k)
    g = np.stack(g, axis=1)
    found = unfound = in_range = 0
    for b in range(B):
        want = np.roots(g[b, ::-1])
        real = want[(np.abs(want.imag) < 1e-9) & (want.real > 0.0) & (want.real <= R.V_MAX)].real
        got = np.array([roots[r][b] for r in range(4) if valid[r][b]])
        for v in got:                                                  # every root found is a root
            assert np.abs(want - v).min() <= 1e-7 * max(1.0, v), (b, v, want)
        found += got.size
        in_range += real.size
        unfound += sum(1 for v in real if not (got.size and np.abs(got - v).min() <= 1e-7 * max(1.0, v)))
    print("roots found %d, real roots of numpy.roots in range %d, of those not found %d" % (found, in_range, unfound))
    assert found >= B and unfound < 0.01 * in_range                     # (the true ratio is a root of every sample)
    # the true pose is among the solutions; the misses (near-double roots) are counted, not skipped
    err = np.full(B, np.inf)
    for Rr, Cc, ok in R.p3p(X, px, k, want_all=True):
        e = np.maximum(np.abs(np.stack(Rr, axis=1) - Rw).max(axis=1), np.abs(np.stack(Cc, axis=1) - C).max(axis=1))
        err = np.where(ok & (e < err), e, err)
    missed = int((err > 1e-6).sum())
    print("no solution within 1e-6 of the truth: %d of %d" % (missed, B))
    assert missed < 0.01 * B
    Rb, Cb, ok = R.p3p(X, px, k)                                        # and the fourth row picks it
    e = np.maximum(np.abs(np.stack(Rb, axis=1) - Rw).max(axis=1), np.abs(np.stack(Cb, axis=1) - C).max(axis=1))
    assert int((~ok | (e > 1e-6)).sum()) < 0.01 * B


def test_small_and_degenerate_inputs():
    c = R.case("side48")
    for n in (0, 3, 4, 5):
        r = R.ransac(c["corr"], n, c["k"], 11)
        assert r["status"] == 1 and r["winner"] == -1 and not r["mask"].any() and r["n_inliers"] == 0, n
        assert np.array_equal(r["Rw"], np.eye(3)) and not r["C"].any()
    r = R.ransac(c["corr"], 4, c["k"], 11, min_inliers=4)               # the single hypothesis of rows 0..3
    assert r["status"] == 0 and r["winner"] == 0 and r["n_inliers"] == 4 and r["mask"][:4].all() and not r["mask"][4:].any()
    assert R.total_hypotheses(4) == 1 and R.sample4(11, 0, 4, np.ones(4, bool)) == [0, 1, 2, 3]
    assert np.abs(r["Rw"] - c["Rw"]).max() < 1e-9 and np.abs(r["C"] - c["C"]).max() < 1e-9
    five = R.ransac(c["corr"], 5, c["k"], 11, min_inliers=5)
    assert five["status"] == 0 and five["n_inliers"] == 5
    bad = c["corr"].copy()                                              # four rows, one invalid: no hypothesis
    bad[2, 6] = 0.0
    assert R.ransac(bad, 4, c["k"], 11, min_inliers=4)["status"] == 1
    # a collinear and a coincident triple are refused
    X, px, k, _, _ = R.random_samples(6, 8)
    for make in (lambda a, b: [0.5 * (a[i] + b[i]) for i in range(3)], lambda a, b: list(a)):
        Xc = [X[0], X[1], make(X[0], X[1]), X[3]]
        assert not R.p3p(Xc, px, k)[2].any()
    # draws: 4 distinct valid rows, the invalid ones never drawn
    valid = np.ones(12, bool)
    valid[[1, 5, 6]] = False
    for h in range(64):
        ids = R.sample4(3, h, 12, valid)
        assert ids is None or (len(set(ids)) == 4 and valid[ids].all())
    assert sum(R.sample4(3, h, 12, valid) is not None for h in range(64)) >= 60
    assert R.sample4(3, 0, 5, np.array([1, 1, 1, 0, 0], bool)) is None


def test_join_takes_the_lowest_landmark_row_and_clamps():
    lm = np.zeros((8, L.LANDMARK_WORDS))
    lm[:, 1:4] = np.arange(24).reshape(8, 3) + 1.0
    lm[:, 7] = [2, 0, 2, -1, 5, 99, 0, 3]                               # duplicates of 2 and 0, no newest point, past the frame
    pts = np.arange(12, dtype=np.float64).reshape(6, 2)
    match = np.array([[0, 1, .1], [2, 0, .2], [3, 3, .3], [5, 5, .4], [4, 2, .5], [7, 9, .6], [2, 4, .7]], dtype=np.float32)
    corr, (n, nv) = R.join(lm, 7, match, 7, pts)                         # row 7 of the landmarks lies past n_landmarks
    assert n == 7 and nv == 5
    assert corr[:, 6].tolist() == [1, 1, 0, 1, 0, 1, 1]
    assert corr[:, 5].tolist() == [1, 0, 0, 4, 0, 4, 0]                  # lowest rows; (7, 9) is clamped to (5, 5)
    assert np.array_equal(corr[1, :5], [1, 2, 3, 0, 1]) and np.array_equal(corr[5, :5], [13, 14, 15, 10, 11])
    assert not corr[[2, 4]].any()
    assert R.join(lm, 0, match, 7, pts)[1] == (7, 0) and R.join(lm, 8, match, 0, pts)[1] == (0, 0)
    assert R.join(lm, 8, match, 7, pts)[0][2, 6] == 1.0                  # with all 8 rows, point 3 has a landmark
    lm[1, 2] = np.nan                                                   # a landmark that is not finite gives no row
    assert R.join(lm, 7, match, 7, pts)[0][0, 6] == 0.0


def test_refit_parts():
    rng = np.random.RandomState(3)
    worst = 0.0
    for _ in range(200):
        Rw = P._rodrigues(rng.uniform(-40, 40, 3)).reshape(9)
        t = rng.uniform(-2, 2, 3)
        delta = np.concatenate([rng.uniform(-0.5, 0.5, 3), rng.uniform(-1, 1, 3)])
        Rn, tn = R.cayley_update(Rw, t, delta)
        M = Rn.reshape(3, 3)
        worst = max(worst, float(np.abs(M.T @ M - np.eye(3)).max()))
        a = 0.5 * delta[:3]                                             # the Cayley map is the rotation by 2 atan(|a|) about a
        th = 2.0 * np.arctan(np.linalg.norm(a))
        want = P._rodrigues(np.degrees(a / np.linalg.norm(a) * th)) @ Rw.reshape(3, 3)
        assert np.abs(M - want).max() < 1e-13 and np.abs(tn - (want @ Rw.reshape(3, 3).T @ t + delta[3:])).max() < 1e-13
        assert np.linalg.det(M) > 0.999
    print("largest |R^T R - I| after the update: %.3e" % worst)
    assert worst <= 8 * np.finfo(np.float64).eps
    for _ in range(100):
        J = rng.randn(12, 6)
        A, b = J.T @ J, rng.randn(6)
        x, ok = R.solve_pivot(np.concatenate([A, b[:, None]], axis=1))
        want = np.linalg.solve(A, b)
        assert ok and np.abs(x - want).max() <= 1e-9 * max(1.0, np.abs(want).max())
    x, ok = R.solve_pivot(np.concatenate([np.zeros((6, 6)), np.ones((6, 1))], axis=1))
    assert not ok


def test_the_pivoting_is_section_22s():
    """solve_pivot on an 8 x 9 system takes epipolar_ref.null_vector's pivots and gives its result to the last bit whenever the
    ninth column never holds the largest entry (null_vector may pivot on it, a solver may not)."""
    rng = np.random.RandomState(4)
    for _ in range(20):
        A = rng.randn(8, 8)
        b = 1e-3 * rng.randn(8)
        t1, t2 = [], []
        f, ok1 = E.null_vector(np.concatenate([A, b[:, None]], axis=1)[None], trace=t1)
        x, ok2 = R.solve_pivot(np.concatenate([A, -b[:, None]], axis=1), trace=t2)
        assert ok1[0] and ok2 and t1 == t2 and f[0, 8] == 1.0
        assert np.array_equal(f[0, :8], x)


def test_block_sum_is_the_kernels_order():
    rng = np.random.RandomState(8)
    v = rng.randn(700, 3) * 10.0 ** rng.uniform(-6, 6, (700, 1))
    act = rng.rand(700) < 0.7
    got = R.block_sum(v, act)
    part = np.zeros((256, 3))
    for i in range(700):                                               # thread i % 256 adds row i
        if act[i]:
            part[i % 256] = part[i % 256] + v[i]
    red = []
    for w in range(4):
        lanes = part[64 * w:64 * w + 64].copy()
        for o in (32, 16, 8, 4, 2, 1):
            lanes = np.stack([lanes[l] + lanes[l ^ o] for l in range(64)])
        red.append(lanes[0])
    assert np.array_equal(got, ((red[0] + red[1]) + red[2]) + red[3])
    assert np.abs(got - v[act].sum(axis=0)).max() <= 1e-9 * np.abs(v[act]).sum()


def _flagged_table():
    table = np.zeros((6, P.ROW_WORDS))
    table[:, [0, 4, 8]] = 1.0
    table[:, 12] = [1.0, 1.0, 0.8, 0.8, 0.0, 0.0]
    table[:, 14] = [3, 2, 0, 3, 0, 0]
    table[1, 9:12], table[2, 9:12], table[3, 9:12] = [1.0, 0, 0], [1.8, 0.1, 0], [1.8, 0.1, 0]
    state = np.zeros(P.STATE_WORDS)
    state[0], state[1], state[2:11], state[11:14] = 4, 0.8, table[3, :9], [-1.8, -0.1, 0.0]
    return state, table


def test_repair_rule():
    state, table = _flagged_table()
    Rw = P._rodrigues(np.array([3.0, -8.0, 2.0]))
    good = {"Rw": Rw, "C": np.array([2.5, 0.2, -0.1]), "status": 0}
    s1, t1 = R.repair(good, state, table)
    assert np.array_equal(t1[3, :9], Rw.reshape(9)) and np.array_equal(t1[3, 9:12], good["C"]) and t1[3, 14] == R.FLAG_ABSOLUTE
    step = np.linalg.norm(good["C"] - table[2, 9:12])
    assert abs(t1[3, 12] - step) < 1e-15 and s1[1] == t1[3, 12] and s1[0] == 4
    assert np.array_equal(s1[2:11], Rw.reshape(9)) and np.abs(s1[11:14] + Rw @ good["C"]).max() < 1e-15
    assert np.array_equal(t1[[0, 1, 2, 4, 5]], table[[0, 1, 2, 4, 5]]) and np.array_equal(t1[3, [13, 15]], table[3, [13, 15]])
    # an unflagged row, an absolute pose without status 0, a pose that is not finite, a full table, an empty one: bit-identical
    unflagged = table.copy()
    unflagged[3, 14] = 0.0
    cases = [(good, state, unflagged), (dict(good, status=1), state, table), (dict(good, C=np.array([np.nan, 0, 0])), state, table),
             (good, state, table[:4])]
    empty = state.copy()
    empty[0] = 0.0
    cases.append((good, empty, table))
    for a, s, t in cases:
        s2, t2 = R.repair(a, s, t)
        assert np.array_equal(s2, s) and np.array_equal(t2, t)
    # a step too short to set the scale: s is kept, bit 1 stays; where bit 1 was clear it stays clear
    near = dict(good, C=table[2, 9:12] + np.array([0.8 / 65.0, 0.0, 0.0]))
    s3, t3 = R.repair(near, state, table)
    assert t3[3, 12] == 0.8 and s3[1] == 0.8 and t3[3, 14] == (2 | R.FLAG_ABSOLUTE)
    only0 = table.copy()
    only0[3, 14] = 1.0
    assert R.repair(near, state, only0)[1][3, 14] == R.FLAG_ABSOLUTE
    # bit 2 is no break for the window
    assert L.window_start(t1[:, 14], 4, 5, 6) == 0 and L.window_start(table[:, 14], 4, 5, 6) == 3


@pytest.fixture(scope="module")
def broken_runs():
    seq = R.broken_sequence()
    seed0 = P.case(R.BROKEN[0])["seeds"][0] - 1
    return seq, {mode: R.run_sequence(seq, 5, 64, mode, seed0) for mode in (None, "observe", "repair")}


def test_repair_mends_the_broken_sequence(broken_runs):
    seq, runs = broken_runs
    plain, observe, repair = (runs[m] for m in (None, "observe", "repair"))
    assert seq["pairs"][R.BROKEN[1]]["match"].shape[0] == R.BROKEN[2] < 8
    assert [p["status"] for p in plain["pose"]] == [1, 0, 0, 1, 0]
    assert plain["table"][:, 14].tolist() == [3, 2, 0, 3, 2]
    assert np.array_equal(observe["table"], plain["table"])                        # observing changes nothing
    assert np.array_equal(observe["tracks"].ids, plain["tracks"].ids)
    assert [a is not None and a["status"] == 0 for a in observe["absolute"]] == [False, False, True, True, False]
    assert observe["absolute"][3]["n_inliers"] == R.BROKEN[2] and observe["corr"][3][2] == R.BROKEN[2]
    assert repair["table"][:, 14].tolist() == [3, 2, 0, 4, 4]
    assert L.window_start(repair["table"][:, 14], 5, 5, 6) == 0 and L.window_start(plain["table"][:, 14], 5, 5, 6) == 3
    err, err_plain = R.sequence_centre_error(seq, repair["table"]), R.sequence_centre_error(seq, plain["table"])
    print("centres against the truth, first baseline = 1: repaired %.3e (recorded %.3e), unrepaired %.3e"
          % (err, R.SEQUENCE_CENTRE_ERROR, err_plain))
    assert err <= R.SEQUENCE_CENTRE_ERROR * 1.0000001 and err_plain > 0.1
    unit = seq["pairs"][0]["length"]                                               # every absolute pose is the true camera, in the chain's unit
    Rws, Cs = L.true_poses(seq)
    for f in (2, 3, 4):
        a = repair["absolute"][f]
        assert a["status"] == 0 and np.abs(a["Rw"] - Rws[f]).max() < 1e-11 and np.abs(a["C"] - Cs[f] / unit).max() < 1e-11
    assert (repair["landmarks"][4][:, 4] == 5).sum() == R.BROKEN[2] and plain["landmarks"][4][:, 4].max() == 2    # views of a landmark


def test_slow_camera_inside_one_window():
    """The newest of 16 slow frames against the landmarks of the 15 before it (L = 16, true cameras): the true camera comes out."""
    c = R.slow_problem()
    r = c["res"]
    assert c["landmarks"].shape[0] >= 30 and c["landmarks"][:, 4].max() == 15 and c["n_valid"] >= 30
    assert r["status"] == 0 and np.array_equal(r["mask"], c["truth"]) and r["n_inliers"] == int(c["truth"].sum()) >= 30
    err = max(float(np.abs(r["Rw"] - c["Rw"]).max()), float(np.abs(r["C"] - c["C"]).max()))
    print("slow camera: %d landmarks, %d correspondences, |pose - truth| %.3e" % (c["landmarks"].shape[0], c["n_valid"], err))
    assert err <= 16.0 * (L.TRUTH_ERROR + R.TRUTH_ERROR)      # the landmarks carry the triangulation's own error on top of the solve's


def test_tolerance_and_truth_bound_are_the_measured_ones():
    d = R.way_difference()
    print("largest WAY1 / WAY2 difference of Rw, C, rms: %.3e (recorded %.3e, tolerance %.3e)" % (d, R.WAY_DIFFERENCE, R.TOLERANCE))
    assert d <= R.WAY_DIFFERENCE * 1.0000001 and R.TOLERANCE == 16.0 * R.WAY_DIFFERENCE
    if P.WIDE:
        assert d > 0.0
    worst = max(max(R.truth_error(nm)) for nm in R.NOISE_FREE if nm != "four")
    print("largest |Rw - truth|, |C - truth| on the noise-free fixtures: %.3e (recorded %.3e)" % (worst, R.TRUTH_ERROR))
    assert worst <= R.TRUTH_ERROR * 1.0000001 and R.TRUTH_BOUND == 16.0 * R.TRUTH_ERROR
