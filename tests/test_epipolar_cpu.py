"""The rules of the fundamental-matrix RANSAC as tests/epipolar_ref.py restates them: hand-checked
pieces (complete pivoting with ties, the Jacobi sweeps, the rank-2 step), the small match counts, synthetic two-view scenes
with known truth, and the summation-order measurement the device tolerance comes from.  No GPU."""
import numpy as np
import pytest

from tests import epipolar_ref as E

# (inliers, outliers) -> scene seeds; the RANSAC seed is 100 + the scene seed.  Searched with the restatement: the 25 px
# margin of the outliers does not by itself make the winner's mask equal the truth with few matches.
SCENES = {(32, 16): (0, 1, 2), (150, 100): (0, 1), (40, 40): (0, 1, 2), (24, 8): (0, 1, 2), (20, 12): (0, 1, 2),
          (8, 0): (0, 1, 2), (9, 0): (0, 1, 2)}


def _sampson(F, m):
    d2, usable = E.sampson2(np.asarray(F, dtype=np.float64).reshape(1, 9), m)
    assert usable.all()
    return np.sqrt(d2[0])


@pytest.mark.parametrize("n_in,n_out", sorted(SCENES))
def test_scenes_with_known_truth(n_in, n_out):
    for seed in SCENES[(n_in, n_out)]:
        sc = E.make_scene(seed, n_in, n_out)
        d1, d2 = E.line_dist(sc["F"], sc["m"][~sc["truth"], :2], sc["m"][~sc["truth"], 2:])
        assert n_out == 0 or min(d1.min(), d2.min()) >= E.MARGIN
        assert _sampson(sc["F"] / np.linalg.norm(sc["F"]), sc["m"][sc["truth"]]).max() < 1e-11   # exact projections
        r = E.ransac(sc["m"], 100 + seed)
        assert r["status"] == 0 and np.array_equal(r["mask"], sc["truth"]), (n_in, n_out, seed, r["winner"], r["n_inliers"])
        assert r["n_inliers"] == n_in and 0 <= r["winner"] < (1 if n_in + n_out == 8 else E.HYPOTHESES)
        assert _sampson(r["F"], sc["m"][sc["truth"]]).max() < 1e-11
        s = np.linalg.svd(r["F"], compute_uv=False)
        assert s[2] / s[0] < 1e-15
        assert abs(np.linalg.norm(r["F"]) - 1.0) < 1e-15 and r["F"].ravel()[np.argmax(np.abs(r["F"]))] > 0.0
        t = sc["F"] / np.linalg.norm(sc["F"])
        t = t if t.ravel()[np.argmax(np.abs(t))] > 0 else -t
        assert np.abs(r["F"] - t).max() < 1e-9
        assert r["err"] < 1e-11


def test_complete_pivoting_ties():
    """A diagonal-plus-one-entry matrix whose largest |entry| 5 occurs at (1,1), (1,7) [as -5], (2,2) and (4,4): the lowest row
    wins, then the lowest column; the pivots that follow are worked out by hand."""
    diag = [2.0, 5.0, 5.0, 1.0, 5.0, 3.0, 4.0, 0.5]
    A = np.zeros((8, 9))
    A[np.arange(8), np.arange(8)] = diag
    A[1, 7] = -5.0
    A[:, 8] = [0.25, -0.125, 0.0625, 0.25, -0.25, 0.125, 0.03125, 0.25]
    trace = []
    f, ok = E.null_vector(A[None], trace=trace)
    assert ok[0]
    # step 0: (1,1) (row 1 before rows 2 and 4, column 1 before column 7); the swaps move the 2 of (0,0) to (1,1).  step 1:
    # (2,2) before (4,4); the 2 moves to (2,2).  step 2: (4,4); the 2 moves to (4,4).  step 3: the 4 at (6,6); the 1 moves
    # there.  step 4: the 3 at (5,5); the 2 moves there.  Then 2 at (5,5), 1 at (6,6), 0.5 at (7,7).
    assert trace == [(1, 1), (2, 2), (4, 4), (6, 6), (5, 5), (5, 5), (6, 6), (7, 7)]
    assert f[0, 8] == 1.0 and np.abs(A @ f[0]).max() < 1e-16
    want = np.array([-0.25 / 2, 0.0, -0.0625 / 5, -0.25, 0.25 / 5, -0.125 / 3, -0.03125 / 4, -0.5, 1.0])
    want[1] = (0.125 + 5.0 * want[7]) / 5.0
    assert np.allclose(f[0], want, rtol=0, atol=1e-16)
    # a pivot at the limit is refused, one just above it is taken
    B = A.copy()
    B[7, 7], B[7, 8] = 1e-12, 1e-13
    assert not E.null_vector(B[None])[1][0]
    B[7, 7] = 1.0000001e-12
    assert E.null_vector(B[None])[1][0]


def test_null_vector_of_random_systems():
    rng = np.random.RandomState(5)
    A = rng.randn(64, 8, 9)
    f, ok = E.null_vector(A)
    assert ok.all()
    for b in range(64):
        v = np.linalg.svd(A[b])[2][-1]
        g = f[b] / np.linalg.norm(f[b])
        assert min(np.abs(g - v).max(), np.abs(g + v).max()) < 1e-12


def test_jacobi_against_eigh():
    rng = np.random.RandomState(6)
    for k in range(50):
        Fm = rng.randn(3, 3) * (10.0 ** rng.uniform(-3, 3))
        if k % 5 == 0:
            Fm[:, 2] = 0.0           # exact zeros off the diagonal: the skipped rotations
        G = Fm.T @ Fm
        d, V = E.jacobi3(G)
        w, _ = np.linalg.eigh(G)
        assert np.allclose(np.sort(d), w, rtol=1e-13, atol=1e-15 * abs(w).max())
        assert np.abs(V.T @ V - np.eye(3)).max() < 1e-14
        assert np.abs(G @ V - V * d[None, :]).max() < 1e-13 * abs(w).max()
    d, V = E.jacobi3(np.diag([3.0, 1.0, 2.0]))
    assert list(d) == [3.0, 1.0, 2.0] and np.array_equal(V, np.eye(3))


def test_rank2_against_svd():
    rng = np.random.RandomState(7)
    for _ in range(50):
        Fm = rng.randn(3, 3)
        U, s, Vt = np.linalg.svd(Fm)
        want = (U[:, :2] * s[:2]) @ Vt[:2]
        got = E.rank2(Fm.ravel()).reshape(3, 3)
        assert np.abs(got - want).max() < 1e-13
        assert np.linalg.svd(got, compute_uv=False)[2] < 16 * np.finfo(np.float64).eps * s[0]   # a few roundings of sigma1


@pytest.mark.parametrize("n", (0, 7, 8, 9))
def test_small_match_counts(n):
    sc = E.make_scene(11, n, 0)
    r = E.ransac(sc["m"], 5)
    if n < 8:
        assert r["status"] == 1 and r["winner"] == -1 and r["n_inliers"] == 0 and not r["mask"].any()
        assert not r["F"].any() and r["err"] == 0.0
        return
    assert r["status"] == 0 and r["mask"].all() and r["n_inliers"] == n
    assert (r["winner"] == 0) if n == 8 else (0 <= r["winner"] < E.HYPOTHESES)
    assert E.sample8(5, 0, 8) == list(range(8)) and E.sample8(5, 123, 8) == list(range(8))
    assert _sampson(r["F"], sc["m"]).max() < 1e-11


def test_sampler_follows_the_four_point_rule():
    from tests import eval_restatement as ER
    for (seed, h, n) in ((1, 0, 9), (77, 1999, 12), (3, 5, 300)):
        ids = E.sample8(seed, h, n)
        assert ids is not None and len(set(ids)) == 8 and all(0 <= v < n for v in ids)
        assert ids[0] == ER.draw(seed, h, 0, n)
        four = ER.sample(seed, h, n)
        assert four is None or ids[:4] == four     # the same stream and redraw rule, carried on to 8


def test_planar_scene_is_answered():
    """All points on one plane: every 8-point system has rank 6.  For this fixture the restatement refuses all 2000 by the
    pivot limit (status 1; tests/test_epipolar_exact_cpu.py asserts that and the margin, 5.2e-16 against 1e-12).  The rule
    itself is wider: were a system to pass, the answer would be an arbitrary member of the family that fits the plane, with
    status 0 and a mask that is the winner's inlier set."""
    c = E.case("planar")
    r = c["ref"]
    assert r["status"] in (0, 1)
    again = E.ransac(c["m"], c["seed"])
    assert again["status"] == r["status"] and again["winner"] == r["winner"] and np.array_equal(again["mask"], r["mask"])
    if r["status"] == 0:
        assert np.array_equal(r["mask"], E.inliers(r["F_winner"].reshape(1, 9), c["m"], 1.0)[0]) and r["n_inliers"] >= 8
        assert np.linalg.svd(r["F"], compute_uv=False)[2] < 1e-15


def test_refit_lowers_the_error_under_noise():
    c = E.case("noisy")
    r = c["ref"]
    assert r["status"] == 0 and r["n_inliers"] >= 100
    mi = c["m"][r["mask"]]
    before = np.mean(_sampson(r["F_winner"], mi))
    after = np.mean(_sampson(r["F"], mi))
    assert after < before and abs(np.sqrt(np.mean(_sampson(r["F"], mi) ** 2)) - r["err"]) < 1e-12


def test_fixture_masks_equal_truth():
    """The noise-free fixtures of the GPU tests: the restatement's mask is the truth (asserted here, on the CPU, first)."""
    for nm in E.NOISE_FREE:
        c = E.case(nm)
        assert c["ref"]["status"] == 0 and np.array_equal(c["ref"]["mask"], c["truth"]), nm
    assert E.case("five")["ref"]["status"] == 1 and E.case("empty")["ref"]["status"] == 1


def test_tolerance_is_the_measured_order_difference():
    """The device tolerance is 16 x the largest difference between the ascending and the pairwise refit over the compared
    fixtures; the recorded figure is what this measurement gives."""
    d = E.order_difference(E.F_COMPARED)
    print("order difference", d, "tolerance", 16.0 * d)
    assert d == pytest.approx(E.ORDER_DIFFERENCE, rel=1e-6)
    assert E.TOLERANCE == 16.0 * E.ORDER_DIFFERENCE
