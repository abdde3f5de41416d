"""The loop-closure restatement (tests/loop_ref.py) against what it must compute: the block tridiagonal plus
low-rank solve against numpy's dense solve, the pose graph on a consistent loop, a planted drift and a transformed world, the edge
rule, the join against old rows and the write-back through hand-made cases.  No GPU."""
import numpy as np
import pytest

from tests import loop_ref as G
from tests import pose_ref as P
from tests import world_ref as W

LD = np.longdouble


@pytest.mark.parametrize("m,n_inner", [(m, k) for m in (1, 2, 3, 7, 8, 9, 65) for k in (0, 1, 8) if m >= 2 or k == 0])
def test_solve_against_dense(m, n_inner):
    """Block cyclic reduction plus Woodbury against numpy.linalg.solve on the assembled matrix; the bound is 16 times the
    restatement's own float64 / longdouble difference on the same inputs.  (A both-ends-free edge needs two free nodes.)"""
    D, U, b, inner = G.solve_case(m, n_inner, 100 * m + n_inner)
    x = G.solve_tridiagonal_low_rank(D, U, b, inner)
    wide = G.solve_tridiagonal_low_rank(D.astype(LD), U.astype(LD), b.astype(LD), [(p, q, a.astype(LD), c.astype(LD)) for p, q, a, c in inner])
    dense = np.linalg.solve(G.assemble_dense(D, U, inner), b.reshape(-1)).reshape(m, 7)
    way = float(np.abs(x - wide).max())
    got = float(np.abs(x - dense).max())
    print("m %d inner %d: against dense %.3e, float64 / longdouble %.3e" % (m, n_inner, got, way))
    assert P.WIDE and way > 0.0
    assert got <= 16.0 * way


def test_jacobians_against_differences():
    rng = np.random.RandomState(0)
    n = 5
    Ri, Rj = np.stack([G._rot(rng.randn(3) * 20) for _ in range(n)]), np.stack([G._rot(rng.randn(3) * 20) for _ in range(n)])
    Ci, Cj, li, lj = rng.randn(n, 3), rng.randn(n, 3), rng.randn(n) * 0.1, rng.randn(n) * 0.1
    Rz = np.stack([Rj[k] @ Ri[k].T @ G._rot(rng.randn(3) * 5) for k in range(n)])
    tz, lz = rng.randn(n, 3), rng.randn(n) * 0.1
    bz = np.linalg.norm(tz, axis=1)
    r, Ji, Jj = G._residuals(Ri, Ci, li, Rj, Cj, lj, Rz, tz, lz, bz)
    eps = 1e-6
    for side, J in ((0, Ji), (1, Jj)):
        for c in range(7):
            d = np.zeros((n, 7))
            d[:, c] = eps
            args = [Ri, Ci, li, Rj, Cj, lj]
            args[3 * side], args[3 * side + 1], args[3 * side + 2] = (G._cayley(args[3 * side], d[:, :3]), args[3 * side + 1] + d[:, 3:6],
                                                                      args[3 * side + 2] + d[:, 6])
            r2, _, _ = G._residuals(*args, Rz, tz, lz, bz, want_jacobian=False)
            assert np.abs((r2 - r) / eps - J[:, :, c]).max() < 1e-5


def test_consistent_loop_is_left_alone():
    table, edges, state, f = G.consistent_case()
    Rw, C, sigma, info = G.pose_graph(table, edges, state, f)
    assert info[0] == 1.0 and info[1] == 0.0 and info[5] == 0.0
    assert (Rw == table[:, 0:9]).all() and (C == table[:, 9:12]).all() and (sigma == 1.0).all()


def test_nothing_to_do_without_an_accepted_edge():
    _, table, edges, state, f = G.graph_case(10, 0)
    state[G.ACCEPTED] = 0
    Rw, C, sigma, info = G.pose_graph(table, edges, state, f)
    assert info[0] == 1.0 and (C == table[:, 9:12]).all() and (Rw == table[:, 0:9]).all() and (sigma == 1.0).all()


def test_planted_drift():
    """64 frames on a circuit; rows a + 1 .. f drift by one constant twist, shift and scale factor 1.002 per edge; the loop edge is
    the truth.  The cost falls and every free node's centre error falls (by 7.3 in the largest error, 1.0033 at the least: the
    first free node, whose error was one step's drift)."""
    a, m = 3, 60
    truth, table, edges, state, f = G.graph_case(m, 0, a=a)
    assert f + 1 == 64
    trace = []
    Rw, C, sigma, info = G.pose_graph(table, edges, state, f, trace=trace)
    assert info[0] == 0.0 and info[3] == m and info[4] == m + 1 and info[6] == 0.0
    assert info[2] < info[1]
    before = np.linalg.norm(table[a + 1:f + 1, 9:12] - truth[a + 1:f + 1, 9:12], axis=1)
    after = np.linalg.norm(C[a + 1:f + 1] - truth[a + 1:f + 1, 9:12], axis=1)
    print("cost %.6e -> %.6e, largest error %.4f -> %.4f (factor %.2f), least factor %.4f" %
          (info[1], info[2], before.max(), after.max(), before.max() / after.max(), (before / after).min()))
    assert (after < before).all()
    assert (Rw[:a + 1] == table[:a + 1, 0:9]).all() and (C[:a + 1] == table[:a + 1, 9:12]).all() and (sigma[:a + 1] == 1.0).all()
    want = G.DRIFT_SCALE ** -np.arange(1, m + 1)
    assert np.abs(sigma[a + 1:f + 1] / want - 1.0).max() < 0.02


def test_ninth_free_edge_is_left_out_oldest_first():
    _, table, edges, state, f = G.graph_case(65, 9)
    fixed, inner, left = G.graph_edges(edges, state[G.N_EDGES], int(state[G.ANCHOR]), f)
    assert fixed == [9] and inner == list(range(1, 9)) and left == [0]
    info = G.pose_graph(table, edges, state, f)[3]
    assert info[0] == 0.0 and info[6] == 1.0 and info[4] == 65 + 9
    less = edges.copy()
    less[0, 1] = 0.0                                                # the edge (i, 0) ends before the anchor: not in the graph
    for x, y in zip(G.pose_graph(table, edges, state, f)[:3], G.pose_graph(table, less, state, f)[:3]):
        assert (x == y).all()


def test_equivariance():
    """The whole input under one similarity of the world gives the transformed output, within the measured bound."""
    _, table, edges, state, f = G.graph_case(64, 8)
    a = int(state[G.ANCHOR])
    sim = (1.7, G._rot([20.0, -35.0, 10.0]), np.array([0.4, -1.1, 2.0]))
    t2, e2 = G.transform_case(table, edges, sim)
    Rw, C, sigma, info = G.pose_graph(table, edges, state, f)
    Rw2, C2, sigma2, info2 = G.pose_graph(t2, e2, state, f)
    assert info[0] == info2[0] == 0.0
    s, Q, t = sim
    want_R = np.stack([(Rw[k].reshape(3, 3) @ Q.T).reshape(9) for k in range(f + 1)])
    want_C = s * (C[:f + 1] @ Q.T) + t
    d = (float(np.abs(Rw2[:f + 1] - want_R).max()), float(np.abs(C2[:f + 1] - want_C).max()) / s, float(np.abs(sigma2 - sigma).max()))
    print("equivariance: Rw %.3e, C %.3e, sigma %.3e (bounds %s)" % (d + (G.GRAPH_BOUND,)))
    assert all(x <= b for x, b in zip(d, G.GRAPH_BOUND))
    assert a == 2


def test_measured_bounds():
    """The recorded float64 / longdouble differences are what the restatement gives (the graphs up to 65 nodes here; the recorded
    figure is the largest over loop_ref.GRAPH_SIZES)."""
    assert P.WIDE
    small = tuple(s for s in G.GRAPH_SIZES if s[0] <= 65)
    d = G.graph_way_difference(small)
    print("graph way difference (Rw, C, sigma) up to 65 nodes:", d, "recorded:", G.GRAPH_WAY_DIFFERENCE)
    assert all(0.0 < x <= y for x, y in zip(d, G.GRAPH_WAY_DIFFERENCE))
    worst = 0.0
    for name in G.EDGE_CASES:
        c = G.edge_case(name)
        e1, s1, c1 = G.run_edge(c)
        e2, s2, c2 = G.run_edge(c, dt=LD)
        assert (s1 == s2).all()
        worst = max(worst, float(np.abs(e1 - e2).max()), float(np.abs(c1 - c2).max()))
    assert 0.0 < worst <= G.EDGE_WAY_DIFFERENCE


@pytest.mark.parametrize("name", sorted(G.EDGE_CASES))
def test_edge_rule(name):
    c = G.edge_case(name)
    edges, state, cand = G.run_edge(c)
    reason = G.EDGE_CASES[name]
    n0 = int(c["state"][G.N_EDGES])
    assert int(cand[8]) == reason and cand[0] == c["f"]
    assert state[G.ACCEPTED] == (1 if reason == 0 else 0) == int(cand[7])
    assert state[G.REFUSED] == c["state"][G.REFUSED] + (1 if 1 <= reason <= 5 else 0)
    assert state[G.DROPPED] == c["state"][G.DROPPED] + (1 if reason == 6 else 0)
    if reason == 0:
        assert state[G.N_EDGES] == n0 + 1 and state[G.LAST_FRAME] == c["f"]
        row = edges[n0]
        a = int(state[G.ANCHOR])
        assert row[0] == a == 5 and row[1] == c["f"] and row[15] == c["weight"]
        assert abs(np.exp(row[14]) - 0.93) < 1e-12 and abs(cand[4] - 0.93) < 1e-12
        Rl, Cl = c["absolute"]["Rw"], c["absolute"]["C"]
        Ra, Ca = c["table"][a, 0:9].reshape(3, 3), c["table"][a, 9:12]
        assert np.abs(row[2:11].reshape(3, 3) - Rl @ Ra.T).max() < 1e-14 and np.abs(row[11:14] - Ra @ (Cl - Ca)).max() < 1e-14
        assert (edges[:n0] == c["edges"][:n0]).all() and (edges[n0 + 1:] == 0.0).all()
    else:
        assert (edges == c["edges"]).all() and state[G.N_EDGES] == n0 and state[G.LAST_FRAME] == c["state"][G.LAST_FRAME]
    if name == "few_shared":
        assert cand[3] == 7
    if name == "few_inliers":
        assert cand[2] == 9


def test_join_hand_made():
    d = G.join_case(12, 20, 1, hand=True)
    corr, xnew, n = G.run_join(d)
    assert n == (12, int(corr[:, 6].sum()), int(xnew[:, 3].sum()))
    r, j = d["match"][:6, 0].astype(int), d["match"][:6, 1].astype(int)
    assert corr[0, 6] == 1.0 and corr[0, 5] == r[0] and tuple(xnew[0]) == (1.0, 2.0, 3.0, 1.0)        # exactly at f - min_gap: old
    assert (corr[1] == 0.0).all() and (xnew[1] == 0.0).all()                                            # one frame newer: not old
    assert corr[2, 6] == 1.0 and (xnew[2] == 0.0).all()                                                 # no landmark
    assert corr[3, 6] == 1.0 and tuple(xnew[3]) == (4.0, 5.0, 6.0, 1.0)                                 # the lowest row wins
    assert corr[4, 6] == 1.0 and (xnew[4] == 0.0).all()                                                 # non-finite landmark
    assert (corr[5] == 0.0).all() and (xnew[5] == 0.0).all()                                            # non-finite map row
    assert (corr[12:] == 0.0).all() and (xnew[12:] == 0.0).all()                                        # past n_match
    ref, (rows, valid) = W.correspondences(d["w"], d["match"], d["n_match"], d["pts_new"], d["count_new"])
    old = corr[:, 6] != 0.0
    assert (corr[old] == ref[old]).all() and valid > n[1]


@pytest.mark.parametrize("name", G.APPLY_CASES)
def test_apply(name):
    d = G.apply_case(name)
    st, table, X, bad = G.run_apply(d)
    a, f, t0, w = int(d["loop_state"][G.ANCHOR]), d["f"], d["table"], d["w"]
    if name == "no_step":
        assert (st == d["chain_state"]).all() and (table == t0).all() and (X == w["X"]).all() and bad == 0
        return
    rows = np.arange(a + 1, f + 1)
    assert (table[:a + 1] == t0[:a + 1]).all() and (table[f + 1:] == t0[f + 1:]).all()
    assert (table[rows, 14].astype(int) == (t0[rows, 14].astype(int) | 32)).all()              # bit 5 set, bits 0 to 4 kept
    assert int(table[a + 1, 14]) == 63 and int(table[f, 14]) == 32
    assert np.array_equal(table[rows, 0:9], d["Rw"][rows]) and np.array_equal(table[rows, 9:12], d["C"][rows])
    step = np.linalg.norm(d["C"][rows] - d["C"][rows - 1], axis=1)
    for k, ln in zip(rows, step):
        kept = not np.isfinite(ln) or not ln > t0[k, 12] / 64.0
        assert table[k, 12] == (t0[k, 12] if kept else table[k, 12]) and (kept or abs(table[k, 12] - ln) < 1e-15)
    assert table[9, 12] == t0[9, 12] and table[11, 12] == t0[11, 12] and table[12, 12] == t0[12, 12]   # the 1/64 guard; not finite
    if name == "plain":
        assert st[0] == f + 1 and st[1] == table[f, 12] and (st[2:11] == d["Rw"][f]).all()
        assert np.abs(st[11:14] + d["Rw"][f].reshape(3, 3) @ d["C"][f]).max() < 1e-15
    else:
        assert (st == d["chain_state"]).all()
    last = w["last_frame"]
    moved = (X != w["X"]).any(axis=1)
    assert not moved[0] and moved[1] and moved[2] and not moved[3] and not moved[4] and not moved[5] and moved[6] and not moved[7]
    assert not moved[36:].any() and bad == int(((last[:36] == 11)).sum())
    s = 1
    k = int(last[s])
    y = t0[k, 0:9].reshape(3, 3) @ (w["X"][s] - t0[k, 9:12])
    assert np.abs(X[s] - (d["C"][k] + d["sigma"][k] * (d["Rw"][k].reshape(3, 3).T @ y))).max() < 1e-14


# ---- end to end: the restated tracker on a closed circuit ------------------------------------------------------------------------
@pytest.mark.parametrize("seed", G.CIRCUIT_SEEDS)
def test_circuit_apply_reduces_the_centre_error(seed):
    """A camera that drives a circle of 20 frames and re-enters its first stretch for 6 more, 0.3 px noise, L = 4, about 110 points
    per frame, loop_min_gap 12, loop_min_inliers 40: the restatement accepts one edge (frame 19 or 20 against anchor 7 or 8) and the
    centre error of the frames from the closure on, in first baselines and aligned on the first frames, is smaller with "apply"
    than without.  Mean / largest error, observe -> apply: seed 1 0.107 / 0.171 -> 0.068 / 0.161; seed 2 0.176 / 0.210 -> 0.101 /
    0.169; seed 3 0.116 / 0.135 -> 0.047 / 0.070; seed 4 0.242 / 0.288 -> 0.121 / 0.166."""
    seq, runs = G.circuit_runs(seed)
    obs, app = G.closures(runs["observe"]), G.closures(runs["apply"])
    assert len(obs) >= 1 and obs[0] == app[0]
    f0, a0, inl = obs[0]
    assert f0 >= G.CIRCUIT_LAP - 1 and f0 - a0 >= G.CIRCUIT_GAP and inl >= G.CIRCUIT_MIN_INLIERS
    eo, ea = W.centre_errors(seq, runs["observe"]["table"]), W.centre_errors(seq, runs["apply"]["table"])
    print("seed %d: edge %s, points per frame %d to %d, error from frame %d on: mean %.4f -> %.4f, largest %.4f -> %.4f" %
          (seed, obs[0], min(len(p) for p in seq["pts"]), max(len(p) for p in seq["pts"]), f0, eo[f0:].mean(), ea[f0:].mean(),
           eo[f0:].max(), ea[f0:].max()))
    assert ea[f0:].mean() < eo[f0:].mean() and ea[f0:].max() < eo[f0:].max()
    flags = runs["apply"]["table"][:, 14].astype(int)
    info = [x["info"] for x in runs["apply"]["loop"] if x["cand"][7] != 0.0][0]
    assert info[0] == 0.0 and info[2] < info[1]
    assert (flags[a0 + 1:f0 + 1] & 32).all() and not (flags[:a0 + 1] & 32).any() and not (flags[f0 + 1:] & 32).any()
    assert not (runs["observe"]["table"][:, 14].astype(int) & 32).any()
    assert (runs["apply"]["table"][:a0 + 1] == runs["observe"]["table"][:a0 + 1]).all()


def test_circuit_observe_changes_nothing():
    """loop_closure="observe" leaves every old output of the restated tracker as world_ref.run_sequence("observe") gives it."""
    seq, runs = G.circuit_runs(G.CIRCUIT_DEVICE_SEED)
    plain = W.run_sequence(seq, G.CIRCUIT_L, G.CIRCUIT_CAP, "observe", G.CIRCUIT_SEED0)
    obs = runs["observe"]
    assert (plain["table"] == obs["table"]).all()
    for a, b in zip(plain["world"], obs["world"]):
        assert a["status"] == b["status"] and a["n_inliers"] == b["n_inliers"] and (np.asarray(a["C"]) == np.asarray(b["C"])).all()
    for a, b in zip(plain["states"], obs["states"]):
        assert (a == b).all()
    for k in ("X", "desc", "tid", "n_views", "first_frame", "last_frame", "rms", "state"):
        assert (plain["map"][k] == obs["map"][k]).all(), k
    assert (plain["tracks"].ids == obs["tracks"].ids).all()


def test_circuit_measured_bound():
    assert P.WIDE
    seq, runs = G.circuit_runs(G.CIRCUIT_DEVICE_SEED)
    wide = G.run_sequence(seq, G.CIRCUIT_L, G.CIRCUIT_CAP, "apply", G.CIRCUIT_SEED0, min_gap=G.CIRCUIT_GAP,
                          loop_min_inliers=G.CIRCUIT_MIN_INLIERS, way=P.WAY2)
    assert G.closures(wide) == G.closures(runs["apply"]) and (wide["table"][:, 14] == runs["apply"]["table"][:, 14]).all()
    d = float(np.abs(wide["table"][:, 9:12] - runs["apply"]["table"][:, 9:12]).max())
    print("circuit way difference %.6e (recorded %.6e)" % (d, G.CIRCUIT_WAY_DIFFERENCE))
    assert 0.0 < d <= G.CIRCUIT_WAY_DIFFERENCE
