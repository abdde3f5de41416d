"""Loop closure on the device against tests/loop_ref.py: ssp_op_loop_correspondences and ssp_loop_apply with
==; ssp_loop_edge with == on the integers and the table layout and within loop_ref.EDGE_BOUND on the similarity; ssp_pose_graph
within loop_ref.GRAPH_BOUND on planted drifts from 1 to 4095 free nodes with 0, 1, 8 and 9 both-ends-free edges, torch.equal copies
on a consistent loop, a repeated call and two capacities bit-identical; the join followed by op_pnp_ransac and the edge; the argument
checks.  The bounds are measured, not chosen: 16 times the restatement's float64 / numpy.longdouble difference
(tests/test_loop_cpu.py repeats the measurement).  Every comparison prints what the device showed before it asserts."""
import functools

import numpy as np
import pytest
import torch

from tests import loop_ref as G
from tests import pnp_ref as N
from tests import pose_ref as P

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _world_dev(lib, dev, w):
    d = lib.world_buffers(w["map_cap"], w["tid_cap"], dev)
    for k in ("X", "last_frame", "state"):
        d[k].copy_(_t(w[k], dev))
    return d


# ---- the join ------------------------------------------------------------------------------------------------------------------
JOIN_CASES = [("hand", 12, 20, True), ("one", 1, 3, False), ("n63", 63, 80, False), ("n64", 64, 64, False), ("n65", 65, 300, False),
              ("n1131", 1131, 8229, False)]


def _run_join_dev(lib, dev, d, loop=None):
    w = _world_dev(lib, dev, d["w"])
    cap = d["match"].shape[0]
    loop = lib.loop_buffers(cap, 8, dev) if loop is None else loop
    i32 = lambda v: torch.tensor([v], dtype=torch.int32, device=dev)
    lib.op_loop_correspondences(w, _t(d["match"], dev), i32(d["n_match"]), _t(d["pts_new"], dev), i32(d["count_new"]),
                                _t(d["landmarks"], dev), i32(d["n_landmarks"]), d["f"], d["min_gap"], loop)
    torch.cuda.synchronize()
    return loop, w


@pytest.mark.parametrize("name,n_match,n_rows,hand", JOIN_CASES)
def test_loop_correspondences_equal_the_restatement(name, n_match, n_rows, hand):
    from semantic_superpoint_amd import lib
    dev = _dev()
    d = G.join_case(n_match, n_rows, 7 + n_match, hand=hand)
    corr, xnew, n = G.run_join(d)
    loop, _ = _run_join_dev(lib, dev, d)
    got_n = tuple(loop["n"].cpu().tolist())
    print(name, "device n", got_n, "restatement", n)
    assert got_n == n
    assert np.array_equal(loop["corr"].cpu().numpy(), corr)
    assert np.array_equal(loop["xnew"].cpu().numpy(), xnew)


# ---- the edge ------------------------------------------------------------------------------------------------------------------
def _edge_dev(lib, dev, c):
    w = {"map_cap": c["last_frame"].shape[0], "tid_cap": 16, "X": np.zeros((c["last_frame"].shape[0], 3)),
         "last_frame": c["last_frame"], "state": np.array([c["last_frame"].shape[0]] + [0] * 7, dtype=np.int32)}
    wd = _world_dev(lib, dev, w)
    cap, capacity = c["corr"].shape[0], c["table"].shape[0]
    loop = lib.loop_buffers(cap, capacity, dev)
    loop["corr"].copy_(_t(c["corr"], dev))
    loop["xnew"].copy_(_t(c["xnew"], dev))
    loop["n"].copy_(_t(np.array(c["n"], dtype=np.int32), dev))
    loop["edges"].copy_(_t(c["edges"], dev))
    loop["state"].copy_(_t(c["state"], dev))
    a = c["absolute"]
    absolute = {"Rw": _t(np.asarray(a["Rw"], dtype=np.float64).reshape(1, 3, 3), dev), "C": _t(np.asarray(a["C"], dtype=np.float64).reshape(1, 3), dev),
                "mask": _t(a["mask"].reshape(1, -1), dev), "status": torch.tensor([a["status"]], dtype=torch.int32, device=dev)}
    lib.op_loop_edge(wd, absolute, _t(c["table"], dev), c["f"], loop, c["min_inliers"], c["cooldown"], c["weight"])
    torch.cuda.synchronize()
    return loop


@pytest.mark.parametrize("name", sorted(G.EDGE_CASES))
def test_loop_edge_against_the_restatement(name):
    from semantic_superpoint_amd import lib
    dev = _dev()
    c = G.edge_case(name)
    edges, state, cand = G.run_edge(c)
    loop = _edge_dev(lib, dev, c)
    got_e, got_s, got_c = loop["edges"].cpu().numpy(), loop["state"].cpu().numpy(), loop["cand"].cpu().numpy()
    diff = max(float(np.abs(got_e - edges).max()), float(np.abs(got_c - cand).max()))
    print(name, "state", got_s.tolist(), "cand", got_c[:9].tolist(), "largest difference %.3e (bound %.3e)" % (diff, G.EDGE_BOUND))
    assert np.array_equal(got_s, state)
    assert np.array_equal(got_c[[0, 1, 2, 3, 7, 8]], cand[[0, 1, 2, 3, 7, 8]]) and int(got_c[8]) == G.EDGE_CASES[name]
    assert np.array_equal(got_e[:, [0, 1, 15]], edges[:, [0, 1, 15]])
    assert np.array_equal(got_e == 0.0, edges == 0.0)
    assert diff <= G.EDGE_BOUND


# ---- the pose graph ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _graph_ref(m, n_inner, capacity):
    """(inputs, the restatement's result): computed once, read-only."""
    case = G.graph_case(m, n_inner, capacity=capacity)
    return case, G.pose_graph(case[1], case[2], case[3], case[4])


def _graph_dev(lib, dev, table, edges, state, f, loop=None, iterations=10):
    loop = lib.loop_buffers(4, table.shape[0], dev) if loop is None else loop
    loop["edges"].copy_(_t(edges, dev))
    loop["state"].copy_(_t(state, dev))
    td = _t(table, dev)
    out = lib.op_pose_graph(td, f, loop, iterations)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}, loop, td


def _check_graph(got, want, m):
    Rw, C, sigma, info = want
    d = G.graph_difference((got["Rw"], got["C"], got["sigma"]), want)
    gi = got["info"]
    print("nodes %d: device info %s\n  restatement    %s\n  differences Rw %.3e C %.3e sigma %.3e (bounds %.3e %.3e %.3e), bit-equal: %s" %
          ((m, gi.tolist(), info.tolist()) + d + G.GRAPH_BOUND + (d == (0.0, 0.0, 0.0),)))
    assert gi[0] == info[0] and gi[3] == info[3] and gi[4] == info[4] and gi[6] == info[6]
    assert abs(gi[1] - info[1]) <= 1e-9 * info[1] and abs(gi[2] - info[2]) <= 1e-6 * info[1]
    assert all(x <= b for x, b in zip(d, G.GRAPH_BOUND))


@pytest.mark.parametrize("m,n_inner", G.GRAPH_SIZES)
def test_pose_graph_against_the_restatement(m, n_inner):
    from semantic_superpoint_amd import lib
    dev = _dev()
    (truth, table, edges, state, f), want = _graph_ref(m, n_inner, None)
    got, _, _ = _graph_dev(lib, dev, table, edges, state, f)
    _check_graph(got, want, m)
    assert want[3][0] == 0.0 and want[3][6] == max(0, n_inner - G.MAX_INNER)


def test_pose_graph_4095_nodes():
    from semantic_superpoint_amd import lib
    dev = _dev()
    m, n_inner = G.GRAPH_LARGE
    (truth, table, edges, state, f), want = _graph_ref(m, n_inner, 4098)
    assert table.shape[0] == 4098 and f == 4097
    got, _, _ = _graph_dev(lib, dev, table, edges, state, f)
    _check_graph(got, want, m)


def test_pose_graph_consistent_loop_gives_copies():
    from semantic_superpoint_amd import lib
    dev = _dev()
    table, edges, state, f = G.consistent_case()
    got, loop, td = _graph_dev(lib, dev, table, edges, state, f)
    print("info", got["info"].tolist())
    assert got["info"][0] == 1.0 and got["info"][1] == 0.0 and got["info"][5] == 0.0
    assert torch.equal(loop["Rw"], td[:, 0:9]) and torch.equal(loop["C"], td[:, 9:12]) and bool((loop["sigma"] == 1.0).all())
    state = state.copy()
    state[G.ACCEPTED] = 0                                           # no accepted edge this frame: nothing to do either
    got, loop, td = _graph_dev(lib, dev, table, edges, state, f)
    assert got["info"].tolist() == [1.0] + [0.0] * 7
    assert torch.equal(loop["Rw"], td[:, 0:9]) and torch.equal(loop["C"], td[:, 9:12]) and bool((loop["sigma"] == 1.0).all())


def test_pose_graph_repeats_and_ignores_capacity():
    from semantic_superpoint_amd import lib
    dev = _dev()
    (truth, table, edges, state, f), _ = _graph_ref(65, 9, None)
    a, loop, _ = _graph_dev(lib, dev, table, edges, state, f)
    b, _, _ = _graph_dev(lib, dev, table, edges, state, f, loop=loop)
    big = np.zeros((300, P.ROW_WORDS))
    big[:table.shape[0]] = table
    c, _, _ = _graph_dev(lib, dev, big, edges, state, f)
    n = table.shape[0]
    for k in ("Rw", "C", "sigma"):
        assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], c[k][:n])
    assert np.array_equal(a["info"], b["info"]) and np.array_equal(a["info"], c["info"])


# ---- apply ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", G.APPLY_CASES)
def test_loop_apply_equals_the_restatement(name):
    from semantic_superpoint_amd import lib
    dev = _dev()
    d = G.apply_case(name)
    st, table, X, bad = G.run_apply(d)
    w = _world_dev(lib, dev, d["w"])
    loop = lib.loop_buffers(4, d["table"].shape[0], dev)
    for k, v in (("Rw", d["Rw"]), ("C", d["C"]), ("sigma", d["sigma"]), ("info", d["info"]), ("state", d["loop_state"])):
        loop[k].copy_(_t(v, dev))
    sd, td = _t(d["chain_state"], dev), _t(d["table"], dev)
    before = {k: w[k].clone() for k in ("state", "last_frame")}
    lib.op_loop_apply(w, sd, td, d["f"], loop)
    torch.cuda.synchronize()
    got_bad = int(loop["state"][G.NONFINITE]) - int(d["loop_state"][G.NONFINITE])
    print(name, "non-finite map rows", got_bad, "flags", td[:, 14].cpu().numpy().astype(int).tolist())
    assert np.array_equal(td.cpu().numpy(), table, equal_nan=True)
    assert np.array_equal(sd.cpu().numpy(), st)
    assert np.array_equal(w["X"].cpu().numpy(), X)
    assert got_bad == bad
    assert all(torch.equal(w[k], before[k]) for k in before)          # anchored and streak among them
    assert np.array_equal(loop["state"].cpu().numpy()[:7], d["loop_state"][:7])


# ---- the join, the pose and the edge together ------------------------------------------------------------------------------------
def test_join_pnp_edge_chain():
    """A revisited place: 40 old map rows seen again from a drifted camera.  The join keeps the old rows, op_pnp_ransac finds the
    camera in the old frame and the edge measures the planted similarity."""
    from semantic_superpoint_amd import lib
    from tests import world_ref as W
    dev = _dev()
    rng = np.random.RandomState(11)
    f, a, cap, capacity = 40, 5, 64, 64
    _, table = G.circuit(48, 3, capacity)
    k = P.intrinsics_of(0, False)
    Rw, C = table[f, 0:9].reshape(3, 3), table[f, 9:12]
    sigma, Rc, tc = 0.93, G._rot([1.0, -2.0, 0.5]), np.array([0.05, -0.02, 0.03])
    Rl, Cl = Rw @ Rc.T, sigma * (Rc @ C) + tc
    n = 40
    pix = np.stack([rng.uniform(20, 300, n), rng.uniform(20, 220, n)], 1)
    z = rng.uniform(3, 9, n)
    x = np.stack([(pix[:, 0] - k[2]) * z / k[0], (pix[:, 1] - k[3]) * z / k[1], z], 1)
    Xn = C + x @ Rw
    Xo = sigma * (Xn @ Rc.T) + tc
    w = W.new_map(100, 16)
    w["state"][W.N_ROWS] = 60
    w["X"][:n], w["last_frame"][:n] = Xo, rng.randint(0, a + 1, n)
    w["last_frame"][3] = a
    w["X"][n:60], w["last_frame"][n:60] = rng.randn(20, 3), f - 2      # recent rows: not old
    match = np.zeros((cap, 3), dtype=np.float32)
    match[:50, 0], match[:50, 1] = np.arange(50), np.arange(50)
    pts = np.zeros((cap, 2))
    pts[:n] = pix
    pts[n:50] = rng.uniform(0, 300, (10, 2))
    lms = np.zeros((cap, 8))
    lms[:n, 0], lms[:n, 1:4], lms[:n, 7] = np.arange(n), Xn, np.arange(n)
    d = dict(w=w, match=match, n_match=50, pts_new=pts, count_new=50, landmarks=lms, n_landmarks=n, f=f, min_gap=8)
    corr, xnew, nn = G.run_join(d)
    assert nn == (50, 40, 40)
    loop = lib.loop_buffers(cap, capacity, dev)
    loop, wd = _run_join_dev(lib, dev, d, loop)
    assert np.array_equal(loop["corr"].cpu().numpy(), corr) and np.array_equal(loop["xnew"].cpu().numpy(), xnew)
    seeds = torch.tensor([1234], dtype=torch.int64, device=dev)
    res = lib.op_pnp_ransac(loop["corr"], loop["n"][0:1], _t(k[None], dev), seeds, 2.0, 12)
    ref = N.ransac(corr, nn[0], k, 1234, 2.0, 12)
    td = _t(table, dev)
    lib.op_loop_edge(wd, res, td, f, loop, 12, 32, 1.0)
    torch.cuda.synchronize()
    assert int(res["status"][0]) == 0 == ref["status"] and int(res["n_inliers"][0]) == ref["n_inliers"] == 40
    ab = {"Rw": res["Rw"].cpu().numpy()[0], "C": res["C"].cpu().numpy()[0], "mask": res["mask"].cpu().numpy()[0], "status": 0}
    edges, state, cand = G.edge(ab, corr, xnew, nn, w["last_frame"], table, f, 12, 32, 1.0, G.new_edges(), G.new_state())
    got_c, got_e = loop["cand"].cpu().numpy(), loop["edges"].cpu().numpy()
    print("cand", got_c[:9].tolist(), "pose error", float(np.abs(ab["C"] - Cl).max()))
    assert np.array_equal(loop["state"].cpu().numpy(), state) and state[G.ACCEPTED] == 1 and state[G.ANCHOR] == a
    assert np.abs(got_e - edges).max() <= G.EDGE_BOUND and np.abs(got_c - cand).max() <= G.EDGE_BOUND
    assert abs(got_c[4] - sigma) < 1e-9 and np.abs(ab["C"] - Cl).max() < 1e-9
    out = lib.op_pose_graph(td, f, loop, 10)
    torch.cuda.synchronize()
    info = out["info"].cpu().numpy()
    want = G.pose_graph(table, edges, state, f)
    print("graph info", info.tolist(), "restatement", want[3].tolist())
    assert info[0] == 0.0 and info[3] == f - a and info[2] < info[1]
    assert np.abs(out["C"].cpu().numpy()[f] - Cl).max() < 0.1 * np.abs(C - Cl).max()      # a uniform chain leaves the loop edge 1 / (nodes + 1) of the gap


# ---- argument checks -------------------------------------------------------------------------------------------------------------
def test_argument_checks():
    from semantic_superpoint_amd import lib
    dev = _dev()
    with pytest.raises(ValueError):
        lib.loop_buffers(0, 8, dev)
    with pytest.raises(ValueError):
        lib.loop_buffers(8, 1, dev)
    with pytest.raises(RuntimeError):
        lib.loop_buffers(8, 8, "cpu")
    loop = lib.loop_buffers(8, 16, dev)
    w = lib.world_buffers(32, 16, dev)
    i32 = lambda v: torch.tensor([v], dtype=torch.int32, device=dev)
    f64 = dict(dtype=torch.float64, device=dev)
    match, pts, lms = torch.zeros(8, 3, device=dev), torch.zeros(8, 2, **f64), torch.zeros(8, 8, **f64)
    table, st = torch.zeros(16, P.ROW_WORDS, **f64), torch.zeros(P.STATE_WORDS, **f64)
    ok = lambda: lib.op_loop_correspondences(w, match, i32(0), pts, i32(0), lms, i32(0), 5, 2, loop)
    ok()
    bad = [lambda: lib.op_loop_correspondences(w, match[:7], i32(0), pts, i32(0), lms, i32(0), 5, 2, loop),
           lambda: lib.op_loop_correspondences(w, match.double(), i32(0), pts, i32(0), lms, i32(0), 5, 2, loop),
           lambda: lib.op_loop_correspondences(w, match, i32(0), pts.float(), i32(0), lms, i32(0), 5, 2, loop),
           lambda: lib.op_loop_correspondences(w, match, i32(0), pts, i32(0), lms[:, :7].contiguous(), i32(0), 5, 2, loop),
           lambda: lib.op_loop_correspondences(w, match, i32(0), pts, i32(0), lms, i32(0), -1, 2, loop),
           lambda: lib.op_loop_correspondences(w, match, i32(0), pts, i32(0), lms, i32(0), 5, 0, loop),
           lambda: lib.op_loop_correspondences(w, match, i32(0), pts, i32(0), lms, i32(0), 5, 2, {"corr": loop["corr"]}),
           lambda: lib.op_loop_correspondences({"X": w["X"]}, match, i32(0), pts, i32(0), lms, i32(0), 5, 2, loop),
           lambda: lib.op_loop_correspondences(w, match.cpu(), i32(0), pts, i32(0), lms, i32(0), 5, 2, loop)]
    ab = {"Rw": torch.eye(3, **f64)[None], "C": torch.zeros(1, 3, **f64), "mask": torch.zeros(1, 8, dtype=torch.uint8, device=dev),
          "status": i32(1)}
    lib.op_loop_edge(w, ab, table, 5, loop)
    bad += [lambda: lib.op_loop_edge(w, {"Rw": ab["Rw"]}, table, 5, loop),
            lambda: lib.op_loop_edge(w, dict(ab, mask=ab["mask"][:, :7].contiguous()), table, 5, loop),
            lambda: lib.op_loop_edge(w, ab, table[:15], 5, loop),
            lambda: lib.op_loop_edge(w, ab, table, 5, loop, min_inliers=3),
            lambda: lib.op_loop_edge(w, ab, table, 5, loop, cooldown=-1),
            lambda: lib.op_loop_edge(w, ab, table, 5, loop, weight=0.0),
            lambda: lib.op_loop_edge(w, ab, table, 5, loop, weight=float("nan")),
            lambda: lib.op_loop_edge(w, ab, table, -1, loop)]
    lib.op_pose_graph(table, 5, loop)
    bad += [lambda: lib.op_pose_graph(table, 5, loop, iterations=0),
            lambda: lib.op_pose_graph(table, 5, loop, iterations=lib.LOOP_MAX_ITERATIONS + 1),
            lambda: lib.op_pose_graph(table.float(), 5, loop),
            lambda: lib.op_pose_graph(table, -1, loop),
            lambda: lib.op_pose_graph(table, 5, dict(loop, ws=loop["ws"][:64]))]
    lib.op_loop_apply(w, st, table, 5, loop)
    bad += [lambda: lib.op_loop_apply(w, st[:8], table, 5, loop),
            lambda: lib.op_loop_apply(w, st, table, -1, loop),
            lambda: lib.op_loop_apply(w, st, table[:, :8].contiguous(), 5, loop),
            lambda: lib.op_loop_apply(w, st, table, 5, dict(loop, sigma=loop["sigma"][:4]))]
    torch.cuda.synchronize()
    for k, call in enumerate(bad):
        with pytest.raises((ValueError, RuntimeError)):
            call()
            print("call", k, "was accepted")
    assert int(loop["state"][G.REFUSED]) == 1 and float(loop["info"][0]) == 1.0


# ---- the trackers ----------------------------------------------------------------------------------------------------------------
LOOP_KEYS = {"loop_" + k for k in ("Rw", "C", "mask", "n_inliers", "winner", "rms", "status", "corr", "xnew", "n_corr", "cand", "info",
                                   "state")}
LOOP_GAP = 5


def _clone(d):
    return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in d.items()}


@pytest.mark.parametrize("through,which", [("PointTracker", "revisit"), ("SequenceTracker", "revisit"), ("PointTracker", "circuit")])
def test_trackers_loop_closure(through, which):
    """Three trackers in lockstep over world_ref's noise-free revisit (the camera comes back to rows last seen more than LOOP_GAP
    frames ago) and over loop_ref's noisy closed circuit: world_map="observe" alone, plus loop_closure="observe", plus "apply".
    Observing leaves every other output bit-identical; the loop_* results are bit for bit the operators' on copies of the
    tracker's state, the join and the edge's integers equal the restatement's, and on the circuit the accepted edges, the flags and
    the centres equal the restated tracker's (the centres within loop_ref.CIRCUIT_BOUND, measured)."""
    import contextlib
    from semantic_superpoint_amd import lib
    from semantic_superpoint_amd.export import PointTracker, SequenceTracker
    from tests import world_ref as W
    dev = _dev()
    if which == "revisit":
        (seq, _), ref = W.revisit_runs(), None
        Lm, seed0, gap, min_inl = W.REVISIT_L, W.REVISIT_SEED0, LOOP_GAP, 12
    else:
        seq, ref = G.circuit_runs(G.CIRCUIT_DEVICE_SEED)
        Lm, seed0, gap, min_inl = G.CIRCUIT_L, G.CIRCUIT_SEED0, G.CIRCUIT_GAP, G.CIRCUIT_MIN_INLIERS
    frames = len(seq["pts"])
    kw = dict(geometric_check="fundamental", check_seed=seed0, intrinsics=tuple(seq["intr"][0]), trajectory_rows=frames + 1,
              world_map="observe", world_cap=4096)
    lk = dict(loop_min_gap=gap, loop_min_inliers=min_inl, loop_cooldown=32)

    def make(**more):
        if through == "PointTracker":
            top = PointTracker(Lm, W.NN_THRESH, dev, **kw, **more)
            return top, top
        top = SequenceTracker(None, dev, 0.015, 4, False, W.NN_THRESH, Lm, **kw, **more)
        return top, top.tracker

    @contextlib.contextmanager
    def no_host_sync():
        torch.cuda.set_sync_debug_mode("error")
        try:
            yield
        finally:
            torch.cuda.set_sync_debug_mode("default")

    def frame_of(f):
        xy = seq["pts"][f]
        return (_t(xy.reshape(-1, 2), dev), torch.tensor([xy.shape[0]], dtype=torch.int32, device=dev),
                _t(np.asarray(seq["desc"][f], dtype=np.float32).reshape(-1, 256), dev))

    (base_top, base), (obs_top, obs), (app_top, app) = make(), make(loop_closure="observe", **lk), make(loop_closure="apply", **lk)
    assert obs_top.loop_edges_device() is None and obs_top.loop_closures().shape == (0, 9) and base_top.loop_closures().shape == (0, 9)
    k1 = _t(seq["intr"][:1], dev)
    accepted = []
    for f in range(frames):
        w0 = _clone(obs._world) if obs._world is not None else None
        l0 = _clone(obs._loop) if obs._loop is not None else None
        frame = frame_of(f)
        base.update_device(*frame)
        if f >= 2:
            with no_host_sync():
                obs.update_device(*frame)
                app.update_device(*frame)
        else:
            obs.update_device(*frame)
            app.update_device(*frame)
        gb, go, ga = base.last_geometry(), obs.last_geometry(), app.last_geometry()
        assert not any(k.startswith("loop_") for k in gb)               # loop_closure=None: no loop_* key
        if f >= 1:
            assert set(go) == set(ga) == set(gb) | LOOP_KEYS
        for k in gb:                                                     # observing changes nothing the tracker computed before
            assert torch.equal(gb[k], go[k]), (f, k)
        assert torch.equal(base.trajectory()[0], obs.trajectory()[0]) and torch.equal(base.trajectory()[1], obs.trajectory()[1])
        assert torch.equal(base.world_trajectory()[0], obs.world_trajectory()[0])
        assert np.array_equal(base.get_tracks(1), obs.get_tracks(1))
        if f >= 1:
            a, b = base_top.landmarks_device(), obs_top.landmarks_device()
            assert torch.equal(a[1], b[1]) and torch.equal(a[0][:int(a[1])], b[0][:int(b[1])])
        for k in ("X", "desc", "tid", "n_views", "first_frame", "last_frame", "rms", "state"):
            assert torch.equal(base._world[k], obs._world[k]), (f, k)
        if f < 1:
            continue
        # the operators on the map, the landmarks and the edge table as they stood before the frame's loop step, bit for bit
        slot, dslot = f % Lm, f % 2
        cap = obs._cap
        w0 = w0 if w0 is not None else lib.world_buffers(4096, device=dev)
        lp = lib.loop_buffers(cap, frames + 1, dev)
        if l0 is not None:
            lp["edges"].copy_(l0["edges"])
            lp["state"].copy_(l0["state"])
        lms, n_lms = obs._world_lm["landmarks"], obs._world_lm["n_landmarks"]
        count = obs._counts[dslot:dslot + 1]
        lib.op_loop_correspondences(w0, go["world_match"], go["world_n_match"], obs._pts[slot], count, lms, n_lms, f, gap, lp)
        want = lib.op_pnp_ransac(lp["corr"], lp["n"][0:1], k1, torch.tensor([seed0 + f], dtype=torch.int64, device=dev), 2.0, min_inl)
        table = obs.trajectory()[0]
        lib.op_loop_edge(w0, want, table, f, lp, min_inl, 32, 1.0)
        lib.op_pose_graph(table, f, lp, 10)
        torch.cuda.synchronize()
        assert torch.equal(go["loop_corr"], lp["corr"]) and torch.equal(go["loop_xnew"], lp["xnew"]) and torch.equal(go["loop_n_corr"], lp["n"])
        for k in want:
            assert torch.equal(go["loop_" + k], want[k]), (f, k)
        assert torch.equal(go["loop_cand"], lp["cand"]) and torch.equal(go["loop_state"], lp["state"])
        assert torch.equal(go["loop_info"], lp["info"])
        assert torch.equal(obs._loop["edges"], lp["edges"]) and torch.equal(obs._loop["Rw"], lp["Rw"]) and torch.equal(obs._loop["C"], lp["C"])
        # the restatement on the same inputs
        wn = {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in w0.items()}
        corr, xnew, n = G.correspondences(wn, go["world_match"].cpu().numpy(), int(go["world_n_match"]), obs._pts[slot].cpu().numpy(),
                                          int(count), lms.cpu().numpy(), int(n_lms), f, gap)
        assert np.array_equal(lp["corr"].cpu().numpy(), corr) and np.array_equal(lp["xnew"].cpu().numpy(), xnew)
        assert tuple(lp["n"].cpu().tolist()) == n
        ab = {"Rw": want["Rw"].cpu().numpy()[0], "C": want["C"].cpu().numpy()[0], "mask": want["mask"].cpu().numpy()[0],
              "status": int(want["status"][0])}
        e0 = l0["edges"].cpu().numpy() if l0 is not None else G.new_edges()
        s0 = l0["state"].cpu().numpy() if l0 is not None else G.new_state()
        edges, state, cand = G.edge(ab, corr, xnew, n, wn["last_frame"], table.cpu().numpy(), f, min_inl, 32, 1.0, e0, s0)
        got_c = lp["cand"].cpu().numpy()
        print("frame %d: join %s, pose status %d, cand %s, state %s (restatement %s)" %
              (f, n, ab["status"], got_c[:9].tolist(), lp["state"].cpu().tolist(), state.tolist()))
        assert np.array_equal(lp["state"].cpu().numpy(), state) and np.array_equal(got_c[[0, 1, 2, 3, 7, 8]], cand[[0, 1, 2, 3, 7, 8]])
        assert np.abs(lp["edges"].cpu().numpy() - edges).max() <= G.EDGE_BOUND
        if state[G.ACCEPTED]:
            accepted.append((f, int(state[G.ANCHOR]), int(state[G.INLIERS])))
            want_g = G.pose_graph(table.cpu().numpy(), edges, state, f)
            info = lp["info"].cpu().numpy()
            print("  graph info", info.tolist(), "restatement", want_g[3].tolist())
            assert info[3] == want_g[3][3] and info[4] == want_g[3][4]
            assert np.abs(lp["C"].cpu().numpy() - want_g[1]).max() <= G.GRAPH_BOUND[1]
    assert len(accepted) >= 1                                            # the sequence closes at least once
    rows = obs_top.loop_closures()
    print("accepted edges", accepted, "loop_closures()", rows.tolist())
    assert [(int(r[0]), int(r[1]), int(r[2])) for r in rows] == accepted
    edges_dev, state_dev = obs_top.loop_edges_device()
    assert int(state_dev[0]) == len(accepted) and [int(e[1]) for e in edges_dev[:len(accepted)].cpu().numpy()] == [a[0] for a in accepted]
    # "apply": its first closure is the observer's (nothing differs before it); the rows of its span carry bit 5 iff the graph solved
    arows = app_top.loop_closures()
    assert len(arows) >= 1 and tuple(arows[0][:3]) == tuple(rows[0][:3])
    f0, a0, status0 = int(arows[0][0]), int(arows[0][1]), arows[0][8]
    flags_after = app.trajectory()[0][:frames, 14].cpu().numpy().astype(int)
    flags_obs = obs.trajectory()[0][:frames, 14].cpu().numpy().astype(int)
    print("apply: first closure", arows[0].tolist(), "flags", flags_after.tolist())
    assert not (flags_obs & 32).any()
    assert not (flags_after[:a0 + 1] & 32).any()
    if status0 == 0.0:
        assert (flags_after[a0 + 1:f0 + 1] & 32).all() and np.array_equal(flags_after[:f0 + 1] & 31, flags_obs[:f0 + 1] & 31)
    else:
        assert not (flags_after[:f0 + 1] & 32).any()
    if ref is not None:                                                  # the restated tracker on the same circuit
        assert accepted == G.closures(ref["observe"]) and [tuple(int(x) for x in r[:3]) for r in arows] == G.closures(ref["apply"])
        for nm, tr in (("observe", obs), ("apply", app)):
            table = tr.trajectory()[0][:frames].cpu().numpy()
            worst = float(np.abs(table[:, 9:12] - ref[nm]["table"][:, 9:12]).max())
            print("%s: centres against the restated tracker %.3e (bound %.3e), flags %s" % (nm, worst, G.CIRCUIT_BOUND, table[:, 14].tolist()))
            assert table[:, 14].tolist() == ref[nm]["table"][:, 14].tolist()
            assert worst <= G.CIRCUIT_BOUND
        rows_dev, _ = app_top.world_map()
        want_rows, _ = W.map_rows(ref["apply"]["map"])
        assert rows_dev.shape == want_rows.shape and np.array_equal(rows_dev[:, [0, 4, 6, 7]], want_rows[:, [0, 4, 6, 7]])
        print("apply: map X against the restated tracker %.3e" % float(np.abs(rows_dev[:, 1:4] - want_rows[:, 1:4]).max()))


CHECK_POSE_KEYS = {"F", "mask", "n_inliers", "status", "winner", "err", "R", "t", "E", "cand", "counts", "n_front", "pose_status", "front",
                   "depth", "X"}
ABS_KEYS = {"abs_" + k for k in ("Rw", "C", "mask", "n_inliers", "winner", "rms", "status", "corr", "n_corr")}
WORLD_KEYS = {"world_" + k for k in ("Rw", "C", "mask", "n_inliers", "winner", "rms", "status", "corr", "n_corr", "match", "n_match")}


@pytest.mark.parametrize("through", ["PointTracker", "SequenceTracker"])
def test_trackers_all_stages_together(through):
    """One tracker with every stage over loop_ref's closed circuit: absolute_pose="repair", bundle_adjust="apply",
    world_map="relocalise", loop_closure="observe".  This pins the order of a step: the kept landmarks (_abs_lm) and the inserted
    landmarks (_world_lm) are both computed after the bundle adjustment's write-back, so each equals, bit for bit, what
    landmarks_device gives after the update (the observing loop closure writes nothing in between).  The map rows seen in the
    newest frame are copies of those rows, last_geometry() holds every stage's keys, and a step makes no host synchronisation."""
    from semantic_superpoint_amd.export import PointTracker, SequenceTracker
    from tests import world_ref as W
    dev = _dev()
    seq = G.circuit_sequence(G.CIRCUIT_DEVICE_SEED)
    frames = len(seq["pts"])
    kw = dict(geometric_check="fundamental", check_seed=G.CIRCUIT_SEED0, intrinsics=tuple(seq["intr"][0]), trajectory_rows=frames + 1,
              absolute_pose="repair", bundle_adjust="apply", world_map="relocalise", world_cap=4096, loop_closure="observe",
              loop_min_gap=G.CIRCUIT_GAP, loop_min_inliers=G.CIRCUIT_MIN_INLIERS, loop_cooldown=32)
    if through == "PointTracker":
        top = tr = PointTracker(G.CIRCUIT_L, W.NN_THRESH, dev, **kw)
    else:
        top = SequenceTracker(None, dev, 0.015, 4, False, W.NN_THRESH, G.CIRCUIT_L, **kw)             # fed through its tracker: no network
        tr = top.tracker
    seen = 0
    for f in range(frames):
        xy = seq["pts"][f]
        frame = (_t(xy.reshape(-1, 2), dev), torch.tensor([xy.shape[0]], dtype=torch.int32, device=dev),
                 _t(np.asarray(seq["desc"][f], dtype=np.float32).reshape(-1, 256), dev))
        if f >= 2:                                                       # (the first frames allocate)
            torch.cuda.set_sync_debug_mode("error")
            try:
                tr.update_device(*frame)
            finally:
                torch.cuda.set_sync_debug_mode("default")
        else:
            tr.update_device(*frame)
        if f < 1:
            continue
        assert set(tr.last_geometry()) == CHECK_POSE_KEYS | ABS_KEYS | WORLD_KEYS | LOOP_KEYS | {"ba_info"}, f
        lms, n_lms = top.landmarks_device(*tr.landmark_params)
        n = int(n_lms)
        for name, own in (("_abs_lm", tr._abs_lm), ("_world_lm", tr._world_lm)):
            assert own["landmarks"] is not lms                          # the tracker's own buffers, not landmarks_device's
            assert torch.equal(own["n_landmarks"], n_lms), (f, name)
            assert torch.equal(own["landmarks"][:n], lms[:n]), (f, name)
        # the rows seen in the newest frame are copies of the landmark rows the tracker kept for the insert
        rows, _ = top.world_map()
        by_tid = {int(r[0]): r for r in lms[:n].cpu().numpy()}
        newest = rows[rows[:, 7] == f]
        seen += len(newest)
        for r in newest:
            assert np.array_equal(r[1:4], by_tid[int(r[0])][1:4]) and r[5] == by_tid[int(r[0])][5] and r[4] == by_tid[int(r[0])][4]
    ba = top.bundle_adjusted()
    print("%s: %d landmarks at the end, %d map rows written in their frames, ba_info %s, flags %s, closures %s"
          % (through, n, seen, ba[3].tolist(), tr.trajectory()[0][:frames, 14].tolist(), top.loop_closures().tolist()))
    assert seen >= 12 and n >= 12 and ba is not None


def test_trackers_refuse_a_loop_closure_without_a_map():
    from semantic_superpoint_amd.export import PointTracker, SequenceTracker
    dev = _dev()
    k = (300.0, 300.0, 160.0, 120.0)
    ok = dict(geometric_check="fundamental", intrinsics=k, world_map="observe")
    for make in (lambda **kw: PointTracker(3, 0.7, dev, **kw), lambda **kw: SequenceTracker(None, dev, 0.015, 4, False, 0.7, 3, **kw)):
        for kw in (dict(geometric_check="fundamental", intrinsics=k), dict(ok, loop_min_gap=0), dict(ok, loop_min_inliers=3),
                   dict(ok, loop_cooldown=-1), dict(ok, loop_iterations=0), dict(ok, loop_weight=0.0), dict(ok, trajectory_rows=1)):
            with pytest.raises(ValueError):
                make(loop_closure="observe", **kw)
        with pytest.raises(ValueError):
            make(loop_closure="always", **ok)
        t = make(loop_closure="apply", **ok)
        assert t.loop_closures().shape == (0, 9) and t.loop_edges_device() is None
