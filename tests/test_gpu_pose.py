"""The two-view pose on the device: ssp_pose_from_fundamental and ssp_pose_chain against their numpy
restatement (tests/pose_ref.py), fed the restatement's F and mask so that only the new kernels are under test; their
independence of batch and repetition; the pose and trajectory of PointTracker / SequenceTracker against the operators.

Tolerance of the continuous outputs (pose_ref.TOLERANCE = 1.14e-11): measured, not chosen.  The restatement was evaluated a
second way (numpy.longdouble) on the compared fixtures; the largest difference of R, t, E, depth, X (the last two relative to
max(1, |value|)) or a trajectory row was 7.10e-13 (the noisy fixture) and the tolerance is 16 times that;
tests/test_pose_cpu.py repeats the measurement.  cand, counts, n_front, front, status, n_shared and the flags are compared
for equality."""
import functools

import numpy as np
import pytest
import torch

from tests import pose_ref as P

pytestmark = pytest.mark.gpu

GEOMETRY_KEYS = {"F", "mask", "n_inliers", "status", "winner", "err"}
POSE_KEYS = ("R", "t", "E", "cand", "counts", "n_front", "status", "front", "depth", "X")


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@functools.lru_cache(maxsize=None)
def _arrays(pairs, cap, pair_stride, pt_stride, shared_intr):
    """Host inputs of one call over the pairs ((fixture, pair index), ...): pair p at entry p * pair_stride (the other entries
    hold noise), the restatement's F / mask / n_inliers / status, intrinsics [1,2,4] or [P,2,4]."""
    n_p = len(pairs)
    rng = np.random.RandomState(cap + 7 * pair_stride + 13 * pt_stride)
    pts1 = rng.uniform(0, 300, (n_p * pair_stride, cap, pt_stride))
    pts2 = rng.uniform(0, 300, (n_p * pair_stride, cap, pt_stride))
    match = np.zeros((n_p, cap, 3), dtype=np.float32)
    n_match = np.zeros(n_p, dtype=np.int32)
    geo = {"F": np.zeros((n_p, 3, 3)), "mask": np.zeros((n_p, cap), dtype=np.uint8), "n_inliers": np.zeros(n_p, dtype=np.int32),
           "status": np.zeros(n_p, dtype=np.int32)}
    intr = np.zeros((n_p, 2, 4))
    for p, (name, k) in enumerate(pairs):
        c = P.case(name)
        seq, r = c["seq"], c["ransac"][k]
        n = seq["pairs"][k]["m"].shape[0]
        pts1[p * pair_stride, :n, :2], pts2[p * pair_stride, :n, :2] = seq["pts"][k], seq["pts"][k + 1]
        match[p, :n], n_match[p] = seq["pairs"][k]["match"], n
        geo["F"][p], geo["mask"][p, :n], geo["n_inliers"][p], geo["status"][p] = r["F"], r["mask"], r["n_inliers"], r["status"]
        intr[p] = seq["pairs"][k]["intr"]
    if shared_intr:
        assert all(np.array_equal(intr[p], intr[0]) for p in range(n_p))
        intr = intr[:1]
    return pts1, pts2, match, n_match, geo, intr


def _run(pairs, cap, pair_stride=1, pt_stride=2, shared_intr=False, only=None):
    from semantic_superpoint_amd import lib as L
    dev = _dev()
    pts1, pts2, match, n_match, geo, intr = _arrays(tuple(pairs), cap, pair_stride, pt_stride, shared_intr)
    if only is not None:      # a call over one of the pairs
        sl = slice(only * pair_stride, (only + 1) * pair_stride)
        pts1, pts2, match, n_match = pts1[sl], pts2[sl], match[only:only + 1], n_match[only:only + 1]
        geo = {k: v[only:only + 1] for k, v in geo.items()}
        intr = intr if shared_intr else intr[only:only + 1]
    o = L.op_two_view_pose({k: _t(v, dev) for k, v in geo.items()}, _t(pts1, dev), _t(pts2, dev), _t(match, dev), _t(n_match, dev),
                           _t(intr, dev), pair_stride=pair_stride)
    torch.cuda.synchronize()
    return {k: o[k].cpu().numpy() for k in POSE_KEYS}


def _compare(o, p, ref, n, what):
    got = {k: o[k][p] for k in POSE_KEYS}
    worst = 0.0
    for k in ("R", "t", "E"):
        worst = max(worst, float(np.abs(got[k] - ref[k]).max()))
    for k in ("depth", "X"):
        if n:
            worst = max(worst, float((np.abs(got[k][:n] - ref[k]) / np.maximum(1.0, np.abs(ref[k]))).max()))
    bits = all(np.array_equal(got[k][:n] if k in ("depth", "X") else got[k], ref[k]) for k in ("R", "t", "E", "depth", "X"))
    print("%s: status %d cand %d counts %s worst difference %.3e (tolerance %.3e)%s"
          % (what, got["status"], got["cand"], got["counts"].tolist(), worst, P.TOLERANCE, ", bit-equal" if bits else ""))
    assert got["status"] == ref["status"] and got["cand"] == ref["cand"] and got["n_front"] == ref["n_front"], what
    assert np.array_equal(got["counts"], ref["counts"]), what
    assert np.array_equal(got["front"][:n].astype(bool), ref["front"]) and not got["front"][n:].any(), what
    assert not got["depth"][n:].any() and not got["X"][n:].any(), what
    assert not got["depth"][:n][~ref["front"]].any() and not got["X"][:n][~ref["front"]].any(), what
    assert worst <= P.TOLERANCE, (what, worst)
    if ref["status"] == 1:
        assert np.array_equal(got["R"], np.eye(3)) and not got["t"].any() and not got["E"].any() and not got["counts"].any()
        assert got["cand"] == -1 and not got["front"].any() and not got["depth"].any() and not got["X"].any()


def _compare_all(o, pairs):
    for p, (name, k) in enumerate(pairs):
        c = P.case(name)
        _compare(o, p, c["pose"][k], c["seq"]["pairs"][k]["m"].shape[0], "%s[%d]" % (name, k))


FOUR = (("mixed48", 0), ("eight", 0), ("five", 0), ("empty", 0))       # n_match = (48, 8, 5, 0)
FOUR_K = (("mixed48", 0), ("eight_k", 0), ("five", 0), ("empty", 0))   # ... with a pair of other intrinsics among them


@pytest.mark.parametrize("shared_intr", (True, False))
@pytest.mark.parametrize("pair_stride,pt_stride", ((1, 2), (1, 3), (2, 2), (2, 3)))
def test_four_pairs_in_one_call(pair_stride, pt_stride, shared_intr):
    pairs = FOUR if shared_intr else FOUR_K
    assert [P.case(nm)["seq"]["pairs"][k]["m"].shape[0] for nm, k in pairs] == [48, 8, 5, 0]
    k = P.case("mixed48")["seq"]["pairs"][0]["intr"]
    assert not np.array_equal(k[0], k[1])                                # unequal views
    o = _run(pairs, 64, pair_stride, pt_stride, shared_intr)
    _compare_all(o, pairs)
    assert [int(s) for s in o["status"]] == [0, 0, 1, 1]


@pytest.mark.parametrize("name,cap,n", (("n257", 320, 257), ("n4096", 4096, 4096), ("noisy", 256, 250)))
def test_one_pair(name, cap, n):
    assert P.case(name)["seq"]["pairs"][0]["m"].shape[0] == n
    o = _run(((name, 0),), cap, 1, 3)
    _compare_all(o, ((name, 0),))
    assert int(o["status"][0]) == 0 and int(o["n_front"][0]) == P.case(name)["ransac"][0]["n_inliers"]


def _same(a, b, pa=slice(None), pb=slice(None)):
    for k in POSE_KEYS:
        assert np.array_equal(np.ascontiguousarray(a[k][pa]).view(np.uint8), np.ascontiguousarray(b[k][pb]).view(np.uint8)), k


def test_result_does_not_depend_on_batch_or_run():
    base = _run(FOUR_K, 64, 2, 3)
    _same(base, _run(FOUR_K, 64, 2, 3))                       # a repeated call
    for p in range(4):                                        # 4 pairs in one call = 4 single calls
        _same(base, _run(FOUR_K, 64, 2, 3, only=p), slice(p, p + 1))


def test_salted_mask_is_ambiguous():
    from semantic_superpoint_amd import lib as L
    from tests.test_pose_cpu import salted_scene
    dev = _dev()
    pr, m = salted_scene()
    n, cap = m.shape[0], 64
    pts1, pts2 = np.zeros((1, cap, 2)), np.zeros((1, cap, 2))
    pts1[0, :n], pts2[0, :n] = m[:, :2], m[:, 2:]
    match = np.zeros((1, cap, 3), dtype=np.float32)
    match[0, :n, 0] = match[0, :n, 1] = np.arange(n)
    mask = np.zeros((1, cap), dtype=np.uint8)
    mask[0, :n] = 1
    geo = {"F": _t(pr["F"][None], dev), "mask": _t(mask, dev), "n_inliers": _t(np.array([n], dtype=np.int32), dev),
           "status": _t(np.zeros(1, dtype=np.int32), dev)}
    o = L.op_two_view_pose(geo, _t(pts1, dev), _t(pts2, dev), _t(match, dev), _t(np.array([n], dtype=np.int32), dev),
                           _t(pr["intr"][None], dev))
    ref = P.two_view_pose(pr["F"], np.ones(n, dtype=bool), n, 0, m, pr["intr"])
    assert ref["status"] == 2
    _compare({k: o[k].cpu().numpy() for k in POSE_KEYS}, 0, ref, n, "salted")


def test_bad_arguments_are_errors():
    from semantic_superpoint_amd import lib as L
    dev = _dev()
    pts1, pts2, match, n_match, geo, intr = _arrays(FOUR, 64, 1, 2, True)
    g = {k: _t(v, dev) for k, v in geo.items()}
    args = (_t(pts1, dev), _t(pts2, dev), _t(match, dev), _t(n_match, dev))
    with pytest.raises(ValueError):
        L.op_two_view_pose(g, *args, _t(np.zeros((2, 2, 4)), dev))                  # neither 1 nor P
    with pytest.raises(ValueError):
        L.op_two_view_pose(g, *args, _t(intr, dev).float())
    with pytest.raises(ValueError):
        L.op_two_view_pose({k: v for k, v in g.items() if k != "mask"}, *args, _t(intr, dev))
    with pytest.raises(RuntimeError):
        L.op_two_view_pose(g, *args, torch.from_numpy(intr))                        # on the host


# ---- the scale chain and the trajectory -------------------------------------------------------------------------------------
def _chain_scenarios():
    """name -> per pair of seq5 (mask, n_inliers, status) as the pose operator is given them."""
    c = P.case("seq5")
    base = [(r["mask"], r["n_inliers"], r["status"]) for r in c["ransac"]]
    n = base[0][0].shape[0]
    no_pose = list(base)
    no_pose[1] = (np.zeros(n, dtype=bool), 0, 1)                   # one frame with no model in the middle
    # fewer than 8 shared points: pair 0 keeps 20 of its inliers, pair 1 five of those points and 15 others
    seq = c["seq"]
    in0 = np.nonzero(base[0][0])[0]
    keep0 = np.zeros(n, dtype=bool)
    keep0[in0[:20]] = True
    pts_f1 = set(seq["pairs"][0]["match"][in0[:20], 1].astype(int).tolist())        # rows of frame 1 that pair 0 keeps
    in1 = np.nonzero(base[1][0])[0]
    seen = np.array([int(seq["pairs"][1]["match"][k, 0]) in pts_f1 for k in in1])
    keep1 = np.zeros(n, dtype=bool)
    keep1[in1[seen][:5]] = True
    keep1[in1[~seen][:15]] = True
    few = list(base)
    few[0], few[1] = (keep0, 20, 0), (keep1, 20, 0)
    return {"plain": base, "no_pose": no_pose, "few_shared": few}


@pytest.mark.parametrize("scenario", ("plain", "no_pose", "few_shared"))
def test_pose_chain_over_five_frames(scenario):
    from semantic_superpoint_amd import lib as L
    dev = _dev()
    c = P.case("seq5")
    seq = c["seq"]
    geo_in = _chain_scenarios()[scenario]
    n_p, n, cap = len(seq["pairs"]), seq["pts"][0].shape[0], 64
    ref = [P.two_view_pose(c["ransac"][k]["F"], geo_in[k][0], geo_in[k][1], geo_in[k][2], seq["pairs"][k]["m"], seq["pairs"][k]["intr"])
           for k in range(n_p)]
    ref_rows, ref_state = P.run_chain(ref, [pr["match"] for pr in seq["pairs"]], cap=cap)
    pts = np.zeros((n_p + 1, cap, 2))
    match = np.zeros((n_p, cap, 3), dtype=np.float32)
    mask = np.zeros((n_p, cap), dtype=np.uint8)
    for f in range(n_p + 1):
        pts[f, :n] = seq["pts"][f]
    for k in range(n_p):
        match[k, :n], mask[k, :n] = seq["pairs"][k]["match"], geo_in[k][0]
    geo = {"F": _t(np.stack([r["F"] for r in c["ransac"]]), dev), "mask": _t(mask, dev),
           "n_inliers": _t(np.array([g[1] for g in geo_in], dtype=np.int32), dev),
           "status": _t(np.array([g[2] for g in geo_in], dtype=np.int32), dev)}
    pd, md = _t(pts, dev), _t(match, dev)
    nm = _t(np.full(n_p, n, dtype=np.int32), dev)
    o = L.op_two_view_pose(geo, pd[:n_p], pd[1:], md, nm, _t(np.stack([pr["intr"] for pr in seq["pairs"]]), dev))
    host = {k: o[k].cpu().numpy() for k in POSE_KEYS}
    for k in range(n_p):
        _compare(host, k, ref[k], n, "%s pair %d" % (scenario, k))
    state, table = L.pose_state(dev), L.pose_table(n_p + 2, dev)
    sl = lambda d, k: {key: d[key][k:k + 1] for key in POSE_KEYS}
    for k in range(n_p):
        prev = sl(o, k - 1) if k else None
        L.op_pose_chain(prev, sl(o, k), md[k - 1:k] if k else None, md[k:k + 1], nm[k - 1:k] if k else None, nm[k:k + 1], state, table)
    rows, st = table.cpu().numpy(), state.cpu().numpy()
    print("%s: s %s n_shared %s flags %s ratio %s" % (scenario, rows[:n_p, 12], rows[:n_p, 13], rows[:n_p, 14], rows[:n_p, 15]))
    worst = float(np.abs(rows[:n_p] - ref_rows).max())
    print("%s: rows differ by %.3e, state by %.3e (tolerance %.3e)" % (scenario, worst, float(np.abs(st - P.state_words(ref_state)).max()),
                                                                     P.TOLERANCE))
    assert np.array_equal(rows[:n_p, 13:15], ref_rows[:, 13:15])                 # n_shared and flags: exactly
    assert worst <= P.TOLERANCE and np.abs(st - P.state_words(ref_state)).max() <= P.TOLERANCE
    assert st[0] == n_p and not rows[n_p:].any()
    if scenario == "plain":
        assert list(rows[:n_p, 14]) == [2, 0, 0, 0] and (rows[1:n_p, 13] == seq["n_in"]).all()
        want = seq["centres"][1:] / np.linalg.norm(seq["centres"][1])
        assert np.abs(P.scaled_centres(rows[:n_p]) - want).max() <= P.CENTRE_BOUND + P.TOLERANCE
    elif scenario == "no_pose":
        assert list(rows[:n_p, 14]) == [2, 3, 2, 0]                               # flag bit 0 in the middle, the scale carried
        assert np.array_equal(rows[1, :12], rows[0, :12]) and rows[1, 12] == rows[2, 12] == 1.0 and rows[3, 12] != 1.0
    else:
        assert rows[1, 13] == 5 and rows[1, 14] == 2 and rows[1, 12] == 1.0 and rows[2, 14] == 0
    # a full table stops growing; the state still advances
    small, st2 = L.pose_table(2, dev), L.pose_state(dev)
    for k in range(n_p):
        L.op_pose_chain(sl(o, k - 1) if k else None, sl(o, k), md[k - 1:k] if k else None, md[k:k + 1], nm[k - 1:k] if k else None,
                        nm[k:k + 1], st2, small)
    assert torch.equal(small, table[:2]) and float(st2[0]) == 2.0 and torch.equal(st2[1:], state[1:])


# ---- the trackers ------------------------------------------------------------------------------------------------------------
NN_THRESH, MAX_LENGTH = 0.7, 4


@functools.lru_cache(maxsize=None)
def _descriptors():
    """One unit descriptor per point of seq5_k (the strays keep theirs too, so the matcher pairs them up as the fixture does):
    the true correspondences are the mutual nearest neighbours."""
    n = P.case("seq5_k")["seq"]["pts"][0].shape[0]
    d = np.random.RandomState(77).randn(n, 256)
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def _frame(f, dev):
    seq = P.case("seq5_k")["seq"]
    xy, desc = seq["pts"][f], _descriptors()[seq["ids"][f]]
    return _t(xy, dev), torch.tensor([xy.shape[0]], dtype=torch.int32, device=dev), _t(desc, dev)


def test_point_tracker_pose_and_trajectory():
    from semantic_superpoint_amd import lib as L
    from semantic_superpoint_amd.export import PointTracker
    dev = _dev()
    c = P.case("seq5_k")
    seq = c["seq"]
    frames, seed0 = len(seq["pts"]), c["seeds"][0] - 1              # frame f checks with seed0 + f: pair k with the fixture's seed
    intr = tuple(seq["intr"][0])                                     # one camera throughout
    tr = PointTracker(MAX_LENGTH, NN_THRESH, dev, geometric_check="fundamental", check_seed=seed0, intrinsics=intr,
                      trajectory_rows=frames + 1)
    two = PointTracker(MAX_LENGTH, NN_THRESH, dev, geometric_check="fundamental", check_seed=seed0, intrinsics=(intr, intr),
                       trajectory_rows=frames + 1)                   # the same camera given per view
    plain = PointTracker(MAX_LENGTH, NN_THRESH, dev, geometric_check="fundamental", check_seed=seed0)
    assert tr.trajectory() is None and plain.trajectory() is None
    cap = 1024
    kd = _t(np.stack([seq["intr"][0], seq["intr"][0]])[None], dev)
    state, table = L.pose_state(dev), L.pose_table(frames + 1, dev)
    zero = torch.zeros(1, dtype=torch.int32, device=dev)
    prev = prev_pose = None
    for f in range(frames):
        xy, cnt, desc = _frame(f, dev)
        tr.update_device(xy, cnt, desc)
        two.update_device(xy, cnt, desc)
        plain.update_device(xy, cnt, desc)
        # the same frame through the operators
        p, d = torch.zeros(1, cap, 2, dtype=torch.float64, device=dev), torch.zeros(1, cap, 256, device=dev)
        p[0, :xy.shape[0]], d[0, :xy.shape[0]] = xy, desc
        pp, pdsc, pc = prev if prev is not None else (torch.zeros_like(p), torch.zeros_like(d), zero)
        m, nm = L.op_match_two_way(pdsc, pc, d, cnt, NN_THRESH)
        g = L.op_epipolar_ransac(pp, p, m, nm, torch.tensor([seed0 + f], dtype=torch.int64, device=dev))
        pose = L.op_two_view_pose(g, pp, p, m, nm, kd)
        L.op_pose_chain(prev_pose[0] if prev_pose else None, pose, prev_pose[1] if prev_pose else None, m,
                        prev_pose[2] if prev_pose else None, nm, state, table)
        got = tr.last_geometry()
        assert set(got) == GEOMETRY_KEYS | {("pose_status" if k == "status" else k) for k in POSE_KEYS}
        for k in POSE_KEYS:
            assert torch.equal(got["pose_status" if k == "status" else k], pose[k]), (f, k)     # bit for bit
        for k in GEOMETRY_KEYS:
            assert torch.equal(got[k], g[k]), (f, k)
        t_table, t_n = tr.trajectory()
        assert torch.equal(t_table, table) and float(t_n) == f + 1 == float(state[0])
        assert set(plain.last_geometry()) == GEOMETRY_KEYS                                       # exactly the old keys
        for k in ("ids", "tid", "score", "state"):                                               # the tracks do not change
            rows = int(plain.table["state"][0]) if k != "state" else None
            assert torch.equal(tr.table[k][:rows], plain.table[k][:rows]), k
        if f > 0:
            assert int(nm) == xy.shape[0] and int(g["status"]) == 0 and int(pose["status"][0]) == 0
            assert int(pose["n_front"][0]) == int(g["n_inliers"][0]) == seq["n_in"]
            # the device's F is the restatement's to 2.94e-11 per entry of a unit-norm matrix (section 22); K2^T F K1 multiplies an
            # entry by up to f^2 = 9e4, so E and with it R and t follow the restatement to 2.94e-11 * 9e4 = 2.6e-6 at worst
            # (not `cand`: the two leading singular values are equal, the basis of their plane and with it the numbering of the
            # candidates hang on the last bits of F; R and t do not)
            ref = c["pose"][f - 1]
            assert np.abs(pose["R"][0].cpu().numpy() - ref["R"]).max() < 1e-5 and np.abs(pose["t"][0].cpu().numpy() - ref["t"]).max() < 1e-5
            assert P.angle_deg(pose["R"][0].cpu().numpy(), seq["pairs"][f - 1]["R"]) < 1e-3
        for k in two.last_geometry():
            assert torch.equal(two.last_geometry()[k], got[k]), (f, k)
        assert torch.equal(two.trajectory()[0], t_table)
        prev, prev_pose = (p, d, cnt), (pose, m, nm)
    rows = table.cpu().numpy()
    assert list(rows[:frames, 14]) == [3, 2, 0, 0, 0] and not rows[0, 9:12].any() and rows[1, 12] == 1.0
    want = seq["centres"][1:] / np.linalg.norm(seq["centres"][1])      # the trajectory is the true one up to the global scale
    assert np.abs(P.scaled_centres(rows[1:frames]) - want).max() < 1e-4   # (four such poses chained: the same reasoning)


def test_intrinsics_need_the_fundamental_check():
    from semantic_superpoint_amd.export import PointTracker
    dev = _dev()
    for mode in (None, "homography"):
        with pytest.raises(ValueError):
            PointTracker(MAX_LENGTH, NN_THRESH, dev, geometric_check=mode, intrinsics=(300.0, 300.0, 160.0, 120.0))
    with pytest.raises(ValueError):
        PointTracker(MAX_LENGTH, NN_THRESH, dev, geometric_check="fundamental", intrinsics=(300.0, 300.0, 160.0))
    with pytest.raises(ValueError):
        PointTracker(MAX_LENGTH, NN_THRESH, dev, geometric_check="fundamental", intrinsics=(0.0, 300.0, 160.0, 120.0))


def test_sequence_tracker_step_with_intrinsics_does_not_synchronise(tmp_path):
    from semantic_superpoint_amd.export import PointTracker, SequenceTracker
    from tests.test_gpu_tracks import _agent, _no_host_sync, _shifted_frames
    dev = _dev()
    agent = _agent(tmp_path, dev)
    args = (agent.net, dev, agent.conf_thresh, agent.nms_dist, False, agent.nn_thresh, 3)
    intr = (90.0, 92.0, 48.0, 32.0)
    seq = SequenceTracker(*args, geometric_check="fundamental", min_inliers=8, intrinsics=intr, trajectory_rows=8)
    plain = SequenceTracker(*args, geometric_check="fundamental", min_inliers=8)
    fed = PointTracker(3, agent.nn_thresh, dev, geometric_check="fundamental", min_inliers=8, intrinsics=intr, trajectory_rows=8)
    assert seq.tracker.intrinsics.shape == (2, 4) and plain.tracker.intrinsics is None
    for f, im in enumerate(_shifted_frames()):            # 64x96 frames
        on_dev = torch.from_numpy(im).to(dev)
        if f == 0:
            o = seq.step(on_dev)                          # (the first step allocates)
        else:
            with _no_host_sync():
                o = seq.step(on_dev)
        plain.step(on_dev)
        fed.update_device(o["pts"][0][:, :2].to(torch.float64), o["count"][0:1], o["desc"][0])
        g, h = seq.tracker.last_geometry(), fed.last_geometry()
        assert set(g) == set(h) == GEOMETRY_KEYS | {("pose_status" if k == "status" else k) for k in POSE_KEYS}
        for k in g:
            assert torch.equal(g[k], h[k]), (f, k)                                   # bit for bit
        assert torch.equal(seq.trajectory()[0], fed.trajectory()[0]) and float(seq.trajectory()[1]) == f + 1
        assert set(plain.tracker.last_geometry()) == GEOMETRY_KEYS and plain.trajectory() is None
        for k in GEOMETRY_KEYS:
            assert torch.equal(g[k], plain.tracker.last_geometry()[k]), (f, k)       # the check itself is unchanged
        assert int(g["pose_status"]) in (0, 1, 2)
    assert np.array_equal(seq.get_tracks(2), plain.get_tracks(2))
