"""Absolute pose from landmarks on the device: ssp_op_landmark_matches, ssp_pnp_ransac and ssp_pose_repair
against their numpy restatement (tests/pnp_ref.py), their independence of the batch, the workgroup count and repetition, and the
absolute pose and the repair inside PointTracker / SequenceTracker against the operators and the truth.

mask, n_inliers, status and winner are compared for equality.  Tolerance of Rw, C and rms (pnp_ref.TOLERANCE = 2.1e-13):
measured, not chosen - 16 times the largest difference between the restatement in float64 and in numpy.longdouble over the
compared fixtures (1.33e-14); tests/test_pnp_cpu.py repeats the measurement.  The bound against the truth is 16 times the
restatement's own error.  Every comparison prints what the device showed before it asserts."""
import contextlib
import functools

import numpy as np
import pytest
import torch

from tests import landmarks_ref as LR
from tests import pnp_ref as R
from tests import pose_ref as P

pytestmark = pytest.mark.gpu

SENTINEL = -77


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _pack(problems, cap):
    """corr [P, cap, CORR_WORDS] and n [P] of (corr rows, rows used); the rows past a problem's n are valid copies of the first
    problem's rows: a kernel that read them would count them."""
    P_ = len(problems)
    corr = np.zeros((P_, cap, R.CORR_WORDS))
    n = np.zeros(P_, dtype=np.int32)
    fill = problems[0][0]
    for p, (rows, used) in enumerate(problems):
        reps = -(-cap // fill.shape[0])
        corr[p] = np.tile(fill, (reps, 1))[:cap]
        corr[p, :rows.shape[0]] = rows[:cap]
        n[p] = used
    return corr, n


def _run(corr, n, intr, seeds, dev, **kw):
    from semantic_superpoint_amd import lib
    P_, cap = corr.shape[0], corr.shape[1]
    out = lib.pnp_buffers(P_, cap, dev)
    for k in lib.PNP_KEYS:
        out[k].fill_(SENTINEL if k != "mask" else 7)
    res = lib.op_pnp_ransac(_t(corr, dev), _t(n, dev), _t(np.asarray(intr, dtype=np.float64).reshape(-1, 4), dev),
                            _t(np.asarray(seeds, dtype=np.int64), dev), out=out, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items()}


def _compare(got, p, ref, what):
    worst = max(float(np.abs(got["Rw"][p] - np.asarray(ref["Rw"], dtype=np.float64)).max()),
                float(np.abs(got["C"][p] - np.asarray(ref["C"], dtype=np.float64)).max()), abs(float(got["rms"][p]) - float(ref["rms"])))
    bits = (np.array_equal(got["Rw"][p], np.asarray(ref["Rw"], dtype=np.float64)) and np.array_equal(got["C"][p], np.asarray(ref["C"], dtype=np.float64))
            and float(got["rms"][p]) == float(ref["rms"]))
    print("%s: status %d, winner %d, %d inliers (restatement %d, %d, %d), worst difference %.3e (tolerance %.3e)%s"
          % (what, got["status"][p], got["winner"][p], got["n_inliers"][p], ref["status"], ref["winner"], ref["n_inliers"], worst,
             R.TOLERANCE, ", bit-equal" if bits else ""))
    assert got["status"][p] == ref["status"] and got["winner"][p] == ref["winner"] and got["n_inliers"][p] == ref["n_inliers"], what
    cap = got["mask"].shape[1]
    want = np.zeros(cap, dtype=np.uint8)
    want[:ref["mask"].shape[0]] = ref["mask"][:cap]
    assert np.array_equal(got["mask"][p], want), what
    assert worst <= R.TOLERANCE, (what, worst)


@functools.lru_cache(maxsize=None)
def _batch(per_problem):
    """Four problems in arrays of cap 64: n = 48, 6, 3, 0.  Shared intrinsics: the fixtures side48 and six (one camera);
    per-problem intrinsics: the second problem is the first 6 rows of the zooming fixture under its own camera."""
    a, six, zoom = R.case("side48"), R.case("six"), R.case("zoom")
    assert a["n"] == 48 and six["n"] == 6 and np.array_equal(a["k"], six["k"]) and not np.array_equal(a["k"], zoom["k"])
    second = (zoom["corr"][:6], zoom["k"]) if per_problem else (six["corr"], six["k"])
    problems = [(a["corr"], 48), (second[0], 6), (a["corr"], 3), (a["corr"], 0)]
    ks = [a["k"], second[1], a["k"], a["k"]]
    seeds = [a["seed"], six["seed"], 77, 78]
    corr, n = _pack(problems, 64)
    refs = [R.ransac(corr[p], n[p], ks[p], seeds[p]) for p in range(4)]
    return corr, n, np.stack(ks), seeds, refs


@pytest.mark.parametrize("per_problem", (False, True))
def test_four_problems_in_one_call(per_problem):
    corr, n, ks, seeds, refs = _batch(per_problem)
    got = _run(corr, n, ks if per_problem else ks[:1], seeds, _dev())
    assert [r["status"] for r in refs] == [0, 0, 1, 1] and refs[0]["n_inliers"] == 48 and refs[1]["n_inliers"] == 6
    for p in range(4):
        _compare(got, p, refs[p], "problem %d of 4 (%s intrinsics)" % (p, "per-problem" if per_problem else "shared"))
    for p in (2, 3):                                                    # no pose: identity, zero, an empty mask
        assert np.array_equal(got["Rw"][p], np.eye(3)) and not got["C"][p].any() and not got["mask"][p].any() and got["rms"][p] == 0.0
    for p in (0, 1):
        c = R.case("side48") if p == 0 else (R.case("zoom") if per_problem else R.case("six"))
        err = max(float(np.abs(got["Rw"][p] - c["Rw"]).max()), float(np.abs(got["C"][p] - c["C"]).max()))
        print("problem %d against the truth: %.3e (bound %.3e)" % (p, err, R.TRUTH_BOUND))
        assert err <= R.TRUTH_BOUND


@pytest.mark.parametrize("name,cap", (("n257", 320), ("n4096", 4096), ("noisy", 160), ("salted", 128), ("planar", 96), ("forward", 64)))
def test_fixture_against_the_restatement(name, cap):
    c = R.case(name)
    if name == "n257":
        assert c["n"] == 257                                            # the strided sums and the masks cross waves and the 256-row stride
    if name == "n4096":
        assert c["n"] == cap == 4096                                    # the largest problem
    corr, n = _pack([(c["corr"], c["n"])], cap)
    got = _run(corr, n, c["k"], [c["seed"]], _dev())
    _compare(got, 0, c["res"], name)
    if c["noise"] == 0.0:
        assert np.array_equal(got["mask"][0, :c["n"]].astype(bool), c["truth"])
        err = max(float(np.abs(got["Rw"][0] - c["Rw"]).max()), float(np.abs(got["C"][0] - c["C"]).max()))
        print("%s against the truth: %.3e (bound %.3e)" % (name, err, R.TRUTH_BOUND))
        assert err <= R.TRUTH_BOUND


def test_min_inliers_thresh_and_the_single_hypothesis():
    c = R.case("side48")
    dev = _dev()
    corr, n = _pack([(c["corr"], 4), (c["corr"], 5), (c["corr"], 48)], 64)
    for kw in (dict(min_inliers=4), dict(min_inliers=5), dict(min_inliers=6), dict(thresh=0.5, min_inliers=40), dict(min_inliers=49)):
        got = _run(corr, n, c["k"], [5, 6, 7], dev, **kw)
        for p in range(3):
            _compare(got, p, R.ransac(corr[p], n[p], c["k"], 5 + p, **kw), "n = %d %s" % (n[p], kw))
    got = _run(corr, n, c["k"], [5, 6, 7], dev, min_inliers=4)
    assert got["status"].tolist() == [0, 0, 0] and got["winner"][0] == 0 and got["n_inliers"].tolist() == [4, 5, 48]


def test_result_does_not_depend_on_groups_batch_or_repetition():
    corr, n, ks, seeds, _ = _batch(True)
    big = R.case("n257")
    dev = _dev()
    base = _run(corr, n, ks, seeds, dev)
    for groups in (1, 3, 16, 0):
        got = _run(corr, n, ks, seeds, dev, groups=groups)
        for k in base:
            assert np.array_equal(got[k], base[k]), (groups, k)
    for p in range(4):                                                   # four single calls
        got = _run(corr[p:p + 1], n[p:p + 1], ks[p:p + 1], seeds[p:p + 1], dev)
        for k in base:
            assert np.array_equal(got[k][0], base[k][p]), (p, k)
    c2, n2 = _pack([(big["corr"], big["n"])], 320)
    first = _run(c2, n2, big["k"], [big["seed"]], dev, groups=1)
    for groups in (3, 16, 64, 0):                                        # slices of 171, 32 and 8 hypotheses
        got = _run(c2, n2, big["k"], [big["seed"]], dev, groups=groups)
        for k in first:
            assert np.array_equal(got[k], first[k]), (groups, k)


# ---- the join ------------------------------------------------------------------------------------------------------------------
def _join(lm, n_lm, match, n_match, pts, dev, row_cap=None, pt_stride=2):
    from semantic_superpoint_amd import lib
    row_cap = lm.shape[0] if row_cap is None else row_cap
    rows = np.full((row_cap, LR.LANDMARK_WORDS), 3.0)                    # rows past n_landmarks name point 3: they must not be read
    rows[:lm.shape[0]] = lm
    p = np.full((pts.shape[0], pt_stride), 5.0)
    p[:, :2] = pts
    out = lib.pnp_buffers(1, match.shape[0], dev)
    out["corr"].fill_(SENTINEL)
    corr, n = lib.op_landmark_matches(_t(rows, dev), torch.tensor([n_lm], dtype=torch.int32, device=dev), _t(match, dev),
                                      torch.tensor([n_match], dtype=torch.int32, device=dev), _t(p, dev), out=out)
    torch.cuda.synchronize()
    return corr.cpu().numpy(), n.cpu().numpy()


def test_landmark_matches_against_the_numpy_join():
    dev = _dev()
    lm = np.zeros((8, LR.LANDMARK_WORDS))
    lm[:, 1:4] = np.arange(24).reshape(8, 3) + 1.0
    lm[:, 7] = [2, 0, 2, -1, 5, 99, 0, 3]                               # duplicates, no newest point (-1), past the frame's points
    pts = np.arange(12, dtype=np.float64).reshape(6, 2)
    match = np.zeros((7, 3), dtype=np.float32)
    match[:] = [[0, 1, .1], [2, 0, .2], [3, 3, .3], [5, 5, .4], [4, 2, .5], [7, 9, .6], [2, 4, .7]]
    for n_lm, n_match, row_cap in ((7, 7, 8), (8, 7, 8), (0, 7, 8), (8, 0, 8), (7, 5, 300), (-3, 99, 8)):
        want, (n, nv) = R.join(lm, n_lm, match, n_match, pts)
        got, gn = _join(lm, n_lm, match, n_match, pts, dev, row_cap=row_cap, pt_stride=3)
        assert gn.tolist() == [n, nv], (n_lm, n_match)
        assert np.array_equal(got, want), (n_lm, n_match)               # every row of cap is written: zero where there is none
    nan = lm.copy()
    nan[1, 2] = np.nan
    got, gn = _join(nan, 8, match, 7, pts, dev)
    assert np.array_equal(got, R.join(nan, 8, match, 7, pts)[0]) and got[0, 6] == 0.0
    # a real window: 15 slow frames, the matches of the 16th; n_match = cap
    c = R.slow_problem()
    full = c["match"][:c["n_match"]]
    for match, n_match in ((c["match"], c["n_match"]), (full, c["n_match"])):
        want, (n, nv) = R.join(c["landmarks"], c["landmarks"].shape[0], match, n_match, c["pts_new"])
        got, gn = _join(c["landmarks"], c["landmarks"].shape[0], match, n_match, c["pts_new"], dev, row_cap=16 * 48)
        assert gn.tolist() == [n, nv] and nv >= 30 and np.array_equal(got, want)
    assert full.shape[0] == c["n_match"]
    got = _run(want[None], np.array([n], dtype=np.int32), c["k"], [c["seed"]], dev)
    want_res = R.ransac(want, n, c["k"], c["seed"])
    _compare(got, 0, want_res, "slow camera, one window of 16")
    assert np.array_equal(got["mask"][0, :n].astype(bool), c["truth"][:n])
    err = max(float(np.abs(got["Rw"][0] - c["Rw"]).max()), float(np.abs(got["C"][0] - c["C"]).max()))
    print("slow camera against the truth: %.3e" % err)
    assert err <= 16.0 * (LR.TRUTH_ERROR + R.TRUTH_ERROR)


# ---- the repair ----------------------------------------------------------------------------------------------------------------
def test_pose_repair_against_the_restatement():
    from semantic_superpoint_amd import lib
    from tests.test_pnp_cpu import _flagged_table
    dev = _dev()
    state, table = _flagged_table()
    Rw = P._rodrigues(np.array([3.0, -8.0, 2.0]))
    good = {"Rw": Rw, "C": np.array([2.5, 0.2, -0.1]), "status": 0}
    unflagged = table.copy()
    unflagged[3, 14] = 0.0
    full = table.copy()
    full[4:] = table[3]                                                  # capacity 6, 6 rows: a full table
    full_state = state.copy()
    full_state[0] = 6.0
    only0 = table.copy()
    only0[3, 14] = 1.0
    near = dict(good, C=table[2, 9:12] + np.array([0.8 / 65.0, 0.0, 0.0]))
    first = state.copy()
    first[0] = 1.0                                                       # one row: there is no previous centre
    cases = [(good, state, table), (good, state, unflagged), (dict(good, status=1), state, table), (good, full_state, full),
             (dict(good, C=np.array([np.nan, 0.0, 0.0])), state, table), (near, state, table), (near, state, only0), (good, first, table)]
    S = len(cases)
    absolute = {"Rw": _t(np.stack([c[0]["Rw"].reshape(3, 3) for c in cases]), dev), "C": _t(np.stack([c[0]["C"] for c in cases]), dev),
                "status": _t(np.array([c[0]["status"] for c in cases], dtype=np.int32), dev)}
    st, tb = _t(np.stack([c[1] for c in cases]), dev), _t(np.stack([c[2] for c in cases]), dev)
    lib.op_pose_repair(absolute, st, tb)
    torch.cuda.synchronize()
    st, tb = st.cpu().numpy(), tb.cpu().numpy()
    changed = []
    for q, (a, s, t) in enumerate(cases):
        ws, wt = R.repair(a, s, t)
        assert np.array_equal(st[q], ws) and np.array_equal(tb[q], wt), q           # plain copies, one sqrt: bit for bit
        changed.append(not (np.array_equal(st[q], s) and np.array_equal(tb[q], t)))
    assert changed == [True, False, False, False, False, True, True, True]
    assert tb[0, 3, 14] == lib.POSE_FLAG_ABSOLUTE == 4 and tb[5, 3, 14] == 6 and tb[6, 3, 14] == 4 and tb[7, 0, 14] == 6
    # one sequence through the unbatched shapes
    s1, t1 = _t(state, dev), _t(table, dev)
    lib.op_pose_repair({k: v[:1] for k, v in absolute.items()}, s1, t1)
    assert np.array_equal(s1.cpu().numpy(), st[0]) and np.array_equal(t1.cpu().numpy(), tb[0])


def test_wrappers_validate_their_arguments():
    from semantic_superpoint_amd import lib
    dev = _dev()
    c = R.case("six")
    corr, n = _pack([(c["corr"], 6)], 16)
    corr, n, k, seed = _t(corr, dev), _t(n, dev), _t(c["k"][None], dev), torch.tensor([1], dtype=torch.int64, device=dev)
    with pytest.raises(ValueError):
        lib.op_pnp_ransac(corr, n, k, seed, min_inliers=3)
    with pytest.raises(ValueError):
        lib.op_pnp_ransac(corr.to(torch.float32), n, k, seed)
    with pytest.raises(ValueError):
        lib.op_pnp_ransac(corr, n, k.repeat(2, 1), seed)
    with pytest.raises(ValueError):
        lib.op_pnp_ransac(corr[:, :, :7].contiguous(), n, k, seed)
    with pytest.raises(RuntimeError):
        lib.op_pnp_ransac(corr, n, k, seed, groups=65)
    with pytest.raises(RuntimeError):
        lib.op_pnp_ransac(corr, n, k, seed, thresh=float("nan"))
    with pytest.raises(RuntimeError):
        lib.op_pnp_ransac(corr.cpu(), n, k, seed)
    lm, one = torch.zeros(4, lib.LANDMARK_WORDS, dtype=torch.float64, device=dev), torch.ones(1, dtype=torch.int32, device=dev)
    match, pts = torch.zeros(8, 3, device=dev), torch.zeros(8, 2, dtype=torch.float64, device=dev)
    with pytest.raises(ValueError):
        lib.op_landmark_matches(lm[:, :7].contiguous(), one, match, one, pts)
    with pytest.raises(ValueError):
        lib.op_landmark_matches(lm, one, match.to(torch.float64), one, pts)
    with pytest.raises(ValueError):
        lib.op_landmark_matches(lm, one, match, one, pts, out=lib.pnp_buffers(1, 9, dev))
    res = lib.op_pnp_ransac(corr, n, k, seed)
    with pytest.raises(ValueError):
        lib.op_pose_repair({"Rw": res["Rw"]}, lib.pose_state(dev), lib.pose_table(4, dev))
    with pytest.raises(ValueError):
        lib.op_pose_repair(res, lib.pose_state(dev, 2), lib.pose_table(4, dev))
    assert lib.CORR_WORDS == R.CORR_WORDS and lib.POSE_FLAG_ABSOLUTE == R.FLAG_ABSOLUTE


# ---- the trackers --------------------------------------------------------------------------------------------------------------
NN_THRESH, MAX_LENGTH = 0.7, 5
OLD_KEYS = {"F", "mask", "n_inliers", "status", "winner", "err", "R", "t", "E", "cand", "counts", "n_front", "pose_status", "front",
            "depth", "X"}
ABS_KEYS = {"abs_" + k for k in ("Rw", "C", "mask", "n_inliers", "winner", "rms", "status", "corr", "n_corr")}


@contextlib.contextmanager
def _no_host_sync():
    torch.cuda.set_sync_debug_mode("error")
    try:
        yield
    finally:
        torch.cuda.set_sync_debug_mode("default")


@functools.lru_cache(maxsize=None)
def _descriptors():
    """Per point id a descriptor for the frames up to the broken pair and one for the frames after it: equal for the kept points,
    unrelated for the others, so the matcher finds the kept points alone across the broken pair."""
    seq = R.broken_sequence()
    n = seq["pts"][0].shape[0]
    rng = np.random.RandomState(77)
    a, b = rng.randn(n, 256), rng.randn(n, 256)
    b[:seq["kept"]] = a[:seq["kept"]]
    return tuple((d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32) for d in (a, b))


def _frame(f, dev):
    seq = R.broken_sequence()
    desc = _descriptors()[0 if f <= R.BROKEN[1] else 1][seq["ids"][f]]
    xy = seq["pts"][f]
    return _t(xy, dev), torch.tensor([xy.shape[0]], dtype=torch.int32, device=dev), _t(desc, dev)


@pytest.mark.parametrize("through", ("PointTracker", "SequenceTracker"))
def test_trackers_observe_and_repair_the_broken_sequence(through):
    from semantic_superpoint_amd import lib
    from semantic_superpoint_amd.export import PointTracker, SequenceTracker
    dev = _dev()
    seq = R.broken_sequence()
    frames, seed0 = len(seq["pts"]), P.case(R.BROKEN[0])["seeds"][0] - 1
    intr = tuple(seq["intr"][0])
    kw = dict(geometric_check="fundamental", check_seed=seed0, intrinsics=intr, trajectory_rows=frames + 1)

    def make(**more):
        if through == "PointTracker":
            top = PointTracker(MAX_LENGTH, NN_THRESH, dev, **kw, **more)
            return top, top
        top = SequenceTracker(None, dev, 0.015, 4, False, NN_THRESH, MAX_LENGTH, **kw, **more)   # fed through its tracker: no network
        return top, top.tracker

    (plain_top, plain), (obs_top, obs), (rep_top, rep) = make(), make(absolute_pose="observe"), make(absolute_pose="repair")
    assert plain_top.absolute_trajectory() is None and obs_top.absolute_trajectory() is None
    k1 = _t(seq["intr"][:1], dev)
    for f in range(frames):
        kept = {}
        for nm, tr in (("observe", obs), ("repair", rep)):               # the landmarks each tracker holds before the frame
            kept[nm] = (tr._abs_lm["landmarks"].clone(), tr._abs_lm["n_landmarks"].clone()) if tr._abs_have else None
        frame = _frame(f, dev)
        plain.update_device(*frame)
        if f >= 2:                                                       # (the first frames allocate)
            with _no_host_sync():
                obs.update_device(*frame)
                rep.update_device(*frame)
        else:
            obs.update_device(*frame)
            rep.update_device(*frame)
        gp, go, gr = plain.last_geometry(), obs.last_geometry(), rep.last_geometry()
        assert set(gp) == OLD_KEYS and set(go) == set(gr) == OLD_KEYS | ABS_KEYS
        # observing changes nothing the plain tracker computes
        for k in OLD_KEYS:
            assert torch.equal(gp[k], go[k]), (f, k)
        assert torch.equal(plain.trajectory()[0], obs.trajectory()[0]) and torch.equal(plain.trajectory()[1], obs.trajectory()[1])
        assert np.array_equal(plain.get_tracks(1), obs.get_tracks(1)) and np.array_equal(plain.get_tracks(1), rep.get_tracks(1))
        if f >= 1:
            a, b = plain_top.landmarks_device(), obs_top.landmarks_device()
            assert torch.equal(a[1], b[1]) and torch.equal(a[0][:int(a[1])], b[0][:int(b[1])])
            if obs._abs_have:                                            # asking for landmarks does not disturb the kept ones
                mine = obs._abs_lm["landmarks"].clone()
                obs_top.landmarks_device(min_views=3)
                assert torch.equal(mine, obs._abs_lm["landmarks"])
        # the absolute pose through the operators, bit for bit
        for nm, tr, g in (("observe", obs, go), ("repair", rep, gr)):
            _, m, n_m = tr._pose_prev                                     # the unfiltered matches of the frame
            slot = f % MAX_LENGTH
            if kept[nm] is None:
                assert int(g["abs_status"]) == 1 and int(g["abs_winner"]) == -1 and not g["abs_mask"].any() and f < 2
                assert torch.equal(g["abs_Rw"][0], torch.eye(3, dtype=torch.float64, device=dev)) and g["abs_n_corr"].tolist() == [0, 0]
                continue
            corr, n = lib.op_landmark_matches(kept[nm][0], kept[nm][1], m[0], n_m, tr._pts[slot])
            want = lib.op_pnp_ransac(corr[None], n[0:1], k1, torch.tensor([seed0 + f], dtype=torch.int64, device=dev))
            assert torch.equal(g["abs_corr"], corr) and torch.equal(g["abs_n_corr"], n), (nm, f)
            for k in want:
                assert torch.equal(g["abs_" + k], want[k]), (nm, f, k)
            if nm == "repair":                                           # the repaired row and state are the absolute pose's
                row = tr.trajectory()[0][f]
                flags = int(row[14])
                assert (flags & lib.POSE_FLAG_ABSOLUTE) == (lib.POSE_FLAG_ABSOLUTE if (f >= 3 and int(want["status"]) == 0) else 0), f
                if flags & lib.POSE_FLAG_ABSOLUTE:
                    assert torch.equal(row[0:9], want["Rw"].reshape(9)) and torch.equal(row[9:12], want["C"].reshape(3))
                    assert torch.equal(tr._traj_state[2:11], want["Rw"].reshape(9)) and float(tr._traj_state[1]) == float(row[12])
            table, nf = (obs_top if nm == "observe" else rep_top).absolute_trajectory()
            assert float(nf) == f + 1
            r = table[f]
            assert torch.equal(r[0:9], want["Rw"].reshape(9)) and torch.equal(r[9:12], want["C"].reshape(3))
            assert [float(r[12]), float(r[13]), float(r[14]), float(r[15])] == [float(want["n_inliers"]), float(want["rms"]),
                                                                               float(want["status"]), float(n[1])]
    # the broken pair: no two-view pose, an absolute one from the kept points; the repaired chain is one window and the truth
    flags_plain, flags_rep = plain.trajectory()[0][:frames, 14].tolist(), rep.trajectory()[0][:frames, 14].tolist()
    assert flags_plain == [3, 2, 0, 3, 2] and flags_rep == [3, 2, 0, 4, 4]
    assert obs_top.absolute_trajectory()[0][:frames, 14].tolist() == [1, 1, 0, 0, 1]
    assert rep_top.absolute_trajectory()[0][:frames, 14].tolist() == [1, 1, 0, 0, 0]
    assert rep_top.absolute_trajectory()[0][3:frames, 15].tolist() == [R.BROKEN[2]] * 2
    cams_plain = lib.op_map_window(plain._traj_state, plain.trajectory()[0], k1, MAX_LENGTH, n_frames=frames).cpu().numpy()
    cams_rep = lib.op_map_window(rep._traj_state, rep.trajectory()[0], k1, MAX_LENGTH, n_frames=frames).cpu().numpy()
    assert cams_plain[:, 16].tolist() == [0, 0, 0, 1, 1] and cams_rep[:, 16].tolist() == [1, 1, 1, 1, 1]
    table = rep.trajectory()[0][:frames].cpu().numpy()
    err, err_plain = R.sequence_centre_error(seq, table), R.sequence_centre_error(seq, plain.trajectory()[0][:frames].cpu().numpy())
    print("%s: repaired centres against the truth %.3e first baselines (the restatement's %.3e, bound %.3e); unrepaired %.3e"
          % (through, err, R.SEQUENCE_CENTRE_ERROR, R.SEQUENCE_CENTRE_BOUND, err_plain))
    assert err <= R.SEQUENCE_CENTRE_BOUND and err_plain > 0.1
    lm = rep_top.landmarks()                                             # the map survives the broken pair
    assert (lm[:, 4] == frames).sum() == R.BROKEN[2] and plain_top.landmarks()[:, 4].max() == 2


def test_trackers_refuse_what_cannot_give_an_absolute_pose():
    from semantic_superpoint_amd.export import PointTracker, SequenceTracker
    dev = _dev()
    a, b = (300.0, 300.0, 160.0, 120.0), (310.0, 300.0, 160.0, 120.0)
    for make in (lambda **kw: PointTracker(3, NN_THRESH, dev, **kw), lambda **kw: SequenceTracker(None, dev, 0.015, 4, False, NN_THRESH, 3, **kw)):
        for kw in (dict(), dict(geometric_check="fundamental"), dict(geometric_check="homography"),
                   dict(geometric_check="fundamental", intrinsics=(a, b)),
                   dict(geometric_check="fundamental", intrinsics=a, absolute_min_inliers=3),
                   dict(geometric_check="fundamental", intrinsics=a, absolute_thresh=-1.0),
                   dict(geometric_check="fundamental", intrinsics=a, landmark_params=(1, 1.0, 2.0))):
            with pytest.raises(ValueError):
                make(absolute_pose="observe", **kw)
        with pytest.raises(ValueError):
            make(geometric_check="fundamental", intrinsics=a, absolute_pose="always")
        t = make(geometric_check="fundamental", intrinsics=(a, a), absolute_pose="repair")
        assert t.absolute_trajectory() is None
