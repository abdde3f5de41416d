"""Landmarks from tracks on the device: ssp_map_window, ssp_op_triangulate_tracks and
ssp_op_landmarks_select against their numpy restatement (tests/landmarks_ref.py), their independence of row_cap and repetition,
and the landmarks of PointTracker / SequenceTracker against the operators and the truth.

status, n_views, track ids, newest-frame indices, n_landmarks and the row order are compared for equality; the camera records are
copies and compared for equality too.  Tolerance of X, rms and cos_parallax (landmarks_ref.TOLERANCE = 9.4e-11, relative to
max(1, |value|)): measured, not chosen - 16 times the largest difference between the restatement in float64 and in
numpy.longdouble over the compared fixtures (5.86e-12, a stray track); tests/test_landmarks_cpu.py repeats the measurement.  Every
comparison prints what the device showed before it asserts."""
import contextlib
import functools

import numpy as np
import pytest
import torch

from tests import landmarks_ref as R
from tests import pose_ref as P

pytestmark = pytest.mark.gpu

JUNK = 7          # an id (a valid point of the oldest frame) in the table rows past n_rows: they must not be read into results
SENTINEL = -77    # what the output arrays hold before a call: rows at or past n_rows must keep it


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _table(fx, row_cap, dev, n_rows=None):
    """The device track table of a fixture in arrays of row_cap rows."""
    n, L = fx["ids"].shape
    ids = np.full((row_cap, L), JUNK, dtype=np.int32)
    tid = np.full(row_cap, -5, dtype=np.int32)
    ids[:n], tid[:n] = fx["ids"], fx["tid"]
    state = np.array([n if n_rows is None else n_rows, fx["tracks"].track_count] + list(fx["counts"]), dtype=np.int32)
    return {"ids": _t(ids, dev), "tid": _t(tid, dev), "score": torch.zeros(row_cap, dtype=torch.float64, device=dev),
            "state": _t(state, dev), "L": L, "point_cap": fx["point_cap"], "row_cap": row_cap}


def _buffers(L, row_cap, dev):
    from semantic_superpoint_amd import lib
    out = lib.landmark_buffers(L, row_cap, dev)
    for k in lib.LANDMARK_ROW_KEYS + ("landmarks", "n_landmarks"):
        out[k].fill_(SENTINEL)
    return out


def _run(fx, cams, row_cap=None, n_rows=None, **kw):
    """(rows, landmarks [M, 8], raw device outputs as numpy) of one call of the two operators over a fixture's table."""
    from semantic_superpoint_amd import lib
    dev = _dev()
    row_cap = fx["ids"].shape[0] if row_cap is None else row_cap
    table = _table(fx, row_cap, dev, n_rows)
    out = _buffers(fx["L"], row_cap, dev)
    cams = cams if torch.is_tensor(cams) else _t(cams, dev)
    rows = lib.op_triangulate_tracks(table, _t(fx["pts"], dev), fx["first_slot"], cams, out=out, **kw)
    lm, n_lm = lib.op_landmarks_select(table, rows, out=out)
    torch.cuda.synchronize()
    raw = {k: out[k].cpu().numpy() for k in lib.LANDMARK_ROW_KEYS + ("landmarks", "n_landmarks")}
    n = fx["ids"].shape[0] if n_rows is None else n_rows
    for k in lib.LANDMARK_ROW_KEYS:
        assert (raw[k][n:] == SENTINEL).all(), k                        # rows at or past n_rows are not written
    m = int(raw["n_landmarks"][0])
    assert (raw["landmarks"][m:] == SENTINEL).all()
    return {k: raw[k][:n] for k in lib.LANDMARK_ROW_KEYS}, raw["landmarks"][:m], raw


def _compare(got, ref, what):
    worst = 0.0
    for k in ("X", "rms", "cos_parallax"):
        if ref[k].size:
            worst = max(worst, float((np.abs(got[k] - ref[k]) / np.maximum(1.0, np.abs(ref[k]))).max()))
    bits = all(np.array_equal(got[k], ref[k]) for k in ("X", "rms", "cos_parallax"))
    print("%s: %d rows, status counts %s, worst difference %.3e (tolerance %.3e)%s"
          % (what, ref["status"].size, np.bincount(got["status"], minlength=5).tolist(), worst, R.TOLERANCE, ", bit-equal" if bits else ""))
    assert np.array_equal(got["status"], ref["status"]) and np.array_equal(got["n_views"], ref["n_views"]), what
    assert worst <= R.TOLERANCE, (what, worst)


def _compare_landmarks(lm, fx, got_rows, ref_rows, what, counts=None):
    ref = R.select(fx["ids"], fx["tid"], fx["counts"] if counts is None else counts, fx["point_cap"], ref_rows)
    assert lm.shape == ref.shape, what
    assert np.array_equal(lm[:, [0, 4, 7]], ref[:, [0, 4, 7]]), what                      # track id, n_views, newest index, the order
    keep = got_rows["status"] == R.OK                                                     # and the continuous columns are the rows' own
    assert np.array_equal(lm[:, 1:4], got_rows["X"][keep]) and np.array_equal(lm[:, 5], got_rows["rms"][keep])
    assert np.array_equal(lm[:, 6], got_rows["cos_parallax"][keep])


@pytest.mark.parametrize("name", R.COMPARED)
def test_rows_and_landmarks_under_the_true_cameras(name):
    fx = R.fixture(name)
    if name == "mixed48":
        assert fx["L"] == 2 and fx["point_cap"] == 64 and fx["counts"] == [48, 48]
    if name == "big":
        assert fx["ids"].shape[0] > 2048 and fx["L"] == 5                                # tiles and compaction cross workgroups
    if name == "long16":
        assert fx["L"] == 16 and fx["frames"] == 16
    if name in ("seq5_late", "long16", "big"):
        assert (fx["ids"][:, 0] == -1).any() and (fx["ids"][:, -1] == -1).any()           # tracks that start late, tracks that ended
    if name == "seq5":
        assert not np.array_equal(fx["cams"][0, 12:16], fx["cams"][1, 12:16])             # per-frame intrinsics
    rows, lm, _ = _run(fx, fx["cams"])
    _compare(rows, fx["rows"], name)
    _compare_landmarks(lm, fx, rows, fx["rows"], name)
    if fx["seq"]["noise"] == 0.0:
        err = R.truth_error(name, rows)
        print("%s: |X - scene point| at most %.3e (the restatement %.3e, bound %.3e)" % (name, err, R.truth_error(name), R.TRUTH_BOUND))
        assert err <= R.TRUTH_BOUND


def _chain_on_device(name, dev):
    """(state, table) on the device of a window scenario, as op_pose_chain leaves them: the state's count stops at the capacity."""
    from semantic_superpoint_amd import lib
    _, n, table = R.scenario_inputs(name)
    state = lib.pose_state(dev)
    state[0] = min(n, table.shape[0])
    return state, _t(table, dev), n


@pytest.mark.parametrize("scenario", R.WINDOW_SCENARIOS)
def test_window_scenarios_through_map_window(scenario):
    from semantic_superpoint_amd import lib
    dev = _dev()
    fx, n, table = R.scenario_inputs(scenario)
    L = fx["L"]
    state, table_d, n = _chain_on_device(scenario, dev)
    intr1 = fx["seq"]["intr"][:1]
    want = R.map_window(n, table, intr1, L)
    assert tuple(int(v) for v in want[:, 16]) == R.window_scenario(scenario)[2]
    full = scenario == "full"                                              # the caller's own frame count; else the state's
    cams = lib.op_map_window(state, table_d, _t(intr1, dev), L, n_frames=n if full else None)
    per_frame = lib.op_map_window(state, table_d, _t(np.repeat(intr1, L, axis=0), dev), L, n_frames=n)
    assert np.array_equal(cams.cpu().numpy(), want) and torch.equal(per_frame, cams)  # copies: exactly
    if full:                                                               # the state alone cannot know that frames were lost
        stale = lib.op_map_window(state, table_d, _t(intr1, dev), L).cpu().numpy()
        assert np.array_equal(stale, R.map_window(3, table, intr1, L))
    rows, lm, _ = _run(fx, cams, row_cap=320)
    ref = R.scenario_rows(scenario)
    _compare(rows, ref, scenario)
    _compare_landmarks(lm, fx, rows, ref, scenario)
    if full:
        assert (rows["status"] == R.FEW_VIEWS).all() and lm.shape[0] == 0
        return
    err = R.chain_truth_error(rows, scenario)
    print("%s: |X - scene point| at most %.3e first baselines (restatement %.3e)" % (scenario, err, R.chain_truth_error(None, scenario)))
    if scenario == "plain":
        assert err <= R.CHAIN_TRUTH_BOUND
    # per-frame intrinsics with a frame that is no camera: that view is dropped
    intr = np.repeat(intr1, L, axis=0)
    intr[L - 2, 0] = -1.0
    cams2 = lib.op_map_window(state, table_d, _t(intr, dev), L, n_frames=n)
    want2 = R.map_window(n, table, intr, L)
    assert np.array_equal(cams2.cpu().numpy(), want2) and want2[L - 2, 16] == 0.0
    rows2, _, _ = _run(fx, cams2, row_cap=320)
    _compare(rows2, R.triangulate(fx["ids"], fx["counts"], fx["pts"], fx["first_slot"], want2), scenario + " without a view")


def test_empty_and_full_tables():
    fx = R.fixture("seq3")
    n = fx["ids"].shape[0]
    rows, lm, raw = _run(fx, fx["cams"], row_cap=n, n_rows=0)              # n_rows == 0: nothing is written but the count
    assert lm.shape[0] == 0 and int(raw["n_landmarks"][0]) == 0
    rows, lm, _ = _run(fx, fx["cams"], row_cap=n)                          # n_rows == row_cap
    _compare(rows, fx["rows"], "seq3 in a table of exactly its rows")
    _compare_landmarks(lm, fx, rows, fx["rows"], "seq3")
    big = R.fixture("big")
    n = big["ids"].shape[0]
    rows, lm, _ = _run(big, big["cams"], row_cap=n, n_rows=n - 300)        # a count inside the table: the rows behind it are not used
    part = {k: v[:n - 300] for k, v in big["rows"].items()}
    _compare(rows, part, "big, the first %d rows" % (n - 300))
    cut = dict(big, ids=big["ids"][:n - 300], tid=big["tid"][:n - 300])
    _compare_landmarks(lm, cut, rows, part, "big cut")


@pytest.mark.parametrize("name", ("seq5_late", "big"))
def test_repeated_call_and_larger_row_cap_are_bit_identical(name):
    fx = R.fixture(name)
    n = fx["ids"].shape[0]
    a_rows, a_lm, _ = _run(fx, fx["cams"], row_cap=n)
    b_rows, b_lm, _ = _run(fx, fx["cams"], row_cap=n)
    c_rows, c_lm, _ = _run(fx, fx["cams"], row_cap=2 * n + 391)            # other tiles, other blocks of the compaction
    for k in a_rows:
        assert np.array_equal(a_rows[k], b_rows[k]) and np.array_equal(a_rows[k], c_rows[k]), k
    assert np.array_equal(a_lm, b_lm) and np.array_equal(a_lm, c_lm)


def test_thresholds_and_min_views():
    fx = R.fixture("seq5_late")
    args = (fx["ids"], fx["counts"], fx["pts"], fx["first_slot"], fx["cams"])
    for kw, ref_kw in ((dict(min_views=4), dict(min_views=4)), (dict(min_views=6), dict(min_views=6)),
                       (dict(min_parallax_deg=150.0), dict(cos_min_parallax=R.cos_of(150.0))),
                       (dict(max_reproj=0.0), dict(max_reproj=0.0)), (dict(min_parallax_deg=7.5, max_reproj=1e-14), dict(
                           cos_min_parallax=R.cos_of(7.5), max_reproj=1e-14))):
        rows, lm, _ = _run(fx, fx["cams"], **kw)
        ref = R.triangulate(*args, **ref_kw)
        _compare(rows, ref, "seq5_late %s" % kw)
        _compare_landmarks(lm, fx, rows, ref, str(kw))
    for name in ("forward", "backward"):                                   # the low-parallax fixtures: status 2, values still written
        fx = R.fixture(name)
        rows, _, _ = _run(fx, fx["cams"])
        _compare(rows, fx["rows"], name)
        deg = rows["status"] == R.DEGENERATE
        assert deg.sum() >= 20 and rows["X"][deg].any(axis=1).all() and (rows["cos_parallax"][deg] > R.cos_of(1.0)).all()


def test_wrappers_validate_their_arguments():
    from semantic_superpoint_amd import lib
    dev = _dev()
    fx = R.fixture("seq3")
    table, pts, cams = _table(fx, 64, dev), _t(fx["pts"], dev), _t(fx["cams"], dev)
    with pytest.raises(ValueError):
        lib.op_triangulate_tracks(table, pts, 0, cams, min_views=1)
    with pytest.raises(ValueError):
        lib.op_triangulate_tracks(table, pts, 3, cams)
    with pytest.raises(ValueError):
        lib.op_triangulate_tracks(table, pts.to(torch.float32), 0, cams)
    with pytest.raises(ValueError):
        lib.op_triangulate_tracks(table, pts, 0, cams[:2])
    with pytest.raises(ValueError):
        lib.op_triangulate_tracks(table, pts, 0, cams, max_reproj=-1.0)
    with pytest.raises(RuntimeError):
        lib.op_triangulate_tracks(table, pts.cpu(), 0, cams)
    state, tab = lib.pose_state(dev), lib.pose_table(4, dev)
    with pytest.raises(ValueError):
        lib.op_map_window(state, tab, torch.ones(2, 4, dtype=torch.float64, device=dev), 3)
    with pytest.raises(ValueError):
        lib.op_map_window(state, tab, torch.ones(1, 4, dtype=torch.float64, device=dev), 17)
    with pytest.raises(ValueError):
        lib.op_map_window(state[:8], tab, torch.ones(1, 4, dtype=torch.float64, device=dev), 3)
    rows = lib.op_triangulate_tracks(table, pts, 0, cams)
    with pytest.raises(ValueError):
        lib.op_landmarks_select(table, {k: v for k, v in rows.items() if k != "rms"})
    with pytest.raises(ValueError):
        lib.op_landmarks_select(_table(fx, 128, dev), rows)


# ---- the trackers --------------------------------------------------------------------------------------------------------------
NN_THRESH, MAX_LENGTH = 0.7, 5


@contextlib.contextmanager
def _no_host_sync():
    torch.cuda.set_sync_debug_mode("error")
    try:
        yield
    finally:
        torch.cuda.set_sync_debug_mode("default")


@functools.lru_cache(maxsize=None)
def _descriptors():
    n = P.case("seq5_k")["seq"]["pts"][0].shape[0]
    d = np.random.RandomState(77).randn(n, 256)
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def _frame(f, dev):
    seq = P.case("seq5_k")["seq"]
    xy, desc = seq["pts"][f], _descriptors()[seq["ids"][f]]
    return _t(xy, dev), torch.tensor([xy.shape[0]], dtype=torch.int32, device=dev), _t(desc, dev)


def _snapshot(tr):
    g = {k: v.clone() for k, v in tr.last_geometry().items()}
    return g, tr.trajectory()[0].clone(), tr.trajectory()[1].clone(), tr.get_tracks(1)


@pytest.mark.parametrize("through", ("PointTracker", "SequenceTracker"))
def test_trackers_against_the_operators_and_the_truth(through):
    from semantic_superpoint_amd import lib
    from semantic_superpoint_amd.export import PointTracker, SequenceTracker
    dev = _dev()
    c = P.case("seq5_k")
    seq = c["seq"]
    frames, seed0 = len(seq["pts"]), c["seeds"][0] - 1
    intr = tuple(seq["intr"][0])
    kw = dict(geometric_check="fundamental", check_seed=seed0, intrinsics=intr, trajectory_rows=frames + 1)
    if through == "PointTracker":
        top = tr = PointTracker(MAX_LENGTH, NN_THRESH, dev, **kw)
    else:
        top = SequenceTracker(None, dev, 0.015, 4, False, NN_THRESH, MAX_LENGTH, **kw)      # fed through its tracker: no network
        tr = top.tracker
    fx = R.fixture("seq5_k")
    for f in range(frames):
        if f < 2:                                                          # before the second frame: empty results
            lm, n_lm = top.landmarks_device()
            assert lm.shape == (0, lib.LANDMARK_WORDS) and int(n_lm) == 0 and top.landmarks().shape == (0, lib.LANDMARK_WORDS)
            assert all(v.shape[0] == 0 for v in top.landmark_rows_device().values())
        tr.update_device(*_frame(f, dev))
        if f == 0:
            continue
        before = _snapshot(tr)
        top.landmarks_device()                                             # (the first call allocates)
        with _no_host_sync():
            lm, n_lm = top.landmarks_device()
            rows = top.landmark_rows_device()
        after = _snapshot(tr)
        for k in before[0]:
            assert torch.equal(before[0][k], after[0][k]), k              # last_geometry(), trajectory(), get_tracks: unchanged
        assert torch.equal(before[1], after[1]) and torch.equal(before[2], after[2]) and np.array_equal(before[3], after[3])
        # the same through the operators, bit for bit
        cams = lib.op_map_window(tr._traj_state, tr.trajectory()[0], _t(seq["intr"][:1], dev), MAX_LENGTH, n_frames=f + 1)
        want = lib.op_triangulate_tracks(tr.table, tr._pts, (f + 1) % MAX_LENGTH, cams)
        want_lm, want_n = lib.op_landmarks_select(tr.table, want)
        for k in want:
            assert torch.equal(rows[k], want[k]), (f, k)
        assert int(n_lm) == int(want_n) and torch.equal(lm[:int(n_lm)], want_lm[:int(n_lm)])
        assert np.array_equal(top.landmarks(), lm[:int(n_lm)].cpu().numpy())
        assert np.array_equal(top.landmarks(min_views=f + 2), np.zeros((0, lib.LANDMARK_WORDS)))     # more views than frames
    # the tracker's own table (the check removed the strays' matches, so it is not the fixture's) under its own cameras, restated
    import types
    n = int(tr.table["state"][0])
    ids, counts = tr.table["ids"][:n].cpu().numpy(), tr.table["state"][2:].cpu().numpy().tolist()
    got = {k: v[:n].cpu().numpy() for k, v in top.landmark_rows_device().items()}     # (the buffers are the tracker's: read anew)
    ref = R.triangulate(ids, counts, tr._pts.cpu().numpy(), frames % MAX_LENGTH, cams.cpu().numpy())
    _compare(got, ref, through)
    point, _ = R.row_points(seq, types.SimpleNamespace(ids=ids, counts=counts), MAX_LENGTH, frames)
    full = (point >= 0) & (got["n_views"] == frames)
    assert full.sum() == seq["n_in"] and (got["status"][full] == R.OK).all() and (got["status"][point < 0] != R.OK).all()
    lmn = top.landmarks()
    keep = got["status"] == R.OK
    assert np.array_equal(lmn[:, 0], tr.table["tid"][:n].cpu().numpy()[keep]) and np.array_equal(lmn[:, 1:4], got["X"][keep])
    assert np.array_equal(lmn[:, 7], np.where(ids[keep, -1] >= 0, ids[keep, -1] - sum(counts[:-1]), -1))
    # against the truth, up to the global scale: the unit of the trajectory is the first baseline
    err = float(np.abs(got["X"][full] - fx["seq"]["X0"][point[full]] / seq["pairs"][0]["length"]).max())
    print("%s: |X - scene point| at most %.3e first baselines (the restatement's own error under its own chain %.3e, bound %.3e)"
          % (through, err, R.chain_truth_error(), R.CHAIN_TRUTH_BOUND))
    assert err <= R.CHAIN_TRUTH_BOUND


def test_trackers_refuse_what_cannot_give_landmarks():
    from semantic_superpoint_amd.export import PointTracker, SequenceTracker
    dev = _dev()
    a, b = (300.0, 300.0, 160.0, 120.0), (310.0, 300.0, 160.0, 120.0)
    for make in (lambda **kw: PointTracker(3, NN_THRESH, dev, **kw), lambda **kw: SequenceTracker(None, dev, 0.015, 4, False, NN_THRESH, 3, **kw)):
        for kw in (dict(), dict(geometric_check="fundamental"), dict(geometric_check="fundamental", intrinsics=(a, b))):
            t = make(**kw)
            for call in (t.landmarks, t.landmarks_device, t.landmark_rows_device):
                with pytest.raises(ValueError):
                    call()
        same = make(geometric_check="fundamental", intrinsics=(a, a))      # one camera given per view
        assert same.landmarks().shape == (0, 8)
        with pytest.raises(ValueError):
            same.landmarks(min_views=1)


def test_noisy_sequence_against_the_restatement_only():
    fx = R.fixture("noisy5")
    rows, _, _ = _run(fx, fx["cams"], row_cap=300)
    true = fx["point"] >= 0
    assert (rows["status"][true] == R.OK).all() and 0.3 < rows["rms"][true].max() < 0.4
