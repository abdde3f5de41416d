"""GPU: the track operators on generated sequences, exactly (cases: tests/tracks_cases.py, shown to be what
they claim by tests/test_tracks_cases_cpu.py; oracle: tests/tracks_ref.py behind the capacities restated in tracks_cases).

Every comparison is an equality: the state vector, ids, tid and the fp64 scores over the first n_rows rows, op_track_select for
min_length in (0, 1, 2, L, L + 1) after every frame, op_track_points for every first_slot (NaN included) after the last.  The same
sequences at point_cap = 4096, without `out=` and into tables that still hold an older, longer table give the same rows.  One
PointTracker is fed frames of 900, 1100, 2100, 1000 and 2100 points through the host entry, so that its buffers grow twice, beside
a twin that had the capacity 4096 from the first frame."""
import numpy as np
import pytest
import torch

from tests import tracks_cases as TC
from tests import tracks_ref as TR

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _i32(v, dev):
    return torch.tensor([v], dtype=torch.int32, device=dev)


def _update(lib, table, la, dev, score64=True, out=None):
    return lib.op_track_update(table, _t(la["rows"], dev), _i32(la["n_match"], dev), _i32(la["n_points"], dev),
                               match_score64=_t(la["s64"], dev) if score64 else None, out=out)


def _same(lib, table, want, what):
    """The device table equals the tracks_ref.Tracks `want`: state, rows, and every selection."""
    state = table["state"].cpu().numpy()
    assert np.array_equal(state, TC.state_of(want)), (what, state, TC.state_of(want))
    n = int(state[0])
    assert np.array_equal(table["ids"][:n].cpu().numpy(), want.ids), what
    assert np.array_equal(table["tid"][:n].cpu().numpy(), want.tid), what
    score = table["score"][:n].cpu().numpy()
    assert score.tobytes() == want.score.tobytes(), (what, int((score != want.score).sum()))
    for q in TC.min_lengths(want.L):
        sel = lib.tracks_to_numpy(*lib.op_track_select(table, q))
        ref = TC.select(want, q)
        assert sel.shape == ref.shape and sel.tobytes() == ref.tobytes(), (what, q)


def _run_case(name, dev, point_cap=None, decoys=False, score64=True, reuse=True):
    """The case's launches against its expected tables, frame by frame.  reuse: two tables take turns as `out=` (as in PointTracker),
    so every output array still holds the table of two frames before; returns how often that table was the longer one."""
    from semantic_superpoint_amd import lib
    c = TC.CASES[name]
    cap = c["point_cap"] if point_cap is None else point_cap
    table = lib.track_table(c["L"], cap, dev)
    spare = lib.track_table(c["L"], cap, dev) if reuse else None
    wants = TC.expected(name, decoys=decoys, score64=score64)
    stale_longer, rows = 0, [0, 0]
    for f, (la, want) in enumerate(zip(TC.launches(name, point_cap=cap, decoys=decoys), wants)):
        out = _update(lib, table, la, dev, score64, out=spare)
        if reuse:
            table, spare = out, table
            stale_longer += rows[0] > want.ids.shape[0]
            rows = [rows[1], want.ids.shape[0]]
        else:
            table = out
        _same(lib, table, want, (name, cap, f))
    return table, stale_longer


@pytest.mark.parametrize("name", ["blocks", "full2", "full3", "long", "short"])
def test_case_against_the_restatement(name):
    _, stale_longer = _run_case(name, _dev())
    assert stale_longer >= 1 or name == "short"     # an output table that still held an older, longer table ("short" only grows)


@pytest.mark.parametrize("score64", [True, False])
def test_decoys_and_clamped_counts(score64):
    """Valid-looking matches past n_match, matches outside their frames before it, both counts above the capacity and below zero;
    once with match_score64 and once with the float32 column, whose scores are other numbers."""
    _run_case("decoys", _dev(), decoys=True, score64=score64)


@pytest.mark.parametrize("name", ["blocks", "long"])
def test_rows_do_not_depend_on_point_cap_or_repetition(name):
    """At point_cap = 4096 (another block layout: more old blocks, four blocks of new points) and into fresh arrays: the same expected
    tables, hence the same bits as the run at the case's own capacity."""
    _run_case(name, _dev(), point_cap=4096, reuse=False)
    if name == "blocks":
        _run_case(name, _dev(), reuse=False)


def _device_table(lib, t, point_cap, dev, state=None):
    """tracks_ref.Tracks -> a device table; the rows past n_rows look alive (id 0): a kernel that read them would keep them."""
    tab = lib.track_table(t.L, point_cap, dev)
    n = t.ids.shape[0]
    tab["ids"].zero_()
    tab["tid"].fill_(-9)
    tab["score"].fill_(0.5)
    tab["ids"][:n] = _t(t.ids.astype(np.int32), dev)
    tab["tid"][:n] = _t(t.tid.astype(np.int32), dev)
    tab["score"][:n] = _t(t.score, dev)
    tab["state"].copy_(_t(TC.state_of(t) if state is None else state, dev))
    return tab


def test_hand_made_tables_overflow_and_clamp():
    from semantic_superpoint_amd import lib
    dev = _dev()
    t, state, la, cap, row_cap = TC.overfull()
    tab = _device_table(lib, t, cap, dev, state)
    TC.clamped_update(t, la["rows"], la["s64"], la["n_match"], la["n_points"], cap, row_cap)
    _same(lib, _update(lib, tab, la, dev), t, "overfull")
    held, empty, state, la, cap, row_cap = TC.negative_state()
    tab = _device_table(lib, held, cap, dev, state)
    TC.clamped_update(empty, la["rows"], la["s64"], la["n_match"], la["n_points"], cap, row_cap)
    _same(lib, _update(lib, tab, la, dev), empty, "negative state")


@pytest.mark.parametrize("name", ["blocks", "full2", "long", "short"])
def test_track_points_every_first_slot(name):
    from semantic_superpoint_amd import lib
    dev = _dev()
    c = TC.CASES[name]
    t = TC.expected(name)[-1]
    cap, L = c["point_cap"], c["L"]
    state = _t(TC.state_of(t), dev)
    plain = t.matrix()
    edited, edits = TC.edited_tracks(t)
    for first in range(L):
        ring = TC.ring(name, first)
        for m in (plain, edited):
            track_cap = m.shape[0] + 3                                          # rows past n_tracks name point 0: never read
            rows = np.zeros((track_cap, 2 + L))
            rows[:m.shape[0]] = m
            xy = lib.op_track_points(_t(rows, dev), _i32(m.shape[0], dev), _t(ring, dev), state, first)[:m.shape[0]].cpu().numpy()
            want = TC.track_points_expected(m, ring, t.counts, first, cap)
            assert np.array_equal(np.isnan(xy), np.isnan(want)) and np.array_equal(xy, want, equal_nan=True), (name, first)
            if m is plain:
                assert np.array_equal(np.isnan(xy[:, :, 0]), m[:, 2:] == -1)
            else:
                assert all(np.isnan(xy[r, col]).all() for r, col in edits)
    # a count above the capacity in the state vector, a negative count, n_tracks above track_cap
    bad = TC.state_of(t)
    bad[2] = cap + 11
    bad[2 + L - 1] = -4
    rows = np.ascontiguousarray(plain[:64])
    xy = lib.op_track_points(_t(rows, dev), _i32(64 + 9, dev), _t(ring, dev), _t(bad, dev), first).cpu().numpy()
    assert np.array_equal(xy, TC.track_points_expected(rows, ring, bad[2:], first, cap), equal_nan=True)


# ---- one PointTracker through the host entry: its buffers grow twice --------------------------------------------------------------
GROW_COUNTS, GROW_KEEP, GROW_L, GROW_NN = (900, 1100, 2100, 1000, 2100), (0, 0.6, 0.6, 0.6, 0.6), 3, 0.7


def _growing_frames():
    """[(pts [3, N], desc [256, N], src [N])]: seeded unit descriptors, equal for a continuing point and its predecessor and unrelated
    otherwise (as tests/test_gpu_pnp.py::_descriptors builds them), so the matcher finds exactly the continuing points."""
    rs = np.random.RandomState(4107)
    frames, prev_pts, prev_desc = [], np.zeros((3, 0)), np.zeros((0, 256), np.float32)
    for n, keep in zip(GROW_COUNTS, GROW_KEEP):
        k = min(int(round(keep * prev_desc.shape[0])), n)
        src = np.full(n, -1, np.int64)
        src[rs.permutation(n)[:k]] = rs.permutation(prev_desc.shape[0])[:k]
        d = rs.randn(n, 256)
        desc = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
        desc[src >= 0] = prev_desc[src[src >= 0]]
        pts = np.stack([np.round(rs.uniform(4, 636, n) * 8) / 8, np.round(rs.uniform(4, 476, n) * 8) / 8, rs.uniform(0.015, 1.0, n)])
        frames.append((pts, np.ascontiguousarray(desc.T), src))
        prev_pts, prev_desc = pts, desc
    return frames


def test_point_tracker_grows_twice_and_keeps_its_table():
    from semantic_superpoint_amd.export import PointTracker
    dev = _dev()
    host, twin = PointTracker(GROW_L, GROW_NN, dev), PointTracker(GROW_L, GROW_NN, dev)
    ids_ref, all_ref = TR.Tracks(GROW_L), TR.Tracks(GROW_L)
    caps, prev_pts = [], None
    for f, (pts, desc, src) in enumerate(_growing_frames()):
        n = pts.shape[1]
        host.update(pts, desc)
        caps.append(host._cap)
        p, d = torch.zeros(4096, 2, dtype=torch.float64), torch.zeros(4096, 256)
        p[:n], d[:n] = torch.from_numpy(pts[:2].T.copy()), torch.from_numpy(desc.T.copy())
        p[n:], d[n:] = p[0], d[0]                                                 # the padding is a copy of the first point
        twin.update_device(p.to(dev), _i32(n, dev), d.to(dev))
        assert twin._cap == 4096
        j = np.flatnonzero(src >= 0)
        j = j[np.argsort(src[j])]                                                 # the matcher's order: ascending i
        true = np.stack([src[j].astype(np.float64), j.astype(np.float64), np.zeros(len(j))])
        TR.update(ids_ref, n, true)
        got = host.tracks
        want = ids_ref.matrix()
        assert got.shape == want.shape and np.array_equal(got[:, 0], want[:, 0]) and np.array_equal(got[:, 2:], want[:, 2:]), f
        assert host.track_count == ids_ref.track_count
        gm = host.get_matches()
        if f:
            assert np.array_equal(gm, np.concatenate([prev_pts[:2, src[j]], pts[:2, j]], axis=0)), f
            own = host.get_mscores()                                              # the device's own match rows
            assert np.array_equal(own[:2], true[:2]), f
        else:
            own = np.zeros((3, 0))
            assert gm.shape[1] == 0
        TR.update(all_ref, n, own)
        assert got.tobytes() == all_ref.matrix().tobytes(), f                     # the scores too, bit for bit
        for q in (1, 2, GROW_L):
            a, b = host.get_tracks(q), TR.get_tracks(all_ref, q)
            assert a.shape == b.shape and a.tobytes() == b.tobytes(), (f, q)
        a, b = host.table, twin.table
        rows = int(a["state"][0].item())
        assert torch.equal(a["state"], b["state"]), f
        for k in ("ids", "tid", "score"):
            assert torch.equal(a[k][:rows], b[k][:rows]), (f, k)
        assert np.array_equal(twin.get_matches(), gm), f
        tr = host.get_tracks(1)
        assert np.array_equal(host.track_points(tr), TR.track_points(tr, host.all_pts), equal_nan=True), f
        assert np.array_equal(twin.track_points(tr), host.track_points(tr), equal_nan=True), f
        prev_pts = pts
    assert caps == [1024, 2048, 4096, 4096, 4096]
