"""GPU: point tracks over a frame sequence against the real reference (G19 fixture, tools/make_golden_tracks.py).

  1. the operators alone, fed the reference's recorded matches: every table, row count and track count exact, scores ==
  2. PointTracker end to end from points / descriptors (device matcher): ids, row order and get_matches exact, scores within
     the match-score tolerance of tests/test_gpu_descriptor.py; update_device gives the identical table
  3. max_length = 2: get_matches / get_mscores are what the reference (and the two-frame tracker before) returns
  4. track_points equals indexing all_pts by hand, NaN exactly where the id is -1
  5. SequenceTracker.step on four shifted frames equals Val_model_heatmap + host update
  6. two runs of the largest sequence give bit-identical tables
  7. update_device synchronises nothing with the host (torch's sync debug mode set to "error" around the frames), update and
     update_device mix, and a capacity above MATCH_MAX_POINTS is cut, not refused
"""
import contextlib
import functools
import warnings

import numpy as np
import pytest
import torch

from tests import golden_util as G
from tests import tracks_ref as TR
from tests.golden_tracks import GET_TRACKS_M, NN_THRESH, SEQUENCES, fixture_frames
from tests.test_gpu_descriptor import _score_close, _weights_file

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def g19():
    return G.load("g19_tracks.npz")


@functools.lru_cache(maxsize=None)
def _inputs(name):
    return fixture_frames(G.load("g19_tracks.npz"), name)


def _table_numpy(L, table):
    return L.tracks_to_numpy(*L.op_track_select(table, 0))


@pytest.mark.parametrize("name", sorted(SEQUENCES))
def test_operators_on_recorded_matches(g19, name):
    from semantic_superpoint_amd import lib as L
    dev = _dev()
    spec = SEQUENCES[name]
    ml, cap = spec["max_length"], max(spec["counts"])
    table = L.track_table(ml, cap, dev)
    i32 = dict(dtype=torch.int32, device=dev)
    for f, n in enumerate(spec["counts"]):
        key = "%s/%d/" % (name, f)
        m = g19[key + "matches"]
        k = m.shape[1]
        rows = np.zeros((cap, 3), np.float32)
        rows[:k] = m.T
        s64 = np.zeros(cap)
        s64[:k] = m[2]
        table = L.op_track_update(table, torch.from_numpy(rows).to(dev), torch.tensor([k], **i32), torch.tensor([n], **i32),
                                  match_score64=torch.from_numpy(s64).to(dev))
        ref = g19[key + "tracks"]
        state = table["state"].cpu().numpy()
        assert state[0] == ref.shape[0] and state[1] == int(g19[key + "track_count"]), (key, state)
        assert list(state[2:]) == ([0] * ml + list(spec["counts"][:f + 1]))[-ml:]
        got = _table_numpy(L, table)
        assert np.array_equal(got, ref), key          # ids, track ids, row order and the fp64 scores
        for q in GET_TRACKS_M(ml):
            sel = L.tracks_to_numpy(*L.op_track_select(table, q))
            assert np.array_equal(sel, g19[key + "gt%d" % q]), (key, q)


def _same_tables(a, b):
    n = int(a["state"][0].item())
    return (torch.equal(a["state"], b["state"]) and torch.equal(a["ids"][:n], b["ids"][:n])
            and torch.equal(a["tid"][:n], b["tid"][:n]) and torch.equal(a["score"][:n], b["score"][:n]))


@pytest.mark.parametrize("name", ["B", "C"])
def test_point_tracker_end_to_end(g19, name):
    from semantic_superpoint_amd.export import PointTracker
    dev = _dev()
    spec = SEQUENCES[name]
    ml = spec["max_length"]
    host = PointTracker(ml, NN_THRESH, dev)
    devt = PointTracker(ml, NN_THRESH, dev)
    for f, (pts, desc) in enumerate(_inputs(name)):
        key = "%s/%d/" % (name, f)
        if f in spec["clear_before"]:
            host.clear_desc()
            devt.clear_desc()
        host.update(pts, desc)
        n = pts.shape[1]
        cap = max(n, 1) + 3   # rows past the count are ignored
        p = torch.zeros(cap, 2, dtype=torch.float64)
        p[:n] = torch.from_numpy(pts[:2].T.copy())
        d = torch.zeros(cap, 256)
        d[:n] = torch.from_numpy(desc.T.copy())
        devt.update_device(p.to(dev), torch.tensor([n], dtype=torch.int32, device=dev), d.to(dev))
        ref = g19[key + "tracks"]
        got = host.tracks
        assert got.shape == ref.shape and got.dtype == np.float64, key
        assert np.array_equal(got[:, 0], ref[:, 0]) and np.array_equal(got[:, 2:], ref[:, 2:]), key
        assert _score_close(got[:, 1], ref[:, 1]).all(), (key, np.abs(got[:, 1] - ref[:, 1]).max())
        assert host.track_count == int(g19[key + "track_count"])
        assert np.array_equal(host.get_matches(), g19[key + "get_matches"]), key
        for q in GET_TRACKS_M(ml):
            a, b = host.get_tracks(q), g19[key + "gt%d" % q]
            assert a.shape == b.shape and np.array_equal(a[:, 0], b[:, 0]) and np.array_equal(a[:, 2:], b[:, 2:]), (key, q)
        assert _same_tables(host.table, devt.table), key
        assert np.array_equal(devt.get_matches(), host.get_matches()), key
    counts = ([0] * ml + list(spec["counts"]))[-ml:]
    assert np.array_equal(host.get_offsets(), np.concatenate([[0], np.cumsum(counts)[:-1]]))
    for a, b in zip(devt.all_pts, host.all_pts):
        assert np.array_equal(a, b[:2])


def test_two_frame_tracker_keeps_its_results(g19):
    from semantic_superpoint_amd.export import PointTracker
    dev = _dev()
    t = PointTracker(2, NN_THRESH, dev)
    for f, (pts, desc) in enumerate(_inputs("A")):
        key = "A/%d/" % f
        t.update(pts, desc)
        assert np.array_equal(t.get_matches(), g19[key + "get_matches"]), key
        if key + "mscores" in g19:
            ms, ref = t.get_mscores(), g19[key + "mscores"]
            assert ms.shape == ref.shape and np.array_equal(ms[:2], ref[:2]), key
            assert _score_close(ms[2], ref[2]).all(), key
        else:
            assert t.get_mscores() is None
        # and the standalone matcher gives the same answer as update did
        if f:
            prev = _inputs("A")[f - 1][1]
            assert np.array_equal(PointTracker(2, NN_THRESH, dev).nn_match_two_way(prev, desc, NN_THRESH), t.get_mscores())


def test_track_points_equal_indexing_by_hand(g19):
    from semantic_superpoint_amd.export import PointTracker
    dev = _dev()
    ml = SEQUENCES["B"]["max_length"]
    host, devt = PointTracker(ml, NN_THRESH, dev), PointTracker(ml, NN_THRESH, dev)
    checked = 0
    for f, (pts, desc) in enumerate(_inputs("B")):
        if f in SEQUENCES["B"]["clear_before"]:
            host.clear_desc()
            devt.clear_desc()
        host.update(pts, desc)
        devt.update_device(torch.from_numpy(pts[:2].T.copy()).to(dev).reshape(-1, 2),
                           torch.tensor([pts.shape[1]], dtype=torch.int32, device=dev),
                           torch.from_numpy(desc.T.copy()).to(dev).reshape(-1, 256))
        tracks = g19["B/%d/tracks" % f]
        want = TR.track_points(tracks, host.all_pts)
        for t in (host, devt):   # every ring position: the frame number moves the first slot
            got = t.track_points(tracks)
            assert got.shape == (tracks.shape[0], ml, 2) and got.dtype == np.float64
            assert np.array_equal(np.isnan(got[:, :, 0]), tracks[:, 2:] == -1)
            assert np.array_equal(np.isnan(got[:, :, 1]), tracks[:, 2:] == -1)
            assert np.array_equal(got, want, equal_nan=True), f
        checked += int((tracks[:, 2:] != -1).sum())
    assert checked > 100
    sel, n = devt.get_tracks_device(1)
    xy = devt.track_points_device(sel, n)[:int(n.item())].cpu().numpy()
    assert np.array_equal(xy, TR.track_points(g19["B/6/gt1"], host.all_pts), equal_nan=True)


def _agent(tmp_path, dev):
    from semantic_superpoint_amd.Val_model_heatmap import Val_model_heatmap
    g = G.load("g15_descriptor_ssp_120x160.npz")
    arch, seed = str(g["arch"]), int(g["seed"])
    cfg = {"name": arch, "params": {}, "pretrained": _weights_file(tmp_path, arch, seed), "nms": int(g["nms"]),
           "detection_threshold": float(g["conf_thresh"]), "nn_thresh": float(g["nn_thresh"])}
    agent = Val_model_heatmap(cfg, device=dev)
    agent.loadModel()
    return agent


def _shifted_frames():
    big = np.random.RandomState(1900).uniform(0, 1, (64, 96 + 6)).astype(np.float32)
    return [big[:, 2 * k:2 * k + 96].copy() for k in range(4)]   # a fixed image shifted by 2 px per frame


def _same_sequence_result(seq, host, ml):
    assert seq.get_tracks(2).shape[0] > 0 and seq.get_tracks(2).shape[1] == ml + 2
    assert np.array_equal(seq.get_tracks(2), host.get_tracks(2))
    assert np.array_equal(seq.tracker.get_matches(), host.get_matches())
    for a, b in zip(seq.tracker.all_pts, host.all_pts):
        assert np.array_equal(a, b[:2])
    xy = seq.track_points(seq.get_tracks(2))
    assert not np.isnan(xy[:, -2:]).any()


def test_sequence_tracker_step(tmp_path):
    from semantic_superpoint_amd.export import PointTracker, SequenceTracker
    dev = _dev()
    agent = _agent(tmp_path, dev)
    ml = 3
    seq = SequenceTracker(agent.net, dev, agent.conf_thresh, agent.nms_dist, False, agent.nn_thresh, ml)
    host = PointTracker(ml, agent.nn_thresh, dev)
    for im in _shifted_frames():
        o = seq.step(torch.from_numpy(im))
        assert o["pts"].shape[0] == 1 and o["desc"].shape[2] == 256
        agent.run(torch.from_numpy(im)[None, None].to(dev))
        pts = agent.heatmap_to_pts()
        desc = agent.desc_to_sparseDesc()
        host.update(pts[0], desc[0])
        assert np.array_equal(seq.tracker.tracks, host.tracks)
    _same_sequence_result(seq, host, ml)


def test_sequence_tracker_step_subpixel(tmp_path):
    """subpixel=True: step's device sum x + dx - 2 is the float64 sum of lib.points_to_numpy, so the tracker that is fed the
    read-back points and descriptors through the host `update` ends with the same table, matches and point sets."""
    from semantic_superpoint_amd import lib as L
    from semantic_superpoint_amd.export import PointTracker, SequenceTracker
    dev = _dev()
    agent = _agent(tmp_path, dev)
    ml = 3
    seq = SequenceTracker(agent.net, dev, agent.conf_thresh, agent.nms_dist, True, agent.nn_thresh, ml)
    host = PointTracker(ml, agent.nn_thresh, dev)
    moved = 0
    for im in _shifted_frames():
        o = seq.step(torch.from_numpy(im))
        c = int(o["count"][0].item())
        pts = L.points_to_numpy(o["pts"][0], o["count"][0], True)            # float64 [N, 3], subpixel (x, y)
        moved += int((pts[:, :2] != o["pts"][0, :c, :2].cpu().numpy()).any(axis=1).sum())
        host.update(pts.T.copy(), o["desc"][0, :c].cpu().numpy().T.copy())
        assert np.array_equal(seq.tracker.tracks, host.tracks)
    assert moved > 0   # the offsets did move points off the pixel grid
    _same_sequence_result(seq, host, ml)


@contextlib.contextmanager
def _no_host_sync():
    """Any host synchronisation (a copy to the host, .item(), a blocking upload) raises inside."""
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")   # (torch announces the mode as a prototype)
        torch.cuda.set_sync_debug_mode("error")
    try:
        yield
    finally:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            torch.cuda.set_sync_debug_mode(before)


def _device_frames(name, dev, pad=0):
    out = []
    for pts, desc in _inputs(name):
        n = pts.shape[1]
        p = torch.zeros(n + pad, 2, dtype=torch.float64)
        p[:n] = torch.from_numpy(pts[:2].T.copy())
        d = torch.zeros(n + pad, 256)
        d[:n] = torch.from_numpy(desc.T.copy())
        out.append((p.to(dev), torch.tensor([n], dtype=torch.int32, device=dev), d.to(dev)))
    return out


def _host_tables(name, dev):
    """The PointTracker fed sequence `name` through `update`, and after every frame (table rows, get_matches, get_mscores)."""
    from semantic_superpoint_amd.export import PointTracker
    spec = SEQUENCES[name]
    host = PointTracker(spec["max_length"], NN_THRESH, dev)
    seen = []
    for f, (pts, desc) in enumerate(_inputs(name)):
        if f in spec["clear_before"]:
            host.clear_desc()
        host.update(pts, desc)
        seen.append((host.tracks, host.get_matches(), host.get_mscores()))
    return host, seen


def test_update_device_does_not_synchronise():
    """The claim of update_device: every frame, the first (which allocates) included, is queued without a host copy or a host
    synchronisation, also when the matches of the frames before were never asked for."""
    from semantic_superpoint_amd.export import PointTracker
    dev = _dev()
    spec = SEQUENCES["B"]
    frames = _device_frames("B", dev)
    host, seen = _host_tables("B", dev)
    t = PointTracker(spec["max_length"], NN_THRESH, dev)
    with _no_host_sync():
        with pytest.raises(RuntimeError):      # the guard is live: a read-back raises
            frames[0][1].item()
        for f, (p, c, d) in enumerate(frames):
            if f in spec["clear_before"]:
                t.clear_desc()
            t.update_device(p, c, d)
            t.get_tracks_device(2)
    assert _same_tables(t.table, host.table)
    assert np.array_equal(t.get_matches(), seen[-1][1])
    assert np.array_equal(t.get_mscores(), seen[-1][2])   # the newest frame's, as documented for the device path
    for a, b in zip(t.all_pts, host.all_pts):
        assert np.array_equal(a, b[:2])


def test_sequence_step_does_not_synchronise(tmp_path):
    """SequenceTracker.step inherits the claim once the engine exists (the first step creates it): forward, describe_points,
    matcher and track update of the later frames are queued without a host synchronisation."""
    from semantic_superpoint_amd.export import SequenceTracker
    dev = _dev()
    agent = _agent(tmp_path, dev)
    seq = SequenceTracker(agent.net, dev, agent.conf_thresh, agent.nms_dist, True, agent.nn_thresh, 3)
    ims = [torch.from_numpy(im).to(dev) for im in _shifted_frames()]
    seq.step(ims[0])
    with _no_host_sync():
        for im in ims[1:]:
            seq.step(im)
    assert seq.get_tracks(2).shape[0] > 0


def test_update_after_update_device():
    """The two entry points mix: frames 0-3 of B through update_device (matches never read), the rest through update."""
    from semantic_superpoint_amd.export import PointTracker
    dev = _dev()
    spec = SEQUENCES["B"]
    frames = _device_frames("B", dev)
    _, seen = _host_tables("B", dev)
    t = PointTracker(spec["max_length"], NN_THRESH, dev)
    for f, (pts, desc) in enumerate(_inputs("B")):
        if f in spec["clear_before"]:
            t.clear_desc()
        if f < 4:
            t.update_device(*frames[f])
        else:
            t.update(pts, desc)
            assert np.array_equal(t.tracks, seen[f][0]), f
            assert np.array_equal(t.get_matches(), seen[f][1]), f
    assert np.array_equal(t.get_mscores(), seen[-1][2])


def test_capacity_above_the_matcher_limit_is_cut():
    """describe_points sizes its rows by the image, not by the count: a capacity above MATCH_MAX_POINTS with few points is
    legal and gives the table of the tight buffers."""
    from semantic_superpoint_amd import lib as L
    from semantic_superpoint_amd.export import PointTracker
    dev = _dev()
    host, _ = _host_tables("A", dev)
    t = PointTracker(2, NN_THRESH, dev)
    for p, c, d in _device_frames("A", dev, pad=L.MATCH_MAX_POINTS + 5):
        assert p.shape[0] > L.MATCH_MAX_POINTS
        t.update_device(p, c, d)
    assert _same_tables(t.table, host.table)
    assert np.array_equal(t.get_matches(), host.get_matches())


def test_two_runs_are_bit_identical():
    from semantic_superpoint_amd.export import PointTracker
    dev = _dev()
    runs = []
    for _ in range(2):
        t = PointTracker(SEQUENCES["C"]["max_length"], NN_THRESH, dev)
        for pts, desc in _inputs("C"):
            t.update(pts, desc)
        runs.append(t)
    a, b = runs[0].table, runs[1].table
    assert int(a["state"][0].item()) > 2048
    assert _same_tables(a, b)
    assert a["score"][:int(a["state"][0].item())].cpu().numpy().tobytes() == b["score"][:int(b["state"][0].item())].cpu().numpy().tobytes()
