"""Point tracks without a GPU: the numpy restatement (tests/tracks_ref.py) reproduces every table the reference produced
(G19 fixture, tools/make_golden_tracks.py), the regenerated inputs are the ones the fixture was made from, PointTracker
accepts any supported max_length, and the C entry points refuse bad arguments before they touch a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import golden_util as G
from tests import tracks_ref as TR
from tests.golden_tracks import (GET_TRACKS_M, MATCH_HI, MATCH_LO, NN_THRESH, NONMATCH_LO, SEQUENCES, desc_checksum, fixture_frames,
                                 margins, sequence_inputs)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ssp_track_workspace_bytes", "ssp_op_track_update", "ssp_op_track_select", "ssp_op_track_points")


@pytest.fixture(scope="module")
def g19():
    return G.load("g19_tracks.npz")


@pytest.mark.parametrize("name", sorted(SEQUENCES))
def test_restatement_reproduces_reference_tables(g19, name):
    spec = SEQUENCES[name]
    L = spec["max_length"]
    t = TR.Tracks(L)
    rows = 0
    for f, n in enumerate(spec["counts"]):
        key = "%s/%d/" % (name, f)
        assert g19[key + "pts"].shape == (3, n)
        TR.update(t, n, g19[key + "matches"])
        assert np.array_equal(t.matrix(), g19[key + "tracks"]), key
        assert t.track_count == int(g19[key + "track_count"])
        for m in GET_TRACKS_M(L):
            assert np.array_equal(TR.get_tracks(t, m), g19[key + "gt%d" % m]), (key, m)
        rows = max(rows, t.ids.shape[0])
    if name == "C":  # what the sequence is for: two 1024-row blocks, rows that died of age, ids pushed below -1
        assert rows > 2048 and t.track_count > rows
        assert (g19["C/7/tracks"][:, 2:] == -1).any()
    with pytest.raises(ValueError, match="'min_length' too small."):
        TR.get_tracks(t, 0)


@pytest.mark.parametrize("name", sorted(SEQUENCES))
def test_regenerated_inputs_are_the_fixture_inputs(g19, name):
    frames, srcs = sequence_inputs(name)
    for f, (pts, desc) in enumerate(frames):
        key = "%s/%d/" % (name, f)
        assert np.array_equal(pts, g19[key + "pts"]) and desc.dtype == np.float32
        assert np.allclose(desc_checksum(desc), g19[key + "desc_sum"], rtol=1e-12, atol=1e-9)
        assert (key + "desc" in g19) == SEQUENCES[name]["store_desc"]
        if key + "desc" in g19:   # A and B: the tests read the stored descriptors, and the generator still makes them
            assert g19[key + "desc"].dtype == np.float32 and np.array_equal(g19[key + "desc"], desc)
        # the planned continuations are the reference's matches
        planned = np.flatnonzero(srcs[f] >= 0) if f and f not in SEQUENCES[name]["clear_before"] else np.zeros(0, int)
        m = g19[key + "matches"]
        assert sorted(m[1].astype(int)) == list(planned)
        assert np.array_equal(srcs[f][m[1].astype(int)], m[0].astype(int))
    lo, hi, other = margins(frames, srcs)
    assert MATCH_LO <= lo and hi <= MATCH_HI < NN_THRESH < NONMATCH_LO <= other
    assert np.array_equal(g19[name + "/margins"], [lo, hi, other])
    for (pts, desc), (fp, fd) in zip(frames, fixture_frames(g19, name)):
        assert np.array_equal(pts, fp) and np.array_equal(desc, fd)


def test_track_points_restatement(g19):
    frames, _ = sequence_inputs("B")
    L = SEQUENCES["B"]["max_length"]
    tracks = g19["B/6/tracks"]
    xy = TR.track_points(tracks, [p for p, _ in frames[-L:]])
    assert xy.shape == (tracks.shape[0], L, 2)
    assert np.array_equal(np.isnan(xy[:, :, 0]), tracks[:, 2:] == -1)
    off = np.cumsum([0] + [p.shape[1] for p, _ in frames[-L:]])
    r = int(np.flatnonzero((tracks[:, -2:] != -1).all(axis=1))[0])   # a track through the last two frames
    for c in (L - 2, L - 1):
        assert np.array_equal(xy[r, c], frames[-L + c][0][:2, int(tracks[r, 2 + c]) - off[c]])


def test_symbols_declared_and_exported():
    from semantic_superpoint_amd import lib
    with open(os.path.join(ROOT, "include", "ssp_hip.h")) as f:
        hdr = f.read()
    for n in NEW:
        assert re.search(r"\b%s\(" % n, hdr), n
        assert n in lib.EXPORTS, n
    assert re.search(r"#define SSP_TRACK_MAX_LENGTH %d\b" % lib.TRACK_MAX_LENGTH, hdr)


def test_point_tracker_accepts_any_supported_length():
    from semantic_superpoint_amd import lib
    from semantic_superpoint_amd.export import PointTracker, SequenceTracker
    t = PointTracker(max_length=5, nn_thresh=0.7, device="cpu")   # raised NotImplementedError before tracks existed
    assert t.maxl == 5 and t.track_count == 0
    assert t.get_tracks(1).shape == (0, 7) and t.tracks.shape == (0, 7)
    assert len(t.all_pts) == 5 and all(p.shape == (2, 0) for p in t.all_pts)
    assert np.array_equal(t.get_offsets(), np.zeros(5))
    PointTracker(max_length=lib.TRACK_MAX_LENGTH, nn_thresh=0.7, device="cpu")
    for bad in (1, lib.TRACK_MAX_LENGTH + 1):
        with pytest.raises(ValueError):
            PointTracker(max_length=bad, nn_thresh=0.7, device="cpu")
    with pytest.raises(ValueError, match="'min_length' too small."):
        t.get_tracks(0)
    for m in ("update", "update_device", "get_tracks", "get_offsets", "track_points", "clear_desc", "get_matches", "get_mscores"):
        assert hasattr(PointTracker, m)
    assert callable(SequenceTracker) and hasattr(SequenceTracker, "step")
    with pytest.raises(NotImplementedError, match="track_points"):
        t.draw_tracks(None, None)


def test_update_none_warns_and_returns(capsys):
    from semantic_superpoint_amd.export import PointTracker
    t = PointTracker(max_length=3, nn_thresh=0.7, device="cpu")
    assert t.update(None, None) is None
    assert "no points were added" in capsys.readouterr().out
    assert t.track_count == 0


def test_c_entry_points_refuse_bad_arguments():
    """Every refusal comes back as a code and a message before anything is launched or allocated: no device is needed (the
    non-null pointers below are never dereferenced)."""
    from semantic_superpoint_amd import lib as L
    lib = L.load_library()
    err = lambda: lib.ssp_last_error().decode()  # noqa: E731
    P, big = L.MATCH_MAX_POINTS, L.MATCH_MAX_POINTS + 1
    assert lib.ssp_track_workspace_bytes(5, 1000, 5000) > 0
    assert lib.ssp_track_workspace_bytes(1, 1000, 5000) == 0 and "max_length" in err()
    assert lib.ssp_track_workspace_bytes(L.TRACK_MAX_LENGTH + 1, 1000, 17000) == 0 and "max_length" in err()
    assert lib.ssp_track_workspace_bytes(5, big, 5 * big) == 0 and "point_cap" in err()
    assert lib.ssp_track_workspace_bytes(5, 1000, L.TRACK_MAX_LENGTH * P + 1) == 0 and "row_cap" in err()
    # x stands for a device pointer.  Every call below is refused for at least two independent reasons (the one asserted comes
    # first in the entry point's order), so that no change of a single check lets a made-up pointer reach a kernel.
    x, y = C.c_void_p(4096), C.c_void_p(8192)

    def upd(L_=5, cap=1000, rows=5000, ids_in=x, outs=(y, y, y, y), match=x, ws=None):
        return lib.ssp_op_track_update(ids_in, x, x, x, match, None, x, x, L_, cap, rows, ws, outs[0], outs[1], outs[2], outs[3],
                                       None)

    assert upd(L_=1) != 0 and "max_length" in err()
    assert upd(L_=L.TRACK_MAX_LENGTH + 1) != 0 and "max_length" in err()
    assert upd(cap=big, rows=5 * big) != 0 and "point_cap" in err()
    assert upd(rows=4999) != 0 and "row_cap" in err()
    assert upd(match=None) != 0 and "null pointer" in err()
    assert upd(ids_in=None) != 0 and "null pointer" in err()
    assert upd(outs=(x, x, x, x), ws=x) != 0 and "in place" in err()   # all four arrays alias their inputs

    def sel(L_=5, rows=5000, ml=1, ids=x):
        return lib.ssp_op_track_select(ids, x, x, x, L_, rows, ml, None, x, x, None)

    assert sel(L_=17) != 0 and "max_length" in err()
    assert sel(rows=0) != 0 and "row_cap" in err()
    assert sel(ml=-1) != 0 and "min_length" in err()
    assert sel(ids=None) != 0 and "null pointer" in err()
    assert sel() != 0 and "null pointer" in err()

    def pts(L_=5, cap=1000, tracks=x, first=0, tcap=100):
        return lib.ssp_op_track_points(tracks, x, x, x, L_, cap, tcap, first, None, None)

    assert pts(L_=1) != 0 and "max_length" in err()
    assert pts(cap=big) != 0 and "point_cap" in err()
    assert pts(first=5) != 0 and "first_slot" in err()
    assert pts(tracks=None) != 0 and "null pointer" in err()
    assert pts() != 0 and "null pointer" in err()


# ---- the trackers' constructor: every refusal of the test_trackers_refuse_* GPU tests, with its message ---------------------------
_A, _B = (300.0, 300.0, 160.0, 120.0), (310.0, 300.0, 160.0, 120.0)
_FA = dict(geometric_check="fundamental", intrinsics=_A)
_MAP = dict(_FA, world_map="observe")
_ONE = " needs ONE camera: a fixed (previous, new) pair of different intrinsics cannot describe more than two views"
_LANDMARKS_FROM = " needs intrinsics and geometric_check='fundamental': the landmarks come from the trajectory's cameras"
_CAMERAS_FROM = " needs intrinsics and geometric_check='fundamental': the cameras come from the trajectory"
_PARAMS = "landmark_params must be (min_views >= 2, min_parallax_deg, max_reproj)"
_WORLD_P = "world_thresh must be finite and non-negative, world_min_inliers at least 4"
_WORLD_C = "1 <= world_cap <= 65536 and world_patience >= 0 required"
_BA = "1 <= bundle_iterations <= 16 and bundle_every >= 1 required"
_ABS = "absolute_thresh must be finite and non-negative, absolute_min_inliers at least 4"
_LOOP = "loop_min_gap must be at least 1, loop_min_inliers at least 4, loop_cooldown non-negative"


def _needs(option, tail):
    """The four cases every stage shares: no intrinsics (three ways), two different cameras."""
    return [(dict({option: "observe"}, **kw), option + tail) for kw in (dict(), dict(geometric_check="fundamental"),
                                                                         dict(geometric_check="homography"))] \
        + [(dict(geometric_check="fundamental", intrinsics=(_A, _B), **{option: "observe"}), option + _ONE)]


REFUSALS = _needs("world_map", _LANDMARKS_FROM) + [
    (dict(_MAP, world_min_inliers=3), _WORLD_P), (dict(_MAP, world_thresh=-1.0), _WORLD_P), (dict(_MAP, world_cap=0), _WORLD_C),
    (dict(_MAP, world_cap=65537), _WORLD_C), (dict(_MAP, world_patience=-1), _WORLD_C),
    (dict(_FA, world_map="always"), "world_map must be None, 'observe' or 'relocalise' (got 'always')"),
] + _needs("bundle_adjust", _CAMERAS_FROM) + [
    (dict(_FA, bundle_adjust="observe", bundle_iterations=0), _BA), (dict(_FA, bundle_adjust="observe", bundle_iterations=17), _BA),
    (dict(_FA, bundle_adjust="observe", bundle_every=0), _BA), (dict(_FA, bundle_adjust="observe", landmark_params=(1, 1.0, 2.0)), _PARAMS),
    (dict(_FA, bundle_adjust="always"), "bundle_adjust must be None, 'observe' or 'apply' (got 'always')"),
] + _needs("absolute_pose", _LANDMARKS_FROM) + [
    (dict(_FA, absolute_pose="observe", absolute_min_inliers=3), _ABS), (dict(_FA, absolute_pose="observe", absolute_thresh=-1.0), _ABS),
    (dict(_FA, absolute_pose="observe", landmark_params=(1, 1.0, 2.0)), _PARAMS),
    (dict(_FA, absolute_pose="always"), "absolute_pose must be None, 'observe' or 'repair' (got 'always')"),
    (dict(_FA, loop_closure="observe"), "loop_closure needs world_map: the closure is detected from the frame's matches against the map"),
    (dict(_MAP, loop_closure="observe", loop_min_gap=0), _LOOP), (dict(_MAP, loop_closure="observe", loop_min_inliers=3), _LOOP),
    (dict(_MAP, loop_closure="observe", loop_cooldown=-1), _LOOP),
    (dict(_MAP, loop_closure="observe", loop_iterations=0), "1 <= loop_iterations <= 64 required"),
    (dict(_MAP, loop_closure="observe", loop_weight=0.0), "loop_weight must be finite and positive"),
    (dict(_MAP, loop_closure="observe", trajectory_rows=1), "loop_closure needs trajectory_rows >= 2"),
    (dict(_MAP, loop_closure="always"), "loop_closure must be None, 'observe' or 'apply' (got 'always')"),
    # the order of the checks: the map, the loop closure, the absolute pose, the bundle adjustment
    (dict(world_map="always", loop_closure="always", absolute_pose="always", bundle_adjust="always"),
     "world_map must be None, 'observe' or 'relocalise' (got 'always')"),
    (dict(_FA, loop_closure="always", absolute_pose="always", bundle_adjust="always"),
     "loop_closure must be None, 'observe' or 'apply' (got 'always')"),
    (dict(absolute_pose="observe", bundle_adjust="observe"), "absolute_pose" + _LANDMARKS_FROM),
    (dict(_MAP, world_min_inliers=3, landmark_params=(1, 1.0, 2.0)), _WORLD_P),
]


@pytest.mark.parametrize("through", ["PointTracker", "SequenceTracker"])
@pytest.mark.parametrize("case", range(len(REFUSALS)))
def test_trackers_refuse_with_the_same_messages(through, case):
    """The constructor raises before any device work: the exception and its text for every refused combination."""
    from semantic_superpoint_amd.export import PointTracker, SequenceTracker
    kw, message = REFUSALS[case]
    with pytest.raises(ValueError) as e:
        PointTracker(3, 0.7, "cpu", **kw) if through == "PointTracker" else SequenceTracker(None, "cpu", 0.015, 4, False, 0.7, 3, **kw)
    assert str(e.value) == message


def test_landmark_calls_refuse_with_the_same_messages():
    from semantic_superpoint_amd.export import PointTracker, SequenceTracker
    need = "landmarks need intrinsics (and geometric_check='fundamental'): the cameras come from the trajectory"
    one = ("landmarks need ONE camera: a fixed (previous, new) pair of different intrinsics cannot describe more than two views "
           "(lib.op_map_window takes per-frame intrinsics)")
    for make in (lambda **kw: PointTracker(3, 0.7, "cpu", **kw), lambda **kw: SequenceTracker(None, "cpu", 0.015, 4, False, 0.7, 3, **kw)):
        for kw, message in ((dict(), need), (dict(geometric_check="fundamental"), need),
                            (dict(geometric_check="fundamental", intrinsics=(_A, _B)), one),
                            (dict(geometric_check="fundamental", intrinsics=(_A, _A), min_views=1), "min_views >= 2 required (got 1)")):
            kw = dict(kw)
            min_views = kw.pop("min_views", 2)
            t = make(**kw)
            for call in (t.landmarks, t.landmarks_device, t.landmark_rows_device):
                with pytest.raises(ValueError) as e:
                    call(min_views)
                assert str(e.value) == message
