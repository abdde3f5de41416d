"""G19 fixture of the point tracks (PointTracker over a frame sequence), produced by the REAL reference on the CPU.

  g19_tracks.npz   for every sequence of tests/golden_tracks.py (A: max_length 2, the existing path; B: max_length 3 with an
                   empty frame, a frame that matches nothing and a clear_desc(); C: max_length 5, 650-700 points per frame,
                   more than 2048 rows) and every frame f, under "<seq>/<f>/":
                     pts          [3, N] the points handed to update
                     desc         [256, N] float32, the descriptors handed to update (A and B; those of C would not fit a
                                  committed file and are regenerated from the seed)
                     desc_sum     a checksum of the descriptors (pins the regenerated ones)
                     matches      [3, K] the matches update saw
                     mscores      get_mscores() after the frame (absent while it is None: an empty side returns early)
                     get_matches  what get_matches() returns after the frame ([3, 0] after the first, then [4, K])
                     tracks       the tracker's table after the frame, float64 [M, 2 + L]
                     track_count  the tracker's running track id
                     gt<m>        get_tracks(m) for m in (1, 2, L)
                   and "<seq>/margins" = (smallest, largest match distance, smallest non-match distance).

The generator stops when the descriptor margins of tests/golden_tracks.py do not hold: a track fixture must not depend on how
a matcher rounds.  Needs the reference checkout (oracle/ref_harness.py); run from the repository root:
  python tools/make_golden_tracks.py
"""
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_harness as R  # noqa: E402
from tests.golden_tracks import (GET_TRACKS_M, MATCH_HI, MATCH_LO, NN_THRESH, NONMATCH_LO, SEQUENCES, desc_checksum,  # noqa: E402
                                 margins, sequence_inputs)

OUT = os.path.join(ROOT, "tests", "golden", "g19_tracks.npz")


def run_sequence(name, out):
    from models.model_wrap import PointTracker
    spec = SEQUENCES[name]
    L = spec["max_length"]
    frames, srcs = sequence_inputs(name)
    lo, hi, other = margins(frames, srcs)
    # both sides of nn_thresh: no match distance above MATCH_HI, no other distance below NONMATCH_LO
    assert MATCH_LO <= lo and hi <= MATCH_HI < NN_THRESH < NONMATCH_LO <= other, (name, lo, hi, other)
    assert other - hi >= NONMATCH_LO - MATCH_HI, (name, lo, hi, other)
    out[name + "/margins"] = np.array([lo, hi, other])
    tracker = PointTracker(max_length=L, nn_thresh=NN_THRESH)
    seen = []
    inner = tracker.nn_match_two_way   # observe what update gets back (get_mscores() keeps the last NON-EMPTY call only)
    tracker.nn_match_two_way = lambda *a: seen.append(inner(*a)) or seen[-1]
    rows = 0
    for f, (pts, desc) in enumerate(frames):
        if f in spec["clear_before"]:
            tracker.clear_desc()
        tracker.update(pts, desc)
        m = seen[-1]
        assert len(seen) == f + 1
        expect = np.flatnonzero(srcs[f] >= 0) if f and f not in spec["clear_before"] else np.zeros(0, int)
        assert sorted(m[1].astype(int)) == list(expect), "%s frame %d: the reference matched other points than planned" % (name, f)
        key = "%s/%d/" % (name, f)
        out[key + "pts"] = pts
        if spec["store_desc"]:
            out[key + "desc"] = desc
        out[key + "desc_sum"] = desc_checksum(desc)
        out[key + "matches"] = m.copy()
        out[key + "get_matches"] = tracker.get_matches().copy()
        if tracker.get_mscores() is not None:
            out[key + "mscores"] = tracker.get_mscores().copy()
        out[key + "tracks"] = tracker.tracks.copy()
        out[key + "track_count"] = np.int64(tracker.track_count)
        for ml in GET_TRACKS_M(L):
            out[key + "gt%d" % ml] = tracker.get_tracks(ml)
        rows = max(rows, tracker.tracks.shape[0])
    print("  %s: max_length %d, %d frames, match distances %.3f-%.3f, others >= %.3f, up to %d rows, %d tracks"
          % (name, L, len(frames), lo, hi, other, rows, tracker.track_count))
    return rows


if __name__ == "__main__":
    R.install()
    warnings.simplefilter("ignore", DeprecationWarning)  # the reference converts a 1x1 array with int()
    out = {}
    rows = {name: run_sequence(name, out) for name in SEQUENCES}
    assert rows["C"] > 2048, "sequence C must cross two 1024-row blocks"
    np.savez_compressed(OUT, **out)
    print("  %s: %d bytes" % (OUT, os.path.getsize(OUT)))
    assert os.path.getsize(OUT) < (1 << 20)
