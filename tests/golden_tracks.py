"""Inputs of the G19 track fixtures (shared by tools/make_golden_tracks.py, the tests and bench_tracks.py).  The fixture stores
every frame's points and, for the sequences that fit a committed file (A and B), its descriptors: `fixture_frames` hands those
to the tests as they are.  The descriptors of the longest sequence (C, 5417 x 256 floats) would not fit, so they are regenerated
from the fixed seed by `sequence_inputs`, the generator of all three, and pinned by a checksum per frame.

A sequence is a list of frames (pts float64 [3, N] = x, y, confidence; desc float32 [256, N] unit columns).  A point that
continues into the next frame keeps its descriptor, rotated by a small angle in a random plane, so that the distance to its
predecessor lies in [MATCH_LO, MATCH_HI]; every other pair of descriptors of two consecutive frames is at least NONMATCH_LO
apart.  With NN_THRESH between the two ranges the fp32 device matcher and the fp64 numpy matcher cannot disagree about a
match; `margins()` measures the two ranges and the generator refuses to write a fixture that violates them."""
import numpy as np

NN_THRESH = 0.7
MATCH_LO, MATCH_HI, NONMATCH_LO = 0.05, 0.5, 1.0
GET_TRACKS_M = lambda L: (1, 2, L)  # noqa: E731  (min_length values the fixture stores)

# name -> max_length, seed, points per frame, share of the previous frame's points that continue, clear_desc() before frames,
# whether the fixture holds the descriptors themselves
SEQUENCES = {
    "A": dict(max_length=2, seed=1901, counts=(7, 9, 5, 8), keep=(0, 0.7, 0.6, 0.8), clear_before=(), store_desc=True),
    # frame 2 is empty, frame 4 matches nothing (keep 0), clear_desc() before frame 5 (whose points do continue frame 4's)
    "B": dict(max_length=3, seed=1902, counts=(30, 40, 0, 25, 35, 38, 33), keep=(0, 0.7, 0, 0, 0, 0.6, 0.7),
              clear_before=(5,), store_desc=True),
    # the table passes 2048 rows (two 1024-row blocks), tracks die of age, ids of dropped frames fall below -1
    "C": dict(max_length=5, seed=1903, counts=(690, 655, 700, 668, 650, 697, 673, 684),
              keep=(0, 0.4, 0.42, 0.38, 0.4, 0.41, 0.39, 0.4), clear_before=(), store_desc=False),
}


def unit32(a):
    a = a.astype(np.float32)
    return (a / np.linalg.norm(a.astype(np.float64), axis=0, keepdims=True)).astype(np.float32)


def rotated(rs, d, lo, hi):
    """Columns of d (float64 unit) turned by the angle whose chord is uniform in [lo, hi], each in a random plane."""
    u = rs.randn(*d.shape)
    u -= d * np.sum(u * d, axis=0, keepdims=True)
    u /= np.linalg.norm(u, axis=0, keepdims=True)
    ang = 2.0 * np.arcsin(rs.uniform(lo, hi, size=(1, d.shape[1])) / 2.0)
    return np.cos(ang) * d + np.sin(ang) * u


def sequence_inputs(name):
    """[(pts, desc)] of sequence `name`, and for every frame the array `src` [N]: the index of each point's predecessor in the
    previous frame, -1 for a fresh point."""
    spec = SEQUENCES[name]
    rs = np.random.RandomState(spec["seed"])
    frames, srcs = [], []
    prev_pts = np.zeros((3, 0))
    prev_desc = np.zeros((256, 0), np.float32)
    for n, keep in zip(spec["counts"], spec["keep"]):
        k = min(int(round(keep * prev_desc.shape[1])), n)
        src = np.full(n, -1, np.int64)
        src[rs.permutation(n)[:k]] = rs.permutation(prev_desc.shape[1])[:k]
        cont = src >= 0
        desc = rs.randn(256, n)
        desc /= np.linalg.norm(desc, axis=0, keepdims=True)
        # the margin inside [MATCH_LO, MATCH_HI] absorbs the float32 rounding of the stored descriptors
        desc[:, cont] = rotated(rs, prev_desc[:, src[cont]].astype(np.float64), MATCH_LO + 0.01, MATCH_HI - 0.01)
        desc = unit32(desc)
        pts = np.zeros((3, n))
        pts[0] = np.round(rs.uniform(4, 316, n) * 8) / 8   # multiples of 1/8 pixel: exact in float32
        pts[1] = np.round(rs.uniform(4, 236, n) * 8) / 8
        pts[:2, cont] = prev_pts[:2, src[cont]] + np.round(rs.uniform(-2, 2, (2, k)) * 8) / 8
        pts[2] = np.round(rs.uniform(0.015, 1.0, n) * 4096) / 4096
        frames.append((pts, desc))
        srcs.append(src)
        prev_pts, prev_desc = pts, desc
    return frames, srcs


def fixture_frames(g, name):
    """[(pts, desc)] of sequence `name` for a test: the fixture's points, and its descriptors where it stores them (the
    regenerated ones otherwise)."""
    gen = None if SEQUENCES[name]["store_desc"] else sequence_inputs(name)[0]
    frames = []
    for f in range(len(SEQUENCES[name]["counts"])):
        key = "%s/%d/" % (name, f)
        frames.append((g[key + "pts"], g[key + "desc"] if gen is None else gen[f][1]))
    return frames


def margins(frames, srcs):
    """(smallest and largest distance of a continuing point to its predecessor, smallest distance of any other pair of two
    consecutive frames), fp64."""
    lo, hi, other = np.inf, -np.inf, np.inf
    for f in range(1, len(frames)):
        a, b = frames[f - 1][1].astype(np.float64), frames[f][1].astype(np.float64)
        if a.shape[1] == 0 or b.shape[1] == 0:
            continue
        d = np.sqrt(np.maximum(2.0 - 2.0 * np.clip(a.T @ b, -1, 1), 0.0))
        j = np.flatnonzero(srcs[f] >= 0)
        if len(j):
            m = d[srcs[f][j], j]
            lo, hi = min(lo, m.min()), max(hi, m.max())
            d[srcs[f][j], j] = np.inf
        other = min(other, d.min())
    return lo, hi, other


def desc_checksum(desc):
    """float64 [2]: the sum and the sum of |.| * (1 + row index) of a frame's descriptors (pins the regenerated inputs)."""
    d = desc.astype(np.float64)
    return np.array([d.sum(), (np.abs(d) * (1.0 + np.arange(d.shape[0]))[:, None]).sum()])
