"""World map on the device: ssp_match_world against op_match_two_way (torch.equal wherever both apply) and
against the numpy restatement on sign descriptors (every dot product exact, hundreds of ties: ==), its determinism and its
independence of map_cap; ssp_op_world_insert, ssp_op_world_correspondences and ssp_world_repair against tests/world_ref.py with ==;
the join followed by op_pnp_ransac within section 27's own tolerance (pnp_ref.TOLERANCE); the argument checks; PointTracker and
SequenceTracker on the blackout and the revisit as three trackers in lockstep (plain, "observe", "relocalise").  The bounds on the
centres (world_ref.BLACKOUT_BOUND = 2.33e-11, REVISIT_BOUND = 1.36e-12) are measured, not chosen: 16 times the restatement's float64 /
numpy.longdouble difference; tests/test_world_cpu.py repeats the measurement.  Every comparison prints what the device showed before
it asserts."""
import contextlib
import functools

import numpy as np
import pytest
import torch

from tests import landmarks_ref as LR
from tests import pnp_ref as N
from tests import pose_ref as P
from tests import world_ref as W

pytestmark = pytest.mark.gpu

THR = 0.7


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _unit_rows(seed, n):
    rng = np.random.RandomState(seed)
    d = rng.randn(n, 256).astype(np.float32)
    return d / np.linalg.norm(d, axis=1, keepdims=True).astype(np.float32)


def _world_with(lib, dev, desc, n_rows, map_cap, X=None):
    """A map of map_cap slots whose first rows are desc; the slots past them hold copies of row 0 (a kernel that read them would
    match them)."""
    w = lib.world_buffers(map_cap, 1024, dev)
    full = np.tile(desc[:1] if len(desc) else np.ones((1, 256), np.float32) / 16, (map_cap, 1)).astype(np.float32)
    full[:len(desc)] = desc
    w["desc"].copy_(_t(full, dev))
    w["state"][0] = n_rows
    if X is not None:
        w["X"][:len(X)] = _t(X, dev)
    return w


def _match_world(lib, dev, desc1, n1, desc2, n2, map_cap, cap, thr=THR):
    w = _world_with(lib, dev, desc1, n1, map_cap)
    d2 = np.tile(desc2[:1] if len(desc2) else np.ones((1, 256), np.float32) / 16, (cap, 1)).astype(np.float32)
    d2[:len(desc2)] = desc2
    m, n = lib.op_match_world(w, _t(d2, dev), torch.tensor([n2], dtype=torch.int32, device=dev), thr)
    torch.cuda.synchronize()
    return m, n


# ---- the matcher against op_match_two_way -----------------------------------------------------------------------------------------
TWO_WAY_SHAPES = [(1, 1, 1, 1), (63, 65, 65, 65), (64, 64, 64, 64), (65, 33, 65, 65), (4096, 1131, 4096, 4096),
                  (0, 40, 64, 64), (40, 0, 64, 64),      # one empty side
                  (100, 70, 300, 300),                   # n_rows below map_cap, a cap above the count
                  (129, 200, 256, 256)]


@pytest.mark.parametrize("n1,n2,map_cap,cap", TWO_WAY_SHAPES)
def test_match_world_equals_two_way(n1, n2, map_cap, cap):
    """Both operators apply when both sides fit one [cap, 256] array: same rows, same counts -> torch.equal on the match rows below
    n_match and on n_match."""
    from semantic_superpoint_amd import lib
    dev = _dev()
    both = _unit_rows(1000 + n1 + n2, max(n1, 1) + max(n2, 1))
    d1, d2 = both[:max(n1, 1)], both[max(n1, 1):]
    k = min(n1, n2) // 2                               # planted correspondences: noisy copies
    if k:
        rng = np.random.RandomState(7)
        noisy = d1[:k] + 0.02 * rng.randn(k, 256).astype(np.float32)
        d2[:k] = noisy / np.linalg.norm(noisy, axis=1, keepdims=True)
    m, n = _match_world(lib, dev, d1[:n1] if n1 else d1[:0], n1, d2[:n2] if n2 else d2[:0], n2, map_cap, cap)
    side1, side2 = np.zeros((cap, 256), np.float32), np.zeros((cap, 256), np.float32)
    side1[:n1], side2[:n2] = d1[:n1], d2[:n2]
    m2, n2_ = lib.op_match_two_way(_t(side1[None], dev), torch.tensor([n1], dtype=torch.int32, device=dev), _t(side2[None], dev),
                                   torch.tensor([n2], dtype=torch.int32, device=dev), THR)
    torch.cuda.synchronize()
    nm = int(n.item())
    print("(%d, %d): %d matches (two-way %d)" % (n1, n2, nm, int(n2_.item())))
    assert nm == int(n2_.item())
    assert nm >= k // 2
    assert torch.equal(m[:nm], m2[0, :nm])


# ---- the matcher on sign descriptors ----------------------------------------------------------------------------------------------
def _sign_case(n1, n2, copies=()):
    d1, d2 = W.sign_descriptors(11 + n1, n1), W.sign_descriptors(13 + n2, n2)
    k = min(n1, n2) // 2
    idx = np.random.RandomState(5).permutation(n1)[:k]
    d2[:k] = d1[idx]                                    # exact correspondences
    flip = np.random.RandomState(6).randint(0, 256, k)
    d2[np.arange(k // 2), flip[:k // 2]] *= -1          # half of them with one sign flipped
    for src, dst in copies:                             # exact copies of one map row in other strips: the first index must win
        d1[dst] = d1[src]
    return d1, d2


SIGN_SHAPES = [(4097, 33, ()), (8229, 1131, ((5000, 77), (5000, 8228), (300, 4200)))]


@pytest.mark.parametrize("n1,n2,copies", SIGN_SHAPES)
def test_match_world_sign_descriptors(n1, n2, copies):
    from semantic_superpoint_amd import lib
    dev = _dev()
    d1, d2 = _sign_case(n1, n2, copies)
    ref = W.match_world(d1, n1, d2, n2, THR)
    m, n = _match_world(lib, dev, d1, n1, d2, n2, n1, n2)
    nm = int(n.item())
    print("(%d, %d): %d matches (restatement %d)" % (n1, n2, nm, ref["n_match"]))
    assert nm == ref["n_match"] and nm > 0
    assert np.array_equal(m.cpu().numpy()[:nm], ref["match"][:nm])


def test_match_world_sign_descriptors_full():
    """65 536 x 4 096: every strip, every tile, the largest workspace."""
    from semantic_superpoint_amd import lib
    dev = _dev()
    n1, n2 = 65536, 4096
    d1, d2 = _sign_case(n1, n2, ((60000, 5), (60000, 65535)))
    ref = W.match_world(d1, n1, d2, n2, THR)
    m, n = _match_world(lib, dev, d1, n1, d2, n2, n1, n2)
    nm = int(n.item())
    print("(%d, %d): %d matches (restatement %d)" % (n1, n2, nm, ref["n_match"]))
    assert nm == ref["n_match"] and nm > 0
    assert np.array_equal(m.cpu().numpy()[:nm], ref["match"][:nm])


def test_match_world_deterministic_and_cap_independent():
    from semantic_superpoint_amd import lib
    dev = _dev()
    n1, n2 = 1500, 700
    both = _unit_rows(3, n1 + n2)
    d1, d2 = both[:n1], both[n1:]
    d2[:300] = d1[100:400]
    d2[300:350] = d1[100:150]                          # frame rows that are copies of each other
    w = _world_with(lib, dev, d1, n1, 2048)
    f = _t(np.concatenate([d2, np.zeros((68, 256), np.float32)]), dev)
    c = torch.tensor([n2], dtype=torch.int32, device=dev)
    a = [t.clone() for t in lib.op_match_world(w, f, c, THR)]
    b = [t.clone() for t in lib.op_match_world(w, f, c, THR)]
    w2 = _world_with(lib, dev, d1, n1, 1500)
    e = lib.op_match_world(w2, f, c, THR)
    w3 = _world_with(lib, dev, d1, n1, 65536)
    g = lib.op_match_world(w3, f, c, THR)
    torch.cuda.synchronize()
    nm = int(a[1].item())
    assert nm >= 300
    for other in (b, e, g):
        assert int(other[1].item()) == nm and torch.equal(other[0][:nm], a[0][:nm])


# ---- insert ----------------------------------------------------------------------------------------------------------------------
def _lm(rows):
    """landmark rows from (tid, p, x) triples"""
    out = np.zeros((len(rows), LR.LANDMARK_WORDS))
    for r, (t, p, x) in enumerate(rows):
        out[r] = [t, x, x + 0.5, x + 1.5, 3 + r % 4, 0.125 * r, 0.9, p]
    return out


def _table(flags):
    t = np.zeros((len(flags) + 1, P.ROW_WORDS))
    t[:len(flags), 14] = flags
    return t


def _insert_cases():
    big = [(t, t % 40, float(t)) for t in range(2500)]            # more than two blocks of 1024 landmark rows
    return {
        # name: (map_cap, tid_cap, [(landmark rows, count, flags so far)...])
        "append": (64, 1024, [(_lm([(5, 0, 1.0), (9, 3, 2.0), (2, 7, 3.0)]), 8, [1, 1, 0])]),
        "update": (64, 1024, [(_lm([(5, 0, 1.0), (9, 3, 2.0)]), 8, [1, 1, 0]), (_lm([(9, 1, 7.0), (11, 2, 8.0), (5, 5, 9.0)]), 8, [1, 1, 0, 0])]),
        "stable_order": (4096, 4096, [(_lm(big[:1200]), 40, [1, 1, 0]), (_lm(big[::-1]), 40, [1, 1, 0, 0])]),
        "bad_p": (64, 1024, [(_lm([(5, -1, 1.0), (6, 8, 2.0), (7, 7, 3.0), (8, np.nan, 4.0)]), 8, [1, 1, 0])]),
        "bad_x": (64, 1024, [(_lm([(5, 0, np.inf), (6, 1, 2.0), (-3, 2, 1.0)]), 8, [1, 1, 0])]),
        "tid_cap": (64, 16, [(_lm([(15, 0, 1.0), (16, 1, 2.0), (400, 2, 3.0), (3, 3, 4.0)]), 8, [1, 1, 0])]),
        "full": (5, 1024, [(_lm([(t, t, float(t)) for t in range(4)]), 8, [1, 1, 0]), (_lm([(t, t, 9.0 + t) for t in range(2, 8)]), 8, [1, 1, 0, 0])]),
        "not_anchored": (64, 1024, [(_lm([(5, 0, 1.0)]), 8, [1, 1, 0]), (_lm([(6, 0, 1.0), (5, 1, 4.0)]), 8, [1, 1, 0, 2])]),
    }


def _desc_new(call, count, point_cap=48):
    return W.sign_descriptors(100 + call, point_cap)


def _compare_map(w, ref, what):
    torch.cuda.synchronize()
    state = w["state"].cpu().numpy()
    print("%s: state %s (restatement %s)" % (what, state.tolist(), ref["state"].tolist()))
    assert np.array_equal(state, ref["state"]), what
    n = W.n_rows_of(ref)
    for k in ("X", "desc", "tid", "n_views", "first_frame", "last_frame", "rms"):
        assert np.array_equal(w[k].cpu().numpy()[:n], ref[k][:n]), (what, k)
    sl = w["slot_of_tid"].cpu().numpy()
    for s in range(n):
        assert sl[ref["tid"][s]] == s, (what, s)


@pytest.mark.parametrize("name", sorted(_insert_cases()))
def test_insert_cases(name):
    from semantic_superpoint_amd import lib
    dev = _dev()
    map_cap, tid_cap, calls = _insert_cases()[name]
    w, ref = lib.world_buffers(map_cap, tid_cap, dev), W.new_map(map_cap, tid_cap)
    for c, (lm, count, flags) in enumerate(calls):
        row_cap = lm.shape[0] + 3
        rows = np.full((row_cap, LR.LANDMARK_WORDS), 1.0)      # rows past n_landmarks would be valid ones
        rows[:lm.shape[0]] = lm
        desc = _desc_new(c, count)
        table, n = _table(flags), len(flags)
        W.insert(ref, rows, lm.shape[0], desc, count, table, n)
        lib.op_world_insert(w, _t(rows, dev), torch.tensor([lm.shape[0]], dtype=torch.int32, device=dev), _t(desc, dev),
                            torch.tensor([count], dtype=torch.int32, device=dev), _t(table, dev), n)
        _compare_map(w, ref, "%s call %d" % (name, c))
    if name == "full":
        assert ref["state"][W.DROP_FULL] == 3 and ref["state"][W.N_ROWS] == 5
    if name == "tid_cap":
        assert ref["state"][W.DROP_TID] == 2 and ref["state"][W.N_ROWS] == 2
    if name == "stable_order":
        assert ref["state"][W.N_ROWS] == 2500 and ref["state"][W.UPDATED] == 1200


def test_insert_stale_slot_after_clear_and_patience():
    """A cleared map (patience) leaves slot_of_tid entries behind: they must not be found.  The anchor machine over a flag sequence."""
    from semantic_superpoint_amd import lib
    dev = _dev()
    w, ref = lib.world_buffers(32, 64, dev), W.new_map(32, 64)
    lm = _lm([(5, 0, 1.0), (9, 3, 2.0), (2, 7, 3.0)])
    flags = [1, 1]
    for f, flag in enumerate([0, 0, 1, 1, 1, 0, 0, 2, 0]):
        flags.append(flag)
        rows = lm.copy()
        rows[:, 1] += f
        rows = rows[::-1].copy() if f >= 5 else rows           # after the clear the tracks return in another order
        desc, table = _desc_new(f, 8), _table(flags)
        W.insert(ref, rows, 3, desc, 8, table, len(flags), patience=2)
        lib.op_world_insert(w, _t(rows, dev), torch.tensor([3], dtype=torch.int32, device=dev), _t(desc, dev),
                            torch.tensor([8], dtype=torch.int32, device=dev), _t(table, dev), len(flags), patience=2)
        _compare_map(w, ref, "frame %d (flag %d)" % (f, flag))
    assert ref["state"][W.N_ROWS] == 3 and ref["tid"][0] == 2


# ---- the join, P3P, the repair ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _slow():
    return N.slow_problem()


def _slow_world(lib, dev, map_cap=256):
    """The slow problem's landmarks as a map (row r = landmark row r) and its match rows re-pointed at the map rows."""
    pr = _slow()
    lms = pr["landmarks"]
    owner = {}
    for r in range(lms.shape[0]):
        owner.setdefault(int(lms[r, 7]), r)
    match = pr["match"].copy()
    n = int(pr["n_match"])
    rows = [k for k in range(n) if int(match[k, 0]) in owner]
    wm = np.zeros_like(match)
    for o, k in enumerate(rows):
        wm[o] = (owner[int(match[k, 0])], match[k, 1], match[k, 2])
    ref = W.new_map(map_cap, 1024)
    ref["X"][:lms.shape[0]] = lms[:, 1:4]
    ref["state"][W.N_ROWS] = lms.shape[0]
    w = lib.world_buffers(map_cap, 1024, dev)
    w["X"].copy_(_t(ref["X"], dev))
    w["state"].copy_(_t(ref["state"], dev))
    return pr, w, ref, wm, len(rows)


def test_correspondences_and_pnp():
    from semantic_superpoint_amd import lib
    dev = _dev()
    pr, w, ref, wm, n = _slow_world(lib, dev)
    pts = pr["pts_new"]
    count = pts.shape[0] - 2                                      # the last two points are past the count
    wm2 = wm.copy()
    wm2[1, 0] = ref["state"][W.N_ROWS]                            # a map row at n_rows
    ref["X"][int(wm2[2, 0]), 1] = np.nan                          # a non-finite landmark
    w["X"].copy_(_t(ref["X"], dev))
    want, (rn, rv) = W.correspondences(ref, wm2, n, pts, count)
    corr, cn = lib.op_world_correspondences(w, _t(wm2, dev), torch.tensor([n], dtype=torch.int32, device=dev), _t(pts, dev),
                                            torch.tensor([count], dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    print("join: %s rows/valid (restatement %s)" % (cn.cpu().tolist(), [rn, rv]))
    assert cn.cpu().tolist() == [rn, rv] and rv < rn
    assert np.array_equal(corr.cpu().numpy(), want, equal_nan=False)
    k = pr["k"]
    res = N.ransac(want, rn, k, pr["seed"])
    got = lib.op_pnp_ransac(corr, cn[:1].contiguous(), _t(np.asarray(k, dtype=np.float64).reshape(1, 4), dev),
                            torch.tensor([pr["seed"]], dtype=torch.int64, device=dev))
    torch.cuda.synchronize()
    worst = max(float(np.abs(got["Rw"].cpu().numpy()[0].reshape(9) - np.asarray(res["Rw"]).reshape(9)).max()),
                float(np.abs(got["C"].cpu().numpy()[0] - np.asarray(res["C"]).reshape(3)).max()))
    print("P3P on the join: status %d, %d inliers (restatement %d, %d), worst difference %.3e (tolerance %.3e)"
          % (got["status"].item(), got["n_inliers"].item(), res["status"], res["n_inliers"], worst, N.TOLERANCE))
    assert got["status"].item() == res["status"] == 0 and got["n_inliers"].item() == res["n_inliers"]
    assert worst <= N.TOLERANCE


def _repair_case(name):
    """(world state, absolute, chain state words, table)"""
    rng = np.random.RandomState(3)
    Rw = P._rodrigues(np.array([3.0, -2.0, 1.0]))
    C = np.array([0.3, -0.1, 0.05])
    table = np.zeros((6, P.ROW_WORDS))
    for f in range(4):
        table[f, 0:9], table[f, 9:12], table[f, 12], table[f, 14] = np.eye(3).reshape(9), rng.rand(3) * 0.1 * f, 0.1, 0
    st = np.zeros(P.STATE_WORDS)
    st[0], st[1], st[2:11] = 4, 0.1, np.eye(3).reshape(9)
    ws = np.zeros(W.STATE_WORDS, np.int32)
    ws[W.N_ROWS], ws[W.ANCHORED], ws[W.STREAK] = 10, 1, 0
    a = {"Rw": Rw.copy(), "C": C.copy(), "status": 0}
    if name == "no_pose":
        table[3, 14] = 1
    elif name == "carried":
        table[3, 14] = 2
    elif name == "carried_short":                                  # a step below 1/64 of s keeps s and bit 1
        table[3, 14], a["C"] = 2, table[2, 9:12] + 1e-4
    elif name == "clean_anchored":                                 # nothing to repair: streak is zeroed
        ws[W.STREAK] = 3
    elif name == "clean_lost":                                     # a clean row rewritten while the map is lost
        ws[W.ANCHORED], ws[W.STREAK] = 0, 1
    elif name == "status1":
        table[3, 14], a["status"], ws[W.STREAK] = 1, 1, 2
    elif name == "not_finite":
        table[3, 14], a["C"][1] = 1, np.nan
    elif name == "full_table":
        table[3, 14], st[0] = 1, 6
    elif name == "first_row":
        table[0, 14], st[0] = 1, 1
    elif name == "empty_map_clean":                                # no rows: not lost
        ws[W.N_ROWS], ws[W.ANCHORED] = 0, 0
    else:
        raise KeyError(name)
    return ws, a, st, table


REPAIR_CASES = ("no_pose", "carried", "carried_short", "clean_anchored", "clean_lost", "status1", "not_finite", "full_table",
                "first_row", "empty_map_clean")


@pytest.mark.parametrize("name", REPAIR_CASES)
def test_repair(name):
    from semantic_superpoint_amd import lib
    dev = _dev()
    ws, a, st, table = _repair_case(name)
    ref = W.new_map(16, 16)
    ref["state"][:] = ws
    want_st, want_table = W.repair(ref, a, st, table)
    w = lib.world_buffers(16, 16, dev)
    w["state"].copy_(_t(ws, dev))
    absolute = {"Rw": _t(a["Rw"].reshape(1, 3, 3), dev), "C": _t(a["C"].reshape(1, 3), dev),
                "status": torch.tensor([a["status"]], dtype=torch.int32, device=dev)}
    s_dev, t_dev = _t(st, dev), _t(table, dev)
    lib.op_world_repair(w, absolute, s_dev, t_dev)
    torch.cuda.synchronize()
    print("%s: flags %s -> %s, streak %d (restatement %d)" % (name, table[:4, 14].tolist(), t_dev.cpu().numpy()[:4, 14].tolist(),
                                                             int(w["state"][W.STREAK].item()), int(ref["state"][W.STREAK])))
    assert np.array_equal(w["state"].cpu().numpy(), ref["state"])
    assert np.array_equal(t_dev.cpu().numpy(), want_table, equal_nan=True)
    assert np.array_equal(s_dev.cpu().numpy(), want_st, equal_nan=True)
    fired = name in ("no_pose", "carried", "carried_short", "clean_lost", "first_row")
    assert (int(ref["state"][W.STREAK]) > 0) == fired
    if fired:
        row = want_table[int(st[0]) - 1]
        assert int(row[14]) & (N.FLAG_ABSOLUTE | W.FLAG_WORLD) == (N.FLAG_ABSOLUTE | W.FLAG_WORLD)


# ---- argument checks -----------------------------------------------------------------------------------------------------------
def test_argument_checks():
    from semantic_superpoint_amd import lib
    dev = _dev()
    with pytest.raises(ValueError):
        lib.world_buffers(0, 16, dev)
    with pytest.raises(ValueError):
        lib.world_buffers(65537, 16, dev)
    with pytest.raises(RuntimeError):
        lib.world_buffers(16, 16, "cpu")
    w = lib.world_buffers(16, 16, dev)
    one = torch.ones(1, dtype=torch.int32, device=dev)
    d = torch.zeros(8, 256, device=dev)
    with pytest.raises(ValueError):
        lib.op_match_world(w, d, one, -1.0)
    with pytest.raises(ValueError):
        lib.op_match_world(w, torch.zeros(4097, 256, device=dev), one, 0.7)
    with pytest.raises(ValueError):
        lib.op_match_world(w, d.double(), one, 0.7)
    with pytest.raises(ValueError):
        lib.op_match_world({"desc": d}, d, one, 0.7)
    with pytest.raises(ValueError):
        lib.op_match_world(w, d, one.long(), 0.7)
    lm = torch.zeros(4, LR.LANDMARK_WORDS, dtype=torch.float64, device=dev)
    table = torch.zeros(4, P.ROW_WORDS, dtype=torch.float64, device=dev)
    with pytest.raises(ValueError):
        lib.op_world_insert(w, lm[:, :7].contiguous(), one, d, one, table, 3)
    with pytest.raises(ValueError):
        lib.op_world_insert(w, lm, one, d, one, table, -1)
    with pytest.raises(ValueError):
        lib.op_world_insert(w, lm, one, d, one, table[:, :8].contiguous(), 3)
    m = torch.zeros(8, 3, device=dev)
    pts = torch.zeros(8, 2, dtype=torch.float64, device=dev)
    with pytest.raises(ValueError):
        lib.op_world_correspondences(w, m, one, pts.float(), one)
    with pytest.raises(ValueError):
        lib.op_world_correspondences(w, m[:, :2].contiguous(), one, pts, one)
    a = {"Rw": torch.eye(3, dtype=torch.float64, device=dev), "C": torch.zeros(3, dtype=torch.float64, device=dev),
         "status": torch.zeros(2, dtype=torch.int32, device=dev)}
    st = torch.zeros(P.STATE_WORDS, dtype=torch.float64, device=dev)
    with pytest.raises(ValueError):
        lib.op_world_repair(w, a, st, table)
    with pytest.raises(ValueError):
        lib.op_world_repair(w, {"Rw": a["Rw"]}, st, table)


# ---- the trackers --------------------------------------------------------------------------------------------------------------
OLD_KEYS = {"F", "mask", "n_inliers", "status", "winner", "err", "R", "t", "E", "cand", "counts", "n_front", "pose_status", "front",
            "depth", "X"}
WORLD_KEYS = {"world_" + k for k in ("Rw", "C", "mask", "n_inliers", "winner", "rms", "status", "corr", "n_corr", "match", "n_match")}
TRACKER_CAP = 4096


@contextlib.contextmanager
def _no_host_sync():
    torch.cuda.set_sync_debug_mode("error")
    try:
        yield
    finally:
        torch.cuda.set_sync_debug_mode("default")


def _frame(seq, f, dev):
    xy = seq["pts"][f]
    return (_t(xy.reshape(-1, 2), dev), torch.tensor([xy.shape[0]], dtype=torch.int32, device=dev),
            _t(np.asarray(seq["desc"][f], dtype=np.float32).reshape(-1, 256), dev))


def _clone_map(w):
    return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in w.items()}


@pytest.mark.parametrize("which", ("blackout", "revisit"))
@pytest.mark.parametrize("through", ("PointTracker", "SequenceTracker"))
def test_trackers_world_map(through, which):
    """Trackers in lockstep over the blackout and the revisit: plain, "observe", "relocalise"."""
    from semantic_superpoint_amd import lib
    from semantic_superpoint_amd.export import PointTracker, SequenceTracker
    dev = _dev()
    if which == "blackout":
        (seq, runs), Lm, seed0, bound = W.blackout_runs(), W.BLACKOUT_L, W.BLACKOUT_SEED0, W.BLACKOUT_BOUND
    else:
        (seq, runs), Lm, seed0, bound = W.revisit_runs(), W.REVISIT_L, W.REVISIT_SEED0, W.REVISIT_BOUND
    frames = len(seq["pts"])
    kw = dict(geometric_check="fundamental", check_seed=seed0, intrinsics=tuple(seq["intr"][0]), trajectory_rows=frames + 1)

    def make(**more):
        if through == "PointTracker":
            top = PointTracker(Lm, W.NN_THRESH, dev, **kw, **more)
            return top, top
        top = SequenceTracker(None, dev, 0.015, 4, False, W.NN_THRESH, Lm, **kw, **more)     # fed through its tracker: no network
        return top, top.tracker

    (plain_top, plain), (obs_top, obs) = make(), make(world_map="observe", world_cap=TRACKER_CAP)
    rel_top, rel = make(world_map="relocalise", world_cap=TRACKER_CAP)
    assert plain_top.trajectory() is None and obs_top.world_trajectory() is None and obs_top.world_map_device() is None
    assert obs_top.world_map()[0].shape == (0, 8)
    k1 = _t(seq["intr"][:1], dev)
    for f in range(frames):
        before = {nm: (_clone_map(tr._world) if tr._world is not None else None) for nm, tr in (("observe", obs), ("relocalise", rel))}
        frame = _frame(seq, f, dev)
        plain.update_device(*frame)
        if f >= 2:                                                       # (the first frames allocate)
            with _no_host_sync():
                obs.update_device(*frame)
                rel.update_device(*frame)
        else:
            obs.update_device(*frame)
            rel.update_device(*frame)
        gp, go, gr = plain.last_geometry(), obs.last_geometry(), rel.last_geometry()
        assert set(gp) == OLD_KEYS and set(go) == set(gr) == OLD_KEYS | WORLD_KEYS
        for k in OLD_KEYS:                                               # observing changes nothing the plain tracker computes
            assert torch.equal(gp[k], go[k]), (f, k)
        assert torch.equal(plain.trajectory()[0], obs.trajectory()[0]) and torch.equal(plain.trajectory()[1], obs.trajectory()[1])
        assert np.array_equal(plain.get_tracks(1), obs.get_tracks(1))
        if f >= 1:
            a, b = plain_top.landmarks_device(), obs_top.landmarks_device()
            assert torch.equal(a[1], b[1]) and torch.equal(a[0][:int(a[1])], b[0][:int(b[1])])
        # the world pose through the operators on the map as it stood before the frame, bit for bit
        for nm, tr, top, g in (("observe", obs, obs_top, go), ("relocalise", rel, rel_top, gr)):
            w0 = before[nm] if before[nm] is not None else lib.world_buffers(TRACKER_CAP, device=dev)
            slot, dslot = f % Lm, f % 2
            m, n_m = lib.op_match_world(w0, tr._desc[dslot], tr._counts[dslot:dslot + 1], W.NN_THRESH)
            corr, n = lib.op_world_correspondences(w0, m, n_m, tr._pts[slot], tr._counts[dslot:dslot + 1])
            want = lib.op_pnp_ransac(corr[None], n[0:1], k1, torch.tensor([seed0 + f], dtype=torch.int64, device=dev))
            nm_ = int(n_m)
            assert int(g["world_n_match"]) == nm_ and torch.equal(g["world_match"][:nm_], m[:nm_]), (nm, f)
            assert torch.equal(g["world_corr"], corr) and torch.equal(g["world_n_corr"], n), (nm, f)
            for k in want:
                assert torch.equal(g["world_" + k], want[k]), (nm, f, k)
            table, nf = top.world_trajectory()
            r = table[f]
            assert float(nf) == f + 1 and torch.equal(r[0:9], want["Rw"].reshape(9)) and torch.equal(r[9:12], want["C"].reshape(3))
            assert [float(r[12]), float(r[13]), float(r[14]), float(r[15])] == [float(want["n_inliers"]), float(want["rms"]),
                                                                               float(want["status"]), float(n[1])]
            ref = runs[nm]
            state = tr._world["state"].cpu().numpy()
            print("%s frame %d: world status %d, %d inliers (restatement %d, %d); map state %s (restatement %s)"
                  % (nm, f, int(want["status"]), int(want["n_inliers"]), ref["world"][f]["status"], ref["world"][f]["n_inliers"],
                     state.tolist(), ref["states"][f].tolist()))
            assert int(want["status"]) == ref["world"][f]["status"] and int(want["n_inliers"]) == ref["world"][f]["n_inliers"]
            assert np.array_equal(state, ref["states"][f]), (nm, f)
    for nm, tr, top in (("observe", obs, obs_top), ("relocalise", rel, rel_top)):
        ref = runs[nm]
        table = tr.trajectory()[0][:frames].cpu().numpy()
        worst = float(np.abs(table[:, 9:12] - ref["table"][:, 9:12]).max())
        print("%s %s %s: flags %s (restatement %s), centres against the restatement %.3e (bound %.3e)"
              % (through, which, nm, table[:, 14].tolist(), ref["table"][:, 14].tolist(), worst, bound))
        assert table[:, 14].tolist() == ref["table"][:, 14].tolist()
        assert worst <= bound
        rows, desc = top.world_map()
        want_rows, want_desc = W.map_rows(ref["map"])
        assert rows.shape == want_rows.shape and np.array_equal(rows[:, [0, 4, 6, 7]], want_rows[:, [0, 4, 6, 7]])
        assert np.array_equal(desc, want_desc)
        # the rows seen in the newest frame are copies of the landmark rows the tracker kept for the insert
        lms = tr._world_lm["landmarks"][:int(tr._world_lm["n_landmarks"])].cpu().numpy()
        by_tid = {int(r[0]): r for r in lms}
        newest = rows[rows[:, 7] == frames - 1]
        assert len(newest) >= 12 or not int(ref["states"][-1][W.ANCHORED])      # (a map that is lost takes no rows)
        for r in newest:
            assert np.array_equal(r[1:4], by_tid[int(r[0])][1:4]) and r[5] == by_tid[int(r[0])][5] and r[4] == by_tid[int(r[0])][4]
        assert top.world_map_device() is tr._world
    if which == "blackout":
        dark = seq["dark"]
        flags = rel.trajectory()[0][:frames, 14].tolist()
        assert int(flags[dark + 1]) & 16 and int(flags[dark + 2]) & 16
        assert W.centre_errors(seq, rel.trajectory()[0][:frames].cpu().numpy())[dark + 1:].max() <= bound
        assert W.centre_errors(seq, plain.trajectory()[0][:frames].cpu().numpy())[dark + 1:].min() > 0.1


def test_trackers_refuse_what_cannot_hold_a_world_map():
    from semantic_superpoint_amd.export import PointTracker, SequenceTracker
    dev = _dev()
    a, b = (300.0, 300.0, 160.0, 120.0), (310.0, 300.0, 160.0, 120.0)
    for make in (lambda **kw: PointTracker(3, 0.7, dev, **kw), lambda **kw: SequenceTracker(None, dev, 0.015, 4, False, 0.7, 3, **kw)):
        for kw in (dict(), dict(geometric_check="fundamental"), dict(geometric_check="homography"),
                   dict(geometric_check="fundamental", intrinsics=(a, b)),
                   dict(geometric_check="fundamental", intrinsics=a, world_min_inliers=3),
                   dict(geometric_check="fundamental", intrinsics=a, world_thresh=-1.0),
                   dict(geometric_check="fundamental", intrinsics=a, world_cap=0),
                   dict(geometric_check="fundamental", intrinsics=a, world_cap=65537),
                   dict(geometric_check="fundamental", intrinsics=a, world_patience=-1)):
            with pytest.raises(ValueError):
                make(world_map="observe", **kw)
        with pytest.raises(ValueError):
            make(geometric_check="fundamental", intrinsics=a, world_map="always")
        t = make(geometric_check="fundamental", intrinsics=(a, a), world_map="relocalise")
        assert t.world_trajectory() is None
