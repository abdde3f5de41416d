"""World map classes on the device against tests/world_classes_ref.py, every comparison == or torch.equal:
the class vote and the read-out (in place on a reused buffer, again after re-zeroing); ssp_match_world_classes on sign descriptors
(every dot product exact in any order) with three classes, unknown rows, a dropped class and copies of one descriptor planted across
waves and strips under differing classes, over the shapes at which world_match_kernel takes another path; its bit-identity with
op_match_world when the classes cannot matter; the trackers in lockstep over the revisit with planted aliases."""
import contextlib
import types

import numpy as np
import pytest
import torch

from tests import landmarks_ref as LR
from tests import world_classes_ref as WC
from tests import world_ref as W

pytestmark = pytest.mark.gpu

THR = 0.7
NONE = WC.CLASS_NONE


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _i32(v, dev):
    return torch.tensor([v], dtype=torch.int32, device=dev)


# ---- the vote and the read-out ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nl", (1, 63, 64, 65, 1025))
def test_votes_and_read_out(nl):
    from semantic_superpoint_amd import lib
    dev = _dev()
    rng = np.random.RandomState(100 + nl)
    row_cap, point_cap, tid_cap, map_cap = nl + 3, 50, 2 * nl + 5, nl + 9
    ids = rng.permutation(tid_cap + 4)[:row_cap].astype(np.float64)          # unique; a few at or past tid_cap
    lm = rng.randn(row_cap, LR.LANDMARK_WORDS)
    lm[:, 0], lm[:, 7] = ids, rng.randint(-1, point_cap + 2, row_cap)
    lm[::7, 1] = np.nan                                                      # X plays no part
    cls_new = rng.randint(0, 4, point_cap).astype(np.uint8)
    cls_new[rng.rand(point_cap) < 0.2] = NONE
    count = point_cap - 3
    start = ((rng.choice([0, 0, 1, 2, 254, 255], tid_cap) << 8) | rng.randint(0, 4, tid_cap)).astype(np.uint16)
    classes = lib.world_class_buffers(tid_cap, dev)
    classes["votes"].copy_(_t(start, dev))
    lm_d, cls_d = _t(lm, dev), _t(cls_new, dev)
    want = start.copy()
    for call in range(2):                                                    # in place, on the buffer the first call left
        lib.op_track_class_votes(classes, lm_d, _i32(nl, dev), cls_d, _i32(count, dev))
        WC.vote(want, lm, nl, cls_new, count)
        got = classes["votes"].cpu().numpy()
        print("nl %d call %d: %d entries changed" % (nl, call, int((got != start).sum())))
        assert np.array_equal(got, want)
    assert (want != start).any() or nl == 1
    w = lib.world_buffers(map_cap, tid_cap, dev)
    wr = W.new_map(map_cap, tid_cap)
    wr["tid"][:] = rng.randint(0, tid_cap, map_cap)
    wr["state"][W.N_ROWS] = nl
    w["tid"].copy_(_t(wr["tid"], dev))
    w["state"].copy_(_t(wr["state"], dev))
    out = lib.op_world_classes(w, classes)
    assert out.dtype == torch.uint8 and np.array_equal(out.cpu().numpy(), WC.world_classes(wr, want))
    assert lib.op_world_classes(w, classes, out=out) is out
    classes["votes"].zero_()                                                 # a repeated call after re-zeroing
    lib.op_track_class_votes(classes, lm_d, _i32(nl, dev), cls_d, _i32(count, dev))
    zero = WC.vote(WC.new_votes(tid_cap), lm, nl, cls_new, count)
    assert np.array_equal(classes["votes"].cpu().numpy(), zero)
    assert np.array_equal(lib.op_world_classes(w, classes).cpu().numpy(), WC.world_classes(wr, zero))


# ---- the matcher ------------------------------------------------------------------------------------------------------------------
def _entries(c1, rng):
    """votes entries that decode to c1: unknown rows are 0 or a class byte with no votes"""
    n = len(c1)
    count = rng.randint(1, 256, n)
    v = np.where(c1 == NONE, rng.randint(0, 4, n) * (rng.rand(n) < 0.5), (count << 8) | c1).astype(np.uint16)
    assert np.array_equal(WC.decode(v), c1)
    return v


def _setup(lib, dev, d1, c1, n1, map_cap, d2, c2, cap, seed=0):
    """(world, classes, frame descriptors, frame classes) on the device.  Map slots past the descriptors hold copies of row 0 under
    tracks of class 1, frame rows past d2 copies of its row 0 under class 1: a kernel that read them would match them."""
    rng = np.random.RandomState(seed)
    tid_cap = map_cap + 7
    tids = rng.permutation(tid_cap)[:map_cap].astype(np.int32)
    cm = np.full(map_cap, 1, np.uint8)
    cm[:len(c1)] = c1
    votes = np.zeros(tid_cap, np.uint16)
    votes[tids] = _entries(cm, rng)
    w = lib.world_buffers(map_cap, tid_cap, dev)
    full = np.tile(d1[:1] if len(d1) else np.ones((1, 256), np.float32) / 16, (map_cap, 1)).astype(np.float32)
    full[:len(d1)] = d1
    w["desc"].copy_(_t(full, dev))
    w["tid"].copy_(_t(tids, dev))
    w["state"][0] = n1
    classes = lib.world_class_buffers(tid_cap, dev)
    classes["votes"].copy_(_t(votes, dev))
    f = np.tile(d2[:1] if len(d2) else np.ones((1, 256), np.float32) / 16, (cap, 1)).astype(np.float32)
    f[:len(d2)] = d2
    cf = np.full(cap, 1, np.uint8)
    cf[:len(c2)] = c2
    return w, classes, _t(f, dev), _t(cf, dev)


def _class_case(n1, n2, seed):
    """Sign descriptors, three classes plus unknown rows on both sides; three quarters of the frame rows are exact copies of map
    rows, most under the map row's class, every fifth under another; copies of some of those map rows planted 33, 64 and 133 rows
    on (other waves, other strips) under other classes."""
    rng = np.random.RandomState(seed)
    d1, d2 = W.sign_descriptors(seed + 1, n1), W.sign_descriptors(seed + 2, n2)
    c1 = rng.randint(0, 3, n1).astype(np.uint8)
    c1[rng.rand(n1) < 0.1] = NONE
    take = min(n1, n2 - n2 // 4)
    src = rng.permutation(n1)[:take]
    d2[:take] = d1[src]
    c2 = rng.randint(0, 3, n2).astype(np.uint8)
    c2[:take] = c1[src]
    c2[:take:5] = (c2[:take:5] + 1) % 3
    c2[rng.rand(n2) < 0.05] = NONE
    for q, s in enumerate(src[:6]):
        for k, off in enumerate((33, 64, 133)):
            tgt = (int(s) + off) % n1
            if tgt != s and tgt not in src[:6]:
                d1[tgt] = d1[s]
                c1[tgt] = (int(c1[s]) + 1 + (q + k) % 2) % 3 if c1[s] != NONE else k
        lo = (int(s) - 40) % n1                                 # ... and one below it, so that the first index is the wrong one
        if lo < s and lo not in src[:6]:
            d1[lo], c1[lo] = d1[s], (int(c1[s]) + 1) % 3 if c1[s] != NONE else 0
    return d1, c1, d2, c2


def _check(lib, dev, d1, c1, n1, map_cap, d2, c2, n2, cap, mask, what):
    w, classes, f, cf = _setup(lib, dev, d1, c1, n1, map_cap, d2, c2, cap)
    m, n = lib.op_match_world_classes(w, classes, f, cf, _i32(n2, dev), THR, map_keep=mask)
    ref = WC.match_world_classes(d1, n1, c1, np.asarray(f.cpu()), np.asarray(cf.cpu()), n2, THR, mask if mask is not None else WC.FULL_MASK)
    plain = W.match_world(d1, n1, np.asarray(f.cpu()), n2, THR)
    nm = int(n.item())
    print("%s: %d matches (restatement %d; the plain matcher %d)" % (what, nm, ref["n_match"], plain["n_match"]))
    assert nm == ref["n_match"]
    assert np.array_equal(m.cpu().numpy()[:nm], ref["match"][:nm])
    return nm, ref, plain, (w, classes, f, cf)


MATCH_SHAPES = [(1, 1), (33, 1), (63, 65), (129, 32), (129, 33), (4097, 33)]


@pytest.mark.parametrize("n1,n2", MATCH_SHAPES)
def test_match_world_classes_against_restatement(n1, n2):
    from semantic_superpoint_amd import lib
    dev = _dev()
    d1, c1, d2, c2 = _class_case(n1, n2, 7 * n1 + n2)
    mask = lib.class_mask(drop=(2,), n_classes=3)
    assert mask == WC.mask_of(drop=(2,))
    nm, ref, plain, _ = _check(lib, dev, d1, c1, n1, n1, d2, c2, n2, n2, mask, "(%d, %d) class 2 dropped" % (n1, n2))
    nm_all, ref_all, _, _ = _check(lib, dev, d1, c1, n1, n1, d2, c2, n2, n2, None, "(%d, %d) every class" % (n1, n2))
    assert nm_all >= nm
    if n1 >= 63:
        assert 0 < nm_all < plain["n_match"]                                 # the classes decide something
        assert not np.array_equal(ref_all["match"][:nm_all, :2], plain["match"][:nm_all, :2])


def test_match_world_classes_many_strips():
    """32 800 x 40: more than 256 live strips, so the unsplit path with several tiles."""
    from semantic_superpoint_amd import lib
    dev = _dev()
    n1, n2 = 32800, 40
    d1, c1, d2, c2 = _class_case(n1, n2, 5)
    nm, _, plain, _ = _check(lib, dev, d1, c1, n1, n1, d2, c2, n2, n2, lib.class_mask(drop=(2,), n_classes=3), "(32800, 40)")
    assert 0 < nm < plain["n_match"]


def test_clamped_tail_rows_and_a_cap_above_the_count():
    """n_rows below map_cap and no multiple of 32, the last live row of another class than the rest of its wave (the rows past it
    are loaded as its copies: they must carry its class, not their slots'); cap above count2."""
    from semantic_superpoint_amd import lib
    dev = _dev()
    n1, map_cap, n2, cap = 45, 64, 9, 14
    d1, d2 = W.sign_descriptors(21, n1), W.sign_descriptors(22, n2)
    c1, c2 = np.zeros(n1, np.uint8), np.zeros(n2, np.uint8)
    c1[44] = 2
    d2[3], c2[3] = d1[44], 2                                                 # the last live row's point
    d2[5], c2[5] = d1[40], 0
    d2[8], c2[8] = d1[44], 0                                                 # its descriptor under the wave's other class: nothing
    d2[0], c2[0] = d1[0], 1                                                  # row 0's descriptor under the class of the slots past n_rows
    nm, ref, _, _ = _check(lib, dev, d1, c1, n1, map_cap, d2, c2, n2, cap, None, "clamp")
    assert [tuple(r) for r in ref["match"][:nm, :2].astype(int).tolist()] == [(40, 5), (44, 3)]
    c2[n2 - 1] = 2                                                           # the last live frame row against the tail of the frame
    d2[n2 - 1] = d1[44]
    d2[3] = d1[7]
    c2[3] = 0
    nm, ref, _, _ = _check(lib, dev, d1, c1, n1, map_cap, d2, c2, n2, cap, None, "clamp, frame tail")
    assert [tuple(r) for r in ref["match"][:nm, :2].astype(int).tolist()] == [(7, 3), (40, 5), (44, 8)]


def _unit_rows(seed, n):
    rng = np.random.RandomState(seed)
    d = rng.randn(n, 256).astype(np.float32)
    return d / np.linalg.norm(d, axis=1, keepdims=True).astype(np.float32)


@pytest.mark.parametrize("n1,n2,map_cap,cap", [(1, 1, 1, 1), (100, 70, 300, 90), (129, 33, 129, 33), (1500, 700, 2048, 768)])
def test_equal_classes_and_a_full_mask_are_the_plain_matcher(n1, n2, map_cap, cap):
    from semantic_superpoint_amd import lib
    dev = _dev()
    both = _unit_rows(n1 + n2, n1 + n2)                                      # general unit rows: the same chain, the same keys
    d1, d2 = both[:n1], both[n1:]
    k = min(n1, n2) // 2
    if k:
        noisy = d1[:k] + 0.02 * np.random.RandomState(7).randn(k, 256).astype(np.float32)
        d2[:k] = noisy / np.linalg.norm(noisy, axis=1, keepdims=True)
        d2[k // 2] = d2[0]                                                   # frame rows that are copies of each other
    w, classes, f, cf = _setup(lib, dev, d1, np.full(n1, 1, np.uint8), n1, map_cap, d2, np.full(n2, 1, np.uint8), cap)
    c = _i32(n2, dev)
    zeros = lambda: (torch.zeros(cap, 3, device=dev), torch.zeros(1, dtype=torch.int32, device=dev))
    a = lib.op_match_world(w, f, c, THR, out=zeros())
    for mask in (None, lib.class_mask(keep=(1,), n_classes=3)):
        b = lib.op_match_world_classes(w, classes, f, cf, c, THR, map_keep=mask, out=zeros())
        print("(%d, %d): %d matches, plain %d" % (n1, n2, int(b[1]), int(a[1])))
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and int(a[1]) >= k // 2
    cf.fill_(2)                                                              # disjoint classes
    assert int(lib.op_match_world_classes(w, classes, f, cf, c, THR)[1]) == 0
    cf.fill_(1)
    assert int(lib.op_match_world_classes(w, classes, f, cf, c, THR, map_keep=lib.class_mask(drop=(1,), n_classes=3))[1]) == 0
    cf.fill_(NONE)
    classes["votes"].zero_()                                                 # unknown on both sides: no candidate
    assert int(lib.op_match_world_classes(w, classes, f, cf, c, THR)[1]) == 0


def test_empty_sides_repeats_and_map_cap():
    from semantic_superpoint_amd import lib
    dev = _dev()
    n1, n2 = 300, 77
    d1, c1, d2, c2 = _class_case(n1, n2, 3)
    outs = []
    for map_cap in (300, 1000):
        w, classes, f, cf = _setup(lib, dev, d1, c1, n1, map_cap, d2, c2, n2 + 3)
        a = [t.clone() for t in lib.op_match_world_classes(w, classes, f, cf, _i32(n2, dev), THR)]
        b = lib.op_match_world_classes(w, classes, f, cf, _i32(n2, dev), THR)
        nm = int(a[1])
        assert nm > 0 and torch.equal(a[1], b[1]) and torch.equal(a[0][:nm], b[0][:nm])
        outs.append(a[0][:nm])
        assert int(lib.op_match_world_classes(w, classes, f, cf, _i32(0, dev), THR)[1]) == 0      # an empty frame
        w["state"][0] = 0
        assert int(lib.op_match_world_classes(w, classes, f, cf, _i32(n2, dev), THR)[1]) == 0     # an empty map
    assert torch.equal(outs[0], outs[1])


def test_argument_refusals():
    from semantic_superpoint_amd import lib
    dev = _dev()
    w, classes = lib.world_buffers(16, 32, dev), lib.world_class_buffers(32, dev)
    one = _i32(1, dev)
    d, c = torch.zeros(8, 256, device=dev), torch.zeros(8, dtype=torch.uint8, device=dev)
    lm = torch.zeros(4, LR.LANDMARK_WORDS, dtype=torch.float64, device=dev)
    for bad in (lambda: lib.world_class_buffers(0, dev),
                lambda: lib.op_match_world_classes(w, lib.world_class_buffers(16, dev), d, c, one, THR),     # another tid_cap
                lambda: lib.op_match_world_classes(w, {"votes": classes["votes"]}, d, c, one, THR),
                lambda: lib.op_match_world_classes(w, dict(classes, votes=classes["votes"].view(torch.int16)), d, c, one, THR),
                lambda: lib.op_match_world_classes(w, classes, d, c[:7], one, THR),
                lambda: lib.op_match_world_classes(w, classes, d, c.to(torch.int32), one, THR),
                lambda: lib.op_match_world_classes(w, classes, d, c, one, -1.0),
                lambda: lib.op_match_world_classes(w, classes, d, c, one, THR, map_keep=(1, 2, 3)),
                lambda: lib.op_match_world_classes(w, classes, d, c, one.long(), THR),
                lambda: lib.op_match_world_classes(w, classes, torch.zeros(4097, 256, device=dev), torch.zeros(4097, dtype=torch.uint8, device=dev), one, THR),
                lambda: lib.op_world_classes(w, classes, out=torch.zeros(15, dtype=torch.uint8, device=dev)),
                lambda: lib.op_world_classes(w, lib.world_class_buffers(31, dev)),
                lambda: lib.op_track_class_votes(classes, lm[:, :7].contiguous(), one, c, one),
                lambda: lib.op_track_class_votes(classes, lm, one, c.to(torch.int32), one),
                lambda: lib.op_track_class_votes(classes, lm, one.long(), c, one),
                lambda: lib.op_track_class_votes(None, lm, one, c, one)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(RuntimeError):
        lib.world_class_buffers(16, "cpu")
    with pytest.raises(RuntimeError):
        lib.op_match_world_classes(w, classes, d, c.cpu(), one, THR)


# ---- the trackers -----------------------------------------------------------------------------------------------------------------
TRACKER_CAP = 4096
MAP_KEYS = ("X", "desc", "tid", "n_views", "first_frame", "last_frame", "rms", "slot_of_tid", "state")


@contextlib.contextmanager
def _no_host_sync():
    torch.cuda.set_sync_debug_mode("error")
    try:
        yield
    finally:
        torch.cuda.set_sync_debug_mode("default")


def _frame(seq, f, dev):
    xy = seq["pts"][f]
    return (_t(xy.reshape(-1, 2), dev), _i32(xy.shape[0], dev), _t(np.asarray(seq["desc"][f], dtype=np.float32).reshape(-1, 256), dev),
            _t(np.asarray(seq["cls"][f], dtype=np.uint8), dev))


@pytest.mark.parametrize("through", ("PointTracker", "SequenceTracker"))
def test_trackers_in_lockstep(through):
    """The revisit with planted aliases: world_map alone, world_classes="observe", "match" and "match" with class 2 dropped."""
    from semantic_superpoint_amd.export import PointTracker, SequenceTracker
    dev = _dev()
    seq, runs = WC.alias_runs()
    frames = len(seq["pts"])
    kw = dict(geometric_check="fundamental", check_seed=WC.ALIAS_SEED0, intrinsics=tuple(seq["intr"][0]), trajectory_rows=frames + 1,
              world_map="observe", world_cap=TRACKER_CAP)
    net = types.SimpleNamespace(convSout=None, n_classes=WC.N_CLASSES)       # fed through its tracker: only the head's presence is read

    def make(**more):
        if through == "PointTracker":
            top = PointTracker(WC.ALIAS_L, W.NN_THRESH, dev, **kw, **more)
            return top, top
        top = SequenceTracker(net, dev, 0.015, 4, False, W.NN_THRESH, WC.ALIAS_L, **kw, **more)
        return top, top.tracker

    (plain_top, plain), (obs_top, obs) = make(), make(world_classes="observe")
    (mat_top, mat), (drop_top, drop) = make(world_classes="match"), make(world_classes="match", world_drop_classes=WC.ALIAS_DROP)
    assert obs_top.world_classes_device() is None and obs_top.world_map(classes=True)[0].shape == (0, 9)
    wrong = {"plain": 0, "match": 0}
    for f in range(frames):
        frame = _frame(seq, f, dev)
        tids_before = {nm: (tr._world["tid"].cpu().numpy() if tr._world is not None else None) for nm, tr in (("plain", plain), ("match", mat))}
        plain.update_device(*frame)                                          # (a plain tracker ignores cls)
        if f >= 2:                                                           # (the first frames allocate)
            with _no_host_sync():
                for tr in (obs, mat, drop):
                    tr.update_device(*frame)
        else:
            for tr in (obs, mat, drop):
                tr.update_device(*frame)
        gp, go = plain.last_geometry(), obs.last_geometry()
        assert set(gp) == set(go) == set(mat.last_geometry())
        for k in gp:                                                         # observing changes nothing the tracker computed before
            assert torch.equal(gp[k], go[k]), (f, k)
        for a, b in ((plain.trajectory(), obs.trajectory()), (plain_top.world_trajectory(), obs_top.world_trajectory())):
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        assert np.array_equal(plain.get_tracks(1), obs.get_tracks(1))
        for k in MAP_KEYS:
            assert torch.equal(plain_top.world_map_device()[k], obs_top.world_map_device()[k]), (f, k)
        want = runs["observe"]["classes"][f]
        assert np.array_equal(obs_top.world_classes_device().cpu().numpy(), want), f
        for nm, tr, top in (("match", mat, mat_top), ("match-drop", drop, drop_top)):
            ref, g = runs[nm], tr.last_geometry()
            n_m = int(g["world_n_match"])
            state = tr._world["state"].cpu().numpy()
            print("%s frame %d: %d matches (restatement %d), map state %s" % (nm, f, n_m, ref["world_match"][f]["n_match"], state.tolist()))
            assert n_m == ref["world_match"][f]["n_match"]
            assert np.array_equal(g["world_match"][:n_m].cpu().numpy(), ref["world_match"][f]["match"][:n_m]), (nm, f)
            assert int(g["world_status"]) == ref["world"][f]["status"] and int(g["world_n_inliers"]) == ref["world"][f]["n_inliers"]
            assert np.array_equal(state, ref["states"][f]), (nm, f)
            assert np.array_equal(top.world_classes_device().cpu().numpy(), ref["classes"][f]), (nm, f)
        for nm, tr in (("plain", plain), ("match", mat)):                    # joins of different scene points, by the sequence's identities
            g = tr.last_geometry()
            for i, j, _ in g["world_match"][:int(g["world_n_match"])].cpu().numpy():
                wrong[nm] += runs[nm]["scene_of_tid"][int(tids_before[nm][int(i)])] != int(seq["ids"][f][int(j)])
    print("%s: joins of different scene points: plain %d, match %d" % (through, wrong["plain"], wrong["match"]))
    assert wrong["plain"] == len(runs["plain"]["wrong_joins"]) >= 1 and wrong["match"] == 0
    for nm, top in (("observe", obs_top), ("match", mat_top), ("match-drop", drop_top)):
        ref = runs[nm]
        rows, desc = top.world_map(classes=True)
        want_rows, want_desc = W.map_rows(ref["map"])
        assert rows.shape == (want_rows.shape[0], 9) and np.array_equal(rows[:, [0, 4, 6, 7]], want_rows[:, [0, 4, 6, 7]])
        assert np.array_equal(desc, want_desc) and np.array_equal(rows[:, 8], ref["classes"][-1][:rows.shape[0]].astype(np.float64))
        assert np.array_equal(top.world_map()[0], rows[:, :8])
    votes = mat._world_votes["votes"].view(torch.int16)                    # (the same bits; torch reduces int16)
    assert votes.any()
    mat.reset_world_classes()
    assert not votes.any() and bool((mat_top.world_classes_device() == NONE).all())


def test_trackers_refuse():
    from semantic_superpoint_amd.export import PointTracker, SequenceTracker
    dev = _dev()
    k = (300.0, 300.0, 160.0, 120.0)
    ok = dict(geometric_check="fundamental", intrinsics=k, world_map="observe")
    with_head, without = types.SimpleNamespace(convSout=None, n_classes=3), types.SimpleNamespace()
    for make in (lambda **kw: PointTracker(3, 0.7, dev, **kw), lambda **kw: SequenceTracker(with_head, dev, 0.015, 4, False, 0.7, 3, **kw)):
        for kw in (dict(world_classes="observe"), dict(geometric_check="fundamental", intrinsics=k, world_classes="match"),
                   dict(ok, world_classes="always"), dict(ok, world_keep_classes=(1,)), dict(ok, world_classes="observe", world_drop_classes=(1,)),
                   dict(ok, world_classes="match", world_keep_classes=(1,), world_drop_classes=(2,)),
                   dict(ok, world_classes="match", world_keep_classes=(255,))):
            with pytest.raises(ValueError):
                make(**kw)
        t = make(**ok, world_classes="match", world_keep_classes=(0, 2))
        assert t.world_classes_device() is None
        with pytest.raises(ValueError):
            make(**ok).world_map(classes=True)
    with pytest.raises(ValueError):
        SequenceTracker(without, dev, 0.015, 4, False, 0.7, 3, **ok, world_classes="observe")
    t = PointTracker(3, 0.7, dev, **ok, world_classes="observe")
    pts, cnt, desc = torch.zeros(8, 2, dtype=torch.float64, device=dev), _i32(0, dev), torch.zeros(8, 256, device=dev)
    with pytest.raises(ValueError):
        t.update_device(pts, cnt, desc)
    with pytest.raises(ValueError):
        t.update_device(pts, cnt, desc, torch.zeros(8, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError):
        t.update_device(pts, cnt, desc, torch.zeros(7, dtype=torch.uint8, device=dev))
    with pytest.raises(RuntimeError):
        t.update_device(pts, cnt, desc, torch.zeros(8, dtype=torch.uint8))
    with pytest.raises(ValueError):
        t.update(np.zeros((3, 4)), np.zeros((256, 4)))
