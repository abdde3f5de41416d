"""World map upkeep on the device: lib.op_world_upkeep against tests/world_upkeep_ref.py with == on the nine
store arrays, the report and the totals: only copies, integers and one gated decision are involved, and no fixture's decision lies
near its threshold (tests/test_world_upkeep_cpu.py).  Hand-made cases, random maps at the row counts where the kernels change
path, the radix select on keys that differ in one digit only, determinism, the trackers in lockstep on the revisit and the long
run, and the argument refusals."""
import contextlib

import numpy as np
import pytest
import torch

from tests import world_ref as W
from tests import world_upkeep_cases as K
from tests import world_upkeep_ref as U

pytestmark = pytest.mark.gpu

STORE = ("X", "desc", "tid", "n_views", "first_frame", "last_frame", "rms", "slot_of_tid", "state")


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _device_map(lib, dev, w, map_cap=None):
    """The numpy map w as lib.world_buffers of map_cap (default: its own) slots; the slots past its own hold a pattern."""
    cap0 = w["map_cap"]
    d = lib.world_buffers(map_cap or cap0, w["tid_cap"], dev)
    for c in STORE:
        if c in ("slot_of_tid", "state"):
            d[c].copy_(_t(w[c], dev))
        else:
            d[c].fill_(7)
            d[c][:cap0] = _t(w[c], dev)
    return d


def _call(lib, dev, case, world=None, upkeep=None, map_cap=None):
    """lib.op_world_upkeep on the case; returns (the device map, the upkeep buffers)."""
    d = world if world is not None else _device_map(lib, dev, case["world"], map_cap)
    up = upkeep if upkeep is not None else lib.world_upkeep_buffers(d["map_cap"], dev)
    i32 = lambda v: torch.tensor([v], dtype=torch.int32, device=dev)
    lib.op_world_upkeep(d, _t(case["match"], dev), i32(case["n_match"]), _t(case["landmarks"], dev), i32(case["n_landmarks"]),
                        _t(case["pts_new"], dev), i32(case["count_new"]), _t(case["table"], dev), case["n_frames"], _t(case["k"], dev), up,
                        **case["params"])
    return d, up


def _same_map(d, ref, what, live_only=False):
    n = W.n_rows_of(ref)
    for c in STORE:
        got, want = d[c].cpu().numpy(), ref[c]
        if c not in ("slot_of_tid", "state"):
            got, want = (got[:n], want[:n]) if live_only else (got[:ref["map_cap"]], want)
        assert np.array_equal(got, want), (what, c)


@pytest.mark.parametrize("name", sorted(K.HAND_MADE))
def test_hand_made_cases(name):
    from semantic_superpoint_amd import lib
    dev = _dev()
    case = K.hand_made(name)
    ref, report, _ = K.run_ref(case)
    d, up = _call(lib, dev, case)
    assert up["report"].cpu().numpy().tolist() == report.tolist(), name
    _same_map(d, ref, name)
    assert up["totals"].cpu().numpy().tolist() == [int(report[1]), int(report[2]), int(report[3]), 1]


@pytest.mark.parametrize("n_rows", (1, 63, 64, 65, 1024, 1025, 4097))
@pytest.mark.parametrize("room", (0, 5))
def test_row_counts(n_rows, room):
    """Planted merges, culls and an eviction at row counts that straddle a wave, the select's 1024 threads and the move kernels'
    strides, in a map with room to spare and in a full one."""
    from semantic_superpoint_amd import lib
    dev = _dev()
    case = K.random_case(100 + n_rows, n_rows, n_rows + room)
    ref, report, info = K.run_ref(case)
    assert not info["ambiguous"]
    d, up = _call(lib, dev, case)
    print("n_rows %d: report %s" % (n_rows, report.tolist()))
    assert up["report"].cpu().numpy().tolist() == report.tolist()
    _same_map(d, ref, n_rows)
    if n_rows >= 63:
        assert report[U.MERGED] > 0 and report[U.CULLED] > 0 and report[U.EVICTED] > 0


def test_full_map_half_dying():
    """65 536 rows, half of them culled: every strip of the move kernels, once."""
    from semantic_superpoint_amd import lib
    dev = _dev()
    case = K.random_case(5, 65536, 65536, dying=0.55)
    ref, report, info = K.run_ref(case)
    assert 30000 < report[U.AFTER] < 36000 and not info["ambiguous"]
    d, up = _call(lib, dev, case)
    assert up["report"].cpu().numpy().tolist() == report.tolist()
    _same_map(d, ref, "full")


@pytest.mark.parametrize("digit", ("lowest", "highest", "middle"))
def test_selection_by_one_digit(digit):
    """The radix select where the keys differ in one 8-bit digit only: the slot's low byte (equal views and ages, 256 rows), the
    views (equal ages; the slot only breaks no tie), and one byte of last_frame."""
    from semantic_superpoint_amd import lib
    dev = _dev()
    n = 256 if digit == "lowest" else 200
    f = 1 << 16
    rng = np.random.RandomState(17)
    w = K.base_map(n, n, tid_cap=1024, views=3, last=4)
    if digit == "highest":
        w["n_views"][:n] = rng.permutation(n) + 1
    if digit == "middle":
        w["last_frame"][:n] = 256 * rng.permutation(n)
    w["last_frame"][[3, 50]] = f                                 # two protected rows
    case = K._case(w, dict(high_water=n - 1, low_water=n - 101), n_frames=f + 1, table=np.zeros((f + 1, 16)))
    ref, report, info = K.run_ref(case)
    assert report.tolist() == [n, 0, 0, 101, n - 101, 1, 0, 0] and info["dead"][[3, 50]].tolist() == [0, 0]
    d, up = _call(lib, dev, case)
    assert up["report"].cpu().numpy().tolist() == report.tolist()
    _same_map(d, ref, digit)


def test_deterministic_and_cap_independent():
    from semantic_superpoint_amd import lib
    dev = _dev()
    case = K.random_case(3, 3000, 3000)
    ref, report, _ = K.run_ref(case)
    a, up_a = _call(lib, dev, case)
    b, up_b = _call(lib, dev, case)
    for c in STORE:
        assert torch.equal(a[c], b[c]), c
    assert torch.equal(up_a["report"], up_b["report"])
    big, up_c = _call(lib, dev, case, map_cap=8192)
    assert torch.equal(up_c["report"], up_a["report"])
    _same_map(big, ref, "map_cap 8192", live_only=True)
    # a second call on the result, without matches and without the eviction, finds nothing left to do; the totals add up
    again = dict(case, n_match=0, params=dict(case["params"], high_water=-1))
    want, _ = U.upkeep(ref, *[again[k] for k in ("match", "n_match", "landmarks", "n_landmarks", "pts_new", "count_new", "table", "n_frames",
                                                  "k")], **again["params"])
    _call(lib, dev, again, world=a, upkeep=up_a)
    assert up_a["report"].cpu().numpy().tolist() == want.tolist() == [report[U.AFTER], 0, 0, 0, report[U.AFTER], 0, 0, 0]
    _same_map(a, ref, "second call")
    assert up_a["totals"].cpu().numpy().tolist() == [int(report[1]), int(report[2]), int(report[3]), 2]


# ---- the trackers --------------------------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("which", ("revisit", "long_run"))
@pytest.mark.parametrize("through", ("PointTracker", "SequenceTracker"))
def test_trackers_in_lockstep(through, which):
    """Three trackers over one sequence: without upkeep, with upkeep whose every phase is off, with upkeep.  The first two agree bit
    for bit in everything the first computes; the third equals the restated tracker."""
    from semantic_superpoint_amd.export import PointTracker, SequenceTracker
    dev = _dev()
    if which == "revisit":
        (seq, runs), Lm, seed0, cap, bound = U.revisit_runs(), W.REVISIT_L, W.REVISIT_SEED0, 4096, W.REVISIT_BOUND
    else:
        (seq, runs), Lm, seed0, cap, bound = U.long_runs(), U.LONG_RUN_L, U.LONG_RUN_SEED0, U.LONG_RUN_WORLD_CAP, U.LONG_RUN_BOUND
    frames = len(seq["pts"])
    kw = dict(geometric_check="fundamental", check_seed=seed0, intrinsics=tuple(seq["intr"][0]), trajectory_rows=frames + 1,
              world_map="observe", world_cap=cap)

    def make(**more):
        if through == "PointTracker":
            top = PointTracker(Lm, W.NN_THRESH, dev, **kw, **more)
            return top, top
        top = SequenceTracker(None, dev, 0.015, 4, False, W.NN_THRESH, Lm, **kw, **more)     # fed through its tracker: no network
        return top, top.tracker

    (plain_top, plain), (on_top, on) = make(), make(world_upkeep="on")
    off_top, off = make(world_upkeep="on", world_merge=False, world_cull_age=-1, world_high_water=-1)
    ref, ref_plain = runs["on"], runs["plain"]
    assert on_top.world_upkeep_report().tolist() == [0, 0, 0, 0]
    for f in range(frames):
        frame = _frame(seq, f, dev)
        plain.update_device(*frame)
        if f >= 2:                                                       # (the first frames allocate)
            with _no_host_sync():
                off.update_device(*frame)
                on.update_device(*frame)
        else:
            off.update_device(*frame)
            on.update_device(*frame)
        gp, gf, gn = plain.last_geometry(), off.last_geometry(), on.last_geometry()
        assert set(gf) - set(gp) == ({"world_upkeep_report"} if f >= 1 else set()) and set(gn) == set(gf)
        for k in gp:                                                     # upkeep with every phase off changes nothing
            assert torch.equal(gp[k], gf[k]), (f, k)
        for a, b in zip(plain.trajectory() + plain.world_trajectory(), off.trajectory() + off.world_trajectory()):
            assert torch.equal(a, b), f
        assert np.array_equal(plain.get_tracks(1), off.get_tracks(1))
        if f >= 1:
            a, b = plain_top.landmarks_device(), off_top.landmarks_device()
            assert torch.equal(a[1], b[1]) and torch.equal(a[0][:int(a[1])], b[0][:int(b[1])])
        for c in STORE:
            assert torch.equal(plain.world_map_device()[c], off.world_map_device()[c]), (f, c)
        # the tracker with upkeep against the restatement: the report, the map's state and rows, the world pose of the frame
        want = ref["reports"][f]
        if want is None:
            assert "world_upkeep_report" not in gn
        else:
            assert gn["world_upkeep_report"].cpu().numpy().tolist() == want.tolist(), f
            n_rows = int(ref_plain["states"][f][W.N_ROWS])
            assert gf["world_upkeep_report"].cpu().numpy().tolist() == [n_rows, 0, 0, 0, n_rows, 0, 0, int(want[U.SKIPPED])], f
        assert np.array_equal(on.world_map_device()["state"].cpu().numpy(), ref["states"][f]), f
        rows, desc = on_top.world_map()
        want_rows, want_desc = ref["maps"][f]
        assert rows.shape == want_rows.shape and np.array_equal(rows[:, [0, 4, 6, 7]], want_rows[:, [0, 4, 6, 7]]), f
        assert np.array_equal(desc, want_desc), f
        assert int(gn["world_status"]) == ref["world"][f]["status"] and int(gn["world_n_inliers"]) == ref["world"][f]["n_inliers"], f
    table = on.trajectory()[0][:frames].cpu().numpy()
    wtable = on.world_trajectory()[0][:frames].cpu().numpy()
    ok = np.array([r["status"] == 0 for r in ref["world"]])
    want_c = np.array([np.asarray(r["C"], dtype=np.float64).reshape(3) for r in ref["world"]])
    worst = max(float(np.abs(table[:, 9:12] - ref["table"][:, 9:12]).max()), float(np.abs(wtable[ok, 9:12] - want_c[ok]).max()))
    print("%s %s: centres against the restatement %.3e (bound %.3e)" % (through, which, worst, bound))
    assert worst <= bound
    totals = on_top.world_upkeep_report()
    calls = [r for r in ref["reports"] if r is not None]
    assert totals.tolist() == [sum(int(r[1]) for r in calls), sum(int(r[2]) for r in calls), sum(int(r[3]) for r in calls), len(calls)]
    assert totals[0] > 0 if which == "revisit" else totals[2] > 0
    if which == "long_run":
        assert int(on.world_map_device()["state"][W.DROP_FULL]) == 0 and int(plain.world_map_device()["state"][W.DROP_FULL]) > 0


def test_argument_refusals():
    from semantic_superpoint_amd import lib
    from semantic_superpoint_amd.export import PointTracker, SequenceTracker
    dev = _dev()
    k = (300.0, 300.0, 160.0, 120.0)
    ok = dict(geometric_check="fundamental", intrinsics=k, world_map="observe", world_cap=256)
    for make in (lambda **kw: PointTracker(3, 0.7, dev, **kw), lambda **kw: SequenceTracker(None, dev, 0.015, 4, False, 0.7, 3, **kw)):
        for kw in (dict(geometric_check="fundamental", intrinsics=k),                      # no world_map
                   dict(ok, world_low_water=200, world_high_water=100), dict(ok, world_high_water=257),
                   dict(ok, world_low_water=-1), dict(ok, world_merge_thresh=-1.0), dict(ok, world_merge_thresh=float("nan"))):
            with pytest.raises(ValueError):
                make(world_upkeep="on", **kw)
        with pytest.raises(ValueError):
            make(world_upkeep="always", **ok)
        t = make(world_upkeep="on", **ok)
        assert t.world_upkeep_report().tolist() == [0, 0, 0, 0]
    case = K.hand_made("mixed")
    d = _device_map(lib, dev, case["world"])
    before = {c: d[c].clone() for c in STORE}
    up = lib.world_upkeep_buffers(d["map_cap"], dev)
    i32 = lambda v: torch.tensor([v], dtype=torch.int32, device=dev)
    args = [_t(case["match"], dev), i32(case["n_match"]), _t(case["landmarks"], dev), i32(case["n_landmarks"]), _t(case["pts_new"], dev),
            i32(case["count_new"]), _t(case["table"], dev), case["n_frames"], _t(case["k"], dev)]
    for params in (dict(high_water=3, low_water=4), dict(high_water=d["map_cap"] + 1), dict(merge=True, merge_thresh=-1.0)):
        with pytest.raises(ValueError):
            lib.op_world_upkeep(d, *args, up, **dict(case["params"], **params))
    small = dict(up, ws=up["ws"][:up["ws"].numel() // 2])
    with pytest.raises(ValueError, match="ws"):
        lib.op_world_upkeep(d, *args, small, **case["params"])
    with pytest.raises(ValueError):
        lib.op_world_upkeep(d, *args, dict(up, report=up["report"][:4]), **case["params"])
    with pytest.raises(ValueError):
        lib.op_world_upkeep(d, *args[:8], _t(case["k"][:3], dev), up, **case["params"])
    with pytest.raises(ValueError):
        lib.world_upkeep_buffers(0, dev)
    for c in STORE:                                                      # a refused call touches nothing
        assert torch.equal(d[c], before[c]), c
