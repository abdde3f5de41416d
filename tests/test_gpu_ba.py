"""Windowed bundle adjustment on the device: ssp_bundle_adjust and ssp_ba_apply against their numpy
restatement (tests/ba_ref.py), their independence of row_cap and repetition, and the trackers that run them.

status, n_obs, rows used, accepted steps and refused solves are compared for equality.  Tolerance of the cameras, the points, the
rms and the two costs (ba_ref.TOLERANCE, relative to max(1, |value|)): measured, not chosen - 16 times the largest difference
between the restatement in float64 and in numpy.longdouble over the compared problems; tests/test_ba_cpu.py repeats the
measurement.  Every comparison prints what the device showed, and whether it came out bit-equal, before it asserts."""
import contextlib

import numpy as np
import pytest
import torch

from tests import ba_ref as B
from tests import landmarks_ref as R
from tests import pose_ref as P

pytestmark = pytest.mark.gpu

JUNK = 7          # an id (a valid point of the oldest frame) in the table rows past n_rows: they must not be read into results
SENTINEL = -77.0  # what rms holds before a call


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _table(pr, row_cap, dev, n_rows=None):
    n, L = pr["ids"].shape
    ids = np.full((row_cap, L), JUNK, dtype=np.int32)
    ids[:n] = pr["ids"]
    state = np.array([n if n_rows is None else n_rows, pr["tracks"].track_count] + list(pr["counts"]), dtype=np.int32)
    return {"ids": _t(ids, dev), "state": _t(state, dev), "L": L, "point_cap": pr["point_cap"], "row_cap": row_cap}


def _rows(pr, row_cap, dev, status=None):
    """X and status of the problem's triangulation in arrays of row_cap rows; the rows past the table's carry status 0 and a
    point, which nothing may read."""
    n = pr["ids"].shape[0]
    X = np.full((row_cap, 3), 5.0)
    st = np.zeros(row_cap, dtype=np.int32)
    X[:n], st[:n] = pr["rows"]["X"], pr["rows"]["status"] if status is None else status
    return {"X": _t(X, dev), "status": _t(st, dev)}, X


def _run(pr, iterations=B.ITERATIONS, row_cap=None, n_rows=None, cams=None, status=None, out=None):
    from semantic_superpoint_amd import lib
    dev = _dev()
    n = pr["ids"].shape[0]
    row_cap = max(n, 1) if row_cap is None else row_cap
    rows, X_in = _rows(pr, row_cap, dev, status)
    out = lib.ba_buffers(pr["L"], row_cap, dev) if out is None else out
    out["rms"].fill_(SENTINEL)
    got = lib.op_bundle_adjust(_table(pr, row_cap, dev, n_rows), _t(pr["pts"], dev), pr["first_slot"],
                               _t(pr["cams"] if cams is None else cams, dev), rows, iterations, out=out)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in got.items()}
    used = n if n_rows is None else n_rows
    assert np.array_equal(got["X"][used:], X_in[used:])                 # rows at or past n_rows are copies ...
    assert (got["rms"][used:] == 0.0).all()                             # ... and carry no error
    return {"cams": got["cams"], "X": got["X"][:n], "rms": got["rms"][:n], "info": got["info"]}


def _compare(got, ref, what):
    worst = 0.0
    for x, y in ((got["cams"], ref["cams"]), (got["X"], ref["X"]), (got["rms"], ref["rms"]), (got["info"][1:3], ref["info"][1:3])):
        if y.size:
            worst = max(worst, float((np.abs(x - y) / np.maximum(1.0, np.abs(y))).max()))
    bits = all(np.array_equal(got[k], ref[k]) for k in ("cams", "X", "rms", "info"))
    print("%s: info %s (restatement %s), worst difference %.3e (tolerance %.3e)%s"
          % (what, got["info"].tolist(), ref["info"].tolist(), worst, B.TOLERANCE, ", bit-equal" if bits else ""))
    for k in (0, 3, 4, 5, 6):
        assert got["info"][k] == ref["info"][k], (what, k)
    assert worst <= B.TOLERANCE, (what, worst)
    if got["info"][5] == ref["info"][5]:
        assert got["info"][7] == ref["info"][7], what                   # lambda is a function of the decisions alone


@pytest.mark.parametrize("name", B.COMPARED)
def test_against_the_restatement(name):
    pr = B.problem(name)
    if name == "long16":
        assert pr["L"] == 16                                            # the full 96 x 96 system
    if name == "big":
        assert pr["ids"].shape[0] > 2048                                # nine tiles: the partials cross workgroups
    if name == "mixed48":
        assert pr["L"] == 2                                             # one free camera with 5 unknowns
    if name in B.SCENARIOS:
        assert (pr["cams"][:, 16] == 0.0).any()                         # invalid views: held identity blocks
    ref, _ = B.solved(name)
    got = _run(pr)
    _compare(got, ref, name)
    assert ref["info"][0] == B.ADJUSTED
    if name in B.NOISE_FREE:
        ex, ec, rms = B.truth_error(name, got)
        print("%s: |X - truth| %.3e, |C - truth| %.3e, rms %.3e" % (name, ex, ec, rms))
        assert ex <= B.TRUTH_BOUND_X and ec <= B.TRUTH_BOUND_C and rms <= B.TRUTH_BOUND_RMS
    if name in B.CHAINS:
        before, after = B.chain_errors(name, got)
        print("%s: centre error %.3f -> %.3f" % (name, before, after))
        assert after < 0.5 * before


@pytest.mark.parametrize("name", B.FIXTURES + B.CHAINS[:1])
def test_one_iteration(name):
    """One linearisation, one solve, one back-substitution: pure linear algebra, which is where a wrong sum shows."""
    ref, _ = B.solved(name, 1)
    _compare(_run(B.problem(name), iterations=1), ref, name + " (1 iteration)")


@pytest.mark.parametrize("scenario", B.SCENARIOS)
@pytest.mark.parametrize("per_frame", (False, True))
def test_scenarios_through_the_operators(scenario, per_frame):
    """map window, triangulate, adjust on the device, with shared and with per-frame intrinsics."""
    from semantic_superpoint_amd import lib
    dev = _dev()
    pr = B.problem(scenario)
    fx, n, table = R.scenario_inputs(scenario)
    L = pr["L"]
    row_cap = pr["ids"].shape[0]
    state = lib.pose_state(dev)
    state[0] = min(n, table.shape[0])
    k = fx["seq"]["intr"][:1]
    cams = lib.op_map_window(state, _t(table, dev), _t(np.repeat(k, L, axis=0) if per_frame else k, dev), L, n_frames=n)
    tb, pts = _table(pr, row_cap, dev), _t(pr["pts"], dev)
    rows = lib.op_triangulate_tracks(tb, pts, pr["first_slot"], cams)
    got = lib.op_bundle_adjust(tb, pts, pr["first_slot"], cams, rows)
    torch.cuda.synchronize()
    assert np.array_equal(cams.cpu().numpy(), pr["cams"]) and np.array_equal(rows["status"].cpu().numpy(), pr["rows"]["status"])
    ref = B.adjust(pr["ids"], pr["counts"], pr["pts"], pr["first_slot"], pr["cams"], rows["X"].cpu().numpy(), pr["rows"]["status"])
    _compare({k: v.cpu().numpy() for k, v in got.items()}, ref, "%s, %s intrinsics" % (scenario, "per-frame" if per_frame else "shared"))
    invalid = pr["cams"][:, 16] == 0.0
    assert (got["cams"].cpu().numpy()[invalid] == 0.0).all()


def test_nothing_to_adjust():
    pr = B.problem("seq5_late")
    n = pr["ids"].shape[0]
    one = pr["cams"].copy()
    one[1:] = 0.0
    cases = (("n_rows 0", dict(n_rows=0), pr["cams"], np.zeros(n, dtype=np.int64) + 1),
             ("one valid view", dict(cams=one), one, None),
             ("no row with status 0", dict(status=np.full(n, 2, dtype=np.int32)), pr["cams"], np.full(n, 2)))
    for what, kw, cams, status in cases:
        got = _run(pr, **kw)
        print(what, got["info"].tolist())
        assert got["info"][0] == B.NOTHING and got["info"][5] == 0 and got["info"][7] == B.LAMBDA0, what
        assert np.array_equal(got["cams"], cams) and np.array_equal(got["X"], pr["rows"]["X"]), what
        if status is not None:
            assert got["info"][3] == 0 and got["info"][4] == 0 and (got["rms"] == 0.0).all(), what
        else:
            ref = B.adjust(pr["ids"], pr["counts"], pr["pts"], pr["first_slot"], one, pr["rows"]["X"], pr["rows"]["status"])
            assert ref["info"][0] == B.NOTHING
            _compare(got, ref, what)


def test_no_step_accepted():
    """A valid view no track sees: its pivot is refused in every iteration, lambda climbs to its cap, the outputs are copies."""
    un = B.unobserved_problem()
    ref = B.adjust(un["ids"], un["counts"], un["pts"], un["first_slot"], un["cams"], un["rows"]["X"], un["rows"]["status"])
    got = _run(un)
    _compare(got, ref, "a valid view no track sees")
    assert got["info"][0] == B.NO_STEP and got["info"][7] == B.LAMBDA_MAX
    assert np.array_equal(got["cams"], un["cams"]) and np.array_equal(got["X"], un["rows"]["X"])


@pytest.mark.parametrize("name", ("seq5_late", "big"))
def test_row_cap_and_repetition_change_nothing(name):
    from semantic_superpoint_amd import lib
    pr = B.problem(name)
    n = pr["ids"].shape[0]
    a = _run(pr)
    wide = 2 * n + 391
    out = lib.ba_buffers(pr["L"], wide, _dev())
    b = _run(pr, row_cap=wide, out=out)
    c = _run(pr, row_cap=wide, out=out)                                 # the same buffers again: nothing is left over
    for k in ("cams", "X", "rms", "info"):
        assert np.array_equal(a[k], b[k]), (name, k, "row_cap")
        assert np.array_equal(b[k], c[k]), (name, k, "repeated")


def test_argument_checks():
    from semantic_superpoint_amd import lib
    dev = _dev()
    pr = B.problem("seq3")
    n, L = pr["ids"].shape
    tb, pts, cams = _table(pr, n, dev), _t(pr["pts"], dev), _t(pr["cams"], dev)
    rows, _ = _rows(pr, n, dev)
    out = lib.ba_buffers(L, n, dev)
    for bad in (0, B.MAX_ITERATIONS + 1):
        with pytest.raises(ValueError):
            lib.op_bundle_adjust(tb, pts, pr["first_slot"], cams, rows, iterations=bad, out=out)
    with pytest.raises(ValueError):
        lib.op_bundle_adjust(tb, pts, L, cams, rows, out=out)
    with pytest.raises(ValueError):
        lib.op_bundle_adjust(tb, pts, 0, cams[:, :19].contiguous(), rows, out=out)
    with pytest.raises(ValueError):
        lib.op_bundle_adjust(tb, pts, 0, cams, {"X": rows["X"]}, out=out)
    with pytest.raises(ValueError):
        lib.op_bundle_adjust(tb, pts, 0, cams, {"X": rows["X"], "status": rows["status"].to(torch.int64)}, out=out)
    with pytest.raises(ValueError):
        lib.op_bundle_adjust(tb, pts, 0, cams, rows, out=dict(out, ws=out["ws"][:64]))
    with pytest.raises(ValueError):
        lib.op_bundle_adjust(tb, pts, 0, cams, rows, out=dict(out, X=rows["X"]))
    with pytest.raises(ValueError):
        lib.op_bundle_adjust(tb, pts, 0, cams, rows, out={"cams": out["cams"]})
    with pytest.raises((ValueError, RuntimeError)):
        lib.op_bundle_adjust(tb, pts.cpu(), 0, cams, rows, out=out)
    adjusted = {"info": out["info"], "cams": out["cams"]}
    with pytest.raises(ValueError):
        lib.op_ba_apply(adjusted, lib.pose_state(dev, 2), lib.pose_table(4, dev), L)
    with pytest.raises(ValueError):
        lib.op_ba_apply(adjusted, lib.pose_state(dev), lib.pose_table(4, dev), L + 1)
    with pytest.raises(ValueError):
        lib.op_ba_apply({"info": out["info"]}, lib.pose_state(dev), lib.pose_table(4, dev), L)
    with pytest.raises(ValueError):
        lib.op_ba_apply(adjusted, lib.pose_state(dev), lib.pose_table(4, dev), L, n_frames=-2)


def _apply_cases():
    """(info, cams, state, table, n_frames) of sequences of one window length: two adjusted chains, one with a status that is not
    0, one whose table is full, one whose state counts fewer frames than the caller."""
    out = []
    for name, variant in (("chain41", "plain"), ("chain44", "plain"), ("chain42", "status"), ("chain43", "full"), ("chain45", "behind")):
        pr = B.problem(name)
        res, _ = B.solved(name)
        info = np.asarray(res["info"], dtype=np.float64).copy()
        state = np.zeros(P.STATE_WORDS)
        state[0], state[1] = pr["n_frames"], 1.0
        table = pr["table"].copy()
        if variant == "status":
            info[0] = B.NO_STEP
        if variant == "full":
            table[pr["n_frames"]:] = 0.0
        if variant == "behind":
            state[0] = pr["n_frames"] - 1
        out.append((info, np.asarray(res["cams"], dtype=np.float64), state, table, variant))
    return out


def test_apply_on_several_sequences():
    from semantic_superpoint_amd import lib
    dev = _dev()
    cases = _apply_cases()
    n, L = B.problem("chain41")["n_frames"], B.CHAIN_L
    for capacity in (n + 3, n):                                          # a table with room, a full table
        info = np.stack([c[0] for c in cases])
        cams = np.stack([c[1] for c in cases])
        state = np.stack([c[2] for c in cases])
        table = np.stack([c[3][:capacity] for c in cases])
        st, tb = _t(state, dev), _t(table, dev)
        lib.op_ba_apply({"info": _t(info, dev), "cams": _t(cams, dev)}, st, tb, L, n_frames=n)
        torch.cuda.synchronize()
        st, tb = st.cpu().numpy(), tb.cpu().numpy()
        for q, c in enumerate(cases):
            want_state, want_table = B.apply(c[0], c[1], c[2], c[3][:capacity], L, n_frames=n)
            assert np.array_equal(st[q], want_state), (capacity, c[4])
            assert np.array_equal(tb[q], want_table), (capacity, c[4])
            changed = not np.array_equal(tb[q], table[q])
            assert changed == (c[4] != "status"), (capacity, c[4])
            if c[4] == "plain":
                assert (tb[q][1:n, 14].astype(np.int64) & B.FLAG_ADJUSTED).all() and not int(tb[q][0, 14]) & B.FLAG_ADJUSTED
                assert np.array_equal(st[q] != state[q], want_state != state[q])
                assert (st[q, 2:11] != state[q, 2:11]).any() == (capacity > n)       # a full table leaves the state alone


# ---- the trackers --------------------------------------------------------------------------------------------------------------
NN_THRESH = 0.7
TRACKED_CHAIN = 44


@contextlib.contextmanager
def _no_host_sync():
    torch.cuda.set_sync_debug_mode("error")
    try:
        yield
    finally:
        torch.cuda.set_sync_debug_mode("default")


def _frames(dev):
    """The frames of a noisy chain as update_device takes them: one random unit descriptor per point id."""
    seq = B.problem("chain%d" % TRACKED_CHAIN)["seq"]
    n = seq["pts"][0].shape[0]
    d = np.random.RandomState(78).randn(n, 256)
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    return seq, [(_t(seq["pts"][f], dev), torch.tensor([n], dtype=torch.int32, device=dev), _t(d[seq["ids"][f]], dev))
                 for f in range(len(seq["pts"]))]


@pytest.mark.parametrize("through", ("PointTracker", "SequenceTracker"))
def test_trackers_observe_and_apply(through):
    """Four trackers in lockstep on a noisy chain: plain, "observe", "apply", and a plain one whose trajectory the test itself
    adjusts with the operators after every frame."""
    from semantic_superpoint_amd import lib
    from semantic_superpoint_amd.export import PointTracker, SequenceTracker
    from tests import pnp_ref
    dev = _dev()
    seq, frames = _frames(dev)
    Lw = B.CHAIN_L
    kw = dict(geometric_check="fundamental", check_seed=B.CHAIN_SEED0, intrinsics=tuple(seq["intr"][0]), trajectory_rows=len(frames) + 1)

    def make(**more):
        if through == "PointTracker":
            top = PointTracker(Lw, NN_THRESH, dev, **kw, **more)
            return top, top
        top = SequenceTracker(None, dev, 0.015, 4, False, NN_THRESH, Lw, **kw, **more)           # fed through its tracker: no network
        return top, top.tracker

    (plain_top, plain), (obs_top, obs), (app_top, app), (_, hand) = (make(), make(bundle_adjust="observe"), make(bundle_adjust="apply"),
                                                                     make())
    assert plain_top.bundle_adjusted() is None and obs_top.bundle_adjusted() is None
    k1 = _t(seq["intr"][:1], dev)

    def by_hand(tr, apply):
        cams = lib.op_map_window(tr._traj_state, tr._traj_table, k1, Lw, n_frames=tr._frames)
        rows = lib.op_triangulate_tracks(tr._table, tr._pts, tr._frames % Lw, cams)
        res = lib.op_bundle_adjust(tr._table, tr._pts, tr._frames % Lw, cams, rows)
        if apply:
            lib.op_ba_apply(res, tr._traj_state, tr._traj_table, Lw, n_frames=tr._frames)
        return res

    for f, frame in enumerate(frames):
        plain.update_device(*frame)
        hand.update_device(*frame)
        if f >= 2:                                                       # (the first frames allocate)
            with _no_host_sync():
                obs.update_device(*frame)
                app.update_device(*frame)
        else:
            obs.update_device(*frame)
            app.update_device(*frame)
        gp, go, ga = plain.last_geometry(), obs.last_geometry(), app.last_geometry()
        assert "ba_info" not in gp and set(go) == set(ga) == set(gp) | {"ba_info"}
        for k in gp:                                                     # observing changes nothing the plain tracker computes
            assert torch.equal(gp[k], go[k]), (f, k)
        assert torch.equal(plain.trajectory()[0], obs.trajectory()[0]) and torch.equal(plain._traj_state, obs._traj_state)
        assert np.array_equal(plain.get_tracks(1), obs.get_tracks(1)) and np.array_equal(plain.get_tracks(1), app.get_tracks(1))
        if f == 0:
            assert obs_top.bundle_adjusted() is None and float(go["ba_info"][0]) == lib.BA_NOTHING
            continue
        a, b = plain_top.landmarks_device(), obs_top.landmarks_device()
        assert torch.equal(a[1], b[1]) and torch.equal(a[0][:int(a[1])], b[0][:int(b[1])])
        # the operators' result, bit for bit
        want_obs, want_app = by_hand(plain, False), by_hand(hand, True)
        for top, want, g in ((obs_top, want_obs, go), (app_top, want_app, ga)):
            got = dict(zip(lib.BA_KEYS, top.bundle_adjusted()))
            for k in lib.BA_KEYS:
                assert torch.equal(got[k], want[k]), (f, k)
            assert torch.equal(g["ba_info"], want["info"])
        assert torch.equal(app.trajectory()[0], hand.trajectory()[0]) and torch.equal(app._traj_state, hand._traj_state), f
        info = want_app["info"].tolist()
        print("%s frame %d: info %s" % (through, f, info))
        flags = app.trajectory()[0][:f + 1, 14].to(torch.int64).tolist()
        if info[0] == lib.BA_ADJUSTED:
            assert flags[f] & lib.POSE_FLAG_ADJUSTED and not flags[0] & lib.POSE_FLAG_ADJUSTED, (f, flags)
        assert not any(int(v) & lib.POSE_FLAG_ADJUSTED for v in plain.trajectory()[0][:, 14].tolist())
    n = len(frames)
    err_plain = pnp_ref.sequence_centre_error(seq, plain.trajectory()[0][:n].cpu().numpy())
    err_app = pnp_ref.sequence_centre_error(seq, app.trajectory()[0][:n].cpu().numpy())
    print("%s: centre error %.3f first baselines plain, %.3f applied" % (through, err_plain, err_app))
    assert all(int(v) & lib.POSE_FLAG_ADJUSTED for v in app.trajectory()[0][1:n, 14].tolist())
    assert err_app < 0.5 * err_plain


def test_trackers_refuse_what_cannot_be_adjusted():
    from semantic_superpoint_amd.export import PointTracker, SequenceTracker
    dev = _dev()
    a, b = (300.0, 300.0, 160.0, 120.0), (310.0, 300.0, 160.0, 120.0)
    for make in (lambda **kw: PointTracker(3, NN_THRESH, dev, **kw), lambda **kw: SequenceTracker(None, dev, 0.015, 4, False, NN_THRESH, 3, **kw)):
        for kw in (dict(), dict(geometric_check="fundamental"), dict(geometric_check="homography"),
                   dict(geometric_check="fundamental", intrinsics=(a, b)),
                   dict(geometric_check="fundamental", intrinsics=a, bundle_iterations=0),
                   dict(geometric_check="fundamental", intrinsics=a, bundle_iterations=17),
                   dict(geometric_check="fundamental", intrinsics=a, bundle_every=0),
                   dict(geometric_check="fundamental", intrinsics=a, landmark_params=(1, 1.0, 2.0))):
            with pytest.raises(ValueError):
                make(bundle_adjust="observe", **kw)
        with pytest.raises(ValueError):
            make(geometric_check="fundamental", intrinsics=a, bundle_adjust="always")
        t = make(geometric_check="fundamental", intrinsics=(a, a), bundle_adjust="apply", bundle_every=2)
        assert t.bundle_adjusted() is None
