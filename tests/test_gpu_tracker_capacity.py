"""GPU: a PointTracker's results do not depend on its capacity or on the frame at which its buffers grow.

Three trackers with equal options are fed one sequence (tests/tracker_capacity_cases.py): `tight` (every frame padded to 64 rows above
its count: capacity 1024 throughout), `wide` (2048 rows from the first frame) and `growing` (as tight, but frame g has 1025 rows and
a later frame 2049: capacity 1024 -> 2048 -> 4096).  After every frame they must agree, with == and no tolerance, on the track table,
the three trajectories, every entry of last_geometry() (per-match arrays over the common rows, zeros behind them), the landmarks, the
bundle adjustment, the world map and its upkeep report, the loop edges, get_tracks, get_matches and track_points.  A frame that does
not grow the buffers runs without a host synchronisation.  The sequences and options are those of the stages' own tests.
lib.op_pose_chain with two different capacities is compared with its run at equal capacities (bytes) and with pose_ref.chain_step."""
import contextlib

import numpy as np
import pytest
import torch

from tests import tracker_capacity_cases as K
from tests.test_gpu_point_classes import front  # noqa: F401  (the fixture: a front end whose keypoints spread over classes)

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@contextlib.contextmanager
def _no_host_sync(on):
    if on:
        torch.cuda.set_sync_debug_mode("error")
    try:
        yield
    finally:
        torch.cuda.set_sync_debug_mode("default")


def _pair(problems, what, a, b, cap_a, cap_b):
    """One entry of two trackers: equal, or recorded in `problems`."""
    if a is None or b is None:
        if a is not b:
            problems.append(what + ("None in one tracker only",))
        return
    if isinstance(a, (tuple, list)):
        if len(a) != len(b):
            problems.append(what + ("lengths",))
            return
        for k, (x, y) in enumerate(zip(a, b)):
            _pair(problems, what + (k,), x, y, cap_a, cap_b)
        return
    if isinstance(a, np.ndarray):
        if not (a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()):
            problems.append(what + ("numpy",))
        return
    got = K.slice_to_common(a, b, cap_a, cap_b)
    if got is None:
        problems.append(what + ("shapes %s %s" % (list(a.shape), list(b.shape)),))
        return
    x, y, rest = got
    if not K.same_bytes(x, y):
        problems.append(what + ("differs",))
    if not all(K.all_zero(r) for r in rest):
        problems.append(what + ("not zero behind the common rows",))


def _table_rows(tr):
    t = tr.table
    n = int(t["state"][0].item())
    return [t["state"]] + [t[k][:n] for k in ("ids", "tid", "score")]


def _outputs(tr, landmarks, ba_rows):
    """Everything the trackers must agree on, by name."""
    out = {"table": _table_rows(tr), "trajectory": tr.trajectory(), "absolute_trajectory": tr.absolute_trajectory(),
           "world_trajectory": tr.world_trajectory(), "world_map": tr.world_map(), "world_upkeep_report": tr.world_upkeep_report(),
           "loop_edges_device": tr.loop_edges_device(), "loop_closures": tr.loop_closures(), "get_matches": tr.get_matches()}
    tracks = tr.get_tracks(1)
    out["get_tracks"] = (tracks, tr.get_tracks(2), tr.get_tracks(tr.maxl))
    out["track_points"] = tr.track_points(tracks)
    if landmarks:
        lms, n = tr.landmarks_device()
        out["landmarks_device"] = (lms[:int(n.item())] if lms.shape[0] else lms, n)
    ba = tr.bundle_adjusted()
    out["bundle_adjusted"] = None if ba is None else (ba[0], ba[1][:ba_rows], ba[2][:ba_rows], ba[3])
    return out


def _lockstep(make, frames, g, g2=None, landmarks=True, every=0):
    """tight, wide and growing trackers over `frames` (tight device tuples).  every: bundle_every (0: no bundle adjustment), to know
    how many rows of X and rms the newest adjustment aligned with the table."""
    rows, caps = K.plans([int(fr[1].item()) for fr in frames], g, g2)
    names = ("tight", "wide", "growing")
    trackers = {nm: make() for nm in names}
    problems, ba_rows = [], 0
    for f, frame in enumerate(frames):
        for nm in names:
            grows = f == 0 or caps[nm][f] != caps[nm][f - 1]
            with _no_host_sync(f >= 2 and not grows):     # (the first frames allocate; a growing frame may)
                trackers[nm].update_device(*K.padded(frame, rows[nm][f]))
            assert trackers[nm]._cap == caps[nm][f], (nm, f, trackers[nm]._cap)
        if every and f + 1 >= 2 and (f + 1) % every == 0:
            ba_rows = int(trackers["tight"].table["state"][0].item())
        outs = {nm: _outputs(trackers[nm], landmarks and f >= 1, ba_rows) for nm in names}
        geo = {nm: trackers[nm].last_geometry() for nm in names}
        for nm in names[1:]:
            ca, cb = caps["tight"][f], caps[nm][f]
            for key in outs["tight"]:
                _pair(problems, (f, nm, key), outs["tight"][key], outs[nm][key], ca, cb)
            if geo["tight"] is None or geo[nm] is None or set(geo["tight"]) != set(geo[nm]):
                if geo["tight"] is not geo[nm]:
                    problems.append((f, nm, "last_geometry keys"))
                continue
            for key in sorted(geo["tight"]):
                _pair(problems, (f, nm, "last_geometry", key), geo["tight"][key], geo[nm][key], ca, cb)
    assert caps["growing"][-1] > caps["growing"][0] and caps["tight"][-1] == K.FIRST_CAP
    for p in problems:
        print("disagrees:", p)
    assert not problems, "%d disagreements, the first: %s" % (len(problems), problems[0])
    return trackers


def _device_frames(seq, desc_of, dev):
    out = []
    for f in range(len(seq["pts"])):
        xy = np.ascontiguousarray(seq["pts"][f]).reshape(-1, 2)
        out.append((torch.from_numpy(xy).to(dev), torch.tensor([xy.shape[0]], dtype=torch.int32, device=dev),
                    torch.from_numpy(np.ascontiguousarray(desc_of(f), dtype=np.float32).reshape(-1, 256)).to(dev)))
    return out


# ---- absolute pose over the broken sequence (tests/test_gpu_pnp.py) ---------------------------------------------------------------
@pytest.mark.parametrize("g", (1, 2, 3, 4))     # before any landmark, the two frames of the broken pair, the frame after it
@pytest.mark.parametrize("mode", ("observe", "repair"))
def test_absolute_pose_over_the_broken_sequence(mode, g):
    from semantic_superpoint_amd.export import PointTracker
    from tests import pnp_ref as R
    from tests import pose_ref as P
    from tests import test_gpu_pnp as T
    dev = _dev()
    seq = R.broken_sequence()
    assert R.BROKEN[1] == 2 and len(seq["pts"]) == 5
    frames = [T._frame(f, dev) for f in range(len(seq["pts"]))]
    kw = dict(geometric_check="fundamental", check_seed=P.case(R.BROKEN[0])["seeds"][0] - 1, intrinsics=tuple(seq["intr"][0]),
              trajectory_rows=len(frames) + 1, absolute_pose=mode)
    tr = _lockstep(lambda: PointTracker(T.MAX_LENGTH, T.NN_THRESH, dev, **kw), frames, g)
    for t in tr.values():     # what the sequence is for, in every tracker: the frames after the broken pair get an absolute pose
        assert t.absolute_trajectory()[0][:5, 14].tolist() == ([1, 1, 0, 0, 1] if mode == "observe" else [1, 1, 0, 0, 0])
        assert t.trajectory()[0][:5, 14].tolist() == ([3, 2, 0, 3, 2] if mode == "observe" else [3, 2, 0, 4, 4])


# ---- every stage over the closed circuit (tests/test_gpu_loop.py) -----------------------------------------------------------------
def _circuit(dev, **more):
    from tests import loop_ref as G
    from tests import world_ref as W
    from semantic_superpoint_amd.export import PointTracker
    seq = G.circuit_sequence(G.CIRCUIT_DEVICE_SEED)
    frames = _device_frames(seq, lambda f: seq["desc"][f], dev)
    kw = dict(geometric_check="fundamental", check_seed=G.CIRCUIT_SEED0, intrinsics=tuple(seq["intr"][0]), trajectory_rows=len(frames) + 1,
              absolute_pose="repair", bundle_adjust="apply", world_map="relocalise", world_cap=4096, loop_closure="observe",
              loop_min_gap=G.CIRCUIT_GAP, loop_min_inliers=G.CIRCUIT_MIN_INLIERS, loop_cooldown=32, **more)
    return frames, (lambda: PointTracker(G.CIRCUIT_L, W.NN_THRESH, dev, **kw))


def test_every_stage_over_the_closed_circuit():
    """Growth at frame 2 and at the frame at which the loop edge is accepted (found by a tracker of its own first)."""
    dev = _dev()
    frames, make = _circuit(dev)
    scout = make()
    for frame in frames:
        scout.update_device(*frame)
    closures = scout.loop_closures()
    print("the loop edge is accepted at frame", closures[:, 0].tolist())
    assert closures.shape[0] >= 1 and int(closures[0, 0]) > 2
    tr = _lockstep(make, frames, 2, int(closures[0, 0]), every=1)
    for t in tr.values():
        assert np.array_equal(t.loop_closures(), closures) and t.bundle_adjusted() is not None


def test_bundle_every_two_growth_on_a_frame_without_an_adjustment():
    """bundle_every=2 adjusts after the frames 1, 3, 5, ...; the buffers grow at frames 4 and 6, on which no adjustment runs: the newest
    one must still be there."""
    dev = _dev()
    frames, make = _circuit(dev, bundle_every=2)
    tr = _lockstep(make, frames[:10], 4, 6, every=2)
    assert all(t.bundle_adjusted() is not None for t in tr.values())


# ---- world map upkeep (tests/test_gpu_world_upkeep.py) ----------------------------------------------------------------------------
def test_world_upkeep_over_the_revisit():
    from semantic_superpoint_amd.export import PointTracker
    from tests import world_ref as W
    from tests import world_upkeep_ref as U
    dev = _dev()
    seq, _ = U.revisit_runs()
    frames = _device_frames(seq, lambda f: seq["desc"][f], dev)
    kw = dict(geometric_check="fundamental", check_seed=W.REVISIT_SEED0, intrinsics=tuple(seq["intr"][0]), trajectory_rows=len(frames) + 1,
              world_map="observe", world_cap=4096, world_upkeep="on")
    tr = _lockstep(lambda: PointTracker(W.REVISIT_L, W.NN_THRESH, dev, **kw), frames, len(frames) // 2)
    assert tr["growing"].world_upkeep_report()[0] > 0            # the revisit does merge rows


# ---- the planar sequence under geometric_check="auto" (tests/test_gpu_pose_h.py) --------------------------------------------------
def test_planar_sequence_under_auto():
    from semantic_superpoint_amd.export import PointTracker
    from tests import pose_h_ref as H
    from tests import test_gpu_pose_h as T
    dev = _dev()
    seq = H.scene("planar5")
    frames = T._frames(seq, dev)
    kw = dict(geometric_check="auto", check_seed=H.SEQ_SEED - 1, intrinsics=tuple(seq["intr"][0]), trajectory_rows=8)
    tr = _lockstep(lambda: PointTracker(T.MAX_LENGTH, T.NN_THRESH, dev, **kw), frames, 2)
    assert all(list(t.trajectory()[0][:5, 14].cpu().numpy()) == [3, 3, 2, 0, 0] for t in tr.values())


# ---- a class-consistent sequence (tests/test_gpu_point_classes.py) ----------------------------------------------------------------
def test_class_consistent_sequence(front):  # noqa: F811
    from semantic_superpoint_amd.export import PointTracker, SequenceTracker
    agent, dev = front["agent"], front["dev"]
    seq = SequenceTracker(agent.net, dev, agent.conf_thresh, agent.nms_dist, False, agent.nn_thresh, 3, class_consistent=True)
    frames = []
    for im in front["frames"]:
        o = seq.describe(im)
        n = int(o["count"][0])
        assert n >= 30
        frames.append((o["pts"][0, :n, :2].to(torch.float64).contiguous(), o["count"][0:1].clone(), o["desc"][0, :n].clone(),
                       o["cls"][0, :n].clone()))
    assert len(set(frames[0][3].cpu().tolist())) >= 3
    tr = _lockstep(lambda: PointTracker(3, agent.nn_thresh, dev, class_consistent=True), frames, 2, landmarks=False)
    assert tr["growing"].get_tracks(2).shape[0] > 0


# ---- lib.op_pose_chain with two different capacities ------------------------------------------------------------------------------
def test_pose_chain_with_unequal_capacities():
    """The previous pair's arrays at cap_prev = cap + 37 and at cap - 5 (its 48 matches fit), decoy rows behind n_match_prev that
    look like matches of points in front of both cameras.  The device's row and state are byte-equal to its run at equal capacities.
    pose_ref.chain_step at those capacities, given the device's own poses, gives byte-equal rows at the three capacity pairs too.
    The kernel adds the shared depths per thread and then over the workgroup (block_sum<256>), chain_step in ascending order: with
    its two sums taken in the kernel's order (tracker_capacity_cases.chain_step_block_order) the restatement's row and state are the
    device's, byte for byte; in ascending order they are within pose_ref.TOLERANCE, the measured spread of the restatement."""
    from semantic_superpoint_amd import lib as L
    from tests import pose_ref as P
    from tests.test_gpu_pose import POSE_KEYS, _chain_scenarios, _t
    dev = _dev()
    c = P.case("seq5")
    seq = c["seq"]
    geo_in = _chain_scenarios()["plain"]
    n_p, n, cap = len(seq["pairs"]), seq["pts"][0].shape[0], 64
    ref = [P.two_view_pose(c["ransac"][k]["F"], geo_in[k][0], geo_in[k][1], geo_in[k][2], seq["pairs"][k]["m"], seq["pairs"][k]["intr"])
           for k in range(n_p)]

    def poses(cp):
        """op_two_view_pose of every pair in arrays of cp rows, and its match rows; rows past n are copies of the first rows."""
        pts = np.zeros((n_p + 1, cp, 2))
        match = np.zeros((n_p, cp, 3), dtype=np.float32)
        mask = np.zeros((n_p, cp), dtype=np.uint8)
        for f in range(n_p + 1):
            pts[f, :n] = seq["pts"][f]
        for k in range(n_p):
            match[k, :n], mask[k, :n] = seq["pairs"][k]["match"], geo_in[k][0]
            match[k, n:] = np.resize(seq["pairs"][k]["match"], (cp - n, 3))
        geo = {"F": _t(np.stack([r["F"] for r in c["ransac"]]), dev), "mask": _t(mask, dev),
               "n_inliers": _t(np.array([g[1] for g in geo_in], dtype=np.int32), dev),
               "status": _t(np.array([g[2] for g in geo_in], dtype=np.int32), dev)}
        pd, md = _t(pts, dev), _t(match, dev)
        nm = _t(np.full(n_p, n, dtype=np.int32), dev)
        o = L.op_two_view_pose(geo, pd[:n_p], pd[1:], md, nm, _t(np.stack([pr["intr"] for pr in seq["pairs"]]), dev))
        o = {k: o[k].clone() for k in POSE_KEYS}
        o["front"][:, n:] = 1                    # decoys: the rows behind n_match look like points in front of both cameras
        o["depth"][:, n:] = 7.0
        return o, md, nm

    sl = lambda d, k: {key: d[key][k:k + 1] for key in POSE_KEYS}  # noqa: E731
    runs = {}
    for cp in (cap, cap + 37, cap - 5):
        (o, md, nm), (op, mdp, nmp) = poses(cap), poses(cp)
        for key in ("R", "t", "status", "front", "depth"):
            assert torch.equal(o[key][:, :n] if key in ("front", "depth") else o[key], op[key][:, :n] if key in ("front", "depth") else op[key])
        state, table = L.pose_state(dev), L.pose_table(n_p + 2, dev)
        for k in range(n_p):                     # the previous pair at cp rows, the new pair at cap rows
            L.op_pose_chain(sl(op, k - 1) if k else None, sl(o, k), mdp[k - 1:k] if k else None, md[k:k + 1], nmp[k - 1:k] if k else None,
                            nm[k:k + 1], state, table)
        runs[cp] = (table.cpu().numpy(), state.cpu().numpy())
        # the restatements at these capacities, given the device's own poses: chain_step (ascending sums) and the kernel's order
        host = lambda d, k: {key: d[key][k].cpu().numpy() for key in ("front", "depth", "status", "R", "t")}  # noqa: E731
        rows = {"ascending": np.zeros((n_p, P.ROW_WORDS)), "block": np.zeros((n_p, P.ROW_WORDS))}
        st = {"ascending": P.new_state(), "block": P.new_state()}
        for k in range(n_p):
            mp = mdp[k - 1].cpu().numpy() if k else None
            args = (host(op, k - 1) if k else None, host(o, k), mp, md[k].cpu().numpy(), n, n)
            rows["ascending"][k], st["ascending"] = P.chain_step(*args, st["ascending"], cp, cap)
            rows["block"][k], st["block"] = K.chain_step_block_order(*args, st["block"], cp, cap)
        runs[cp] += (rows["block"], P.state_words(st["block"]), rows["ascending"], P.state_words(st["ascending"]))
    base = runs[cap]
    assert list(base[0][:n_p, 14]) == [2, 0, 0, 0] and (base[0][1:n_p, 13] == seq["n_in"]).all()
    for cp in (cap + 37, cap - 5):
        got = runs[cp]
        assert got[0].tobytes() == base[0].tobytes() and got[1].tobytes() == base[1].tobytes(), cp      # device: bytes
        assert got[2].tobytes() == base[2].tobytes() and got[3].tobytes() == base[3].tobytes(), cp      # restatement: bytes
    for cp, (rows, st, blk_rows, blk_st, asc_rows, asc_st) in runs.items():
        worst = max(float(np.abs(rows[:n_p] - asc_rows).max()), float(np.abs(st - asc_st).max()))
        block = max(float(np.abs(rows[:n_p] - blk_rows).max()), float(np.abs(st - blk_st).max()))
        print("cap_prev %d: device against chain_step in the kernel's order of addition %.3e, in ascending order %.3e (pose_ref.TOLERANCE %.3e)"
              % (cp, block, worst, P.TOLERANCE))
        assert rows[:n_p].tobytes() == blk_rows.tobytes() and st.tobytes() == blk_st.tobytes(), cp      # the row and the state: bytes
        assert np.array_equal(rows[:n_p, 13:15], asc_rows[:, 13:15]) and worst <= P.TOLERANCE
