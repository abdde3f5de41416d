"""The trajectory evaluation on the device against its numpy restatement tests/traj_eval_ref.py, on the
fixtures of tests/traj_eval_cases.py: every fixture through every operator.  Integer outputs (n_valid, status, valid, f1, the counts,
info) and the selected statistics (min, max, the median's order statistics on the hand-made arrays) equal the restatement's with ==;
a floating output is within 16 times the float64 / longdouble difference of the restatement on that fixture
(traj_eval_cases.WAY_DIFFERENCE, measured without a device), and the test prints how many are bit-equal.  A problem alone equals the
same problem inside a batch of 11, a repeated call equals the first, and evaluate_many equals the single calls, bit for bit."""
import numpy as np
import pytest
import torch

from tests import traj_eval_cases as TC
from tests import traj_eval_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def L():
    from semantic_superpoint_amd import lib
    return lib


def _dev(x, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).to(DEV)


def _run(L, c, mode=None):
    """Every operator on one fixture -> a traj_eval_ref.evaluate-shaped dict of numpy arrays"""
    cap = len(c["table"])
    traj = L.traj_eval_buffers(cap, 1, len(c["lengths"]), c["step"], DEV, n_stat=2 + 2 * len(c["deltas"]))
    traj["lengths"].copy_(torch.tensor(c["lengths"], dtype=torch.float64))
    table, gt, nf = _dev(c["table"]), _dev(c["gt"]), _dev([c["n_frames"]], torch.int32)
    index = None if c["index"] is None else _dev(c["index"], torch.int32)
    out = {}
    sim = L.op_traj_align(table, nf, gt, traj, index, mode or c["mode"])
    out["sim"] = sim[0].cpu().numpy()
    et, er, v = L.op_traj_ape(table, nf, gt, traj, index)
    out["ape"] = (et[0].cpu().numpy(), er[0].cpu().numpy(), v[0].cpu().numpy())
    out["ate"] = L.op_traj_stats(et, v, traj["stats"][0])[0].cpu().numpy()
    out["ape_rot"] = L.op_traj_stats(er, v, traj["stats"][1])[0].cpu().numpy()
    out["rpe"] = {}
    for k, d in enumerate(c["deltas"]):
        rt, rr, rv = L.op_traj_rpe_delta(table, nf, gt, traj, index, d, scale=sim)
        st = L.op_traj_stats(rt, rv, traj["stats"][2 + 2 * k])[0].cpu().numpy()
        sr = L.op_traj_stats(rr, rv, traj["stats"][3 + 2 * k])[0].cpu().numpy()
        out["rpe"][d] = (rt[0].cpu().numpy(), rr[0].cpu().numpy(), rv[0].cpu().numpy(), st, sr)
    seg, summary, info = L.op_traj_rpe_segments(table, nf, gt, traj, index, scale=sim)
    out["dist"], out["seg"], out["summary"], out["info"] = (traj["dist"][0].cpu().numpy(), seg[0].cpu().numpy(), summary[0].cpu().numpy(),
                                                             info[0].cpu().numpy())
    return out


def _integers(ev):
    return [ev["sim"][13:15], ev["ape"][2], ev["info"], ev["seg"][:, :, 0], ev["seg"][:, :, 3], ev["summary"][2::3], ev["ate"][:1],
            ev["ape_rot"][:1]] + [x for d in sorted(ev["rpe"]) for x in (ev["rpe"][d][2], ev["rpe"][d][3][:1], ev["rpe"][d][4][:1])]


@pytest.mark.parametrize("name", list(TC.cases()))
def test_every_operator_on_every_fixture(L, name):
    c = TC.cases()[name]
    want, got = TC.reference(name), _run(L, c)
    for a, b in zip(_integers(want), _integers(got)):
        assert np.array_equal(a, b), name
    fw, fg = TC.flatten(want), TC.flatten(got)
    exact = []
    for k in TC.OUTPUTS:
        diff = float(np.abs(fw[k] - fg[k]).max()) if fw[k].size else 0.0
        print(name, k, "device - restatement", diff, "bound", TC.bound(name, k), "bit-equal", np.array_equal(fw[k], fg[k]))
        exact.append(np.array_equal(fw[k], fg[k]))
        assert diff <= TC.bound(name, k), (name, k, diff, TC.bound(name, k))
    print(name, "bit-equal outputs", sum(exact), "of", len(exact))


@pytest.mark.parametrize("mode", list(R.MODES))
def test_every_alignment_mode(L, mode):
    """The four modes on fixtures with noise, invalid rows and too few frames: the integers equal, the similarity within 16 times the
    difference of the restatement's two ways on that fixture and mode."""
    for name in ("n2", "n3", "n65", "invalid", "mirror", "planar", "collinear", "mode_origin_scale"):
        c = TC.cases()[name]
        got = _run(L, c, mode)["sim"]
        a = R.align(c["table"], c["n_frames"], c["gt"], c["index"], mode)
        b = R.align(c["table"], c["n_frames"], c["gt"], c["index"], mode, way=R.WAY2)
        assert np.array_equal(got[13:15], a[13:15]), (name, mode)
        for sl in (slice(0, 1), slice(1, 10), slice(10, 13), slice(15, 16)):
            bound = 16.0 * float(np.abs(a[sl].astype(np.longdouble) - b[sl]).max())
            diff = float(np.abs(got[sl] - a[sl]).max())
            print(name, mode, "device - restatement", diff, "bound", bound)
            assert diff <= bound, (name, mode, diff, bound)


@pytest.mark.parametrize("name", list(TC.stats_cases()))
def test_stats_on_hand_made_arrays(L, name):
    e, v = TC.stats_cases()[name]
    got = L.op_traj_stats(_dev(e)[None], _dev(v, torch.int32)[None], torch.zeros(1, 8, dtype=torch.float64, device=DEV))[0].cpu().numpy()
    want = R.stats(e, v)
    lo, hi = R.order_statistics(e, v)
    assert got[0] == want[0] and got[4] == want[4] and got[5] == want[5]
    if lo is not None:
        assert got[6] == 0.5 * (lo + hi) == np.median(e[v != 0])
    for sl, d in zip((slice(1, 7), slice(7, 8)), TC.STATS_WAY_DIFFERENCE[name]):
        print(name, "device - restatement", np.abs(got[sl] - want[sl]).max(), "bound", 16.0 * d, "bit-equal", np.array_equal(got, want))
        assert np.abs(got[sl] - want[sl]).max() <= 16.0 * d


def _evaluator(c, **kw):
    from semantic_superpoint_amd.trajectory_evaluation import TrajectoryEvaluator
    return TrajectoryEvaluator(c["gt"], c["index"], capacity=len(c["table"]), device=DEV, align=c["mode"], lengths=c["lengths"],
                               step=c["step"], deltas=c["deltas"], **kw)


def _snapshot(out):
    flat = [out[k] for k in ("sim", "err_t", "err_r", "valid", "dist", "seg", "summary", "info", "stats")]
    flat += [x for d in sorted(out["rpe"]) for x in out["rpe"][d]]
    return [x.cpu().numpy().copy() for x in flat]


def test_alone_in_a_batch_of_11_and_repeated(L):
    """A problem's result does not depend on its batch or on the run: the fixture alone, as problem 4 of 11 different tables with a
    ground truth each, and alone again, bit for bit."""
    c = TC.cases()["n257"]
    traj1 = L.traj_eval_buffers(257, 1, len(c["lengths"]), c["step"], DEV)
    traj11 = L.traj_eval_buffers(257, 11, len(c["lengths"]), c["step"], DEV)
    for t in (traj1, traj11):
        t["lengths"].copy_(torch.tensor(c["lengths"], dtype=torch.float64))
    tables = np.stack([TC.estimate(c["gt"], 0.5 + k, TC.ROT_A, noise=0.01 * k, seed=k) for k in range(11)])
    gts = np.stack([np.roll(c["gt"], 3 * k, axis=0) for k in range(11)])
    tables[4], gts[4] = c["table"], c["gt"]
    nfs = np.array([257 - 20 * k for k in range(11)], np.int32)
    nfs[4] = 257

    def run(traj, table, nf, gt):
        table, nf, gt = _dev(table), _dev(nf, torch.int32), _dev(gt)
        sim = L.op_traj_align(table, nf, gt, traj).clone()
        ape = [x.clone() for x in L.op_traj_ape(table, nf, gt, traj)]
        st = L.op_traj_stats(ape[0], ape[2], traj["stats"][0]).clone()
        rpe = [x.clone() for x in L.op_traj_rpe_delta(table, nf, gt, traj, scale=sim)]
        seg = [x.clone() for x in L.op_traj_rpe_segments(table, nf, gt, traj, scale=sim)]
        return [x.cpu().numpy() for x in [sim, st, traj["dist"].clone()] + ape + rpe + seg]

    alone = run(traj1, c["table"], [257], c["gt"])
    batch = run(traj11, tables, nfs, gts)
    again = run(traj1, c["table"], [257], c["gt"])
    for a, b, r in zip(alone, batch, again):
        assert np.array_equal(a[0], b[4], equal_nan=True) and np.array_equal(a, r, equal_nan=True)
    want = TC.reference("n257")
    assert np.array_equal(alone[0][0][13:15], want["sim"][13:15])


def test_shared_ground_truth_equals_a_copy_per_problem(L):
    c = TC.cases()["permuted"]
    traj = L.traj_eval_buffers(257, 3, len(c["lengths"]), c["step"], DEV)
    traj["lengths"].copy_(torch.tensor(c["lengths"], dtype=torch.float64))
    tables = _dev(np.stack([c["table"], TC.cases()["n257"]["table"], c["table"]]))
    nf, index = _dev([257, 200, 100], torch.int32), _dev(c["index"], torch.int32)
    shared, own = _dev(c["gt"]), _dev(np.stack([c["gt"]] * 3))
    outs = []
    for gt in (shared, own):
        sim = L.op_traj_align(tables, nf, gt, traj, index).clone()
        outs.append([sim] + [x.clone() for x in L.op_traj_ape(tables, nf, gt, traj, index)]
                    + [x.clone() for x in L.op_traj_rpe_segments(tables, nf, gt, traj, index, scale=sim)])
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert outs[0][0][:, 13].tolist() == [257.0, 200.0, 100.0]


def test_evaluate_many_equals_five_evaluate_calls_and_result_names_the_numbers():
    c = TC.cases()["n65"]
    ev = _evaluator(c)
    tables = np.stack([c["table"]] + [TC.estimate(c["gt"][:65], 1.0 + k, TC.ROT_A, noise=0.02 * k, seed=k) for k in range(1, 5)])
    nfs = [65, 64, 30, 2, 65]
    single, results = [], []
    for t, n in zip(tables, nfs):
        single.append(_snapshot(ev.evaluate(_dev(t), n)))
        results.append(ev.result())
    many = _snapshot(ev.evaluate_many(_dev(tables), nfs))
    many_results = ev.result()
    for k in range(5):
        for i, (a, b) in enumerate(zip(single[k], many)):   # (the problem is the second axis of stats, entry 8, the first elsewhere)
            assert np.array_equal(a[:, 0] if i == 8 else a[0], b[:, k] if i == 8 else b[k], equal_nan=True), (k, i)
        assert str(results[k]) == str(many_results[k])
    want = TC.reference("n65")
    r = results[0]
    assert r["n_valid"] == 65 and r["status"] == 0 and r["scale"] == many[0][0][0] and r["align"] == "sim3"
    assert r["ate_rmse"] == single[0][8][0, 0, 1] and abs(r["ate_rmse"] - want["ate"][1]) <= TC.bound("n65", "ate")
    assert abs(r["ate_median"] - want["ate"][6]) <= TC.bound("n65", "ate") and set(r["rpe"]) == {1, 7}
    assert abs(r["rpe"][7]["trans_rmse"] - want["rpe"][7][3][1]) <= TC.bound("n65", "rpe_t_stats")
    assert r["kitti_segments"] == want["info"][0] and abs(r["kitti_t_rel_percent"] - 100 * want["summary"][0]) <= 100 * TC.bound("n65", "summary_t")
    assert [row[1] for row in r["kitti_lengths"]] == [int(v) for v in want["summary"][2::3]]
    assert results[3]["status"] == 1 and results[3]["ate_rmse"] == 0.0


def test_kitti_numbers_of_the_analytic_case():
    c = TC.cases()["kitti_scale"]
    ev = _evaluator(c)
    ev.evaluate(_dev(c["table"]), 1000)
    r = ev.result()
    assert r["status"] == 2 and r["kitti_segments"] == TC.reference("kitti_scale")["info"][0]
    for (Lm, n, t_percent, r_deg), want_n in zip(r["kitti_lengths"], TC.reference("kitti_scale")["summary"][2::3]):
        assert n == want_n and abs(t_percent - 10.0 * (Lm + 1) / Lm) <= 1e-9 and r_deg == 0.0


def test_evaluate_queues_without_a_host_synchronisation():
    c = TC.cases()["n257"]
    ev = _evaluator(c)
    table = _dev(c["table"])
    ev.evaluate(table, 257)   # (the buffers of the batch size are allocated at its first use)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ev.evaluate(table, 200)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert ev.result()["n_valid"] == 200


# ---- the trackers ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("through", ("PointTracker", "SequenceTracker"))
def test_trackers_in_lockstep(through):
    """Three trackers over world_ref's revisit (13 frames): trajectory_eval None, "observe", and "observe" with eval_table="world".
    The first two are bit-identical in every last_geometry() key they share, trajectory(), world_trajectory(), get_tracks and the
    map; the steps from the third frame on run under torch's sync debug mode "error".  Every row of each log equals, with ==, the
    restatement applied to the table the device held at that frame; and the trajectory log follows the log of the restated tracker's
    table: the device's centres are within REVISIT_BOUND of the restated ones (section 29), the alignment is a least-squares
    projection, so an aligned residual moves by at most twice the scaled displacement of a centre, and rmse, mean and max with it."""
    from semantic_superpoint_amd.export import PointTracker, SequenceTracker
    from tests import world_ref as W
    from tests.test_gpu_world import TRACKER_CAP, _frame, _no_host_sync
    dev = torch.device("cuda:0")
    seq, runs = W.revisit_runs()
    frames, gt = len(seq["pts"]), TC.sequence_truth(seq)
    kw = dict(geometric_check="fundamental", check_seed=W.REVISIT_SEED0, intrinsics=tuple(seq["intr"][0]), trajectory_rows=frames + 1,
              world_map="observe", world_cap=TRACKER_CAP)

    def make(**more):
        if through == "PointTracker":
            top = PointTracker(W.REVISIT_L, W.NN_THRESH, dev, **kw, **more)
            return top, top
        top = SequenceTracker(None, dev, 0.015, 4, False, W.NN_THRESH, W.REVISIT_L, **kw, **more)   # fed through its tracker: no network
        return top, top.tracker

    (plain_top, plain), (obs_top, obs) = make(), make(ground_truth=gt, trajectory_eval="observe")
    wld_top, wld = make(ground_truth=gt, trajectory_eval="observe", eval_table="world", eval_align="se3")
    assert obs_top.trajectory_eval_log().shape == (0, 8) and obs_top.evaluate_trajectory() is None
    want_obs, want_wld = np.zeros((frames, 8)), np.zeros((frames, 8))
    for f in range(frames):
        frame = _frame(seq, f, dev)
        plain.update_device(*frame)
        if f >= 2:                                                       # (the first frames allocate)
            with _no_host_sync():
                obs.update_device(*frame)
                wld.update_device(*frame)
        else:
            obs.update_device(*frame)
            wld.update_device(*frame)
        gp, go = plain.last_geometry(), obs.last_geometry()
        assert set(go) == set(gp) | {"trajectory_eval"} == set(wld.last_geometry())
        for k in gp:
            assert torch.equal(gp[k], go[k]), (f, k)
        for a, b in ((plain.trajectory(), obs.trajectory()), (plain.world_trajectory(), obs.world_trajectory())):
            assert (a is None and b is None) or (torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]))
        assert np.array_equal(plain.get_tracks(1), obs.get_tracks(1))
        for k, v in plain.world_map_device().items():
            assert not torch.is_tensor(v) or torch.equal(v, obs.world_map_device()[k]), (f, k)
        want_obs[f] = TC.observe_row(plain.trajectory()[0].cpu().numpy(), f + 1, gt)
        if plain.world_trajectory() is not None:
            want_wld[f] = TC.observe_row(plain.world_trajectory()[0].cpu().numpy(), f + 1, gt, "se3")
        assert np.array_equal(go["trajectory_eval"].cpu().numpy(), want_obs[f]), f
    log, log_w = obs_top.trajectory_eval_log(), wld_top.trajectory_eval_log()
    assert log.shape == (frames, 8) and np.array_equal(log, want_obs) and np.array_equal(log_w, want_wld)
    assert log[-1, 4] >= 3 and log[-1, 5] == 0
    restated = TC.observe_log(runs["observe"]["table"], frames, gt)
    assert np.array_equal(restated[:, 4:6], log[:, 4:6])
    scale = np.abs(log[:, 3]).max()
    print("log against the restated tracker's", np.abs(log[:, :3] - restated[:, :3]).max(), "bound", 2 * scale * W.REVISIT_BOUND)
    assert np.abs(log[:, :3] - restated[:, :3]).max() <= 2 * scale * W.REVISIT_BOUND
    # on demand: the same numbers as the log's last row, and the other tables
    r = obs_top.evaluate_trajectory()
    assert (r["ate_rmse"], r["ate_mean"], r["ate_max"], r["scale"], r["n_valid"], r["status"]) == tuple(log[-1, :4]) + (int(log[-1, 4]), 0)
    w = obs_top.evaluate_trajectory("world", align="se3")
    assert (w["ate_rmse"], w["n_valid"]) == (log_w[-1, 0], int(log_w[-1, 4]))
    assert obs_top.evaluate_trajectory("absolute") is None
    with pytest.raises(ValueError, match="which"):
        obs_top.evaluate_trajectory("best")
    with pytest.raises(ValueError, match="ground_truth"):
        plain_top.evaluate_trajectory()
    assert plain_top.trajectory_eval_log().shape == (0, 8)
