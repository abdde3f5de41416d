"""The trajectory evaluation without a device: the numpy restatement tests/traj_eval_ref.py against the
textbook SVD form of Umeyama's alignment and against scipy, the analytic KITTI cases whose truth is known without any code, the
invariances of the metrics, the margins of the fixtures' decisions, the measured float64 / longdouble difference that bounds the GPU
tests, the pose-file readers and the time-stamp association, and the Python argument errors that need no device."""
import numpy as np
import pytest
import torch

from tests import traj_eval_cases as TC
from tests import traj_eval_ref as R

EPS = float(np.finfo(np.float64).eps)
ALIGNABLE = [n for n, c in TC.cases().items() if c["mode"] in ("sim3", "se3") and c["status"] == R.OK]


def _centres(c):
    valid, g = R.frames(c["table"], c["n_frames"], c["gt"], c["index"])
    return c["table"][valid, 9:12], c["gt"].reshape(-1, 3, 4)[g[valid], :, 3]


def _rotation_bound(p, q):
    """Both forms are backward stable, so they differ by the conditioning of the problem times a few dozen roundings: the rotation
    that maximises tr(R^T H) moves by about eps * sigma_1 / min over pairs (sigma_i + sigma_j) under a rounding of H, the third
    singular value entering with the sign of det H.  256 covers the 3x3 products, the eight Jacobi sweeps and the SVD's own error."""
    dp, dq = p - p.mean(axis=0), q - q.mean(axis=0)
    H = dq.T @ dp
    sv = np.linalg.svd(H, compute_uv=False)
    s3 = sv[2] * np.sign(np.linalg.det(H))
    return 256.0 * EPS * sv[0] / (sv[1] + s3)


@pytest.mark.parametrize("name", ALIGNABLE)
def test_alignment_equals_the_textbook_svd_form(name):
    c = TC.cases()[name]
    p, q = _centres(c)
    sim = R.align(c["table"], c["n_frames"], c["gt"], c["index"], c["mode"])
    assert sim[14] == R.OK and sim[13] == len(p)
    s, Rm, t = R.umeyama_svd(p, q, with_scale=c["mode"] == "sim3")
    bound = _rotation_bound(p, q)
    got = sim[1:10].reshape(3, 3)
    print(name, "R", np.abs(got - Rm).max(), "s", abs(sim[0] / s - 1), "bound", bound)
    assert np.abs(got - Rm).max() <= bound
    assert abs(np.linalg.det(got) - 1.0) <= 64 * EPS and np.abs(got @ got.T - np.eye(3)).max() <= 64 * EPS
    assert abs(sim[0] / s - 1.0) <= bound
    extent = np.abs(q).max() + s * np.abs(p).max()
    assert np.abs(sim[10:13] - t).max() <= bound * extent
    assert abs(sim[15] - ((p - p.mean(axis=0)) ** 2).sum() / len(p)) <= 64 * EPS * sim[15]


@pytest.mark.parametrize("name", ALIGNABLE)
def test_rotation_equals_scipy_align_vectors(name):
    Rotation = pytest.importorskip("scipy.spatial.transform").Rotation
    c = TC.cases()[name]
    p, q = _centres(c)
    sim = R.align(c["table"], c["n_frames"], c["gt"], c["index"], c["mode"])
    rot, _ = Rotation.align_vectors(q - q.mean(axis=0), p - p.mean(axis=0))
    assert np.abs(sim[1:10].reshape(3, 3) - rot.as_matrix()).max() <= _rotation_bound(p, q)


def test_mirrored_fixtures_have_a_negative_determinant():
    for name in ("mirror", "mirror4", "mirror5"):
        p, q = _centres(TC.cases()[name])
        assert np.linalg.det((q - q.mean(axis=0)).T @ (p - p.mean(axis=0))) < 0


def test_planted_transforms_are_recovered():
    """Without noise the planted scale comes back to rounding (relative to the conditioning bound above) and ATE is zero to the
    rounding of coordinates of the fixture's extent"""
    for name, s in (("s0037", 0.037), ("s41", 41.0), ("rot180", 1.7), ("planar", 2.5)):
        c = TC.cases()[name]
        p, q = _centres(c)
        ev = TC.reference(name)
        assert abs(ev["sim"][0] / s - 1.0) <= _rotation_bound(p, q)
        assert ev["ate"][1] <= 1e3 * EPS * (np.abs(q).max() + s * np.abs(p).max())
    assert abs(TC.reference("rot180")["ape_rot"][5]) <= 1e-9   # degrees; atan2 keeps the small angle


def test_statuses():
    for name, c in TC.cases().items():
        assert TC.reference(name)["sim"][14] == c["status"], name
    ev = TC.reference("collinear")
    assert np.array_equal(ev["sim"][:13], np.concatenate([[1.0], np.eye(3).ravel(), np.zeros(3)]))
    assert not ev["ape"][2].any() and ev["ate"][0] == 0


def test_invalid_rows_are_left_out():
    c = TC.cases()["invalid"]
    valid, g = R.frames(c["table"], c["n_frames"], c["gt"], c["index"])
    f = np.arange(257)
    want = (f % 9 != 0) & (f % 31 != 5) & (f % 37 != 6) & (f != 100) & (f != 101) & (f % 23 != 3) & (f != 250)
    want &= f % 41 != 7   # (the index map is the identity where it names a row)
    assert np.array_equal(valid, want) and valid[1] and c["table"][1, 14] == 46.0
    assert TC.reference("invalid")["sim"][13] == valid.sum()
    c = TC.cases()["overlong"]
    assert c["n_frames"] > len(c["table"]) and TC.reference("overlong")["sim"][13] == 200


def test_permuted_ground_truth_equals_the_plain_one():
    c = TC.cases()["permuted"]
    plain = R.evaluate(c["table"], 257, TC.truth(257), None, "sim3", lengths=TC.LENGTHS)
    got = TC.reference("permuted")
    for k in ("sim", "dist", "seg", "summary"):
        assert np.array_equal(plain[k], got[k]), k


# ---- the analytic KITTI cases ----
def test_kitti_scale_case():
    """1 m steps, the estimate 1.1 times the truth under SE(3): dist[f0 + L] equals dist[f0] + L exactly (integers), so the first
    frame beyond it is f1 = f0 + L + 1 and the segment spans L + 1 metres of truth: t_err = 0.1 (L + 1), r_err = 0."""
    ev = TC.reference("kitti_scale")
    seg, summary, info = ev["seg"], ev["summary"], ev["info"]
    assert np.array_equal(ev["dist"], np.arange(1000.0))
    n = 0
    for k in range(100):
        for l, L in enumerate(R.KITTI_LENGTHS):
            f0, f1 = 10 * k, 10 * k + int(L) + 1
            if f1 < 1000:
                n += 1
                assert seg[k, l, 0] == f1 and seg[k, l, 3] == L and seg[k, l, 2] == 0.0
                assert abs(seg[k, l, 1] - 0.1 * (L + 1) / L) <= 64 * EPS * 1.1 * 1000 / L   # (differences of coordinates up to 1 100)
            else:
                assert tuple(seg[k, l]) == (-1.0, 0.0, 0.0, 0.0)
    assert tuple(info) == (n, 0, 800 - n, 100)
    for l, L in enumerate(R.KITTI_LENGTHS):
        assert abs(summary[3 + 3 * l] - 0.1 * (L + 1) / L) <= 64 * EPS * 1100 / L and summary[4 + 3 * l] == 0.0


def test_kitti_yaw_case():
    """A constant yaw drift d per frame: r_err / L = d (L + 1) / L.  The estimate's heading at f0 is off by d f0, so the L + 1 metres
    it moves forward point elsewhere in its own camera frame: t_err = 2 (L + 1) sin(d f0 / 2)."""
    ev = TC.reference("kitti_yaw")
    seg = ev["seg"]
    on = seg[:, :, 3] > 0
    assert on.sum() == ev["info"][0] > 0
    L = seg[:, :, 3][on]
    f0 = (10 * np.arange(100))[:, None].repeat(8, axis=1)[on]
    assert np.abs(seg[:, :, 2][on] - TC.YAW_DRIFT * (L + 1) / L).max() <= 64 * EPS   # (angles below 1 rad from entries of size 1)
    assert np.abs(seg[:, :, 1][on] - 2 * (L + 1) * np.sin(TC.YAW_DRIFT * f0 / 2) / L).max() <= 64 * EPS * 1000   # (coordinates up to 1 000)


def test_kitti_short_and_bad_end_cases():
    ev = TC.reference("kitti_short")
    assert tuple(ev["info"]) == (0, 0, 72, 9) and not ev["summary"].any() and (ev["seg"][:9, :, 0] == -1).all()
    good, bad = TC.reference("kitti_scale"), TC.reference("kitti_bad_end")
    assert bad["info"][1] == 1 and bad["info"][0] == good["info"][0] - 1
    assert tuple(bad["seg"][0, 0]) == (101.0, 0.0, 0.0, 0.0) and bad["summary"][2] == good["summary"][2] - 1


# ---- invariances ----
def _moved(table, s, Rm, t):
    """The estimate under the similarity x -> s Rm x + t: centres moved, camera-to-world rotations turned"""
    out = table.copy()
    out[:, 9:12] = s * table[:, 9:12] @ Rm.T + t
    out[:, :9] = (table[:, :9].reshape(-1, 3, 3) @ Rm.T).reshape(-1, 9)   # Rw' = Rw Rm^T
    return out


def test_rpe_is_unchanged_by_a_rigid_motion_of_the_estimate():
    """Bound: a moved centre carries the rounding of its coordinates (eps x extent); an error is a difference of two such."""
    c = TC.cases()["n257"]
    moved = _moved(c["table"], 1.0, TC.rot((0.2, 0.5, -1.0), 2.1), np.array([30.0, -70.0, 11.0]))
    extent = np.abs(moved[:, 9:12]).max()
    a = R.rpe_delta(c["table"], 257, c["gt"], delta=1, scale=0.037)
    b = R.rpe_delta(moved, 257, c["gt"], delta=1, scale=0.037)
    assert np.array_equal(a[2], b[2]) and a[2].sum() == 256
    assert np.abs(a[0] - b[0]).max() <= 64 * EPS * extent and np.abs(a[1] - b[1]).max() <= 1e3 * EPS * 57.3


def test_ate_under_sim3_is_unchanged_by_a_similarity_of_the_estimate():
    c = TC.cases()["n257"]
    moved = _moved(c["table"], 7.5, TC.rot((0.2, 0.5, -1.0), 2.1), np.array([30.0, -70.0, 11.0]))
    a = R.evaluate(c["table"], 257, c["gt"], lengths=TC.LENGTHS)
    b = R.evaluate(moved, 257, c["gt"], lengths=TC.LENGTHS)
    p, q = _centres(c)
    bound = _rotation_bound(p, q) * np.abs(q).max() * 2
    assert np.abs(a["ape"][0] - b["ape"][0]).max() <= bound and abs(a["ate"][1] - b["ate"][1]) <= bound
    assert abs(b["sim"][0] * 7.5 / a["sim"][0] - 1.0) <= _rotation_bound(p, q)


# ---- margins and the tolerance of the GPU tests ----
def test_no_fixture_rests_on_a_close_decision():
    """The share of segments and alignments left out for a margin below MARGIN_MIN is capped at 0.  The analytic KITTI cases decide
    between integers, which every number format here holds exactly: their margin towards dist[f1 - 1] is 0 by construction and the
    comparison is exact, so they are held to the exact f1 by the tests above instead."""
    close = total = 0
    for name, c in TC.cases().items():
        m = []
        sim = R.align(c["table"], c["n_frames"], c["gt"], c["index"], c["mode"], margin=m)
        if not name.startswith("kitti_"):
            R.rpe_segments(c["table"], c["n_frames"], c["gt"], c["index"], sim[0], c["lengths"], c["step"], margin=m)
        total += len(m)
        close += sum(1 for v in m if not v >= TC.MARGIN_MIN)
    print("decisions", total, "closer than MARGIN_MIN", close)
    assert total > 1000 and close == 0


def test_way_difference_is_the_recorded_one():
    for name in TC.cases():
        d = TC.way_difference(name)
        assert tuple(d[k] for k in TC.OUTPUTS) == TC.WAY_DIFFERENCE[name], name
        assert TC.bound(name, "err_t") == 16.0 * d["err_t"]
    for name in TC.stats_cases():
        assert TC.stats_way_difference(name) == TC.STATS_WAY_DIFFERENCE[name], name


def test_the_two_ways_agree_on_every_integer():
    for name in TC.cases():
        a, b = TC.reference(name), TC.reference(name, True)
        assert a["sim"][13] == b["sim"][13] and a["sim"][14] == b["sim"][14], name
        assert np.array_equal(a["ape"][2], b["ape"][2]) and np.array_equal(a["info"], b["info"]), name
        assert np.array_equal(a["seg"][:, :, 0], b["seg"][:, :, 0]), name


# ---- statistics ----
@pytest.mark.parametrize("name", list(TC.stats_cases()))
def test_stats_equal_numpy(name):
    e, v = TC.stats_cases()[name]
    got = R.stats(e, v)
    x = e[v != 0]
    if len(x) == 0:
        assert not got.any()
        return
    assert got[0] == len(x) and got[4] == x.min() and got[5] == x.max() and got[6] == np.median(x)
    tol = 64 * EPS
    assert abs(got[1] - np.sqrt((x * x).mean())) <= tol * got[1] + 0.0 and abs(got[2] - x.mean()) <= tol * x.max()
    assert abs(got[3] - x.std()) <= tol * x.max() and abs(got[7] - (x * x).sum()) <= tol * got[7]


# ---- the host steps ----
def test_readers_and_associate(tmp_path):
    from semantic_superpoint_amd import trajectory_evaluation as TE
    gt = TC.truth(7)
    kitti = tmp_path / "00.txt"
    np.savetxt(kitti, gt, fmt="%.17e")
    assert np.array_equal(TE.read_kitti_poses(str(kitti)), gt)
    bad = tmp_path / "bad.txt"
    np.savetxt(bad, gt[:, :11])
    with pytest.raises(ValueError, match="12 numbers"):
        TE.read_kitti_poses(str(bad))
    Rotation = pytest.importorskip("scipy.spatial.transform").Rotation
    G = gt.reshape(-1, 3, 4)
    quat = Rotation.from_matrix(G[:, :, :3]).as_quat() * 3.0   # (x, y, z, w), not normalised in the file
    stamps = 100.0 + 0.1 * np.arange(7)
    tum = tmp_path / "traj.txt"
    with open(tum, "w") as f:
        f.write("# timestamp tx ty tz qx qy qz qw\n")
        for k in range(7):
            f.write(" ".join("%.17e" % v for v in [stamps[k], *G[k, :, 3], *quat[k]]) + "\n")
    st, poses = TE.read_tum_trajectory(str(tum))
    assert np.array_equal(st, stamps) and np.abs(poses - gt).max() <= 16 * EPS * np.abs(gt).max()
    # all pairs within max_diff, the closest first, one-to-one
    idx = TE.associate([0.0, 0.1, 0.2, 0.31, 5.0], [0.105, 0.0, 0.3, 0.2], max_diff=0.02)
    assert idx.dtype == np.int32 and idx.tolist() == [1, 0, 3, 2, -1]
    assert TE.associate([0.0, 0.01], [0.004], 0.02).tolist() == [0, -1]      # the closer one wins the only row
    assert TE.associate([0.0, 0.01], [0.006], 0.02).tolist() == [-1, 0]
    assert TE.associate([1.0, 1.0], [1.0, 1.0], 0.0).tolist() == [0, 1]      # ties: by index
    assert TE.associate([], [1.0]).tolist() == [] and TE.associate([1.0], []).tolist() == [-1]


# ---- Python argument errors that need no device ----
def test_argument_errors_without_a_device():
    from semantic_superpoint_amd import lib as L
    from semantic_superpoint_amd import trajectory_evaluation as TE
    for kw in (dict(capacity=0), dict(capacity=L.TRAJ_MAX_FRAMES + 1), dict(capacity=8, n_problems=0), dict(capacity=8, n_len=9),
               dict(capacity=8, n_len=0), dict(capacity=8, step=0), dict(capacity=8, n_stat=0)):
        with pytest.raises(ValueError):
            L.traj_eval_buffers(device="cpu", **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        L.traj_eval_buffers(8, device="cpu")
    gt = TC.truth(4)
    for kw in (dict(align="best"), dict(capacity=None), dict(lengths=()), dict(lengths=(1.0,) * 9), dict(lengths=(-1.0,)), dict(deltas=(0,)),
               dict(deltas=(9,)), dict(deltas=(1, 1)), dict(step=0), dict(index=np.zeros(3, np.int32))):
        with pytest.raises(ValueError):
            TE.TrajectoryEvaluator(gt, **{**dict(capacity=8, device="cpu"), **kw})
    with pytest.raises(ValueError, match="gt must be"):
        TE.TrajectoryEvaluator(gt[:, :11], capacity=8, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        TE.TrajectoryEvaluator(gt, capacity=8, device="cpu")
    traj = dict(capacity=8, n_problems=1, n_len=2, step=10, n_stat=4)
    traj.update(L._alloc(L.TRAJ_SPEC, L._traj_dims(traj), "cpu"))
    table, nf, g = torch.zeros(8, 16, dtype=torch.float64), torch.zeros(1, dtype=torch.int32), torch.as_tensor(gt)
    with pytest.raises(ValueError, match="mode"):
        L.op_traj_align(table, nf, g, traj, mode="best")
    with pytest.raises(RuntimeError, match="HIP device"):
        L.op_traj_align(table, nf, g, traj)
    with pytest.raises(ValueError, match="traj_eval_buffers"):
        L.op_traj_ape(table, nf, g, {})
    with pytest.raises(RuntimeError, match="HIP device"):
        L.op_traj_stats(traj["err_t"], traj["valid"], traj["stats"][0])


def test_written_out_atan2_is_numpy_arctan2_to_an_ulp():
    """The kernels' atan2 is written out so that the restatement repeats it bit for bit; against the math library's it may differ
    in the last place only: every band of the reduction, its breakpoints, both signs of x and the axes."""
    rng = np.random.default_rng(0)
    t = np.concatenate([np.exp(rng.uniform(-25, 25, 20000)), [0.4375, 0.6875, 1.1875, 2.4375, 1.0, 1.5, 0.5, 2.0 ** -29, 2.0 ** 66, 1e300]])
    got, want = R.atan_pos(t), np.arctan(t)
    assert (np.abs(got - want) <= np.spacing(want)).all()
    y, x = np.abs(rng.standard_normal(20000)), rng.standard_normal(20000)
    y[:100], x[100:200] = 0.0, 0.0
    y[200:300] *= 1e-12   # the small angles of a nearly perfect estimate
    got, want = R.atan2_pos(y, x), np.arctan2(y, x)
    assert (np.abs(got - want) <= np.spacing(want)).all() and (got[:100] == want[:100]).all()


# ---- the restated trackers on their existing sequences ----
def _report(tag, ev):
    print("%s: ATE rmse %.3e mean %.3e max %.3e, s %.6f, n_valid %d, status %d" %
          (tag, ev["ate"][1], ev["ate"][2], ev["ate"][5], ev["sim"][0], ev["sim"][13], ev["sim"][14]))


def test_restated_pose_chain_is_scored():
    """pose_ref's noise-free sequences (seq3, seq5): the restated chain's table under "sim3" against the sequence's own truth.  The
    chain's centres follow the truth to CENTRE_BOUND first baselines (tests/test_pose_cpu.py), in the frame and the scale that the
    first pair fixes; Sim(3) over all frames can only fit better, so ATE in metres is at most that times the first baseline,
    and the fitted scale is the first baseline."""
    from tests import pose_ref as P
    for name in ("seq3", "seq5"):
        c = P.case(name)
        seq, rows = c["seq"], c["rows"]
        frames = len(seq["pts"])
        table = np.zeros((frames, R.ROW_WORDS))                               # the chain's rows are the pairs': frame 0, the world, goes
        table[0, :9], table[0, 14] = np.eye(3).ravel(), 1.0                   # in front, as the tracker's row 0 (POSE_FLAG_NO_POSE)
        table[1:] = np.asarray(rows)[:frames - 1]
        ev = R.evaluate(table, frames, TC.sequence_truth(seq), lengths=(1.0,), step=1)
        _report(name, ev)
        unit = np.linalg.norm(seq["centres"][1] - seq["centres"][0])
        assert ev["sim"][13] == frames - 1                                    # (row 0 carries POSE_FLAG_NO_POSE)
        if frames - 1 < 3:                                                    # seq3: two scored frames are too few for Sim(3)
            assert ev["sim"][14] == R.FEW and ev["ate"][0] == 0
            continue
        assert ev["sim"][14] == R.OK
        assert ev["ate"][1] <= np.sqrt(3) * P.CENTRE_BOUND * unit and abs(ev["sim"][0] / unit - 1.0) <= 8 * P.CENTRE_BOUND


def test_restated_world_tracker_is_scored():
    """world_ref's revisit: the trajectory of the restated tracker under "observe" and "relocalise", ATE reported"""
    from tests import world_ref as W
    seq, runs = W.revisit_runs()
    gt, frames = TC.sequence_truth(seq), len(seq["pts"])
    for mode in ("observe", "relocalise"):
        ev = R.evaluate(runs[mode]["table"], frames, gt, lengths=(1.0,), step=1)
        _report("revisit " + mode, ev)
        assert ev["sim"][14] == R.OK and ev["sim"][13] >= frames - 2
        unit = np.linalg.norm(seq["centres"][1] - seq["centres"][0])
        worst = W.centre_errors(seq, runs[mode]["table"]).max()
        assert ev["ate"][1] <= np.sqrt(3) * worst * unit                       # (the fit over all frames is no worse than the first-pair frame)


def test_loop_closure_lowers_the_final_row_of_the_observe_log():
    """loop_ref's circuit (the seed the device test uses): the last row of the restated "observe" log under loop_closure="apply" is
    below the one under observe-only loop closure, in rmse, mean and max; so is the planted drift of test_loop_cpu.py after its
    pose graph."""
    from tests import loop_ref as G
    seq, runs = G.circuit_runs(G.CIRCUIT_DEVICE_SEED)
    gt, frames = TC.sequence_truth(seq), len(seq["pts"])
    obs, app = TC.observe_row(runs["observe"]["table"], frames, gt), TC.observe_row(runs["apply"]["table"], frames, gt)
    print("circuit: final log row observe", obs[:6], "apply", app[:6])
    assert obs[5] == app[5] == 0 and obs[4] == app[4] and (app[:3] < obs[:3]).all()
    truth, table, edges, state, f = G.graph_case(60, 0, a=3)
    Rw, C, sigma, info = G.pose_graph(table, edges, state, f)
    after = table.copy()
    after[:f + 1, 0:9], after[:f + 1, 9:12] = Rw[:f + 1], C[:f + 1]
    gt = np.zeros((f + 1, 3, 4))
    gt[:, :, :3], gt[:, :, 3] = np.swapaxes(truth[:f + 1, :9].reshape(-1, 3, 3), 1, 2), truth[:f + 1, 9:12]
    gt = gt.reshape(-1, 12)
    before_row, after_row = TC.observe_row(table[:f + 1], f + 1, gt, "se3"), TC.observe_row(after[:f + 1], f + 1, gt, "se3")
    print("planted drift: ATE rmse %.4f -> %.4f, max %.4f -> %.4f" % (before_row[0], after_row[0], before_row[2], after_row[2]))
    assert after_row[0] < before_row[0] and after_row[2] < before_row[2]


def test_tracker_argument_errors_without_a_device():
    from semantic_superpoint_amd.tracker import PointTracker, SequenceTracker
    gt = TC.truth(5)
    ok = dict(geometric_check="fundamental", intrinsics=(300.0, 300.0, 160.0, 120.0))
    for make in (lambda **kw: PointTracker(4, 0.7, "cpu", **kw), lambda **kw: SequenceTracker(None, "cpu", 0.015, 4, False, 0.7, 4, **kw)):
        for kw in (dict(trajectory_eval="observe"), dict(ground_truth=gt), dict(trajectory_eval="observe", **ok),
                   dict(ground_truth=gt, trajectory_eval="on", **ok), dict(ground_truth=gt, eval_align="best", **ok),
                   dict(ground_truth=gt, eval_table="absolute", **ok), dict(ground_truth=gt[:, :11], **ok),
                   dict(ground_truth=gt, gt_index=np.zeros(3, np.int32), **ok), dict(gt_index=np.zeros(4096, np.int32), **ok),
                   dict(ground_truth=gt, trajectory_eval="observe", eval_table="world", **ok)):
            with pytest.raises(ValueError):
                make(**kw)
        t = make(ground_truth=gt, trajectory_eval="observe", **ok)
        assert t.trajectory_eval_log().shape == (0, 8) and t.evaluate_trajectory() is None
        with pytest.raises(ValueError, match="ground_truth"):
            make(**ok).evaluate_trajectory()
