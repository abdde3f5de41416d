"""The homography pose and the model selection on the device (lib.op_homography_pose, lib.op_model_select)
against their numpy restatement tests/pose_h_ref.py.  The operators are fed the restatement's H, F and masks, so only the new
kernels are under test: the discrete outputs must be equal, the continuous ones within pose_h_ref.TOLERANCE (whether they are
bit-equal is printed)."""
import functools

import numpy as np
import pytest
import torch

from tests import pose_h_ref as H

pytestmark = pytest.mark.gpu

POSE_KEYS = ("R", "t", "cand", "counts", "n_front", "status", "front", "depth", "X", "model", "normal", "normals2")
SELECT_KEYS = ("scores", "use_h", "mask", "n_inliers", "status")


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@functools.lru_cache(maxsize=None)
def _arrays(names, cap, pair_stride, pt_stride, shared_intr):
    """Host inputs of one call over the named cases: pair p at entry p * pair_stride of the point arrays (the other entries and
    the rows past n hold noise)."""
    n_p = len(names)
    rng = np.random.RandomState(cap + 7 * pair_stride + 13 * pt_stride)
    pts1 = rng.uniform(0, 300, (n_p * pair_stride, cap, pt_stride))
    pts2 = rng.uniform(0, 300, (n_p * pair_stride, cap, pt_stride))
    match = np.zeros((n_p, cap, 3), dtype=np.float32)
    n_match = np.zeros(n_p, dtype=np.int32)
    gh = {"H": np.zeros((n_p, 3, 3)), "mask": np.zeros((n_p, cap), dtype=np.uint8), "n_inliers": np.zeros(n_p, dtype=np.int32),
          "status": np.zeros(n_p, dtype=np.int32)}
    gf = {"F": np.zeros((n_p, 3, 3)), "mask": np.zeros((n_p, cap), dtype=np.uint8), "n_inliers": np.zeros(n_p, dtype=np.int32),
          "status": np.zeros(n_p, dtype=np.int32)}
    intr, prior = np.zeros((n_p, 2, 4)), np.zeros((n_p, 2, 3))
    for p, name in enumerate(names):
        c = H.case(name)
        sc = H.scene(H.CASES[name][0])
        n = c["m"].shape[0]
        pts1[p * pair_stride, :n, :2], pts2[p * pair_stride, :n, :2] = sc["pts"][0], sc["pts"][1]
        match[p, :n], n_match[p] = c["match"], n
        gh["H"][p], gh["mask"][p, :n], gh["n_inliers"][p], gh["status"][p] = c["H"], c["h_mask"], c["h_n"], c["h_status"]
        gf["F"][p], gf["mask"][p, :n], gf["n_inliers"][p], gf["status"][p] = c["F"], c["f_mask"], c["f_n"], c["f_status"]
        intr[p] = c["intr"]
        if c["prior"] is not None:
            prior[p] = c["prior"]
    if shared_intr:
        assert all(np.array_equal(intr[p], intr[0]) for p in range(n_p))
        intr = intr[:1]
    return pts1, pts2, match, n_match, gh, gf, intr, prior


def _run(names, cap, pair_stride=1, pt_stride=2, shared_intr=False, only=None, rotation_eps=H.ROTATION_EPS, with_prior=True):
    from semantic_superpoint_amd import lib as L
    dev = _dev()
    pts1, pts2, match, n_match, gh, gf, intr, prior = _arrays(tuple(names), cap, pair_stride, pt_stride, shared_intr)
    if only is not None:
        sl = slice(only * pair_stride, (only + 1) * pair_stride)
        pts1, pts2, match, n_match, prior = pts1[sl], pts2[sl], match[only:only + 1], n_match[only:only + 1], prior[only:only + 1]
        gh, gf = {k: v[only:only + 1] for k, v in gh.items()}, {k: v[only:only + 1] for k, v in gf.items()}
        intr = intr if shared_intr else intr[only:only + 1]
    d = [_t(a, dev) for a in (pts1, pts2, match, n_match)]
    gh_d, gf_d = {k: _t(v, dev) for k, v in gh.items()}, {k: _t(v, dev) for k, v in gf.items()}
    o = L.op_homography_pose(gh_d, *d, _t(intr, dev), prior=_t(prior, dev) if with_prior else None, rotation_eps=rotation_eps,
                             normal_margin=H.NORMAL_MARGIN, pair_stride=pair_stride)
    s = L.op_model_select(gf_d, gh_d, *d, model_ratio=H.MODEL_RATIO, pair_stride=pair_stride)
    torch.cuda.synchronize()
    return {k: o[k].cpu().numpy() for k in POSE_KEYS}, {k: s[k].cpu().numpy() for k in SELECT_KEYS}


def _compare(o, s, p, name):
    c = H.case(name)
    ref, sel = c["pose"], c["select"]
    n = c["m"].shape[0]
    got = {k: o[k][p] for k in POSE_KEYS}
    worst = 0.0
    for k in ("R", "t", "normal", "normals2"):
        worst = max(worst, float(np.abs(got[k] - ref[k]).max()))
    for k in ("depth", "X"):
        if n:
            worst = max(worst, float((np.abs(got[k][:n] - ref[k]) / np.maximum(1.0, np.abs(ref[k]))).max()))
    worst = max(worst, float((np.abs(s["scores"][p] - sel["scores"]) / np.maximum(1.0, np.abs(sel["scores"]))).max()))
    bits = all(np.array_equal(got[k][:n] if k in ("depth", "X") else got[k], ref[k]) for k in ("R", "t", "normal", "normals2", "depth", "X"))
    bits = bits and np.array_equal(s["scores"][p], sel["scores"])
    print("%s: model %d status %d cand %d counts %s use_h %d worst difference %.3e (tolerance %.3e)%s"
          % (name, got["model"], got["status"], got["cand"], got["counts"].tolist(), s["use_h"][p], worst, H.TOLERANCE,
             ", bit-equal" if bits else ""))
    for k in ("model", "cand", "n_front", "status"):
        assert got[k] == ref[k], (name, k, got[k], ref[k])
    assert np.array_equal(got["counts"], ref["counts"]), name
    assert np.array_equal(got["front"][:n].astype(bool), ref["front"]) and not got["front"][n:].any(), name
    assert not got["depth"][n:].any() and not got["X"][n:].any(), name
    assert not got["depth"][:n][~ref["front"]].any() and not got["X"][:n][~ref["front"]].any(), name
    assert s["use_h"][p] == sel["use_h"], name
    want = (c["h_mask"], c["h_n"], c["h_status"]) if sel["use_h"] else (c["f_mask"], c["f_n"], c["f_status"])
    assert np.array_equal(s["mask"][p][:n].astype(bool), want[0]) and not s["mask"][p][n:].any(), name
    assert s["n_inliers"][p] == want[1] and s["status"][p] == want[2], name
    assert worst <= H.TOLERANCE, (name, worst)
    if ref["status"] == 1:
        assert np.array_equal(got["R"], np.eye(3)) and not got["t"].any() and not got["counts"].any() and got["model"] == 0
        assert not got["normal"].any() and not got["normals2"].any()


@pytest.mark.parametrize("shared_intr", (True, False))
@pytest.mark.parametrize("pair_stride,pt_stride", ((1, 2), (1, 3), (2, 2), (2, 3)))
def test_four_pairs_in_one_call(pair_stride, pt_stride, shared_intr):
    names = H.FOUR if shared_intr else H.FOUR_K                   # n_match = (48, 8, 7, 0) / (48, 48, 3, 48)
    o, s = _run(names, 64, pair_stride, pt_stride, shared_intr)
    for p, name in enumerate(names):
        _compare(o, s, p, name)


@pytest.mark.parametrize("name,cap", (("n257", 320), ("n4096", 4096), ("noisy", 256), ("one_alive", 16), ("plane48b", 48)))
def test_one_pair(name, cap):
    o, s = _run((name,), cap)
    _compare(o, s, 0, name)


DECISIONS = ("negative", "no_model", "salted", "prior_true", "prior_other", "prior_tie", "rotate_prior", "singular", "no_f", "solid")


def test_decisions_in_one_call():
    """H with a negative sign, status_in = 1, a salted mask, two alive with priors for either and priors that tie, a rotation
    that carries its prior, a singular H, no F, and a scene that is not planar."""
    o, s = _run(DECISIONS, 64)
    for p, name in enumerate(DECISIONS):
        _compare(o, s, p, name)
    assert o["status"][DECISIONS.index("prior_tie")] == 2 and o["status"][DECISIONS.index("prior_true")] == 0
    assert s["use_h"].tolist() == [1, 0, 1, 1, 1, 1, 1, 0, 1, 0]


@pytest.mark.parametrize("name", ("small_in", "small_out"))
def test_rotation_threshold(name):
    """One homography just inside and just outside rotation_eps."""
    o, s = _run((name,), 64, rotation_eps=H.case(name)["rotation_eps"])
    _compare(o, s, 0, name)
    assert o["model"][0] == (2 if name == "small_in" else 1)


def test_without_prior_argument():
    o, s = _run(("plane48", "rotate"), 64, with_prior=False)
    _compare(o, s, 0, "plane48")
    _compare(o, s, 1, "rotate")


def test_result_does_not_depend_on_batch_or_run():
    a, sa = _run(H.FOUR_K, 64)
    b, sb = _run(H.FOUR_K, 64)
    for k in POSE_KEYS:
        assert np.array_equal(a[k], b[k]), k
    for k in SELECT_KEYS:
        assert np.array_equal(sa[k], sb[k]), k
    for p in range(len(H.FOUR_K)):
        one, sone = _run(H.FOUR_K, 64, only=p)
        for k in POSE_KEYS:
            assert np.array_equal(one[k][0], a[k][p]), (p, k)
        for k in SELECT_KEYS:
            assert np.array_equal(sone[k][0], sa[k][p]), (p, k)


def test_use_h_leaves_the_other_pairs_alone():
    """With use_h, a pair that keeps its fundamental matrix keeps every output of op_two_view_pose bit for bit."""
    from semantic_superpoint_amd import lib as L
    dev = _dev()
    names = ("plane48", "solid", "rotate", "no_model")
    pts1, pts2, match, n_match, gh, gf, intr, prior = _arrays(names, 64, 1, 2, False)
    d = [_t(a, dev) for a in (pts1, pts2, match, n_match)]
    gh_d, gf_d = {k: _t(v, dev) for k, v in gh.items()}, {k: _t(v, dev) for k, v in gf.items()}
    pose = L.op_two_view_pose(gf_d, *d, _t(intr, dev))
    before = {k: v.clone() for k, v in pose.items()}
    s = L.op_model_select(gf_d, gh_d, *d)
    assert s["use_h"].tolist() == [1, 0, 1, 0]
    o = L.op_homography_pose(gh_d, *d, _t(intr, dev), use_h=s["use_h"], out=pose)
    free = L.op_homography_pose(gh_d, *d, _t(intr, dev))
    assert o is pose and o["model"].tolist() == [1, 0, 2, 0]
    for k in before:
        for p in (1, 3):
            assert torch.equal(o[k][p], before[k][p]), (k, p)
        if k != "E":
            for p in (0, 2):
                assert torch.equal(o[k][p], free[k][p]), (k, p)
    assert not o["normal"][1].any() and not o["normals2"][1].any() and not o["normals2"][3].any()
    with pytest.raises(ValueError):
        L.op_homography_pose(gh_d, *d, _t(intr, dev), use_h=s["use_h"])


def test_bad_arguments_are_errors():
    from semantic_superpoint_amd import lib as L
    dev = _dev()
    pts1, pts2, match, n_match, gh, gf, intr, prior = _arrays(("plane48",), 64, 1, 2, False)
    d = [_t(a, dev) for a in (pts1, pts2, match, n_match)]
    gh_d, gf_d = {k: _t(v, dev) for k, v in gh.items()}, {k: _t(v, dev) for k, v in gf.items()}
    with pytest.raises(ValueError):
        L.op_homography_pose(gf_d, *d, _t(intr, dev))                                  # no "H"
    with pytest.raises(ValueError):
        L.op_homography_pose(gh_d, *d, _t(intr[:, :1], dev))
    with pytest.raises(ValueError):
        L.op_homography_pose(gh_d, *d, _t(intr, dev), prior=_t(prior[0], dev))
    with pytest.raises(ValueError):
        L.op_homography_pose(gh_d, *d, _t(intr, dev), rotation_eps=-1.0)
    with pytest.raises(ValueError):
        L.op_model_select(gf_d, gh_d, *d, model_ratio=1.5)
    with pytest.raises(ValueError):
        L.op_model_select(gh_d, gf_d, *d)


# ---- the trackers under geometric_check="auto" ---------------------------------------------------------------------------------
NN_THRESH, MAX_LENGTH = 0.7, 4
AUTO_KEYS = {"model", "scores", "H", "h_mask", "h_n_inliers", "h_status", "normal", "normals2"}


@functools.lru_cache(maxsize=None)
def _descriptors(n):
    """One unit descriptor per point id: the true correspondences are the mutual nearest neighbours."""
    d = np.random.RandomState(77).randn(n, 256)
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def _frames(seq, dev):
    out = []
    for f in range(len(seq["pts"])):
        xy, desc = seq["pts"][f], _descriptors(seq["pts"][f].shape[0])[seq["ids"][f]]
        out.append((_t(xy, dev), torch.tensor([xy.shape[0]], dtype=torch.int32, device=dev), _t(desc, dev)))
    return out


def test_auto_follows_fundamental_on_a_scene_that_is_not_planar():
    """pose_ref's seq5_k (the one-camera twin of seq5: a tracker has one set of intrinsics): "auto" selects F on every frame and
    every old key, the trajectory, the tracks and the landmarks are bit-identical to "fundamental"."""
    from tests import pose_ref as P
    from semantic_superpoint_amd.export import PointTracker
    dev = _dev()
    c = P.case("seq5_k")
    seq, seed0 = c["seq"], c["seeds"][0] - 1
    kw = dict(check_seed=seed0, intrinsics=tuple(seq["intr"][0]), trajectory_rows=8)
    auto = PointTracker(MAX_LENGTH, NN_THRESH, dev, geometric_check="auto", **kw)
    fund = PointTracker(MAX_LENGTH, NN_THRESH, dev, geometric_check="fundamental", **kw)
    for f, (xy, cnt, desc) in enumerate(_frames(seq, dev)):
        auto.update_device(xy, cnt, desc)
        fund.update_device(xy, cnt, desc)
        ga, gf = auto.last_geometry(), fund.last_geometry()
        assert set(ga) == set(gf) | AUTO_KEYS
        assert int(ga["model"]) == 0 and not ga["normal"].any() and not ga["normals2"].any(), f
        print("frame %d: scores %s" % (f, ga["scores"].cpu().numpy().tolist()))
        for k in gf:
            assert torch.equal(ga[k], gf[k]), (f, k)
        assert torch.equal(auto.trajectory()[0], fund.trajectory()[0]) and torch.equal(auto.trajectory()[1], fund.trajectory()[1])
        if f > 0:
            assert int(ga["h_status"]) == 0 and int(ga["status"]) == 0
    assert np.array_equal(auto.get_tracks(2), fund.get_tracks(2)) and auto.get_tracks(2).shape[0] > 0
    (la, na), (lf, nf) = auto.landmarks_device(), fund.landmarks_device()
    assert torch.equal(la, lf) and torch.equal(na, nf) and int(na) > 0


def test_planar_sequence():
    """Every frame obeys the homography.  The first planar pair has no prior and stays ambiguous (out of scope); from the second
    on the transported normals decide with status 0, and the trajectory from frame 1 on is the true one up to the global scale
    within the bound tests/test_pose_h_cpu.py measured."""
    from semantic_superpoint_amd.export import PointTracker
    dev = _dev()
    seq = H.scene("planar5")
    tr = PointTracker(MAX_LENGTH, NN_THRESH, dev, geometric_check="auto", check_seed=H.SEQ_SEED - 1, intrinsics=tuple(seq["intr"][0]),
                      trajectory_rows=8)
    ref = H.auto_sequence("planar5", "H_lanes")
    for f, (xy, cnt, desc) in enumerate(_frames(seq, dev)):
        tr.update_device(xy, cnt, desc)
        g = tr.last_geometry()
        if f == 0:
            continue
        want = ref["frames"][f - 1]["pose"]
        print("frame %d: model %d status %d cand %d scores %s" % (f, int(g["model"]), int(g["pose_status"]), int(g["cand"]),
                                                                 g["scores"].cpu().numpy().tolist()))
        assert int(g["model"]) == 1 and int(g["pose_status"]) == (2 if f == 1 else 0), f
        assert int(g["cand"]) == want["cand"] and g["counts"][0].cpu().numpy().tolist() == want["counts"].tolist(), f
        assert torch.equal(g["mask"], g["h_mask"]) and int(g["n_inliers"]) == seq["n_in"] == int(g["n_front"])
        assert tr.get_matches().shape[1] == seq["n_in"]                         # the tracks continue on the selected mask
    rows = tr.trajectory()[0].cpu().numpy()
    assert list(rows[:5, 14]) == [3, 3, 2, 0, 0]
    err = float(np.abs(H.planar_centres(rows[1:5]) - H.planar_truth()).max())
    print("planar centres against the truth: %.3e (bound %.3e)" % (err, H.PLANAR_CENTRE_BOUND))
    assert err <= H.PLANAR_CENTRE_BOUND


def test_rotation_in_place_between_two_steps():
    """Side - rotate in place - side: the middle frame is a rotation (model 2); its row keeps the true rotation, repeats the centre
    and carries the scale.  Under "fundamental" the same frame has no pose or a wrong rotation."""
    from tests import pose_ref as P
    from semantic_superpoint_amd.export import PointTracker
    dev = _dev()
    seq = H.scene("srs")
    kw = dict(check_seed=H.SEQ_SEED - 1, intrinsics=tuple(seq["intr"][0]), trajectory_rows=8)
    auto = PointTracker(MAX_LENGTH, NN_THRESH, dev, geometric_check="auto", **kw)
    fund = PointTracker(MAX_LENGTH, NN_THRESH, dev, geometric_check="fundamental", **kw)
    models = []
    for xy, cnt, desc in _frames(seq, dev):
        auto.update_device(xy, cnt, desc)
        fund.update_device(xy, cnt, desc)
        models.append(int(auto.last_geometry()["model"]))
    assert models == [0, 0, 2, 0]
    ra, rf = auto.trajectory()[0].cpu().numpy(), fund.trajectory()[0].cpu().numpy()
    assert np.array_equal(ra[:2], rf[:2])
    # the rotation is read off a homography whose entries follow the restatement's to 1e-10 or better: 1e-6 degrees is generous
    ang = P.angle_deg(ra[2, :9].reshape(3, 3), seq["Rf"][2])
    ang_f = P.angle_deg(rf[2, :9].reshape(3, 3), seq["Rf"][2])
    print("rotation frame: auto %.3e degrees from the truth, flags %d; fundamental %.3e degrees, flags %d"
          % (ang, ra[2, 14], ang_f, rf[2, 14]))
    assert ang <= 1e-6 and ra[2, 14] == 2 and np.abs(ra[2, 9:12] - ra[1, 9:12]).max() <= 1e-12
    # "wrong" is measured with the bound that "right" is held to above.  Measured on an MI355X: 4.9e-3 degrees against 6.4e-14, and
    # a centre that leaves its place by 0.010 first baselines with a "measured" scale (flags 0) where there is no baseline at all
    moved = float(np.linalg.norm(rf[2, 9:12] - rf[1, 9:12]) / np.linalg.norm(rf[1, 9:12]))
    print("fundamental: the centre of the rotation frame moves by %.4f first baselines" % moved)
    assert (int(rf[2, 14]) & 1) or ang_f > 1e-6
    assert P.angle_deg(ra[3, :9].reshape(3, 3), seq["Rf"][3]) <= 1e-3      # the rotation is not lost to the frames behind it


def test_auto_needs_intrinsics():
    from semantic_superpoint_amd.export import PointTracker
    dev = _dev()
    with pytest.raises(ValueError):
        PointTracker(MAX_LENGTH, NN_THRESH, dev, geometric_check="auto")
    with pytest.raises(ValueError):
        PointTracker(MAX_LENGTH, NN_THRESH, dev, geometric_check="auto", intrinsics=(300.0, 300.0, 160.0, 120.0), model_ratio=1.5)
    with pytest.raises(ValueError):
        PointTracker(MAX_LENGTH, NN_THRESH, dev, geometric_check="auto", intrinsics=(300.0, 300.0, 160.0, 120.0), rotation_eps=-1.0)
    for mode in (None, "homography"):                                   # unchanged
        with pytest.raises(ValueError):
            PointTracker(MAX_LENGTH, NN_THRESH, dev, geometric_check=mode, intrinsics=(300.0, 300.0, 160.0, 120.0))
    PointTracker(MAX_LENGTH, NN_THRESH, dev, geometric_check="auto", intrinsics=(300.0, 300.0, 160.0, 120.0), world_map="observe")


def test_sequence_tracker_step_under_auto_does_not_synchronise(tmp_path):
    from semantic_superpoint_amd.export import PointTracker, SequenceTracker
    from tests.test_gpu_tracks import _agent, _no_host_sync, _shifted_frames
    dev = _dev()
    agent = _agent(tmp_path, dev)
    args = (agent.net, dev, agent.conf_thresh, agent.nms_dist, False, agent.nn_thresh, 3)
    intr = (90.0, 92.0, 48.0, 32.0)
    with pytest.raises(ValueError):
        SequenceTracker(*args, geometric_check="auto", min_inliers=8)
    seq = SequenceTracker(*args, geometric_check="auto", min_inliers=8, intrinsics=intr, trajectory_rows=8)
    fed = PointTracker(3, agent.nn_thresh, dev, geometric_check="auto", min_inliers=8, intrinsics=intr, trajectory_rows=8)
    for f, im in enumerate(_shifted_frames()):            # 64x96 frames
        on_dev = torch.from_numpy(im).to(dev)
        if f == 0:
            o = seq.step(on_dev)                          # (the first step allocates)
        else:
            with _no_host_sync():
                o = seq.step(on_dev)
        fed.update_device(o["pts"][0][:, :2].to(torch.float64), o["count"][0:1], o["desc"][0])
        g, h = seq.tracker.last_geometry(), fed.last_geometry()
        assert set(g) == set(h) and AUTO_KEYS <= set(g)
        for k in g:
            assert torch.equal(g[k], h[k]), (f, k)                                   # bit for bit
        assert torch.equal(seq.trajectory()[0], fed.trajectory()[0]) and float(seq.trajectory()[1]) == f + 1
        assert int(g["model"]) in (0, 1, 2) and int(g["pose_status"]) in (0, 1, 2)
