"""GPU: the streamed descriptor metrics: op_eval_pixel_homographies and op_eval_accumulate against
their numpy restatement (tests/descriptor_metrics_ref.py) bit for bit, StreamingEvaluator against Evaluator.run_points
and the G16 fixture of the real reference, and the trainer's `ssp_descriptor_metrics`."""
import os

import numpy as np
import pytest
import torch

from oracle import cpu_ref as C
from tests import descriptor_metrics_ref as R
from tests.golden_evaluation import CASES, case_pair
from tests.test_descriptor_metrics_cpu import check_g16_summary

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ARCH = "SuperPointNet_gauss2_ssmall"


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _normalised(Hpx, hh, ww):
    """float32 normalised form T @ Hpx @ inv(T) of a pixel homography."""
    T = np.array([[2.0 / ww, 0, -1], [0, 2.0 / hh, -1], [0, 0, 1]])
    return (T @ Hpx @ np.linalg.inv(T)).astype(np.float32)


@pytest.mark.parametrize("hh,ww", [(240, 320), (48, 64)])
def test_pixel_homographies_equal_restatement(hh, ww):
    from semantic_superpoint_amd import lib as L
    c, s = np.cos(0.3), np.sin(0.3)
    hn = np.stack([np.eye(3, dtype=np.float32),
                   _normalised(np.array([[1.0, 0, 5], [0, 1.0, -3], [0, 0, 1]]), hh, ww),
                   np.array([[c, -s, 0.05], [s, c, -0.1], [0, 0, 1]], np.float32),
                   np.array([[1.1, 0.05, 0.2], [-0.07, 0.93, -0.15], [0.12, -0.2, 1.0]], np.float32),
                   np.array([[0.8, -0.2, -0.3], [0.15, 1.2, 0.25], [-0.25, 0.1, 0.9]], np.float32)])
    hom, inv = L.op_eval_pixel_homographies(_t(hn), hh, ww)
    want, want_inv = R.pixel_homographies(hn, hh, ww)
    assert _same_bits(hom.cpu().numpy(), want)
    assert _same_bits(inv.cpu().numpy(), want_inv)
    # a swapped height / width would show: the translation of 5 px along x comes back as 5 px along x
    np.testing.assert_allclose(want[1], [[1, 0, 5], [0, 1, -3], [0, 0, 1]], atol=1e-5)
    np.testing.assert_allclose(want_inv[1] @ want[1], np.eye(3), atol=1e-12)


def _hand_pairs():
    """Seven pairs (numbers 3 .. 9) that take every branch of the accumulation."""
    G = np.array([[1.0, 0, 4], [0, 1.0, -2], [0, 0, 1]])
    P1 = np.array([[1.02, 0.01, 3.5], [-0.02, 0.97, -1.25], [1e-4, -5e-5, 1.0]])
    P2 = np.array([[0.95, -0.03, -6.0], [0.04, 1.05, 2.5], [-8e-5, 1.2e-4, 1.0]])
    shift = lambda d: np.array([[1.0, 0, d], [0, 1.0, 0], [0, 0, 1]])  # noqa: E731
    rep = np.array([[10, 8, 0, 0, 0, 0, 5, 0],               # nothing repeats
                    [40, 42, 20, 22, 17.5, 19.125, 30, 0],   # no model
                    [6, 7, 3, 2, 1.75, 2.5, 0, 0],           # n1 + n_unwarped = 0
                    [55, 50, 31, 29, 33.3, 28.1, 41, 0],     # ap = 0
                    [120, 110, 90, 85, 77.7, 70.3, 95, 0],   # the truth shifted by exactly 3 px
                    [300, 280, 211, 190, 260.4, 250.9, 250, 0],
                    [33, 31, 7, 9, 12.6, 15.3, 20, 0]], np.float64)
    ransac = {"H": np.stack([P1, np.eye(3), P1, P2, shift(3.0) @ G, shift(0.4) @ P1, shift(12.0) @ P2]),
              "n_inliers": np.array([14, 0, 4, 25, 80, 170, 9], np.int32),
              "status": np.array([0, 1, 0, 0, 0, 0, 0], np.int32),
              "ap": np.array([0.7, 0.0, 0.5, 0.0, 0.91, 0.83, 0.4]),
              "n1": np.array([12, 50, 0, 60, 130, 333, 40], np.int32),
              "hom": np.stack([P1, P2, P1, P2, G, P1, P2])}
    return rep, ransac


def test_accumulate_equals_restatement():
    from semantic_superpoint_amd import lib as L
    rep, ra = _hand_pairs()
    P, f0, cap = 7, 3, 12
    want_rows, want_state = np.zeros((cap, R.ROW_WORDS)), np.zeros(R.STATE_WORDS)
    new = R.accumulate(f0, want_rows, want_state, rep=rep, ransac=ra)
    rows, state = L.eval_metrics_state(cap, DEV)
    n1 = np.zeros(2 * P, np.int32)
    n1[0::2], n1[1::2] = ra["n1"], 77  # interleaved counts: the warped side's entries must not be read
    L.op_eval_accumulate(rows, state, f0, rep=_t(rep), ransac={k: _t(ra[k]) for k in ("H", "n_inliers", "status")},
                         ap=_t(ra["ap"]), n1=_t(n1), pair_stride=2, hom=_t(ra["hom"]))
    got_rows, got_state = rows.cpu().numpy(), state.cpu().numpy()
    assert _same_bits(got_rows, want_rows)
    assert _same_bits(got_state, want_state)
    r = got_rows[f0:f0 + P]
    assert list(r[:, 15]) == list(range(3, 10)) and not got_rows[:f0].any() and not got_rows[f0 + P:].any()
    assert r[0, 0] == 0 and r[0, 1] == -1                       # nothing repeats: not in the loc mean
    assert got_state[3] == 6 and got_state[0] == 7
    assert r[1, 10] == 1 and not r[1, 2:8].any() and np.isinf(r[1, 14]) and got_state[12] == 1
    assert r[2, 8] == 0 and r[2, 12] == 0 and r[2, 13] == 0     # zero denominator
    assert r[3, 9] == 0
    assert r[4, 14] == 3.0 and list(r[4, 2:8]) == [0, 1, 1, 1, 1, 1]
    assert _same_bits(new, r)
    # the groups switched off: their slots stay 0
    rows2, state2 = L.eval_metrics_state(cap, DEV)
    L.op_eval_accumulate(rows2, state2, 0, rep=_t(rep))
    w_rows, w_state = np.zeros((cap, R.ROW_WORDS)), np.zeros(R.STATE_WORDS)
    R.accumulate(0, w_rows, w_state, rep=rep)
    assert _same_bits(rows2.cpu().numpy(), w_rows) and _same_bits(state2.cpu().numpy(), w_state)
    assert not w_rows[:, 2:15].any() and not w_state[4:].any()
    rows3, state3 = L.eval_metrics_state(cap, DEV)
    L.op_eval_accumulate(rows3, state3, 0, ransac={k: _t(ra[k]) for k in ("H", "n_inliers", "status")}, ap=_t(ra["ap"]),
                         n1=_t(ra["n1"]), hom=_t(ra["hom"]))
    w_rows, w_state = np.zeros((cap, R.ROW_WORDS)), np.zeros(R.STATE_WORDS)
    R.accumulate(0, w_rows, w_state, ransac=ra)
    assert _same_bits(rows3.cpu().numpy(), w_rows) and _same_bits(state3.cpu().numpy(), w_state)
    assert not w_rows[:, :2].any() and not w_state[1:4].any()


class _G16:
    """One upload of the 12 G16 pairs and every evaluation of it the tests share."""

    def __init__(self):
        from semantic_superpoint_amd.evaluation import Evaluator, _upload
        self.datas = [case_pair(c)[0] for c in CASES]
        self.pts, self.cnt, self.desc = _upload(self.datas, torch.device(DEV))
        self.Hs = np.stack([d["homography"] for d in self.datas])
        self.per_file = Evaluator(240, 320).run_points(self.pts, self.cnt, self.desc, self.Hs, list(range(12)))
        self._runs = {}

    def stream(self, split, capacity=12):
        from semantic_superpoint_amd.evaluation import StreamingEvaluator
        key = (tuple(split), capacity)
        if key not in self._runs:
            ev = StreamingEvaluator(240, 320, DEV, capacity)
            k = 0
            for n in split:
                ev.update_points(self.pts[2 * k:2 * (k + n)], self.cnt[2 * k:2 * (k + n)], self.desc[2 * k:2 * (k + n)],
                                 self.Hs[k:k + n])
                k += n
            assert k == 12 and ev.pairs == 12
            self._runs[key] = (ev, ev.state.clone(), ev.rows.clone(), ev.result())
        return self._runs[key]


@pytest.fixture(scope="module")
def g16():
    return _G16()


def test_g16_end_to_end(g16, tmp_path):
    ev, _, _, res = g16.stream([5, 5, 2])
    rows = res["rows"]
    assert rows.shape == (12, 16)
    for k, want in enumerate(g16.per_file):
        assert rows[k, 0] == want["rep"] and rows[k, 1] == want["loc_err"], CASES[k][0]
        assert rows[k, 8] == want["mscore"] and rows[k, 9] == want["mAP"], CASES[k][0]
        np.testing.assert_array_equal(rows[k, 2:8] != 0, want["correctness"], err_msg=CASES[k][0])
        assert rows[k, 15] == k
    print("summary:", {k: v for k, v in res.items() if k != "rows"})
    assert res["pairs"] == 12 and res["rows_dropped"] == 0 and res["no_model"] == 0
    check_g16_summary(dict(res, loc_pairs=int(ev.state[3].item())))
    out = ev.write(str(tmp_path), ["%d.npz" % k for k in range(12)])
    f = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g16_evaluation.npz"))
    np.testing.assert_array_equal(out["correctness"], f["result_correctness"])
    np.testing.assert_array_equal(out["mscore"], f["result_mscore"])
    assert os.path.exists(tmp_path / "result.txt") and os.path.exists(tmp_path / "result.npz")


def test_split_invariance_on_the_device(g16):
    _, state, rows, _ = g16.stream([12])
    for split in ([5, 5, 2], [1] * 12):
        _, s, r, _ = g16.stream(split)
        assert torch.equal(s, state), split
        assert torch.equal(r, rows), split


def test_capacity(g16):
    _, state, rows, _ = g16.stream([5, 5, 2])
    ev, s8, r8, res = g16.stream([5, 5, 2], capacity=8)
    assert res["pairs"] == 12 and res["rows_dropped"] == 4 and res["rows"].shape == (8, 16)
    assert torch.equal(s8[:13], state[:13]) and s8[13].item() == 4
    assert torch.equal(r8, rows[:8])


def _net():
    from semantic_superpoint_amd import models
    net = getattr(models, ARCH)()
    net.load_state_dict({k: torch.as_tensor(np.array(v)) for k, v in C.init_state_dict(ARCH, seed=0).items()})
    return net.to(DEV).eval()


def test_views_path_equals_operators_by_hand():
    from semantic_superpoint_amd import lib as L
    from semantic_superpoint_amd.evaluation import HOMOGRAPHY_THRESH, StreamingEvaluator, pair_seeds
    B, hh, ww = 2, 64, 96
    rs = np.random.RandomState(3)
    a = torch.from_numpy(rs.uniform(0, 1, (B, 1, hh, ww)).astype(np.float32))
    b = a.clone()
    b[1] = torch.roll(a[1], (2, 3), (1, 2))
    hn = np.stack([np.eye(3, dtype=np.float32), np.array([[1, 0, 2 * 3 / ww], [0, 1, 2 * 2 / hh], [0, 0, 1]], np.float32)])
    eng = _net().engine(B, hh, ww, torch.device(DEV))
    x0, x1 = a.to(DEV).contiguous(), b.to(DEV).contiguous()
    with torch.no_grad():
        eng.forward(x0, slot=0, train=False, want=())
        eng.forward(x1, slot=1, train=False, want=())
    kw = dict(conf_thresh=0.0155, nms_dist=4, subpixel=True, border_remove=4)
    d0, d1 = eng.describe_points(0, B, **kw), eng.describe_points(1, B, **kw)
    counts = torch.cat([d0["count"], d1["count"]]).cpu().tolist()
    print("points per image:", counts)
    assert min(counts) >= 16
    ev = StreamingEvaluator(hh, ww, DEV, 4, corner_shape=(hh, ww))
    ev.update_views(d0, d1, _t(hn), subpixel=True)

    def p64(d):
        p = d["pts"][:, :, :3].double()
        p[:, :, :2] = p[:, :, :2] + d["pts"][:, :, 3:5].double() - 2
        return p.contiguous()

    p0, p1 = p64(d0), p64(d1)
    M, Mi = R.pixel_homographies(hn, hh, ww)
    Hd, Hi = _t(M), _t(Mi)
    rep = L.op_eval_repeatability(p0, d0["count"], p1, d1["count"], Hd, Hi, hh, ww, 1000, 3.0, pair_stride=1, n_pairs=B)
    s_cc, s_nn = pair_seeds(np.arange(B))
    m, nm = L.op_match_two_way(d0["desc"], d0["count"], d1["desc"], d1["count"], float("inf"), pair_stride=1, n_pairs=B)
    cc = L.op_eval_ransac(p0, p1, m, nm, _t(s_cc), pair_stride=1)
    m, nm = L.op_match_two_way(d0["desc"], d0["count"], d1["desc"], d1["count"], 1.2, pair_stride=1, n_pairs=B)
    nn = L.op_eval_ransac(p0, p1, m, nm, _t(s_nn), pair_stride=1, want_ap=True)
    rows, state = L.eval_metrics_state(4, DEV)
    L.op_eval_accumulate(rows, state, 0, rep=rep, ransac=cc, ap=nn["ap"], n1=d0["count"], pair_stride=1, hom=Hd,
                         corner_shape=(hh, ww), thresholds=HOMOGRAPHY_THRESH)
    assert torch.equal(ev.rows, rows) and torch.equal(ev.state, state)
    r = ev.result()["rows"]
    print("rows:", r)
    assert r.shape == (2, 16)
    assert r[0, 0] == 1.0 and list(r[0, 2:8]) == [1] * 6 and r[0, 9] == 1.0 and r[0, 10] == 0
    # mscore is not asserted to be 1: the reference's (y, x) quirk drops points with x > H - 1 on a wide image
    assert r[0, 8] > 0


def test_evaluate_descriptor_equals_export_then_evaluate(tmp_path):
    """evaluate_descriptor over an in-memory loader against export_descriptor + evaluate on the files it writes: the same pairs,
    pair numbers = file numbers (the RANSAC seeds), host homographies inverted by np.linalg.inv on both paths."""
    import argparse
    from semantic_superpoint_amd.evaluation import evaluate
    from semantic_superpoint_amd.export import evaluate_descriptor, export_descriptor
    rs = np.random.RandomState(7)
    samples = []
    for k in range(3):
        a = rs.uniform(0, 1, (1, 240, 320)).astype(np.float32)
        samples.append({"image": torch.from_numpy(a)[None], "warped_image": torch.from_numpy(np.roll(a, (8, 16), axis=(1, 2)).copy())[None],
                        "homography": torch.tensor([[1.0, 0, 16], [0, 1.0, 8], [0, 0, 1]])[None]})
    weights = str(tmp_path / "weights.pth")
    torch.save({k: torch.as_tensor(np.array(v)) for k, v in C.init_state_dict(ARCH, seed=21).items()}, weights)
    config = {"data": {"dataset": "in-memory"},
              "model": {"name": ARCH, "params": {}, "pretrained": weights, "nms": 4, "detection_threshold": 0.0155,
                        "nn_thresh": 0.7, "subpixel": {"enable": True, "patch_size": 5}}}
    res = evaluate_descriptor(config, None, test_loader=samples, pairs_per_flush=2)
    out = tmp_path / "export"
    assert export_descriptor(config, str(out), None, test_loader=samples, pairs_per_flush=2) == 3
    args = argparse.Namespace(path=str(out / "predictions"), sift=False, outputImg=False, repeatibility=True, homography=True,
                              plotMatching=False, split=False)
    ref = evaluate(args)
    rows = res["rows"]
    print("evaluate_descriptor:", {k: v for k, v in res.items() if k != "rows"})
    assert res["pairs"] == 3 and rows.shape == (3, 16) and res["rows_dropped"] == 0
    assert list(rows[:, 0]) == list(ref["repeatability"])
    np.testing.assert_array_equal(rows[:, 2:8] != 0, ref["correctness"])
    assert list(rows[:, 8]) == list(ref["mscore"]) and list(rows[:, 9]) == list(ref["mAP"])
    assert list(rows[rows[:, 1] > 0, 1]) == list(ref["localization_err"])
    assert np.isfinite(rows[:, :14]).all()


def _cfg(B, on, warped=True):
    cfg = {"data": {"semantic": True, "gaussian_label": {"enable": True},
                    "warped_pair": {"enable": warped, "valid_border_margin": 3,
                                    "params": dict(translation=True, rotation=True, scaling=True, perspective=True,
                                                   scaling_amplitude=0.2, perspective_amplitude_x=0.2,
                                                   perspective_amplitude_y=0.2, patch_ratio=0.85, max_angle=0.5,
                                                   allow_artifacts=True)}},
           "model": {"name": ARCH, "params": {}, "batch_size": B, "real_batch_size": B, "learning_rate": 1e-3,
                     "lambda_loss": 1, "multi_task_loss": True, "dense_loss": {"enable": False},
                     "detector_loss": {"loss_type": "softmax"}, "detection_threshold": 0.0155, "nms": 4,
                     "subpixel": {"enable": True},
                     "sparse_loss": {"enable": True, "params": {"num_matching_attempts": 600,
                                                                "num_masked_non_matches_per_match": 100, "lamda_d": 1}}},
           "validation_interval": 1000, "validation_size": 3, "tensorboard_interval": 1, "retrain": True, "reset_iter": True,
           "ssp_seed": 3, "ssp_device_pairs": True}
    if on:
        cfg["ssp_descriptor_metrics"] = True
    return cfg


def _val_run(cfg, tmp_path, samples):
    from semantic_superpoint_amd.Train_model_heatmap_all import Train_model_heatmap_all as T
    agent = T(cfg, save_path=tmp_path, device=DEV)
    agent.loadModel()
    agent.net.load_state_dict({k: torch.as_tensor(np.array(v)) for k, v in C.init_state_dict(ARCH, seed=6).items()})
    agent.dataParallel()
    losses = [agent.train_val_sample(s, n_iter=it, train=False) for it, s in enumerate(samples)]
    eng = agent.net.engine()
    torch.cuda.synchronize()
    return agent, losses, eng.params.clone(), eng.bn_running.clone()


def test_trainer_descriptor_metrics(tmp_path):
    from semantic_superpoint_amd import lib as L
    from semantic_superpoint_amd.Train_model_heatmap_all import Train_model_heatmap_all as T
    B, hh, ww = 2, 64, 96
    samples = []
    for it in range(2):
        g = torch.Generator().manual_seed(20 + it)
        # keypoints 8 pixels apart: no two of them scatter into one pixel of the warped label maps (colliding ones are covered by
        # tests/test_gpu_trainer_device_pairs.py); with deterministic accumulation the steps repeat bit for bit
        lab = torch.zeros(B, 1, hh, ww)
        lab[:, :, 4::8, 4::8] = (torch.rand(B, 1, hh // 8, ww // 8, generator=g) < 0.3).float()
        samples.append({"image": torch.rand(B, 1, hh, ww, generator=g), "labels_2D": lab,
                        "semantic": torch.randint(0, 134, (B, hh, ww), generator=g)})
    L.set_deterministic(True)
    try:
        _trainer_checks(T, B, hh, ww, samples, tmp_path)
    finally:
        L.set_deterministic(False)


def _trainer_checks(T, B, hh, ww, samples, tmp_path):
    agent, losses, params, bn = _val_run(_cfg(B, True), tmp_path, samples)
    ev = agent.descriptor_eval_val
    assert ev is not None and ev.pairs == 4 and ev.capacity == (3 + 2) * B and ev.corner_shape == (hh, ww)
    sc = agent.descriptor_round_scalars()
    print("round scalars:", sc)
    names = ["repeatability_round", "localization_err_round", "matching_score_round", "nn_mAP_round"] + \
            ["homography_correctness_%d_round" % t for t in (1, 3, 5, 10, 20, 50)]
    assert sorted(sc) == sorted(names)
    for k, v in sc.items():  # localization_err is NaN when nothing repeated in the round: the documented case
        assert np.isfinite(v) or (k == "localization_err_round" and np.isnan(v)), (k, v)
    assert ev.result()["pairs"] == 4
    state, rows = ev.state.clone(), ev.rows.clone()
    agent2, losses2, params2, bn2 = _val_run(_cfg(B, True), tmp_path, samples)
    assert torch.equal(agent2.descriptor_eval_val.state, state) and torch.equal(agent2.descriptor_eval_val.rows, rows)
    agent2.reset_descriptor_eval()
    assert agent2.descriptor_eval_val.pairs == 0 and not agent2.descriptor_eval_val.state.any()
    off, losses_off, params_off, bn_off = _val_run(_cfg(B, False), tmp_path, samples)
    assert off.descriptor_eval_val is None and not off.descriptor_metrics
    assert losses == losses2 == losses_off and np.isfinite(losses).all()
    assert torch.equal(params, params_off) and torch.equal(bn, bn_off)
    assert torch.equal(params, params2) and torch.equal(bn, bn2)
    with pytest.raises(ValueError):
        T(_cfg(B, True, warped=False), save_path=tmp_path, device=DEV)


def test_refusals():
    from semantic_superpoint_amd import lib as L
    from semantic_superpoint_amd.evaluation import StreamingEvaluator
    with pytest.raises(ValueError):
        StreamingEvaluator(240, 320, DEV, 0)
    ev = StreamingEvaluator(240, 320, DEV, 4)
    H = np.eye(3)[None]

    def arrays(n, cap):
        return (torch.zeros(n, cap, 3, dtype=torch.float64, device=DEV), torch.ones(n, dtype=torch.int32, device=DEV),
                torch.zeros(n, cap, 256, device=DEV))

    with pytest.raises(ValueError):
        ev.update_points(*arrays(2, L.MATCH_MAX_POINTS + 1), H)
    p, c, d = arrays(2, 8)
    with pytest.raises(ValueError):
        ev.update_points(p, c, d, np.stack([np.eye(3)] * 2))          # two homographies, one interleaved pair
    hn = torch.eye(3, device=DEV)[None]
    with pytest.raises(ValueError):
        ev.update_points(p, c, d, normalised=hn.double())              # wrong dtype
    with pytest.raises(ValueError):
        ev.update_points(p, c, d, normalised=hn[:, :2])                # wrong shape
    with pytest.raises(ValueError):
        ev.update_points(p, c, d, normalised=torch.eye(3, device=DEV)[None].repeat(2, 1, 1))  # mismatched P
    with pytest.raises(ValueError):
        L.op_eval_pixel_homographies(hn.double(), 240, 320)
    with pytest.raises(ValueError):
        L.op_eval_pixel_homographies(hn[0], 240, 320)
    rows, state = L.eval_metrics_state(4, DEV)
    with pytest.raises(ValueError):
        L.op_eval_accumulate(rows, state, 0, rep=torch.zeros(L.EVAL_ACC_MAX_PAIRS + 1, 8, dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError):
        L.op_eval_accumulate(rows, state, 0, rep=torch.zeros(1, 8, dtype=torch.float64, device=DEV), ap=state[:1])
    with pytest.raises(ValueError):
        L.eval_metrics_state(0, DEV)
    assert ev.pairs == 0 and not ev.state.any()   # a refused update leaves the evaluator as it was
