"""GPU: detector evaluation on the device - true / false positives, precision-recall curve, mAP and
localisation error against the real reference's results (G20) and against the numpy restatement (tests/detector_eval_ref.py,
itself pinned to G20 by tests/test_detector_eval_cpu.py).

Everything but mAP and the localisation error is compared for equality.  Those two are sums whose order differs from numpy's:
N terms <= distance_thresh in fp64, so the bound is N * 2^-52 (N = number of records), as in the CPU test."""
import copy
import json
import os

import numpy as np
import pytest
import torch

from tests import detector_eval_ref as R
from tests import golden_detector_eval as G

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DEV = "cuda:0"
EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def g20():
    return np.load(os.path.join(HERE, "golden", "g20_detector_eval.npz"))


@pytest.fixture(scope="module")
def sets():
    return {name: G.make_set(name) for name in G.SETS}


def _mods():
    from semantic_superpoint_amd import detector_evaluation as DE
    from semantic_superpoint_amd import lib as L
    return DE, L


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _points_batch(maps):
    cap = max(max(int((m != 0).sum()) for m in maps), 1)
    rows = [G.point_list(m, cap) for m in maps]
    return _t(np.stack([r[0] for r in rows])), _t(np.array([r[1] for r in rows], np.int32))


def _feed(ev, images, points=False, f32_labels=False, split=None):
    """images: [(prob map, keypoint map)]; split: batch sizes (default: one call)."""
    i = 0
    for n in (split or [len(images)]):
        part = images[i:i + n]
        i += n
        lab = np.stack([kp for _, kp in part])
        lab = _t(lab.astype(np.float32)) if f32_labels else _t(lab.astype(np.uint8))
        if points:
            pts, cnt = _points_batch([p for p, _ in part])
            ev.update(pts=pts, count=cnt, labels=lab)
        else:
            ev.update(prob=_t(np.stack([p for p, _ in part]).astype(np.float32)), labels=lab)
    assert i == len(images)


def _run(images, points=False, capacity=None, f32_labels=False, split=None, **kw):
    DE, _ = _mods()
    H, W = images[0][1].shape
    ev = DE.DetectorEvaluator(H, W, DEV, capacity or max(len(images) * H * W, 1), **kw)
    _feed(ev, images, points, f32_labels, split)
    r = ev.result()
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in r.items()}, ev


def _same_nan(a, b, tol):
    return (np.isnan(a) and np.isnan(b)) or abs(a - b) <= tol


def _check(got, want):
    n = len(want["prob"])
    print("records %d n_gt %d mAP %.17g / %.17g loc %.17g / %.17g" % (n, want["n_gt"], got["mAP"], want["mAP"], got["loc_error"],
                                                                      want["loc_error"]))
    assert got["prob"].dtype == np.float32 and np.array_equal(got["prob"], want["prob"])
    assert np.array_equal(got["tp"].astype(bool), want["tp"])
    assert got["n_gt"] == want["n_gt"]
    assert got["precision"].dtype == np.float64 and np.array_equal(got["precision"], want["precision"])
    assert got["recall"].dtype == np.float64 and np.array_equal(got["recall"], want["recall"])
    assert abs(got["mAP"] - want["mAP"]) <= max(n, 1) * EPS
    assert _same_nan(got["loc_error"], want["loc_error"], max(n, 1) * EPS)


def _ref(images, points=False, **kw):
    return R.evaluate([(((G.point_list(p)[0],), kp) if points else (p, kp)) for p, kp in images], **kw)


# ---- G20: the real reference's results ----
@pytest.mark.parametrize("name", sorted(G.SETS))
@pytest.mark.parametrize("variant", G.VARIANTS)
@pytest.mark.parametrize("simplified", G.SIMPLIFIED)
@pytest.mark.parametrize("dt", G.DISTANCE_THRESH)
def test_g20_end_to_end(g20, sets, name, variant, simplified, dt):
    images = sets[name]
    assert np.array_equal(G.checksum(images), g20[name + "/checksum"])
    key, base = G.case_key(name, variant, simplified, dt), G.case_key(name, variant)
    points = variant == "nms"   # the nms map goes in as the exporter's point lists
    maps = [(im[1] if points else im[0], im[2]) for im in images]
    kw = dict(remove_zero=G.REMOVE_ZERO, distance_thresh=dt, prob_thresh=G.PROB_THRESH, simplified=simplified)
    for i, im in enumerate(maps):  # compute_tp_fp per image
        got, _ = _run([im], points, **kw)
        assert np.array_equal(got["tp"].astype(bool), g20["%s/tp/%d" % (key, i)])
        assert np.array_equal(got["prob"], g20["%s/prob_sorted/%d" % (base, i)])
        assert got["n_gt"] == g20[key + "/n_gt"][i]
    got, _ = _run(maps, points, **kw)
    n = len(got["prob"])
    assert np.array_equal(got["prob"], g20[base + "/prob"])
    assert np.array_equal(got["precision"], g20[key + "/precision"]) and np.array_equal(got["recall"], g20[key + "/recall"])
    assert got["n_gt"] == int(g20[key + "/n_gt"].sum())
    loc = g20[G.case_key(name, variant, None, dt) + ("/loc_error_nms" if points else "/loc_error")]
    print("records %d mAP %.17g / %.17g loc %.17g / %.17g" % (n, got["mAP"], g20[key + "/mAP"], got["loc_error"], loc))
    assert abs(got["mAP"] - g20[key + "/mAP"]) <= n * EPS
    assert abs(got["loc_error"] - loc) <= n * EPS


# ---- random cases against the restatement ----
def _scenario(kind, H, W, B, seed):
    rs = np.random.RandomState(seed)
    images = []
    for b in range(B):
        kp = np.zeros((H, W), np.uint8)
        prob = np.zeros((H, W), np.float32)
        if kind == "borders":      # ground truth and predictions in all four corners and along the borders (the clipped window)
            for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H - 1, W // 3), (H // 2, 0), (H // 3, W - 1)):
                kp[y, x] = 1
            m = np.zeros((H, W), bool)
            m[:3, :] = m[-3:, :] = m[:, :3] = m[:, -3:] = True
            prob[m] = rs.uniform(0.001, 1.0, int(m.sum())).astype(np.float32)
            prob[0, 0] = prob[0, W - 1] = prob[H - 1, 0] = prob[H - 1, W - 1] = 0.75
        elif kind == "crowd":      # one ground-truth point reachable from many predictions
            kp[H // 2, W // 2] = kp[2, 2] = 1
            prob[H // 2 - 4:H // 2 + 5, W // 2 - 4:W // 2 + 5] = rs.uniform(0.3, 1.0, (9, 9)).astype(np.float32)
            prob[:5, :5] = rs.uniform(0.3, 1.0, (5, 5)).astype(np.float32)
        elif kind == "several":    # predictions with several ground-truth points in range: first in row-major order, not nearest
            kp[rs.random_sample((H, W)) < 0.25] = 1
            prob[rs.random_sample((H, W)) < 0.4] = 1
            prob *= rs.uniform(0.001, 1.0, (H, W)).astype(np.float32)
        else:                      # "ties": probabilities from a 4-value set
            kp[rs.random_sample((H, W)) < 0.06] = 1
            prob = rs.choice(np.array([0.0, 0.25, 0.5, 0.625, 0.75], np.float32), size=(H, W), p=[0.4, 0.15, 0.15, 0.15, 0.15])
        images.append((prob.astype(np.float32), kp))
    return images


@pytest.mark.parametrize("shape", [(23, 37), (24, 32)])
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("kind", ["borders", "crowd", "several", "ties"])
def test_random_cases_against_restatement(shape, B, kind):
    images = _scenario(kind, shape[0], shape[1], B, seed=100 * B + shape[0])
    for simplified, dt, f32 in ((False, 2, True), (True, 3, False)):
        kw = dict(distance_thresh=dt, simplified=simplified)
        got, _ = _run(images, f32_labels=f32, **kw)
        _check(got, _ref(images, **kw))
    if kind == "ties":  # point lists: the position is the list position
        sparse = [(np.where(np.indices(p.shape).sum(0) % 3 == 0, p, 0).astype(np.float32), kp) for p, kp in images]
        got, _ = _run(sparse, points=True)
        _check(got, _ref(sparse, points=True))


# ---- boundary counts ----
def _counted(counts, H, W, seed, gt=True, ties=False):
    """One image per entry of counts with exactly that many predictions."""
    rs = np.random.RandomState(seed)
    images = []
    for c in counts:
        prob = np.zeros(H * W, np.float32)
        idx = rs.permutation(H * W)[:c]
        prob[idx] = rs.choice(np.array([0.25, 0.5, 0.75], np.float32), c) if ties else rs.uniform(0.01, 1.0, c).astype(np.float32)
        kp = (rs.random_sample((H, W)) < 0.05).astype(np.uint8) if gt else np.zeros((H, W), np.uint8)
        images.append((prob.reshape(H, W), kp))
    return images


def test_candidate_counts_around_wave_and_block_sizes():
    images = _counted([0, 1, 63, 64, 65, 255, 256, 257], 24, 32, seed=5)
    images[3] = (images[3][0], np.zeros((24, 32), np.uint8))  # an image without ground truth
    got, _ = _run(images)
    _check(got, _ref(images))
    for im in images:
        got, _ = _run([im])
        _check(got, _ref([im]))


def test_no_ground_truth_and_no_predictions():
    images = _counted([40, 0, 17], 23, 37, seed=6, gt=False)      # n_gt == 0: div0's branch
    got, _ = _run(images)
    want = _ref(images)
    assert want["n_gt"] == 0 and np.array_equal(want["recall"], np.r_[0.0, np.ones(58)]) and np.isnan(want["loc_error"])
    _check(got, want)
    images = _counted([0, 0], 23, 37, seed=7)                     # no predictions at all
    for points in (False, True):
        got, _ = _run(images, points=points)
        assert got["precision"].tolist() == [0.0, 0.0] and got["recall"].tolist() == [0.0, 1.0] and got["mAP"] == 0.0
        assert len(got["prob"]) == 0 and len(got["tp"]) == 0 and got["n_gt"] > 0 and np.isnan(got["loc_error"])


def test_record_counts_around_the_curve_tile():
    _, L = _mods()
    T = L.DET_CURVE_TILE
    H, W = 24, 32
    for total in (T - 1, T, T + 1, 3 * T + 5):
        counts = [H * W] * (total // (H * W)) + [total % (H * W)]
        images = _counted(counts, H, W, seed=total, ties=True)
        got, _ = _run(images)
        assert len(got["prob"]) == total
        _check(got, _ref(images))


# ---- streaming, determinism, capacity ----
def test_streaming_and_repeat_are_bit_identical(sets):
    images = [(im[0], im[2]) for im in sets["A"]]
    runs = [_run(images), _run(images, split=[3, 1, 2]), _run(images, split=[1] * 6), _run(images)]
    n = len(runs[0][0]["prob"])
    for got, ev in runs[1:]:
        assert torch.equal(ev.keys[:n], runs[0][1].keys[:n]) and torch.equal(ev.state, runs[0][1].state)
        for k in ("precision", "recall", "prob", "tp"):
            assert np.array_equal(got[k], runs[0][0][k])
        assert got["mAP"] == runs[0][0]["mAP"] and got["loc_error"] == runs[0][0]["loc_error"]


def test_capacity_overflow_raises_and_reset_recovers(sets):
    DE, _ = _mods()
    images = [(im[0], im[2]) for im in sets["B"]]
    want = _ref(images)
    n = len(want["prob"])
    ev = DE.DetectorEvaluator(23, 37, DEV, n - 1)
    _feed(ev, images)                      # completes: the record over capacity only sets the flag
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="capacity"):
        ev.compute_pr()
    ev.reset()
    _feed(ev, images[:2])                  # the same evaluator is usable again
    r = ev.result()
    _check({k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in r.items()}, _ref(images[:2]))
    got, _ = _run(images, capacity=n)      # exactly enough
    _check(got, want)


def test_bad_arguments_are_refused():
    DE, L = _mods()
    with pytest.raises(ValueError, match="distance_thresh"):
        DE.DetectorEvaluator(24, 32, DEV, 100, distance_thresh=8.1)
    keys, state = torch.empty(16, dtype=torch.int64, device=DEV), L.detector_eval_state(DEV)
    prob, lab = torch.zeros(1, 24, 32, device=DEV), torch.zeros(1, 24, 32, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="r2"):
        L.op_detector_tp_fp(prob, lab, keys, state, r2=L.DET_EVAL_MAX_R2 + 1)
    with pytest.raises(RuntimeError, match="remove_zero"):
        L.op_detector_tp_fp(prob, lab, keys, state, remove_zero=-1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        L.op_detector_tp_fp(prob.cpu(), lab, keys, state)
    assert int(state.abs().sum()) == 0


# ---- drop-ins ----
def test_drop_ins_on_reference_files(g20, sets, tmp_path):
    DE, _ = _mods()
    for name, variant, dt in (("A", "dense", 2), ("B", "nms", 3)):
        d = tmp_path / ("%s_%s" % (name, variant))
        d.mkdir()
        for i, (prob, prob_nms, kp) in enumerate(sets[name]):
            extra = {"prob_nms": prob_nms} if variant == "nms" else {}
            np.savez(str(d / ("%d.npz" % i)), prob=prob, keypoint_map=kp.astype(np.int32), **extra)
        for s in G.SIMPLIFIED:
            key = G.case_key(name, variant, s, dt)
            precision, recall, prob = DE.compute_pr(str(d), distance_thresh=dt, simplified=s)
            assert np.array_equal(precision, g20[key + "/precision"]) and np.array_equal(recall, g20[key + "/recall"])
            assert prob.dtype == np.float32 and np.array_equal(prob, g20[G.case_key(name, variant) + "/prob"])
            assert abs(DE.compute_mAP(precision, recall) - g20[key + "/mAP"]) <= len(prob) * EPS
            tp, fp, p0, n_gt = DE.compute_tp_fp(np.load(str(d / "0.npz")), distance_thresh=dt, simplified=s)
            assert np.array_equal(tp, g20[key + "/tp/0"]) and np.array_equal(fp, ~tp) and n_gt == g20[key + "/n_gt"][0]
            assert np.array_equal(p0, g20[G.case_key(name, variant) + "/prob_sorted/0"])
        loc = DE.compute_loc_error(str(d), prob_thresh=G.PROB_THRESH, distance_thresh=dt)
        assert abs(loc - g20[G.case_key(name, variant, None, dt) + "/loc_error"]) <= len(prob) * EPS


# ---- evaluate_detector and the trainer ----
ARCH = "SuperPointNet_gauss2"


def _shapes_cfg(B):
    from tests import shapes_ref
    with open(os.path.join(HERE, "golden", "g18_shapes_config.json")) as f:
        cfg = json.load(f)
    data = shapes_ref.small_config(cfg["data"])
    data["generation"] = dict(data["generation"], image_size=[384, 512])
    data["preprocessing"] = dict(data["preprocessing"], resize=[48, 64])
    return {"data": data, "model": dict(cfg["model"], batch_size=B, eval_batch_size=B, real_batch_size=B, multi_task_loss=False)}


def _seeded_net():
    from oracle import cpu_ref as C
    from semantic_superpoint_amd.models import SuperPointNet_gauss2
    net = SuperPointNet_gauss2().to(DEV)
    sd = C.init_state_dict(ARCH, seed=11)
    net.load_state_dict({k: torch.as_tensor(np.array(v)) for k, v in sd.items()})
    net.eval()
    return net


def test_evaluate_detector_on_synthetic_shapes():
    DE, _ = _mods()
    from semantic_superpoint_amd import shapes
    B, H, W = 4, 48, 64
    loader = shapes.SyntheticShapes(_shapes_cfg(B), "val", device=DEV, seed=3, length=2)
    net = _seeded_net()
    res = DE.evaluate_detector(net, loader)
    images = []
    eng = net.engine(B, H, W, torch.device(DEV))
    for s in loader:   # the validation feed repeats itself: the same batches again, maps copied to the host
        eng.forward(s["image"].float().contiguous(), slot=0, train=False, want=("semi",))
        heat = eng.detector_heatmap(0, B, H, W).cpu().numpy()[:, 0]
        lab = s["labels_2D"].cpu().numpy()[:, 0]
        images += [(heat[b], (lab[b] != 0).astype(np.uint8)) for b in range(B)]
    assert sum(int(kp.sum()) for _, kp in images) > 0
    _check({k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in res.items()}, _ref(images))
    # the NMS point path: the points of describe_points against the same labels
    res = DE.evaluate_detector(net, loader, nms_dist=4, conf_thresh=1.0 / 65.0 + 1e-4)
    pts_images = []
    for j, s in enumerate(loader):
        eng.forward(s["image"].float().contiguous(), slot=0, train=False, want=("semi", "desc"))
        d = eng.describe_points(0, B, conf_thresh=1.0 / 65.0 + 1e-4, nms_dist=4, subpixel=False)
        pts, cnt = d["pts"].cpu().numpy(), d["count"].cpu().numpy()
        pts_images += [((pts[b, :cnt[b]],), images[j * B + b][1]) for b in range(B)]
    _check({k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in res.items()}, R.evaluate(pts_images))


class _Writer:
    def __init__(self):
        self.scalars = {}

    def add_scalar(self, name, value, n_iter=0):
        self.scalars.setdefault(name, []).append(float(value))

    def add_histogram(self, *a, **k):
        pass


def _train_round(tmp_path, on):
    """One training step, then a validation round of 2 steps (validation_size 0: train() stops after j = 1)."""
    from semantic_superpoint_amd import shapes
    from semantic_superpoint_amd.Train_model_heatmap_all import Train_model_heatmap_all as T
    B = 2
    c = _shapes_cfg(B)
    c["data"] = dict(c["data"], gaussian_label={"enable": True})
    c.update({"validation_interval": 1, "validation_size": 0, "tensorboard_interval": 10 ** 9, "save_interval": 10 ** 9,
              "train_iter": 1, "retrain": True, "reset_iter": True})
    if on:
        c["ssp_detector_map"] = True
    torch.manual_seed(0)
    a = T(copy.deepcopy(c), save_path=str(tmp_path), device=DEV)
    a.loadModel()
    a.dataParallel()
    a.writer = _Writer()
    a.train_loader = shapes.SyntheticShapes(c, "train", device=DEV, seed=1, length=1)
    a.val_loader = shapes.SyntheticShapes(c, "val", device=DEV, seed=1, length=4)
    fed = []
    if on:
        inner = a.log_detector_map

        def spy(eng, dev, B, H, W):
            fed.append((eng.detector_heatmap(0, B, H, W).clone(), dev["labels_2D"].clone()))
            inner(eng, dev, B, H, W)
        a.log_detector_map = spy
    a.train()
    return a, fed


def test_trainer_logs_detector_map_per_round(tmp_path):
    DE, _ = _mods()
    on, fed = _train_round(tmp_path / "on", True)
    off, _ = _train_round(tmp_path / "off", False)
    new = {"val-detector_mAP_round", "val-detector_loc_err_round"}
    assert set(on.writer.scalars) == set(off.writer.scalars) | new and not new & set(off.writer.scalars)
    assert off.detector_eval_val is None
    assert len(fed) == 2 and len(on.writer.scalars["val-detector_mAP_round"]) == 1
    ev = DE.DetectorEvaluator(48, 64, DEV, 2 * 2 * 48 * 64)
    for heat, lab in fed:
        ev.update(prob=heat, labels=lab.float().contiguous())
    r = ev.result()
    assert on.writer.scalars["val-detector_mAP_round"][0] == r["mAP"] and 0.0 <= r["mAP"] <= 1.0
    assert _same_nan(on.writer.scalars["val-detector_loc_err_round"][0], r["loc_error"], 0.0)
    images = [(h[b, 0].cpu().numpy(), (l[b, 0] != 0).cpu().numpy().astype(np.uint8)) for h, l in fed for b in range(2)]
    _check({k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in r.items()}, _ref(images))


# ---- the evaluator's own rules ----
def test_point_rows_outside_the_image_are_counted(sets):
    DE, L = _mods()
    prob, _, kp = sets["B"][0]
    H, W = kp.shape
    pts, cnt = G.point_list(prob)
    pts = np.asarray(pts, np.float32)[:cnt][:40].copy()
    bad = [3, 11, 29]
    pts[3, 0], pts[11, 1], pts[29, 0] = W, -1.0, np.nan      # right of the image, above it, not a number
    inside = np.delete(pts, bad, axis=0)
    ev = DE.DetectorEvaluator(H, W, DEV, 64)
    ev.update(pts=_t(pts[None]), count=_t(np.array([len(pts)], np.int32)), labels=_t(kp[None].astype(np.uint8)))
    with pytest.warns(UserWarning, match="outside"):
        r = ev.result()
    assert r["outside_points"] == 3 and int(ev.state[L.DET_EVAL_OUTSIDE]) == 3
    _check({k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in r.items()}, R.evaluate([((inside,), kp)]))
    got, _ = _run([(prob, kp)], points=True)                 # a list inside the image counts none
    assert got["outside_points"] == 0


def test_prob_thresh_below_remove_zero_is_refused():
    DE, L = _mods()
    with pytest.raises(ValueError, match="prob_thresh"):
        DE.DetectorEvaluator(24, 32, DEV, 100, remove_zero=0.3, prob_thresh=0.2)
    keys, state = torch.empty(16, dtype=torch.int64, device=DEV), L.detector_eval_state(DEV)
    prob, lab = torch.zeros(1, 24, 32, device=DEV), torch.zeros(1, 24, 32, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="prob_thresh"):
        L.op_detector_tp_fp(prob, lab, keys, state, remove_zero=0.3, prob_thresh=0.2)
    assert int(state.abs().sum()) == 0
    DE.DetectorEvaluator(24, 32, DEV, 100, remove_zero=0.5, prob_thresh=0.5)   # equal is fine


def test_reserve_keeps_what_was_fed(sets):
    DE, _ = _mods()
    images = [(im[0], im[2]) for im in sets["A"]]
    want = _ref(images)
    ev = DE.DetectorEvaluator(24, 32, DEV, 2 * 24 * 32)
    _feed(ev, images[:2])
    ev.reserve(100)                                          # smaller: nothing happens
    assert ev.capacity == 2 * 24 * 32
    ev.reserve(6 * 24 * 32)
    _feed(ev, images[2:], split=[3, 1])
    r = ev.result()
    _check({k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in r.items()}, want)
    assert isinstance(ev._final["mAP"], float) and ev.compute_mAP() == r["mAP"]   # the scalar was read once and kept
    with pytest.raises(ValueError, match="capacity"):
        ev.reserve(2 ** 31)


def test_trainer_refuses_a_round_that_cannot_fit(tmp_path):
    from semantic_superpoint_amd.Train_model_heatmap_all import Train_model_heatmap_all as T
    c = _shapes_cfg(2)
    c["data"] = dict(c["data"], gaussian_label={"enable": True})
    c.update({"validation_interval": 1, "validation_size": 2 ** 31 // (2 * 48 * 64), "tensorboard_interval": 10, "save_interval": 10,
              "train_iter": 1, "retrain": True, "reset_iter": True})
    T(copy.deepcopy(c), save_path=str(tmp_path), device=DEV)            # off: the size of a round is nobody's business
    c["ssp_detector_map"] = True
    with pytest.raises(ValueError, match="validation_size"):
        T(copy.deepcopy(c), save_path=str(tmp_path), device=DEV)
    c["validation_size"] = 2 ** 31 // (2 * 48 * 64) - 3                 # (validation_size + 2) x 2 x 48 x 64 < 2^31
    a = T(copy.deepcopy(c), save_path=str(tmp_path), device=DEV)
    assert a._detector_capacity(1, 2, 48, 64) < 2 ** 31
