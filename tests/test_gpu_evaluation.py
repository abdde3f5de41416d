"""GPU: evaluation of descriptor exports (evaluation.py:86-500 with -r -homo) against the real reference (G16 fixtures,
tools/make_golden_evaluation.py) and against the numpy restatement of the device RANSAC (tests/eval_restatement.py)."""
import argparse
import os

import numpy as np
import pytest
import torch

from tests import eval_restatement as ER
from tests.golden_evaluation import AP_CASES, CASES, EMPTY_CASE, ap_case, ap_matches, case_pair

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G16 = os.path.join(ROOT, "tests", "golden", "g16_evaluation.npz")
DEV = "cuda:0"


def _ident_matches(m, cap=None):
    """Device inputs of the RANSAC for a list of [n,4] match sets (match k = row k of both sides)."""
    P = len(m)
    cap = cap or max(1, max(x.shape[0] for x in m))
    p1, p2 = np.zeros((P, cap, 3)), np.zeros((P, cap, 3))
    mt = np.zeros((P, cap, 3), np.float32)
    for p, x in enumerate(m):
        n = x.shape[0]
        p1[p, :n, :2], p2[p, :n, :2] = x[:, :2], x[:, 2:]
        mt[p, :n, 0] = mt[p, :n, 1] = np.arange(n)
    nm = torch.tensor([x.shape[0] for x in m], dtype=torch.int32, device=DEV)
    t = lambda a: torch.from_numpy(a).to(DEV)  # noqa: E731
    return t(p1), t(p2), t(mt), nm


def _ransac(m, seeds, scores=None):
    from semantic_superpoint_amd import lib as L
    p1, p2, mt, nm = _ident_matches(m)
    if scores is not None:
        for p, s in enumerate(scores):
            mt[p, :len(s), 2] = torch.from_numpy(np.asarray(s, np.float32)).to(DEV)
    o = L.op_eval_ransac(p1, p2, mt, nm, torch.tensor(seeds, dtype=torch.int64, device=DEV), want_ap=scores is not None)
    return {k: v.cpu().numpy() for k, v in o.items()}


def test_repeatability_and_unwarped_counts_against_g16():
    from semantic_superpoint_amd.evaluation import Evaluator, _upload
    f = np.load(G16)
    allc = CASES + [EMPTY_CASE]
    datas = [case_pair(c)[0] for c in allc]
    pts, cnt, desc = _upload(datas, torch.device(DEV))
    ev = Evaluator(240, 320, True, True)
    res = ev.run_points(pts, cnt, desc, np.stack([d["homography"] for d in datas]), list(range(len(allc))))
    from semantic_superpoint_amd import lib as L
    Hs = np.stack([d["homography"] for d in datas])
    raw = L.op_eval_repeatability(pts, cnt, pts[1:], cnt[1:], torch.from_numpy(Hs).to(DEV),
                                  torch.from_numpy(np.stack([np.linalg.inv(h) for h in Hs])).to(DEV), 240, 320,
                                  pair_stride=2, n_pairs=len(allc)).cpu().numpy()
    for k, c in enumerate(allc):
        assert res[k]["rep"] == f["rep"][k], c[0]
        loc = res[k]["loc_err"]
        assert abs(loc - f["loc_err"][k]) <= 1e-12 * max(1.0, abs(f["loc_err"][k])), c[0]
        assert raw[k][6] == f["n_unwarped"][k], c[0]


def test_average_precision_against_sklearn_record():
    f = np.load(G16)
    ms, ds = [], []
    for a in AP_CASES:
        labels, d = ap_case(*a)
        p, q, _ = ap_matches(labels, a[0])
        ms.append(np.concatenate([p, q], 1))
        ds.append(d)
    o = _ransac(ms, list(range(len(ms))), ds)
    for k, a in enumerate(AP_CASES):
        labels, _ = ap_case(*a)
        assert o["status"][k] == 0
        np.testing.assert_array_equal(o["mask"][k, :labels.size].astype(bool), labels)
        assert abs(o["ap"][k] - f["ap"][k]) <= 1e-12, a


def _random_sets(seed, count=6):
    rng = np.random.default_rng(seed)
    sets, truth = [], []
    for k in range(count):
        n = int(rng.integers(40, 400))
        H = np.array([[1 + rng.uniform(-.1, .1), rng.uniform(-.1, .1), rng.uniform(-20, 20)],
                      [rng.uniform(-.1, .1), 1 + rng.uniform(-.1, .1), rng.uniform(-20, 20)],
                      [rng.uniform(-3e-4, 3e-4), rng.uniform(-3e-4, 3e-4), 1.0]])
        p = np.stack([rng.uniform(0, 320, n), rng.uniform(0, 240, n)], 1)
        w = np.concatenate([p, np.ones((n, 1))], 1) @ H.T
        q = w[:, :2] / w[:, 2:] + rng.normal(0, 0.5 * (k % 2), (n, 2))
        out = rng.uniform(size=n) < 0.6 * k / max(count - 1, 1)  # outlier fractions up to 0.6
        q[out] = q[out] + rng.uniform(25, 80, (out.sum(), 2)) * rng.choice([-1, 1], (out.sum(), 2))
        sets.append(np.concatenate([p, q], 1))
        truth.append((H, out))
    return sets, truth


def test_device_ransac_equals_restatement():
    sets, _ = _random_sets(11)
    seeds = [101 + k for k in range(len(sets))]
    scores = [np.random.default_rng(k).uniform(0.1, 1.0, s.shape[0]).astype(np.float32) for k, s in enumerate(sets)]
    o = _ransac(sets, seeds, scores)
    for k, m in enumerate(sets):
        r = ER.ransac(m, seeds[k], scores=scores[k])
        assert o["status"][k] == r["status"] == 0
        near = np.abs(ER.resid2(r["H"].reshape(1, 9), m)[0] - 9.0) <= 1e-6
        dm = o["mask"][k, :m.shape[0]].astype(bool)
        assert np.all((dm == r["mask"]) | near)
        np.testing.assert_allclose(o["H"][k], r["H"], rtol=1e-9, atol=1e-9 * np.abs(r["H"]).max())
        assert abs(o["ap"][k] - r["ap"]) <= 1e-12


def _corner_err(H, G):
    c = np.array([[0, 0, 1], [0, 239, 1], [319, 0, 1], [319, 239, 1]], float)
    a, b = c @ H.T, c @ G.T
    return np.linalg.norm(a[:, :2] / a[:, 2:] - b[:, :2] / b[:, 2:], axis=1).mean()


def test_accuracy_against_ground_truth():
    sets, truth = _random_sets(12, 8)
    o = _ransac(sets, list(range(len(sets))))
    for k, (H, out) in enumerate(truth):
        mask = o["mask"][k, :sets[k].shape[0]].astype(bool)
        w = np.concatenate([sets[k][:, :2], np.ones((len(out), 1))], 1) @ H.T
        true_res = np.linalg.norm(w[:, :2] / w[:, 2:] - sets[k][:, 2:], axis=1)
        assert not np.any(mask & (true_res > 20))
        if k % 2 == 0:  # noise-free: the exact inlier set, corner error < 1e-6 px
            np.testing.assert_array_equal(mask, ~out)
            assert _corner_err(o["H"][k], H) < 1e-6
        else:
            assert _corner_err(o["H"][k], H) < 1.0


def test_degenerate_sizes():
    rng = np.random.default_rng(5)
    line = np.stack([np.arange(10.0), 2 * np.arange(10.0) + 1, np.arange(10.0) + 5, np.arange(10.0)], 1)
    four = np.array([[0, 0, 10, 10], [100, 0, 110, 12], [0, 100, 9, 111], [100, 100, 112, 108]], float)
    sets = [rng.uniform(0, 100, (n, 4)) for n in range(4)] + [four, line]
    o = _ransac(sets, [1] * len(sets), [np.ones(max(1, s.shape[0])) for s in sets])
    for k in range(4):
        assert o["status"][k] == 1 and o["n_inliers"][k] == 0 and o["ap"][k] == 0
        np.testing.assert_array_equal(o["H"][k], np.eye(3))
    assert o["status"][4] == 0 and o["n_inliers"][4] == 4 and o["ap"][4] == 1.0
    w = np.concatenate([four[:, :2], np.ones((4, 1))], 1) @ o["H"][4].T
    np.testing.assert_allclose(w[:, :2] / w[:, 2:], four[:, 2:], atol=1e-9)
    assert o["status"][5] == 1


def test_deterministic_and_batch_independent():
    sets, _ = _random_sets(13, 16)
    seeds = list(range(40, 56))
    a, b = _ransac(sets, seeds), _ransac(sets, seeds)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])
    for p in range(16):
        s = _ransac([sets[p]], [seeds[p]])
        np.testing.assert_array_equal(s["H"][0], a["H"][p])
        n = sets[p].shape[0]
        np.testing.assert_array_equal(s["mask"][0, :n], a["mask"][p, :n])


def _write_cases(path):
    for k, c in enumerate(CASES):
        np.savez(os.path.join(path, "%d.npz" % k), **case_pair(c)[0])


def test_evaluate_reproduces_g16_result(tmp_path):
    from semantic_superpoint_amd.evaluation import evaluate
    f = np.load(G16)
    _write_cases(str(tmp_path))
    args = argparse.Namespace(path=str(tmp_path), sift=False, outputImg=False, repeatibility=True, homography=True,
                              plotMatching=False, split=False)
    evaluate(args, batch_pairs=5)
    res = np.load(tmp_path / "result.npz")
    np.testing.assert_array_equal(res["correctness"], f["result_correctness"])
    np.testing.assert_array_equal(res["mscore"], f["result_mscore"])
    np.testing.assert_array_equal(res["homography_thresh"], f["result_homography_thresh"])
    for k in ("repeatability", "localization_err", "mAP"):
        np.testing.assert_allclose(res[k], f["result_" + k], rtol=1e-12, atol=0, err_msg=k)
    with open(tmp_path / "result.txt") as fh:
        lines = fh.read().replace(str(tmp_path), "<path>").splitlines()
    ref = str(f["result_txt"]).splitlines()
    assert len(lines) == len(ref)
    for a, b in zip(lines, ref):  # the same lines; float digits may differ in the last places for the 1e-12 metrics
        assert a.split(":")[0] == b.split(":")[0]
    assert lines[-1] == "======== end ========"


def test_fused_export_and_evaluation_equal_npz_path(tmp_path):
    from oracle import cpu_ref as C
    from semantic_superpoint_amd import models
    from semantic_superpoint_amd.evaluation import Evaluator, evaluate
    from semantic_superpoint_amd.export import DescriptorExporter
    arch = "SuperPointNet_gauss2_ssmall"
    net = getattr(models, arch)()
    net.load_state_dict({k: torch.as_tensor(np.array(v)) for k, v in C.init_state_dict(arch, seed=0).items()})
    net = net.to(DEV).eval()
    ex = DescriptorExporter(net, DEV, conf_thresh=0.0155, nms_dist=4, subpixel=True, nn_thresh=0.7, batch_pairs=4)
    rs = np.random.RandomState(1)
    pairs, Hs = [], []
    for k in range(3):
        a = torch.from_numpy(rs.uniform(0, 1, (240, 320)).astype(np.float32))
        pairs.append((a.to(DEV), torch.roll(a, (2, 3 + k), (0, 1)).to(DEV)))
        Hs.append(np.array([[1.0, 0, 3 + k], [0, 1.0, 2], [0, 0, 1]]))
    fused = Evaluator(240, 320).run_device(ex.run_device(pairs), Hs, [0, 1, 2], subpixel=True)
    for k, pred in enumerate(ex(pairs, homographies=Hs)):
        np.savez(os.path.join(str(tmp_path), "%d.npz" % k), **pred)
    args = argparse.Namespace(path=str(tmp_path), sift=False, outputImg=False, repeatibility=True, homography=True,
                              plotMatching=False, split=False)
    res = evaluate(args)
    assert [r["rep"] for r in fused] == list(res["repeatability"])
    np.testing.assert_array_equal(np.array([r["correctness"] for r in fused]), res["correctness"])
    assert [r["mscore"] for r in fused] == list(res["mscore"])
    assert [r["mAP"] for r in fused] == list(res["mAP"])


def test_refusals():
    from semantic_superpoint_amd import lib as L
    p = torch.zeros(2, 8, 3, dtype=torch.float64, device=DEV)
    c = torch.ones(2, dtype=torch.int32, device=DEV)
    H = torch.eye(3, dtype=torch.float64, device=DEV)[None]
    big = torch.zeros(2, L.MATCH_MAX_POINTS + 1, 3, dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError):
        L.op_eval_repeatability(big, c, big[1:], c[1:], H, H, 240, 320, pair_stride=2, n_pairs=1)
    with pytest.raises(RuntimeError):
        L.op_eval_repeatability(p.cpu(), c, p[1:], c[1:], H, H, 240, 320, pair_stride=2, n_pairs=1)
    with pytest.raises(ValueError):
        L.op_eval_repeatability(p, c, p[1:], c[1:], H[:, :2], H, 240, 320, pair_stride=2, n_pairs=1)
    mt = torch.zeros(1, 8, 3, device=DEV)
    s = torch.zeros(1, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError):
        L.op_eval_ransac(p, p[1:], torch.zeros(1, L.MATCH_MAX_POINTS + 1, 3, device=DEV), c[:1], s)
    with pytest.raises(ValueError):
        L.op_eval_ransac(p.float(), p[1:], mt, c[:1], s)
    with pytest.raises(RuntimeError):
        L.op_eval_ransac(p, p[1:], mt.cpu(), c[:1], s)
