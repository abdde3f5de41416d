"""Evaluation of descriptor exports (evaluation.py:86-500) without a GPU: the C ABI is declared and exported, the G16
fixture inputs regenerate from their seeds, the numpy restatement of the device RANSAC reproduces the reference's
homography outputs, the summary writer reproduces result.txt / result.npz, and the unsupported flags are refused."""
import argparse
import os
import re

import numpy as np
import pytest

from tests import eval_restatement as ER
from tests.golden_evaluation import AP_CASES, CASES, EMPTY_CASE, ap_case, case_pair

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G16 = os.path.join(ROOT, "tests", "golden", "g16_evaluation.npz")
NEW = ("ssp_eval_repeatability", "ssp_eval_ransac_workspace_bytes", "ssp_eval_ransac")


def g16():
    return np.load(G16)


def test_symbols_declared_and_exported():
    from semantic_superpoint_amd import lib
    with open(os.path.join(ROOT, "include", "ssp_hip.h")) as f:
        hdr = f.read()
    for n in NEW:
        assert re.search(r"\b%s\(" % n, hdr), n
        assert n in lib.EXPORTS, n
    for n in ("op_eval_repeatability", "op_eval_ransac"):
        assert callable(getattr(lib, n))


def _repeatability_np(data, k=1000, thr=3.0):
    """compute_repeatability restated in numpy (detector_evaluation.py:153-275) -> (rep, loc_err)."""
    H = data["homography"]
    hh, ww = data["image"].shape

    def warp(p, M):
        w = np.dot(np.concatenate([p, np.ones((p.shape[0], 1))], 1), M.T)
        return w[:, :2] / w[:, 2:]

    def inside(p):
        return (p[:, 0] >= 0) & (p[:, 0] < ww) & (p[:, 1] >= 0) & (p[:, 1] < hh)

    w2 = data["warped_prob"]
    w2 = w2[inside(warp(w2[:, :2], np.linalg.inv(H)))]
    p1 = data["prob"].copy()
    p1[:, :2] = warp(p1[:, :2], H)
    p1 = p1[inside(p1)]
    a = p1[np.argsort(p1[:, 2]), :2][-min(k, len(p1)):] if len(p1) else p1[:, :2]
    b = w2[np.argsort(w2[:, 2]), :2][-min(k, len(w2)):] if len(w2) else w2[:, :2]
    c1 = c2 = 0
    s = 0.0
    if len(a) and len(b):
        d = np.linalg.norm(a[:, None] - b[None], axis=2)
        m1, m2 = d.min(1), d.min(0)
        c1, c2 = np.sum(m1 <= thr), np.sum(m2 <= thr)
        if c1 + c2:
            s = m1[m1 <= thr].sum() / (c1 + c2) + m2[m2 <= thr].sum() / (c1 + c2)
    if c1 + c2 == 0:
        return 0, -1
    return (c1 + c2) / (len(a) + len(b)), s


def test_seeds_regenerate_fixture_inputs():
    f = g16()
    allc = CASES + [EMPTY_CASE]
    assert list(f["case_seed"]) == [c[1] for c in allc]
    for k, c in enumerate(allc):
        data, _ = case_pair(c)
        rep, loc = _repeatability_np(data)
        assert rep == f["rep"][k], c[0]
        assert abs(loc - f["loc_err"][k]) <= 1e-12 * max(1.0, abs(loc)), c[0]
    assert f["rep"][-1] == 0 and f["loc_err"][-1] == -1  # the empty side


def _mutual_nn(a, b, thresh=np.inf):
    d = np.sqrt(np.maximum(2 - 2 * np.clip(a.astype(np.float32) @ b.astype(np.float32).T, -1, 1), 0))
    r, c = d.argmin(1), d.argmin(0)
    i = np.nonzero((c[r] == np.arange(len(r))) & (d[np.arange(len(r)), r] < thresh))[0]
    return i, r[i], d[i, r[i]]


def test_restatement_reproduces_g16_homography():
    from semantic_superpoint_amd.evaluation import correctness_of, pair_seeds
    f = g16()
    for k, c in enumerate(CASES):
        data, _ = case_pair(c)
        s_cc, s_nn = pair_seeds([k])
        i, j, _ = _mutual_nn(data["desc"], data["warped_desc"])
        m = np.concatenate([data["prob"][i, :2], data["warped_prob"][j, :2]], 1)
        r = ER.ransac(m, int(s_cc[0]))
        assert r["status"] == 0
        corr = correctness_of(r["H"], data["homography"])
        np.testing.assert_array_equal(corr, f["result_correctness"][k], err_msg=c[0])
        ms = 2 * r["mask"].sum() / (data["prob"].shape[0] + f["n_unwarped"][k])
        assert ms == f["result_mscore"][k], c[0]
        i, j, d = _mutual_nn(data["desc"], data["warped_desc"], 1.2)
        m = np.concatenate([data["prob"][i, :2], data["warped_prob"][j, :2]], 1)
        r = ER.ransac(m, int(s_nn[0]), scores=d)
        assert abs(r["ap"] - f["result_mAP"][k]) <= 1e-12, c[0]


def test_restatement_average_precision_matches_sklearn_record():
    f = g16()
    for k, a in enumerate(AP_CASES):
        labels, d = ap_case(*a)
        assert abs(ER.average_precision(labels, -d.astype(np.float64)) - f["ap"][k]) <= 1e-12


def test_restatement_degenerate_sizes():
    rng = np.random.default_rng(3)
    for n in range(4):
        r = ER.ransac(rng.uniform(0, 100, (n, 4)), 5, scores=np.ones(n))
        assert r["status"] == 1 and r["ap"] == 0.0 and not r["mask"].any()
    line = np.stack([np.arange(10.0), 2 * np.arange(10.0) + 1, np.arange(10.0) + 5, np.arange(10.0)], 1)
    assert ER.ransac(line, 7)["status"] == 1


def test_summary_writer_reproduces_reference(tmp_path):
    from semantic_superpoint_amd.evaluation import summarize
    f = g16()
    n = len(CASES)
    files = ["%d.npz" % k for k in range(n)]
    per = []
    for k in range(n):
        rep = f["rep"][k]
        per.append({"rep": np.float64(rep) if rep > 0 else 0, "loc_err": f["loc_err"][k],
                    "correctness": f["result_correctness"][k], "mscore": np.float64(f["result_mscore"][k]),
                    "mAP": float(f["result_mAP"][k])})
    out = summarize(str(tmp_path), files, per, True, True)
    with open(tmp_path / "result.txt") as fh:
        txt = fh.read().replace(str(tmp_path), "<path>")
    assert txt == str(f["result_txt"])
    res = np.load(tmp_path / "result.npz")
    for k in res.files:
        np.testing.assert_array_equal(res[k], f["result_" + k], err_msg=k)
    assert set(out) == set(res.files)


@pytest.mark.parametrize("flag", ["sift", "outputImg", "plotMatching", "split"])
def test_refusals(flag, tmp_path):
    from semantic_superpoint_amd.evaluation import evaluate, main
    args = argparse.Namespace(path=str(tmp_path), sift=False, outputImg=False, repeatibility=True, homography=True,
                              plotMatching=False, split=False)
    setattr(args, flag, True)
    with pytest.raises(ValueError, match="not supported"):
        evaluate(args)
    opt = {"sift": "--sift", "outputImg": "-o", "plotMatching": "-plm", "split": "-s"}[flag]
    with pytest.raises(SystemExit):
        main([str(tmp_path), "-r", opt])
