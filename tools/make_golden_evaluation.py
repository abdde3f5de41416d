"""G16 fixtures of the evaluation step (evaluation.py:86-500 with -r -homo), produced by the REAL reference on the CPU.

  g16_evaluation.npz   for the export pairs of tests/golden_evaluation.py (regenerated from their seeds):
                       compute_repeatability per case (keep_k_points=1000, distance_thresh=3), the matching score's
                       unwarped-point count (warpLabels of evaluation.py:194-216), the reference's evaluate() run end to
                       end on the CASES folder (its result.npz arrays and result.txt), and average_precision_score on
                       the (label, distance) vectors of AP_CASES

OpenCV is absent, so a cv2 stub goes into sys.modules before the reference's evaluate() runs: BFMatcher is a numpy
mutual nearest neighbour on exact L2 distances, findHomography a small deterministic numpy RANSAC.  The synthetic pairs
make their outputs unique (every match an exact inlier or a > 25 px outlier, large descriptor margins); the near-tie
guards below assert it.  Needs the reference checkout (oracle/ref_harness.py); from the repository root:
  python tools/make_golden_evaluation.py
"""
import argparse
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_harness as R  # noqa: E402
from tests.golden_evaluation import AP_CASES, CASES, EMPTY_CASE, ap_case, case_pair  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g16_evaluation.npz")


class _DMatch:
    def __init__(self, q, t, d):
        self.queryIdx, self.trainIdx, self.distance = int(q), int(t), float(d)


class _BFMatcher:
    def __init__(self, norm, crossCheck=False):
        assert crossCheck

    def match(self, a, b):
        d = np.sqrt(np.maximum(((a.astype(np.float64)[:, None, :] - b.astype(np.float64)[None]) ** 2).sum(-1), 0))
        r, c = d.argmin(1), d.argmin(0)
        for i in range(d.shape[0]):  # margins of the mutual rows: the unique-by-construction guard
            s = np.sort(d[i])
            assert c[r[i]] != i or len(s) < 2 or s[1] - s[0] > 1e-4, "G16: near-tie in a row of the crossCheck matcher"
        return [_DMatch(i, r[i], d[i, r[i]]) for i in range(d.shape[0]) if c[r[i]] == i]


def _dlt(p, q):
    A = []
    for (x, y), (u, v) in zip(p, q):
        A.append([x, y, 1, 0, 0, 0, -x * u, -y * u, -u])
        A.append([0, 0, 0, x, y, 1, -x * v, -y * v, -v])
    H = np.linalg.svd(np.asarray(A))[2][-1].reshape(3, 3)
    return H / H[2, 2]


def _find_homography(src, dst, method=None, thresh=3.0):
    src, dst = np.asarray(src, np.float64).reshape(-1, 2), np.asarray(dst, np.float64).reshape(-1, 2)
    n = src.shape[0]
    if n < 4:
        return None, None
    rng = np.random.default_rng(0)
    best = None
    for _ in range(500):
        idx = rng.choice(n, 4, replace=False)
        H = _dlt(src[idx], dst[idx])
        w = np.concatenate([src, np.ones((n, 1))], 1) @ H.T
        err = np.linalg.norm(w[:, :2] / w[:, 2:] - dst, axis=1)
        m = err <= thresh
        if best is None or m.sum() > best.sum():
            best = m
    H = _dlt(src[best], dst[best])
    return H, best.astype(np.uint8)[:, None]


def _guards(data):
    """No float64 warped coordinate or distance within 1e-9 of a bound or threshold unless exactly on it; the float32
    warp of the matching score at least 1e-3 from its bounds unless exactly on them."""
    from evaluations.detector_evaluation import warp_keypoints
    Hh, Ww = data["image"].shape
    H = data["homography"]

    def check(v, b, tol):
        gap = np.abs(v - b)
        assert np.all((gap == 0) | (gap > tol)), "G16: value within %g of bound %g" % (tol, b)

    if data["warped_prob"].shape[0]:
        w2 = warp_keypoints(data["warped_prob"][:, :2], np.linalg.inv(H))
        check(w2[:, 0], 0, 1e-9), check(w2[:, 0], Ww, 1e-9), check(w2[:, 1], 0, 1e-9), check(w2[:, 1], Hh, 1e-9)
    if data["prob"].shape[0]:
        w1 = warp_keypoints(data["prob"][:, :2], H)
        check(w1[:, 0], 0, 1e-9), check(w1[:, 0], Ww, 1e-9), check(w1[:, 1], 0, 1e-9), check(w1[:, 1], Hh, 1e-9)
        if data["warped_prob"].shape[0]:
            d = np.linalg.norm(w1[:, None] - data["warped_prob"][None, :, :2], axis=2)
            check(d.min(1), 3.0, 1e-9), check(d.min(0), 3.0, 1e-9)
    if data["warped_prob"].shape[0]:
        p = np.trunc(data["warped_prob"][:, [1, 0]]).astype(np.float32)
        Hf = np.linalg.inv(H).astype(np.float32)
        w = np.concatenate([p, np.ones((p.shape[0], 1), np.float32)], 1) @ Hf.T
        u = w[:, :2] / w[:, 2:]
        check(u[:, 0], 0, 1e-3), check(u[:, 0], Ww - 1, 1e-3), check(u[:, 1], 0, 1e-3), check(u[:, 1], Hh - 1, 1e-3)
    if data["desc"].shape[0] and data["warped_desc"].shape[0]:  # nn 1.2 matcher: distances of linked pairs apart
        dd = data["desc"] @ data["warped_desc"].T
        d = np.sqrt(2 - 2 * np.clip(dd, -1, 1))
        r, c = d.argmin(1), d.argmin(0)
        keep = c[r] == np.arange(d.shape[0])
        dm = np.sort(d[np.arange(d.shape[0]), r][keep])
        assert np.all(np.abs(dm - 1.2) > 1e-3) and (len(dm) < 2 or np.min(np.diff(dm)) > 1e-5), "G16: match distance tie"


def _unwarped_count(data):
    import torch as T
    from utils.utils import filter_points, warp_points
    Hh, Ww = data["image"].shape
    pnts = T.tensor(data["warped_prob"][:, [1, 0]]).long()
    hom = T.tensor(np.linalg.inv(data["homography"]), dtype=T.float32)
    w = warp_points(T.stack((pnts[:, 0], pnts[:, 1]), dim=1), hom)
    return int(filter_points(w, T.tensor([Ww, Hh])).shape[0])


def main():
    argparse.ArgumentParser(description=__doc__.splitlines()[0]).parse_args()
    R.install()
    cv2 = sys.modules["cv2"]
    cv2.BFMatcher, cv2.NORM_L2, cv2.NORM_HAMMING, cv2.RANSAC = _BFMatcher, 4, 6, 8
    cv2.findHomography = lambda s, d, m=None, *a, **k: _find_homography(s, d, m)
    import types
    for name, attrs in (("coloredlogs", {"install": lambda *a, **k: None}),
                        ("termcolor", {"colored": lambda t, *a, **k: t, "cprint": print})):
        if name not in sys.modules:
            try:
                __import__(name)
            except ImportError:
                mod = types.ModuleType(name)
                mod.__dict__.update(attrs)
                sys.modules[name] = mod
    from evaluations.detector_evaluation import compute_repeatability
    from sklearn.metrics import average_precision_score
    import evaluation as ref_eval

    torch.set_num_threads(1)
    out = {}
    allc = CASES + [EMPTY_CASE]
    rep, loc, unw = [], [], []
    for c in allc:
        data, _ = case_pair(c)
        _guards(data)
        r, l = compute_repeatability({k: v.copy() for k, v in data.items()}, keep_k_points=1000, distance_thresh=3)
        # evaluate() keeps loc_err only when > 0: an all-exact case (loc_err 0 up to rounding) would flip that filter
        assert l == -1 or l > 1e-9, "G16: localisation error within rounding of 0"
        rep.append(float(r))
        loc.append(float(l))
        unw.append(_unwarped_count(data))
    out["case_seed"] = np.array([c[1] for c in allc])
    out["rep"], out["loc_err"], out["n_unwarped"] = np.array(rep), np.array(loc), np.array(unw)
    out["ap"] = np.array([average_precision_score(l, d.max() - d.astype(np.float64))
                          for l, d in (ap_case(*a) for a in AP_CASES)])
    with tempfile.TemporaryDirectory() as tmp:
        for k, c in enumerate(CASES):
            data, _ = case_pair(c)
            np.savez(os.path.join(tmp, "%d.npz" % k), **data)
        args = argparse.Namespace(path=tmp, sift=False, outputImg=False, repeatibility=True, homography=True,
                                  plotMatching=False, split=False)
        ref_eval.evaluate(args)
        res = np.load(os.path.join(tmp, "result.npz"))
        for k in res.files:
            out["result_" + k] = res[k]
        with open(os.path.join(tmp, "result.txt")) as f:
            out["result_txt"] = np.array(f.read().replace(tmp, "<path>"))
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")
    for k in ("rep", "loc_err", "n_unwarped", "ap"):
        print(k, out[k])
    print(out["result_txt"])


if __name__ == "__main__":
    main()
