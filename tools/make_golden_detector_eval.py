"""G20 fixture of the detector evaluation, produced by the REAL reference on the CPU.

  g20_detector_eval.npz   for every set of tests/golden_detector_eval.py (A: 6 images of 24x32, B: 4 images of 23x37) and both
                          variants (dense: the files hold `prob`; nms: they also hold `prob_nms`, which compute_tp_fp prefers):
      <set>/checksum                    pins the regenerated inputs
      <set>/<variant>/prob              compute_pr's sorted probabilities
      <set>/<variant>/prob_sorted/<i>   compute_tp_fp's sorted probabilities of image i
      <set>/<variant>/s<simplified>/d<distance_thresh>/tp/<i>, n_gt   compute_tp_fp per image
      <set>/<variant>/s<simplified>/d<distance_thresh>/precision, recall, mAP   compute_pr, compute_mAP
      <set>/<variant>/d<distance_thresh>/loc_error        compute_loc_error (it reads `prob` in both variants)
      <set>/nms/d<distance_thresh>/loc_error_nms          compute_loc_error on files whose `prob` is the nms map

The reference reads per-image .npz files under EXPER_PATH/outputs/<name>/: the tool writes them into a temporary directory and
points EXPER_PATH at it.  It stops unless every probability is unique across a set and none lies within 4 ulp of remove_zero
or prob_thresh: the reference's argsort leaves the order of equal probabilities undefined, and its file order is glob's.
Needs the reference checkout (oracle/ref_harness.py); run from the repository root:
  python tools/make_golden_detector_eval.py
"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_harness as R  # noqa: E402
from tests.golden_detector_eval import (DISTANCE_THRESH, PROB_THRESH, REMOVE_ZERO, SETS, SIMPLIFIED, VARIANTS, _near,  # noqa: E402
                                        case_key, checksum, make_set)

OUT = os.path.join(ROOT, "tests", "golden", "g20_detector_eval.npz")


def guards(name, images):
    for k in (0, 1):
        v = np.concatenate([im[k][im[k] > 0] for im in images])
        assert len(np.unique(v)) == len(v), "%s: equal probabilities" % name
        assert not _near(v, REMOVE_ZERO).any() and not _near(v, PROB_THRESH).any(), "%s: a probability next to a threshold" % name
    n_pred = [int((im[0] > np.float32(REMOVE_ZERO)).sum()) for im in images]
    n_gt = [int(im[2].sum()) for im in images]
    assert min(n_pred) > 200 and min(n_gt) > 10, (n_pred, n_gt)
    return n_pred, n_gt


def write_files(tmp, exper, images, variant):
    d = os.path.join(tmp, "outputs", exper)
    os.makedirs(d)
    for i, (prob, prob_nms, kp) in enumerate(images):
        if variant == "dense":
            np.savez(os.path.join(d, "%d.npz" % i), prob=prob, keypoint_map=kp)
        elif variant == "nms":
            np.savez(os.path.join(d, "%d.npz" % i), prob=prob, prob_nms=prob_nms, keypoint_map=kp)
        else:  # the nms map as `prob`: compute_loc_error of the point-list input
            np.savez(os.path.join(d, "%d.npz" % i), prob=prob_nms, keypoint_map=kp)
    return d


if __name__ == "__main__":
    R.install()
    import settings
    from evaluations import detector_evaluation as D
    tmp = tempfile.mkdtemp()
    settings.EXPER_PATH = tmp
    D.EXPER_PATH = tmp
    out = {}
    for name in SETS:
        images = make_set(name)
        n_pred, n_gt = guards(name, images)
        out[name + "/checksum"] = checksum(images)
        for variant in VARIANTS:
            exper = "%s_%s" % (name, variant)
            d = write_files(tmp, exper, images, variant)
            base = case_key(name, variant)
            for s in SIMPLIFIED:
                for dt in DISTANCE_THRESH:
                    key = case_key(name, variant, s, dt)
                    ngt = []
                    for i in range(len(images)):
                        tp, fp, prob, n = D.compute_tp_fp(np.load(os.path.join(d, "%d.npz" % i)), remove_zero=REMOVE_ZERO,
                                                          distance_thresh=dt, simplified=s)
                        assert np.array_equal(fp, ~tp)
                        out["%s/tp/%d" % (key, i)] = tp
                        out["%s/prob_sorted/%d" % (base, i)] = prob
                        ngt.append(int(n))
                    out[key + "/n_gt"] = np.array(ngt, np.int64)
                    precision, recall, prob = D.compute_pr(exper, remove_zero=REMOVE_ZERO, distance_thresh=dt, simplified=s)
                    out[key + "/precision"], out[key + "/recall"], out[base + "/prob"] = precision, recall, prob
                    out[key + "/mAP"] = np.float64(D.compute_mAP(precision, recall))
            for dt in DISTANCE_THRESH:
                out[case_key(name, variant, None, dt) + "/loc_error"] = np.float64(
                    D.compute_loc_error(exper, prob_thresh=PROB_THRESH, distance_thresh=dt))
        write_files(tmp, name + "_nmsprob", images, "nmsprob")
        for dt in DISTANCE_THRESH:
            out[case_key(name, "nms", None, dt) + "/loc_error_nms"] = np.float64(
                D.compute_loc_error(name + "_nmsprob", prob_thresh=PROB_THRESH, distance_thresh=dt))
        print("  %s: predictions per image %s, ground truth %s, mAP(dense, d2) %.6f, loc error %.6f"
              % (name, n_pred, n_gt, out[case_key(name, "dense", False, 2) + "/mAP"],
                 out[case_key(name, "dense", None, 2) + "/loc_error"]))
    np.savez_compressed(OUT, **out)
    print("  %s: %d bytes" % (OUT, os.path.getsize(OUT)))
    assert os.path.getsize(OUT) < (1 << 20)
