"""Detector evaluation, CPU side: the numpy restatement (tests/detector_eval_ref.py) against the real reference's results
(G20, tools/make_golden_detector_eval.py), the tie rule on hand-made cases, and the constants the device code mirrors."""
import os
import re

import numpy as np
import pytest

from tests import detector_eval_ref as R
from tests import golden_detector_eval as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def g20():
    return np.load(os.path.join(ROOT, "tests", "golden", "g20_detector_eval.npz"))


@pytest.fixture(scope="module")
def sets():
    return {name: G.make_set(name) for name in G.SETS}


def test_inputs_match_fixture(g20, sets):
    for name, images in sets.items():
        assert np.array_equal(G.checksum(images), g20[name + "/checksum"]), name


@pytest.mark.parametrize("name", sorted(G.SETS))
@pytest.mark.parametrize("variant", G.VARIANTS)
@pytest.mark.parametrize("simplified", G.SIMPLIFIED)
@pytest.mark.parametrize("dt", G.DISTANCE_THRESH)
def test_restatement_equals_reference(g20, sets, name, variant, simplified, dt):
    images = sets[name]
    key, base = G.case_key(name, variant, simplified, dt), G.case_key(name, variant)
    maps = [(im[0] if variant == "dense" else im[1], im[2]) for im in images]
    recs = []
    for i, (pm, kp) in enumerate(maps):
        tp, fp, prob, n_gt = R.compute_tp_fp(pm, kp, G.REMOVE_ZERO, dt, simplified)
        assert np.array_equal(tp, g20["%s/tp/%d" % (key, i)]) and np.array_equal(fp, ~tp)
        assert prob.dtype == np.float32 and np.array_equal(prob, g20["%s/prob_sorted/%d" % (base, i)])
        assert n_gt == g20[key + "/n_gt"][i]
        yx, p = R.candidates(pm, G.REMOVE_ZERO)
        recs.append(R.tp_fp_records(yx, p, kp, dt, simplified))
    precision, recall, prob, _ = R.compute_pr(recs)
    assert precision.dtype == np.float64 and np.array_equal(precision, g20[key + "/precision"])
    assert recall.dtype == np.float64 and np.array_equal(recall, g20[key + "/recall"])
    assert np.array_equal(prob, g20[base + "/prob"])
    n = len(prob)
    assert abs(R.compute_mAP(precision, recall) - g20[key + "/mAP"]) <= n * EPS
    # the point-list input of the nms map (any list order: the probabilities are unique) gives the same records
    if variant == "nms":
        ev = R.evaluate([((G.point_list(im[1])[0],), im[2]) for im in images], G.REMOVE_ZERO, dt, G.PROB_THRESH, simplified)
        assert np.array_equal(ev["precision"], precision) and np.array_equal(ev["recall"], recall)
        assert abs(ev["loc_error"] - g20[G.case_key(name, "nms", None, dt) + "/loc_error_nms"]) <= n * EPS
    ev = R.evaluate([(im[0], im[2]) for im in images], G.REMOVE_ZERO, dt, G.PROB_THRESH, simplified)
    assert abs(ev["loc_error"] - g20[G.case_key(name, variant, None, dt) + "/loc_error"]) <= len(ev["prob"]) * EPS


def test_tie_rule_two_equal_detections_share_a_point():
    kp = np.zeros((5, 7), np.uint8)
    kp[2, 3] = 1
    prob = np.zeros((5, 7), np.float32)
    prob[2, 2] = prob[2, 4] = 0.5  # both one pixel from the point, equal probability
    prob[0, 0] = 0.5                # and a third equal one that matches nothing
    tp, fp, p, n_gt = R.compute_tp_fp(prob, kp)
    # order: later position first -> (2,4), (2,2), (0,0); the first of the two that share the point is the true positive
    assert n_gt == 1 and tp.tolist() == [True, False, False] and p.tolist() == [0.5, 0.5, 0.5]
    yx, pr = R.candidates(prob)
    tpr, _, _ = R.tp_fp_records(yx, pr, kp)
    assert tpr.tolist() == [False, False, True]  # in position order: (0,0), (2,2), (2,4)
    precision, recall, _, tps = R.compute_pr([(tpr, pr, n_gt)])
    assert tps.tolist() == [True, False, False]
    assert precision.tolist() == [1.0, 1.0, 0.5, 1.0 / 3.0, 0.0] and recall.tolist() == [0.0, 1.0, 1.0, 1.0, 1.0]
    assert R.compute_mAP(precision, recall) == 1.0


def test_tie_rule_across_images_and_first_in_row_major_order():
    # image 0 and image 1 hold one detection each with equal probability: the LATER image comes first
    kp0 = np.zeros((4, 4), np.uint8)
    kp1 = np.zeros((4, 4), np.uint8)
    kp1[1, 1] = 1
    p0 = np.zeros((4, 4), np.float32)
    p1 = np.zeros((4, 4), np.float32)
    p0[0, 0] = p1[1, 1] = 0.25
    recs = []
    for pm, kp in ((p0, kp0), (p1, kp1)):
        yx, p = R.candidates(pm)
        recs.append(R.tp_fp_records(yx, p, kp))
    _, _, _, tp = R.compute_pr(recs)
    assert tp.tolist() == [True, False]
    # a detection with two points in range is assigned to the first in row-major order, not the nearest
    kp = np.zeros((6, 6), np.uint8)
    kp[1, 3] = kp[3, 4] = 1          # d2 = 4 (first) and d2 = 1 (nearest) from (3, 3)
    prob = np.zeros((6, 6), np.float32)
    prob[3, 3], prob[1, 4] = 0.9, 0.8  # the second detection is assigned to (1, 3) too, which the first one took
    tp, _, _, _ = R.compute_tp_fp(prob, kp)
    assert tp.tolist() == [True, False]
    tp, _, _, n_gt = R.compute_tp_fp(prob, kp, simplified=True)
    assert tp.tolist() == [True, True] and n_gt == 2


def test_empty_sets():
    precision, recall, prob, _ = R.compute_pr([])
    assert precision.tolist() == [0.0, 0.0] and recall.tolist() == [0.0, 1.0] and R.compute_mAP(precision, recall) == 0.0
    kp = np.zeros((4, 4), np.uint8)
    prob = np.full((4, 4), 0.3, np.float32)
    yx, p = R.candidates(prob)
    precision, recall, _, _ = R.compute_pr([R.tp_fp_records(yx, p, kp)])  # n_gt == 0: div0 gives recall 1 where tp_cum == 0
    assert recall.tolist() == [0.0] + [1.0] * 17 and precision.tolist() == [0.0] * 18


def test_r2():
    assert [R.r2_of(d) for d in (0, 1, 2, 3, 2.5, 8)] == [0, 1, 4, 9, 6, 64]


def test_constants_mirror_the_sources():
    """lib.py's constants are those of the C header and of the kernel header (read as text: no device needed)."""
    src = open(os.path.join(ROOT, "semantic-superpoint_amd", "lib.py")).read()
    hdr = open(os.path.join(ROOT, "include", "ssp_hip.h")).read()
    ker = open(os.path.join(ROOT, "semantic-superpoint_amd", "csrc", "detector_eval_kernels.hip.h")).read()

    def py(name):
        return int(re.search(r"^%s = (\d+)" % name, src, re.M).group(1))

    def c(text, name):
        return int(re.search(r"#define %s (\d+)" % name, text).group(1))

    assert py("DET_CURVE_TILE") == c(ker, "DET_CURVE_TILE") == c(hdr, "SSP_DET_EVAL_CURVE_TILE")
    assert py("DET_EVAL_MAX_R2") == c(ker, "DET_MAX_R2") == c(hdr, "SSP_DET_EVAL_MAX_R2")
    assert py("DET_EVAL_STATE_WORDS") == c(hdr, "SSP_DET_EVAL_STATE_WORDS")
    assert py("DET_EVAL_HIST") == c(ker, "DET_STATE_HIST")
