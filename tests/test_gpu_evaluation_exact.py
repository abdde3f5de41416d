"""GPU: eval_repeat_kernel, eval_gather_kernel and eval_ransac_kernel (csrc/eval_kernels.hip.h) against their restatements
(tests/evaluation_ref.py, tests/eval_restatement.py) on the cases of tests/evaluation_cases.py.

Counts, masks and statuses compare with ==: tests/test_evaluation_ref_cpu.py asserts that no decision of these inputs is open.
The repeatability sums are held to a derived bound; H and the AP to 4 x the ratio measured on the MI355X
(profiles/evaluation_exact_measure.txt), never below the restatement's own spread between its two summation orders."""
import functools

import numpy as np
import pytest
import torch

from tests import descriptor_metrics_ref as DM
from tests import evaluation_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -53

# worst ratios measured on the MI355X (profiles/evaluation_exact_measure.txt); a tolerance is 4 x the value
MEASURED_H = {"n<=8": 1.619e-10, "n~256": 7.609e-11, "n=4096": 2.181e-15}   # max |dH| / max |H| against the restatement
MEASURED_H_LANES = {"n<=8": 9.416e-18, "n~256": 1.641e-17, "n=4096": 0.0}     # the same against its refit in wave 0's order
MEASURED_AP = 0.03333                                                          # |d ap| in units of (inliers + 2) * 2^-53
# The lane-order refit repeats the kernel's additions one by one, so the device meets it to the last place or two.  Its tolerance
# never goes below 16 roundings of the largest element: eval_denorm alone forms every element of H from 7 rounded operations, and
# a compiler may pick another (still correctly ordered) division or reciprocal sequence.
LANES_FLOOR = 16 * U


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- repeatability ----
@functools.lru_cache(maxsize=None)
def _repeat(name):
    from semantic_superpoint_amd import lib as L
    c = C.repeat_call(name)
    out = L.op_eval_repeatability(_t(c["pts1"]), _t(c["n1"]), _t(c["pts2"]), _t(c["n2"]), _t(c["H"]), _t(c["H_inv"]), c["height"],
                                  c["width"], keep_k=c["keep_k"], dist_thresh=c["thresh"], pair_stride=c["pair_stride"],
                                  n_pairs=c["n_pairs"])
    return out.cpu().numpy()


def sum_ratio(name):
    """The worst |device sum - restatement sum| of a launch in units of count * 2^-53 * sum (0 when every sum agrees bit for bit)."""
    got, want = _repeat(name), C.repeat_call(name)["expect"]
    worst = 0.0
    for p in range(want.shape[0]):
        for cnt, s in ((2, 4), (3, 5)):
            if got[p, s] != want[p, s]:
                worst = max(worst, abs(got[p, s] - want[p, s]) / (want[p, cnt] * U * want[p, s]))
    return worst


@pytest.mark.parametrize("name", C.REPEAT_NAMES)
def test_repeatability_equals_restatement(name):
    c = C.repeat_call(name)
    got, want = _repeat(name), c["expect"]
    for p, pair in enumerate(c["pairs"]):
        for k, slot in enumerate(("N1", "N2", "count1", "count2")):
            assert got[p, k] == want[p, k], (pair, slot)
        assert got[p, 6] == want[p, 6], (pair, "n_unwarped")
        assert got[p, 7] == 0
        for cnt, s in ((2, 4), (3, 5)):
            # each term is <= thresh and each addition rounds once: |sum - exact| <= n 2^-53 sum; two orders are compared
            assert abs(got[p, s] - want[p, s]) <= 2 * want[p, cnt] * U * want[p, s], (pair, s)
    print("%s: sums at %.3g of count * 2^-53 * sum (bound 2)" % (name, sum_ratio(name)))


def test_repeatability_at_96_kb_equals_cap_n():
    assert np.array_equal(_repeat("k2048_cap4096"), _repeat("k2048_cap2500"))


def test_repeatability_refusals():
    from semantic_superpoint_amd import lib as L
    c = C.repeat_call("thresh_3")
    a = (_t(c["pts1"]), _t(c["n1"]), _t(c["pts2"]), _t(c["n2"]), _t(c["H"]), _t(c["H_inv"]), c["height"], c["width"])
    for kw in (dict(keep_k=0), dict(keep_k=2049), dict(dist_thresh=-1.0), dict(dist_thresh=-np.nextafter(0.0, 1)),
               dict(dist_thresh=float("nan"))):
        with pytest.raises(RuntimeError):
            L.op_eval_repeatability(*a, **kw)
    assert L.op_eval_repeatability(*a, keep_k=2048, dist_thresh=0.0)[0, 2] == 1
    big = torch.zeros(1, L.MATCH_MAX_POINTS + 1, 3, dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError):
        L.op_eval_repeatability(big, a[1], big, a[3], *a[4:])


def test_streamed_round_equals_accumulate_of_restatement():
    """One update_points round over the three integer-coordinate pairs (every distance and sum exact): the rows and the state are
    those of descriptor_metrics_ref.accumulate fed with the restatement's counts, bit for bit."""
    from semantic_superpoint_amd.evaluation import StreamingEvaluator
    c = C.repeat_call("stream_48x64")
    ev = StreamingEvaluator(c["height"], c["width"], DEV, 4, repeatability=True, homography=False, keep_k=c["keep_k"],
                            rep_thd=c["thresh"])
    desc = torch.zeros(c["pts1"].shape[0], c["cap"], 256, device=DEV)
    ev.update_points(_t(c["pts1"]), _t(c["n1"]), desc, c["H"], pair_stride=c["pair_stride"], pts2=_t(c["pts2"]), count2=_t(c["n2"]),
                     desc2=desc, hom_inv=c["H_inv"])
    rows, state = np.zeros((4, DM.ROW_WORDS)), np.zeros(DM.STATE_WORDS)
    DM.accumulate(0, rows, state, rep=c["expect"])
    assert rows[0, 0] == 4 / 10 and rows[0, 1] == 3 / 4 + 3 / 4 and rows[1, 0] == 1.0 and rows[2, 1] == 1.0
    assert np.array_equal(ev.rows.cpu().numpy().view(np.int64), rows.view(np.int64))
    assert np.array_equal(ev.state.cpu().numpy().view(np.int64), state.view(np.int64))


# ---- RANSAC ----
def _launch(call):
    from semantic_superpoint_amd import lib as L
    o = L.op_eval_ransac(_t(call["pts1"]), _t(call["pts2"]), _t(call["match"]), _t(call["n_match"]), _t(call["seeds"]),
                         pair_stride=call["pair_stride"], want_ap=True)
    return {k: v.cpu().numpy() for k, v in o.items()}


@functools.lru_cache(maxsize=None)
def _single(name, cap=None):
    return _launch(C.ransac_call((name,), cap=cap, seed=1))


def _same(a, pa, b, pb, n):
    """Every output of problem pa of launch a equals that of problem pb of launch b, bit for bit; the masks past n are 0."""
    for k in ("H", "n_inliers", "status", "ap"):
        assert np.array_equal(a[k][pa], b[k][pb]), k
    assert np.array_equal(a["mask"][pa, :n], b["mask"][pb, :n])
    assert not a["mask"][pa, n:].any() and not b["mask"][pb, n:].any()


def _decisions(o, p, prob):
    ref, n = prob["ref"], min(prob["m"].shape[0], o["mask"].shape[1])
    assert o["status"][p] == ref["status"]
    assert o["n_inliers"][p] == ref["mask"].sum()
    assert np.array_equal(o["mask"][p, :n].astype(bool), ref["mask"])
    assert not o["mask"][p, n:].any()


def ransac_ratios(name):
    """(family, |dH| / max |H| against the restatement, the same against its lane-order refit, the restatement's own spread, |d ap|
    in units of (inliers + 2) * 2^-53) of one problem in a launch of its own."""
    prob = C.ransac_problem(name)
    ref, o = prob["ref"], _single(name)
    top = np.abs(ref["H"]).max()
    return (C.family_of(prob["m"].shape[0]), float(np.abs(o["H"][0] - ref["H"]).max() / top),
            float(np.abs(o["H"][0] - ref["H_lanes"]).max() / top), float(np.abs(ref["H"] - ref["H_lanes"]).max() / top),
            float(abs(o["ap"][0] - ref["ap"]) / ((ref["mask"].sum() + 2) * U)))


@functools.lru_cache(maxsize=None)
def _spread():
    """The restatement's own floor per family: the spread of its refit between the two summation orders, over every problem."""
    s = {}
    for name in C.RANSAC_SPECS:
        p = C.ransac_problem(name)
        if p["ref"]["status"] == 0:
            r = p["ref"]
            fam = C.family_of(p["m"].shape[0])
            s[fam] = max(s.get(fam, 0.0), float(np.abs(r["H"] - r["H_lanes"]).max() / np.abs(r["H"]).max()))
    return s


@functools.lru_cache(maxsize=None)
def _spread_ap():
    """The AP's own floor: its two forms (sklearn's thresholds, the kernel's counting) over every problem, in the same units."""
    from tests import eval_restatement as ER
    worst = 0.0
    for name in C.RANSAC_SPECS:
        p = C.ransac_problem(name)
        if p["ref"]["status"] == 0:
            d = abs(ER.average_precision_counting(p["ref"]["mask"], p["dist"]) - p["ref"]["ap"])
            worst = max(worst, float(d / ((p["ref"]["mask"].sum() + 2) * U)))
    return worst


SINGLES = tuple(n for n in C.RANSAC_SPECS if n != "over_cap")


@pytest.mark.parametrize("name", SINGLES)
def test_ransac_equals_restatement(name):
    prob = C.ransac_problem(name)
    ref, o = prob["ref"], _single(name)
    _decisions(o, 0, prob)
    if ref["status"] != 0:
        assert np.array_equal(o["H"][0], np.eye(3)) and o["ap"][0] == 0
        return
    fam, dh, dl, spread, dap = ransac_ratios(name)
    print("%s [%s]: dH %.3g (lane order %.3g, restatement's spread %.3g), d ap %.3g units" % (name, fam, dh, dl, spread, dap))
    assert dh <= max(4 * MEASURED_H[fam], _spread()[fam])
    assert dl <= max(4 * MEASURED_H_LANES[fam], LANES_FLOOR)
    assert dap <= max(4 * MEASURED_AP, _spread_ap())
    if name == "ap_all_inliers":
        assert o["ap"][0] == 1.0


@pytest.mark.parametrize("cap", [c for c in C.CAPS if c])
def test_ransac_does_not_depend_on_cap(cap):
    """One data set at cap = n and at the caps on both sides of the two LDS boundaries: 1771 / 1772 (64 KiB of dynamic LDS) and
    3321 / 3322 (EVAL_LDS_MAX: the matches stay in global memory from there)."""
    prob = C.ransac_problem("caps_n300")
    n = prob["m"].shape[0]
    _decisions(_single("caps_n300", cap), 0, prob)
    _same(_single("caps_n300", cap), 0, _single("caps_n300"), 0, n)


def test_ransac_count_above_cap():
    prob = C.ransac_problem("over_cap")
    o = _launch(C.ransac_call(("over_cap",), n_match=101, seed=2))
    _decisions(o, 0, prob)
    _same(o, 0, _launch(C.ransac_call(("over_cap",), seed=2)), 0, 64)


@pytest.mark.parametrize("stride", [1, 3])
def test_ransac_pair_stride_with_decoys(stride):
    names = ("n40", "n8_out", "n256_out")
    o = _launch(C.ransac_call(names, pair_stride=stride, seed=3))
    for p, name in enumerate(names):
        prob = C.ransac_problem(name)
        _decisions(o, p, prob)
        _same(o, p, _single(name), 0, prob["m"].shape[0])


def test_ransac_batch_of_mixed_sizes():
    o = _launch(C.ransac_call(C.BATCH, seed=4))
    assert [C.ransac_problem(n)["m"].shape[0] for n in C.BATCH] == [0, 3, 4, 5, 40, 257, 300, 8]
    for p, name in enumerate(C.BATCH):
        prob = C.ransac_problem(name)
        _decisions(o, p, prob)
        _same(o, p, _single(name), 0, prob["m"].shape[0])


def test_ransac_cap_above_the_limit_stays_refused():
    from semantic_superpoint_amd import lib as L
    cap = L.MATCH_MAX_POINTS + 1
    p = torch.zeros(1, cap, 3, dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError):
        L.op_eval_ransac(p, p, torch.zeros(1, cap, 3, device=DEV), torch.ones(1, dtype=torch.int32, device=DEV),
                         torch.zeros(1, dtype=torch.int64, device=DEV))
