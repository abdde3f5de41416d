"""The epipolar check on the device, output by output: epi_hypotheses_kernel, epi_finish_kernel and
match_filter_kernel on the inputs of tests/epipolar_cases.py, which tests/test_epipolar_exact_cpu.py shows to be decided.

status, winner, n_inliers, the whole mask (0 past n), the filter's rows and counts and the pose's integers are compared with
==; there is no "near" set.  Every cap, groups value, batch position, stride and repetition is bit-identical to the single
launch at cap = n.  F and err are compared with the restatement whose refit sums in the kernel's own order (block_sum<256>):
max(|dF|, |derr|) / max|F| <= 4 x the ratio measured on the MI355X per family (epipolar_cases.MEASURED), never below
16 x 2^-53, never above the tolerance of tests/test_gpu_epipolar.py; against the ascending restatement the bound is raised to
the restatement's own spread between its three orders.  A disagreement is judged by the restatement and the margins the CPU
file prints, never by the kernel's own number."""
import functools
import time

import numpy as np
import pytest
import torch

from tests import epipolar_cases as C
from tests import epipolar_ref as E
from tests import pose_ref as PR

pytestmark = pytest.mark.gpu

KEYS = ("F", "mask", "n_inliers", "status", "winner", "err")


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _call(L):
    """One call of the operator on the launch L; numpy outputs and the wall time of the call."""
    from semantic_superpoint_amd import lib as Lib
    args = [_t(L[k]) for k in ("pts1", "pts2", "match", "n_match", "seeds")]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    o = Lib.op_epipolar_ransac(*args, thresh=L["thresh"], pair_stride=L["pair_stride"], groups=L["groups"])
    torch.cuda.synchronize()
    out = {k: o[k].cpu().numpy() for k in KEYS}
    out["seconds"] = time.perf_counter() - t0
    return out


@functools.lru_cache(maxsize=None)
def run(name):
    return _call(C.launch(name))


def single(name):
    """The single launch of a problem at cap = n (cap 1 for the empty one)."""
    return run("single:" + name)


def ratios(got, p, q):
    """(against the block-order restatement, against the ascending one, the restatement's spread), each max(|dF|, |derr|) / max|F|."""
    big = float(np.abs(q["ref_block"]["F"]).max())
    d = lambda ref: max(float(np.abs(got["F"][p] - ref["F"]).max()), abs(float(got["err"][p]) - ref["err"])) / big
    return d(q["ref_block"]), d(q["ref"]), q["spread"] / big


def compare(got, p, q, fam, what):
    """Pair p of the device outputs `got` against the solved problem q (epipolar_cases.solve)."""
    ref, n = q["ref_block"], q["m"].shape[0]
    print("%s: status %d / %d winner %d / %d inliers %d / %d" %
          (what, got["status"][p], ref["status"], got["winner"][p], ref["winner"], got["n_inliers"][p], ref["n_inliers"]))
    assert got["status"][p] == ref["status"] and got["winner"][p] == ref["winner"] and got["n_inliers"][p] == ref["n_inliers"], what
    assert np.array_equal(got["mask"][p, :n], ref["mask"].astype(np.uint8)) and not got["mask"][p, n:].any(), what
    if ref["status"] == 1:
        assert not got["F"][p].any() and got["err"][p] == 0.0, what
        return
    blk, asc, spread = ratios(got, p, q)
    bound = min(max(4.0 * C.MEASURED[fam], C.FLOOR), E.TOLERANCE)
    print("%s: [%s] block order %.3g (bound %.3g), ascending %.3g (bound %.3g), restatement's spread %.3g" %
          (what, fam, blk, bound, asc, min(max(bound, spread), E.TOLERANCE), spread))
    assert blk <= bound and asc <= min(max(bound, spread), E.TOLERANCE), (what, blk, asc, bound, spread)
    F = got["F"][p]
    assert abs(float(np.sqrt((F * F).sum())) - 1.0) <= 1e-14 and F.reshape(-1)[np.argmax(np.abs(F))] > 0.0, what


@pytest.mark.parametrize("name", C.SINGLES)
def test_single_launch(name):
    compare(single(name), 0, C.problem(name), C.family(name), name)


def _same(a, pa, b, n, what):
    """Pair pa of a equals the single launch b, bit for bit (the mask over b's rows, 0 behind them)."""
    for k in KEYS:
        if k == "mask":
            assert np.array_equal(a[k][pa, :n], b[k][0, :n]) and not a[k][pa, n:].any(), (what, k)
        else:
            assert np.array_equal(np.ascontiguousarray(a[k][pa]).view(np.uint8), np.ascontiguousarray(b[k][0]).view(np.uint8)), (what, k)


@pytest.mark.parametrize("name", C.LAUNCHES)
def test_launch_equals_the_single_launches(name):
    L, got = C.launch(name), run(name)
    for p, same in enumerate(L["same_as"]):
        what = "%s[%d]" % (name, p)
        if same is None:
            compare(got, p, C.expected(name, p), "mid_noisy", what)
        else:
            _same(got, p, single(same), C.problem(same)["m"].shape[0], what)


def test_repeated_call_is_bit_identical():
    for name in ("batch9", "single:n4096_noisy"):
        a, b = run(name), _call(C.launch(name))
        for k in KEYS:
            assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (name, k)


def test_library_groups_switch_between_8_and_9_pairs():
    """32 workgroups per pair while 32 x pairs <= 256, else 16: both sides of the switch give the single launches (asserted pair
    by pair in test_launch_equals_the_single_launches); here the two batches agree on their common pairs."""
    a, b = run("batch8"), run("batch9")
    for k in KEYS:
        assert np.array_equal(a[k].view(np.uint8), b[k][:8].view(np.uint8)), k


@pytest.mark.parametrize("name", C.FILTERS)
def test_filter(name):
    from semantic_superpoint_amd import lib as Lib
    c = C.filter_case(name)
    out, n_out = Lib.op_filter_matches(_t(c["match"]), _t(c["n_match"]), _t(c["mask"]), _t(c["status"]), _t(c["n_inliers"]), c["min_inliers"])
    torch.cuda.synchronize()
    want, n_want = c["expect"]
    print("%s: kept %s, expected %s" % (name, n_out.cpu().numpy().tolist(), n_want.tolist()))
    assert np.array_equal(n_out.cpu().numpy(), n_want)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32))           # rows bit for bit, zero rows behind them


def test_filter_of_the_devices_own_mask():
    """The chain the tracker runs: the mask, count and status of a call, filtered on the device, against the restatement."""
    from semantic_superpoint_amd import lib as Lib
    L, got = C.launch("mixed"), run("mixed")
    for min_inl in (0, 10, 11, 192):      # n12_clean has 10 inliers, launch300 191
        out, n_out = Lib.op_filter_matches(_t(L["match"]), _t(L["n_match"]), _t(got["mask"]), _t(got["status"]), _t(got["n_inliers"]), min_inl)
        mask = np.zeros_like(got["mask"])
        for p, nm in enumerate(C.MIXED):
            q = C.problem(nm)
            mask[p, :q["m"].shape[0]] = q["ref_block"]["mask"]
        want, n_want = C.filter_ref(L["match"], L["n_match"], mask, np.array([C.problem(nm)["ref_block"]["status"] for nm in C.MIXED]),
                                    np.array([C.problem(nm)["ref_block"]["n_inliers"] for nm in C.MIXED]), min_inl)
        assert np.array_equal(n_out.cpu().numpy(), n_want), min_inl
        assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32)), min_inl


def test_pose_decisions():
    """op_two_view_pose on the restatement's F and hand-made masks: both sides of n_front = 8 and of 2 n_front = n_inliers."""
    from semantic_superpoint_amd import lib as Lib
    c = C.pose_case()
    L = c["L"]
    geometry = {"F": _t(c["F"]), "mask": _t(c["mask"]), "n_inliers": _t(c["n_inliers"]), "status": _t(c["status"])}
    o = Lib.op_two_view_pose(geometry, _t(L["pts1"]), _t(L["pts2"]), _t(L["match"]), _t(L["n_match"]), _t(c["intr"]))
    torch.cuda.synchronize()
    o = {k: v.cpu().numpy() for k, v in o.items()}
    for k, (front, n_inl) in enumerate(C.POSE_ROWS):
        m = C.gathered(L, k)
        n = m.shape[0]
        r = PR.two_view_pose(c["F"][k], c["mask"][k, :n], n_inl, 0, m, c["intr"][0])
        print("pose row %d: status %d / %d cand %d / %d n_front %d / %d counts %s / %s" %
              (k, o["status"][k], r["status"], o["cand"][k], r["cand"], o["n_front"][k], r["n_front"], o["counts"][k].tolist(), r["counts"].tolist()))
        assert o["status"][k] == r["status"] and o["cand"][k] == r["cand"] and o["n_front"][k] == r["n_front"] == front
        assert np.array_equal(o["counts"][k], r["counts"])
        assert np.array_equal(o["front"][k, :n], r["front"].astype(np.uint8)) and not o["front"][k, n:].any()
    assert o["status"].tolist() == [2, 0, 0, 0, 2, 0, 0, 2]
