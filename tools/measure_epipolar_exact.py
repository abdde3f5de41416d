"""The raw measurement behind profiles/epipolar_exact_measure.txt: every ratio that
tests/test_gpu_epipolar_exact.py turns into a tolerance (tests/epipolar_cases.py MEASURED), case by case, with the margins of
the case and the wall time of the call.  Needs a HIP device.

    python tools/measure_epipolar_exact.py [output file]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import epipolar_cases as C  # noqa: E402
from tests import test_gpu_epipolar_exact as T  # noqa: E402

out = open(sys.argv[1] if len(sys.argv) > 1 else os.devnull, "w")


def say(s=""):
    print(s, flush=True)
    out.write(s + "\n")
    out.flush()


def integers_equal(got, p, q):
    ref, n = q["ref_block"], q["m"].shape[0]
    return bool(got["status"][p] == ref["status"] and got["winner"][p] == ref["winner"] and got["n_inliers"][p] == ref["n_inliers"]
                and np.array_equal(got["mask"][p, :n], ref["mask"].astype(np.uint8)) and not got["mask"][p, n:].any())


say("device: %s" % torch.cuda.get_device_name(0))
T.single("n64_clean")      # (the first call loads the library)
say("== single launches at cap = n against tests/epipolar_ref.py; ratios are max(|dF|, |derr|) / max|F| ==")
fam_b, fam_a, fam_s = {}, {}, {}
for name in C.SINGLES:
    q = C.problem(name)
    got = T._call(C.launch("single:" + name))
    d, r, ref = q["dec"], q["report"], q["ref_block"]
    eq = integers_equal(got, 0, q)
    head = "%-18s n %4d [%-11s] status %d winner %4d inliers %4d  integers and mask equal: %s" % (
        name, q["m"].shape[0], C.family(name), ref["status"], ref["winner"], ref["n_inliers"], eq)
    if not eq:
        say("   device: status %d winner %d inliers %d" % (got["status"][0], got["winner"][0], got["n_inliers"][0]))
    if ref["status"] != 0:
        say("%s  no model  pivots: largest refused %.3g  %.1f ms" % (head, d["pivot_largest_refused"], 1e3 * got["seconds"]))
        continue
    blk, asc, spread = T.ratios(got, 0, q)
    fam = C.family(name)
    fam_b[fam], fam_a[fam], fam_s[fam] = max(fam_b.get(fam, 0.0), blk), max(fam_a.get(fam, 0.0), asc), max(fam_s.get(fam, 0.0), spread)
    say("%s  block order %.4g  ascending %.4g  restatement's spread %.4g | rival slack %s  pivots: least accepted %.3g largest refused "
        "%.3g refit %.3g  gaps: argmax %.3g sign %.3g | %.1f ms" %
        (head, blk, asc, spread, d["slack"], d["pivot_least_accepted"], d["pivot_largest_refused"], r["pivots"].min(), r["gap_G"],
         r["gap_Fd"], 1e3 * got["seconds"]))
say()
for fam in C.FAMILIES:
    say("family %-11s worst ratio against the block order %.4g  (ascending %.4g; restatement's own spread %.4g)" %
        (fam, fam_b.get(fam, 0.0), fam_a.get(fam, 0.0), fam_s.get(fam, 0.0)))
say("MEASURED = {%s}" % ", ".join('"%s": %r' % (f, fam_b.get(f, 0.0)) for f in C.FAMILIES))
say()
say("== launches: every pair against its single launch at cap = n, bit for bit ==")
for name in C.LAUNCHES:
    L, got = C.launch(name), T._call(C.launch(name))
    res = []
    for p, same in enumerate(L["same_as"]):
        if same is None:
            res.append("own problem, integers equal: %s" % integers_equal(got, p, C.expected(name, p)))
            continue
        b, n = T.single(same), C.problem(same)["m"].shape[0]
        eq = all(np.array_equal(got[k][p, :n], b[k][0, :n]) and not got[k][p, n:].any() if k == "mask" else
                 np.array_equal(np.ascontiguousarray(got[k][p]).view(np.uint8), np.ascontiguousarray(b[k][0]).view(np.uint8)) for k in T.KEYS)
        res.append(str(eq))
    say("%-16s cap %4d pairs %d pair_stride %d pt_stride %d groups %2d: %s  %.1f ms" %
        (name, L["cap"], len(L["names"]), L["pair_stride"], L["pt_stride"], L["groups"], " ".join(res), 1e3 * got["seconds"]))
out.close()
