"""The raw measurement behind profiles/evaluation_exact_measure.txt: every ratio that
tests/test_gpu_evaluation_exact.py turns into a tolerance, case by case.  Needs a HIP device.

    python tools/measure_evaluation_exact.py [output file]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import evaluation_cases as C  # noqa: E402
from tests import test_gpu_evaluation_exact as T  # noqa: E402

out = open(sys.argv[1] if len(sys.argv) > 1 else os.devnull, "w")


def say(s=""):
    print(s, flush=True)
    out.write(s + "\n")
    out.flush()


say("device: %s" % torch.cuda.get_device_name(0))
say("== eval_repeat_kernel: integer outputs against tests/evaluation_ref.py, sums in units of count * 2^-53 * sum (bound: 2) ==")
worst = 0.0
for name in C.REPEAT_NAMES:
    c = C.repeat_call(name)
    got = T._repeat(name)
    ints = bool(np.array_equal(got[:, [0, 1, 2, 3, 6]], c["expect"][:, [0, 1, 2, 3, 6]]))
    r = T.sum_ratio(name)
    worst = max(worst, r)
    say("%-24s %dx%d cap %4d stride %d keep_k %4d pairs %d  integers equal: %s  sum ratio %.4g" %
        (name, c["height"], c["width"], c["cap"], c["pair_stride"], c["keep_k"], c["n_pairs"], ints, r))
    if not ints:
        say("   device %s" % got[:, :7].tolist())
        say("   expect %s" % c["expect"][:, :7].tolist())
say("worst sum ratio %.4g" % worst)
say("96 KB launch equals cap = n: %s" % bool(np.array_equal(T._repeat("k2048_cap4096"), T._repeat("k2048_cap2500"))))

say("== eval_ransac_kernel against tests/eval_restatement.py ==")
fam_h, fam_l, fam_s, ap_w = {}, {}, {}, 0.0
for name in T.SINGLES:
    prob = C.ransac_problem(name)
    ref, o = prob["ref"], T._single(name)
    n = prob["m"].shape[0]
    dec = bool(o["status"][0] == ref["status"] and o["n_inliers"][0] == ref["mask"].sum()
               and np.array_equal(o["mask"][0, :n].astype(bool), ref["mask"]))
    if ref["status"] != 0:
        say("%-18s n %4d  no model on both sides: %s" % (name, n, dec))
        continue
    fam, dh, dl, sp, dap = T.ransac_ratios(name)
    fam_h[fam], fam_l[fam], fam_s[fam] = max(fam_h.get(fam, 0), dh), max(fam_l.get(fam, 0), dl), max(fam_s.get(fam, 0), sp)
    ap_w = max(ap_w, dap)
    say("%-18s n %4d [%-6s] decisions equal: %s  dH/max|H| %.4g  against lane order %.4g  restatement spread %.4g  d ap %.4g units"
        % (name, n, fam, dec, dh, dl, sp, dap))
for fam in fam_h:
    say("family %-7s worst dH/max|H| %.4g  (lane order %.4g; restatement's own spread %.4g)" % (fam, fam_h[fam], fam_l[fam], fam_s[fam]))
say("worst d ap %.4g units of (inliers + 2) * 2^-53; the restatement's two forms differ by %.4g" % (ap_w, T._spread_ap()))
base = T._single("caps_n300")
for cap in C.CAPS[1:]:
    o = T._single("caps_n300", cap)
    eq = all(np.array_equal(o[k][0][:300] if k == "mask" else o[k][0], base[k][0][:300] if k == "mask" else base[k][0]) for k in base)
    say("caps_n300 at cap %4d: every output bit-identical to cap = n: %s, mask past n clear: %s" % (cap, eq, not o["mask"][0, 300:].any()))
out.close()
