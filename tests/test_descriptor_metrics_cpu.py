"""CPU: the numpy restatement of the streamed descriptor metrics (tests/descriptor_metrics_ref.py) against numpy's own
linear algebra and against the G16 fixture of the real reference's evaluation.py (tools/make_golden_evaluation.py)."""
import os
import re

import numpy as np

from tests import descriptor_metrics_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G16 = os.path.join(ROOT, "tests", "golden", "g16_evaluation.npz")
NEW = ("ssp_eval_pixel_homographies", "ssp_eval_accumulate")
SUM_TOL = 12 * 2.0 ** -52  # 12 sequential fp64 additions against numpy's pairwise order: at most one ulp each


def test_symbols_declared_and_exported():
    from semantic_superpoint_amd import lib
    with open(os.path.join(ROOT, "include", "ssp_hip.h")) as f:
        hdr = f.read()
    for n in NEW:
        assert re.search(r"\b%s\(" % n, hdr), n
        assert n in lib.EXPORTS, n
    for n in ("op_eval_pixel_homographies", "op_eval_accumulate", "eval_metrics_state"):
        assert callable(getattr(lib, n))
    for c in ("ACC_MAX_PAIRS", "ROW_WORDS", "STATE_WORDS"):
        assert re.search(r"#define SSP_EVAL_%s %d\b" % (c, getattr(lib, "EVAL_" + c)), hdr)
    assert lib.EVAL_ROW_WORDS == R.ROW_WORDS and lib.EVAL_STATE_WORDS == R.STATE_WORDS
    assert "np.linalg.inv" in hdr[hdr.index("ssp_eval_pixel_homographies:"):hdr.index("#define SSP_EVAL_ACC_MAX_PAIRS")]


def random_normalised(rng, n):
    """Normalised homographies like the trainer's sampler draws them: mild affine part, perspective terms, translation."""
    out = np.zeros((n, 3, 3), np.float32)
    for k in range(n):
        a, b, c, d = rng.uniform(-0.3, 0.3, 4)
        out[k] = [[1 + a, b, rng.uniform(-0.4, 0.4)], [c, 1 + d, rng.uniform(-0.4, 0.4)],
                  [rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2), 1.0]]
    return out


def test_scaling_and_adjugate_against_numpy():
    rng = np.random.default_rng(2101)
    for hh, ww in ((240, 320), (48, 64), (384, 1248)):
        T = np.array([[2.0 / ww, 0, -1], [0, 2.0 / hh, -1], [0, 0, 1]])
        for hn in random_normalised(rng, 200):
            M, Mi = R.pixel_homography(hn, hh, ww)
            want = np.linalg.inv(T) @ hn.astype(np.float64) @ T
            assert np.abs(M - want).max() <= 1e-12 * np.abs(want).max()
            inv = np.linalg.inv(M)
            assert np.abs(Mi - inv).max() <= 1e-9 * np.abs(inv).max()


def g16_rows():
    f = np.load(G16)
    n = len(f["result_repeatability"])
    assert n == 12 and len(f["result_localization_err"]) == 12  # every pair repeats: loc_err > 0 for all
    rows = np.zeros((n, R.ROW_WORDS))
    rows[:, 0] = f["result_repeatability"]
    rows[:, 1] = f["result_localization_err"]
    rows[:, 2:8] = f["result_correctness"]
    rows[:, 8] = f["result_mscore"]
    rows[:, 9] = f["result_mAP"]
    rows[:, 15] = np.arange(n)
    return rows


def feed(rows, split, capacity=None):
    out = np.zeros((capacity or len(rows), R.ROW_WORDS))
    state = np.zeros(R.STATE_WORDS)
    k = 0
    for n in split:
        R.accumulate_rows(rows[k:k + n], out, state)
        k += n
    assert k == len(rows)
    return out, state


def check_g16_summary(s):
    """The values of the fixture's result_txt (written by the real reference)."""
    txt = str(np.load(G16)["result_txt"])
    want = {"repeatability": 0.42934576370169036, "localization_err": 1.2474039995543165, "mAP": 0.7270475539271284,
            "mscore": 0.6413869035725571}
    for line, key in (("repeatability: ", "repeatability"), ("localization error: ", "localization_err"),
                      ("nn mean AP: ", "mAP"), ("matching score: ", "mscore")):
        assert float(re.search(r"^" + re.escape(line) + r"(\S+)$", txt, re.M).group(1)) == want[key]
        assert abs(s[key] - want[key]) <= SUM_TOL * want[key], (key, s[key], want[key])
    assert s["pairs"] == 12 and s["loc_pairs"] == 12
    np.testing.assert_array_equal(s["correctness"], np.array([5, 7, 8, 9, 10, 11]) / 12)


def test_g16_summary():
    _, state = feed(g16_rows(), [12])
    check_g16_summary(R.summary(state))
    assert state[12] == 0 and state[13] == 0 and state[14] == 0 and state[15] == 0


def test_split_invariance():
    rows = g16_rows()
    a_rows, a = feed(rows, [12])
    for split in ([5, 5, 2], [1] * 12):
        b_rows, b = feed(rows, split)
        assert a.tobytes() == b.tobytes()
        assert a_rows.tobytes() == b_rows.tobytes()


def test_rows_of_special_pairs():
    """rep_from_counts / correctness_of / the mscore and mAP lines of Evaluator.run_points on the cases the kernel branches on."""
    from semantic_superpoint_amd.evaluation import correctness_of, rep_from_counts
    G = np.array([[1.0, 0, 4], [0, 1.0, -2], [0, 0, 1]])
    E = np.array([[1.0, 0, 7], [0, 1.0, -2], [0, 0, 1]])  # the truth shifted by exactly 3 px
    rep = np.array([30.0, 25.0, 11.0, 9.0, 13.5, 10.25, 17.0, 0.0])
    r = R.pair_row(3, rep=rep, H=E, n_inl=12, status=0, ap=0.625, n1=23, hom=G)
    want_rep, want_loc = rep_from_counts(rep)
    assert r[0] == want_rep and r[1] == want_loc
    assert r[14] == 3.0
    np.testing.assert_array_equal(r[2:8] != 0, correctness_of(E, G))
    np.testing.assert_array_equal(r[2:8], [0, 1, 1, 1, 1, 1])
    assert r[8] == np.float64(24) / np.float64(40) and r[9] == 0.625 and r[15] == 3
    none = R.pair_row(0, rep=np.array([5.0, 4.0, 0, 0, 0, 0, 0, 0]), H=np.eye(3), n_inl=0, status=1, ap=0.0, n1=0, hom=G)
    assert none[0] == 0 and none[1] == -1 and not none[2:8].any() and none[8] == 0 and none[9] == 0
    assert none[10] == 1 and np.isinf(none[14])
    off = R.pair_row(1, rep=rep)
    assert not off[2:15].any() and off[0] == want_rep


def test_capacity_counts_dropped_rows():
    rows = g16_rows()
    kept, state = feed(rows, [5, 5, 2], capacity=8)
    assert state[0] == 12 and state[13] == 4
    np.testing.assert_array_equal(kept, rows[:8])
    assert state.tobytes()[:13 * 8] == feed(rows, [12])[1].tobytes()[:13 * 8]
