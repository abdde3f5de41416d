"""The conditions under which tests/test_gpu_epipolar_exact.py may compare with ==, asserted and printed
on the CPU for exactly the inputs that file uses (tests/epipolar_cases.py): every problem is decided by
epipolar_ref.decisions, every pivot is far from its threshold, the argmax and the sign rule have a gap, the launches hold the
matches they claim to hold, and every mutant of the restatement changes an output of a named case.  Run with -s for the
margins."""
import contextlib

import numpy as np
import pytest

from tests import epipolar_cases as C
from tests import epipolar_ref as E
from tests import eval_restatement as ER
from tests import pose_ref as PR

# Branches of epi_finish_kernel that no decided input reaches, and why (asserted in test_branches_not_covered).
NOT_COVERED = {
    "a best score below 8 from a valid hypothesis": "a valid hypothesis passes through its 8 sampled matches, whose Sampson "
    "distances are rounding noise (1e-13 px and less): its score is at least 8 unless a sampled match sits at the threshold, "
    "which a decided case excludes",
    "the refit's solve8 fallback (fn = G)": "it needs a pivot of the 8x8 moment system at or below 1e-12; with 8 or more "
    "inliers in general position the pivots are above 2e-3 here, and an input that pushes one to 1e-12 has it within rounding "
    "of the threshold: not decided",
    "a non-finite or non-positive inlier norm": "an inlier has a finite positive Sampson denominator, hence finite "
    "coordinates; the sum of 4096 finite pixel coordinates is finite and the spread of 8 distinct inliers is positive",
}


@contextlib.contextmanager
def patched(obj, name, value):
    old = getattr(obj, name)
    setattr(obj, name, value)
    try:
        yield
    finally:
        setattr(obj, name, old)


def _literal_block_sum(terms, index, threads=256):
    """block_sum<256> thread by thread, without numpy's help."""
    part = [0.0] * threads
    for t, i in zip(terms, index):
        part[i % threads] = part[i % threads] + float(t)
    waves = []
    for w in range(threads // 64):
        v = part[64 * w:64 * (w + 1)]
        o = 32
        while o >= 1:
            v = [v[l] + v[l ^ o] for l in range(64)]
            o >>= 1
        assert len(set(v)) == 1            # every lane ends with the same value
        waves.append(v[0])
    total = waves[0]
    for w in waves[1:]:
        total = total + w
    return total


@pytest.mark.parametrize("n", (0, 1, 63, 255, 256, 257, 513, 4096))
def test_block_sum_is_the_kernels_order(n):
    rng = np.random.RandomState(n)
    index = np.nonzero(rng.rand(n) < 0.7)[0]
    terms = rng.randn(index.size) * 10.0 ** rng.uniform(-6, 6, index.size)
    got = E.block_sum(terms, index)
    assert got == _literal_block_sum(terms, index)
    if index.size:
        both = E.block_sum(np.stack([terms, 2.0 * terms], axis=1), index)      # trailing axes are summed independently
        assert both[0] == got and both[1] == 2.0 * got
        assert ER.lane_sum(terms, index) == _literal_block_sum(terms, index, 64)


@pytest.mark.parametrize("name", C.SINGLES)
def test_problem_is_decided(name):
    p = C.problem(name)
    d, r, b = p["dec"], p["report"], p["ref_block"]
    n = p["m"].shape[0]
    print("%s: n %d scene seed %d (redrawn %d) seed %d thresh %g -> status %d winner %d inliers %d" %
          (name, n, p["scene_seed"], p["redraws"], p["seed"], p["thresh"], b["status"], b["winner"], b["n_inliers"]))
    print("  hypotheses: %d valid, winner's ambiguous matches %s, rival slack %s, ambiguous matches over all hypotheses %d" %
          (d["valid"].sum(), d["ambiguous"][d["winner"]] if d["winner"] >= 0 else "-", d["slack"], d["ambiguous"].sum()))
    print("  pivots: least accepted %.3g, largest refused %.3g, log10 margin %.2f" %
          (d["pivot_least_accepted"], d["pivot_largest_refused"], d["pivot_log_margin"]))
    if b["status"] == 0:
        print("  refit: least pivot %.3g, argmax gap of G %.3g, sign gap of F %.3g, spread between the three orders %.3g" %
              (r["pivots"].min(), r["gap_G"], r["gap_Fd"], p["spread"]))
    assert p["why"] == [] and p["redraws"] <= C.REDRAWS
    assert d["pivot_least_accepted"] >= C.PIVOT_ACCEPTED and d["pivot_largest_refused"] <= C.PIVOT_REFUSED
    w = E.winner_of(p["m"], p["seed"], p["thresh"])
    assert w[0] == d["winner"] and w[1] == d["best"]
    assert p["spread"] <= E.TOLERANCE
    for k in ("ref", "ref_pairwise"):
        assert np.array_equal(p[k]["mask"], b["mask"]) and p[k]["n_inliers"] == b["n_inliers"]
    if b["status"] == 0:
        assert d["ambiguous"][d["winner"]] == 0 and not (E.inliers(d["winner_F"][None], p["m"], p["thresh"])[0] ^ b["mask"]).any()
        assert min(r["gap_G"], r["gap_Fd"]) >= C.GAP and r["pivots"].min() >= C.PIVOT_ACCEPTED
    kind, n_in, n_out, noise = C.PROBLEMS[name][:4]
    if kind == "scene" and noise == 0.0 and n_in >= 40:         # noise-free and well determined: the mask is the truth
        assert np.array_equal(b["mask"], p["truth"]) and b["n_inliers"] == n_in
    if name.startswith("in25"):
        assert b["n_inliers"] == int(name[2:5])


def test_sizes_and_families():
    assert [C.problem("n%d_clean" % n)["m"].shape[0] for n in C.SIZES] == list(C.SIZES)
    assert [C.problem(nm)["m"].shape[0] for nm in C.MIXED] == [0, 7, 8, 9, 64, 257, 300, 12]
    assert {C.family(nm) for nm in C.SINGLES} == set(C.FAMILIES)
    assert C.problem("thresh_0.25")["ref_block"]["n_inliers"] < C.problem("thresh_3")["ref_block"]["n_inliers"]


def test_sampler_paths():
    # a sample that spends its 64 draws
    for seed, h in ((80, 1267), (4866, 7)):
        draws = [ER.draw(seed, h, c, 9) for c in range(E.SAMPLE_DRAWS)]
        assert E.sample8(seed, h, 9) is None and len(set(draws)) == 7
    p = C.problem("exhausted_seed80")
    print("exhausted_seed80: winner %d (hypothesis 1267 is refused, after the winner: the path is run, not distinguished)" % p["dec"]["winner"])
    assert not p["dec"]["valid"][1267] and p["dec"]["winner"] < 1267
    # ... ahead of the winner: the hypotheses 0 .. 6 hold the matches 1 and 5 (copies), 7 spends its draws
    p = C.problem("exhausted_first")
    d = p["dec"]
    assert np.array_equal(p["m"][5], p["m"][1])
    assert all({1, 5} <= set(E.sample8(4866, h, 9)) for h in range(7)) and not d["valid"][:8].any()
    with patched(E, "SAMPLE_DRAWS", 250):
        would = E.sample8(4866, 7, 9)
        mutant = E.winner_of(p["m"], 4866)
    print("exhausted_first: winner %d; with more draws hypothesis 7 would hold %s and win (mutant winner %d)" % (d["winner"], would, mutant[0]))
    assert would == [0, 6, 3, 1, 7, 8, 4, 2] and d["winner"] > 7 and mutant[0] == 7 and mutant[1] == d["best"] == 9
    # the direct rule of 8 matches
    p = C.problem("n8_direct")
    with patched(E, "DIRECT_N", -1):
        assert E.sample8(458, 0, 8) is None and E.sample8(458, 1, 8) is not None
        mutant = E.winner_of(p["m"], 458)
    print("n8_direct: winner %d, without the direct rule %d" % (p["dec"]["winner"], mutant[0]))
    assert p["dec"]["winner"] == 0 and len(p["dec"]["valid"]) == 1 and mutant[0] == 1


def test_degenerate_samples():
    p = C.problem("copies")
    d = p["dec"]
    copies = {0, 12, 13, 14, 15}
    two = np.array([len(copies & set(E.sample8(7, h, 16) or ())) >= 2 for h in range(E.HYPOTHESES)])
    print("copies: %d of %d samples hold two copies of match 0, all refused (largest refused pivot %.3g); %d valid" %
          (two.sum(), two.size, d["pivot_largest_refused"], d["valid"].sum()))
    assert two.sum() == 1723 and not d["valid"][two].any() and d["valid"][~two].all() and d["valid"].sum() == 277
    assert p["ref_block"]["n_inliers"] == 16
    p = C.problem("planar")
    d = p["dec"]
    print("planar: %d valid hypotheses, largest refused pivot %.3g (threshold %.0e): status %d by the pivot rule" %
          (d["valid"].sum(), d["pivot_largest_refused"], E.PIVOT_EPS, p["ref_block"]["status"]))
    assert not d["valid"].any() and d["pivot_largest_refused"] <= C.PIVOT_REFUSED and not np.isfinite(d["pivot_least_accepted"])
    assert all(p[k]["status"] == 1 and p[k]["winner"] == -1 for k in ("ref", "ref_pairwise", "ref_block"))


def test_non_finite_rows():
    p = C.problem("nonfinite")
    d, m = p["dec"], p["m"]
    bad = np.nonzero(~np.all(np.abs(m) < 1e100, axis=1))[0]
    assert bad.size == len(C.NONFINITE_ROWS) and not p["truth"][bad].any()
    holds = np.array([bool(set(bad) & set(E.sample8(p["seed"], h, m.shape[0]) or ())) for h in range(E.HYPOTHESES)])
    inl = np.zeros(m.shape[0], dtype=bool)
    for h0 in range(0, E.HYPOTHESES, 250):
        F, valid = E.hypotheses(m, p["seed"], list(range(h0, h0 + 250)))
        inl |= E.inliers(F[valid], m, p["thresh"]).any(axis=0)
    print("nonfinite: %d samples hold a non-finite row, none valid; those rows are inliers of no valid hypothesis" % holds.sum())
    assert holds.sum() > 100 and not d["valid"][holds].any() and not inl[bad].any()
    assert not p["ref_block"]["mask"][bad].any() and p["ref_block"]["status"] == 0 and np.all(np.isfinite(p["ref_block"]["F"]))


@pytest.mark.parametrize("name", C.LAUNCHES)
def test_launch_holds_what_it_claims(name):
    L = C.launch(name)
    cap = L["cap"]
    F_true = E.true_F(np.array([0.5, 0.12, 0.2]))
    for p, same in enumerate(L["same_as"]):
        m = C.gathered(L, p)
        q = C.expected(name, p)
        assert np.array_equal(m, q["m"]), (name, p)                    # the matches the kernel stages are the problem's
        assert C.undecided(q) == [], (name, p, C.undecided(q))
        # every row the call must not read is a decoy: an exact inlier, which would be counted if it were read
        e = p * L["pair_stride"]
        full = L["match"][p].copy()
        rows = E.gather(L["pts1"][e], L["pts2"][e], full, cap)[m.shape[0]:]
        if (name, p) == ("n_match_outside", 1):                       # (this pair holds launch300 again, see there)
            assert np.array_equal(E.gather(L["pts1"][e], L["pts2"][e], full, cap), C.problem("launch300")["m"])
        elif rows.shape[0]:
            d2, usable = E.sampson2(F_true.reshape(1, 9), rows)
            assert usable.all() and float(d2.max()) < 1e-18, (name, p, float(d2.max()))
    if name == "clamped":
        q, base = C.expected(name, 0), C.problem("launch300")
        assert q["ref_block"]["mask"][L["rows"]].all() and q["ref_block"]["n_inliers"] == base["ref_block"]["n_inliers"] + 3
        print("clamped: rows %s are inliers through the clamp: %d inliers against %d" % (L["rows"], q["ref_block"]["n_inliers"], base["ref_block"]["n_inliers"]))


# ---- mutants: changed copies of the restatement; each must change an output of a named case -----------------------------------
def _outputs(r):
    return (r["status"], r["winner"], r["n_inliers"], r["mask"].tobytes())


def _moved(a, b):
    """max(|dF|, |derr|) between two results."""
    return max(float(np.abs(a["F"] - b["F"]).max()), abs(a["err"] - b["err"]))


def _killed(what, case, ref, mut):
    ints = _outputs(ref) != _outputs(mut)
    moved = _moved(ref, mut)
    print("mutant %-42s on %-16s integers change: %-5s F or err moves by %.3g (bound at most %.3g)" % (what, case, ints, moved, E.TOLERANCE))
    assert ints or moved > E.TOLERANCE, what


def _gather_mutant(L, p, clamp_n=True, wrap=False, pair_stride=None, pt_stride=None):
    """epipolar_ref.gather on the launch's flat arrays, with one rule changed."""
    cap, ps, ts = L["cap"], L["pair_stride"] if pair_stride is None else pair_stride, L["pt_stride"] if pt_stride is None else pt_stride
    n = int(L["n_match"][p])
    n = min(max(n, 0), cap) if clamp_n else max(n, 0)
    rows = L["match"].reshape(-1, 3)[p * cap:p * cap + n]
    fix = (lambda v: np.mod(v, cap)) if wrap else (lambda v: np.clip(v, 0, cap - 1))
    i, j = fix(rows[:, 0].astype(np.int64)), fix(rows[:, 1].astype(np.int64))
    f1 = L["pts1"].reshape(-1)[p * ps * cap * L["pt_stride"]:]
    f2 = L["pts2"].reshape(-1)[p * ps * cap * L["pt_stride"]:]
    return np.stack([f1[i * ts], f1[i * ts + 1], f2[j * ts], f2[j * ts + 1]], axis=1)


def test_mutants():
    # the unchanged copy reads what gather reads
    for name, p in (("n_match_outside", 0), ("clamped", 0), ("stride_3_5", 1)):
        assert np.array_equal(_gather_mutant(C.launch(name), p), C.gathered(C.launch(name), p))
    # ties to the higher hypothesis
    p = C.problem("n257_clean")
    d = p["dec"]
    last = int(np.nonzero(d["valid"] & (d["score"] == d["best"]))[0][-1])
    F_last, _ = E.hypotheses(p["m"], p["seed"], [last])
    _killed("ties to the higher hypothesis", "n257_clean", p["ref_block"], E.ransac(p["m"], p["seed"], pairwise="block", winner=(last, d["best"], F_last[0])))
    # the direct rule of 8 matches removed
    p = C.problem("n8_direct")
    with patched(E, "DIRECT_N", -1):
        _killed("n == 8 direct rule removed", "n8_direct", p["ref_block"], E.ransac(p["m"], p["seed"], pairwise="block"))
    # the draw limit removed
    p = C.problem("exhausted_first")
    with patched(E, "SAMPLE_DRAWS", 250):
        _killed("draw limit of a sample removed", "exhausted_first", p["ref_block"], E.ransac(p["m"], p["seed"], pairwise="block"))
    # the launch rules
    for what, name, pair, kw in (("n_match not clamped", "n_match_outside", 0, {"clamp_n": False}),
                                 ("indices wrapped, not clamped", "clamped", 0, {"wrap": True}),
                                 ("pair_stride ignored", "stride_3_2", 1, {"pair_stride": 1}),
                                 ("pt_stride ignored", "stride_1_5", 0, {"pt_stride": 2})):
        L, q = C.launch(name), C.expected(name, pair)
        m = _gather_mutant(L, pair, **kw)
        mut = E.ransac(m, int(L["seeds"][pair]), L["thresh"], pairwise="block")
        if m.shape[0] != q["m"].shape[0]:          # more rows than the mask has: the count is what the caller sees
            mut = dict(mut, mask=mut["mask"][:q["m"].shape[0]])
        _killed(what, "%s[%d]" % (name, pair), q["ref_block"], mut)
    # the refit
    p = C.problem("n257_noisy")
    w = (p["dec"]["winner"], p["dec"]["best"], p["dec"]["winner_F"])
    run = lambda: E.ransac(p["m"], p["seed"], pairwise="block", winner=w)
    with patched(E, "rank2", lambda fn: np.array(fn, dtype=np.float64)):
        _killed("rank-2 step dropped", "n257_noisy", p["ref_block"], run())
    with patched(ER, "solve8", lambda a, pivots=None: (np.zeros((1, 8)), np.zeros(1, dtype=bool))):
        _killed("refit dropped (the winner's F carried through)", "n257_noisy", p["ref_block"], run())
    good = E.sign_rule
    with patched(E, "sign_rule", lambda Fd: -good(Fd)):
        _killed("sign rule flipped", "n257_noisy", p["ref_block"], run())
    norm, calls = E.norm_of, []

    def norm_of_all(pts, pairwise=False, index=None):
        calls.append(1)
        cols = slice(0, 2) if len(calls) % 2 == 1 else slice(2, 4)      # refit() norms the a points, then the b points
        s, _, _ = norm(pts, pairwise, index)
        _, cx, cy = norm(p["m"][:, cols], pairwise, np.arange(p["m"].shape[0]))
        return s, cx, cy
    with patched(E, "norm_of", norm_of_all):
        _killed("centroid over all matches, not the inliers", "n257_noisy", p["ref_block"], run())


def test_branches_not_covered():
    """The branches listed in NOT_COVERED are reached by no case: asserted, so that a case that reaches one is noticed."""
    for name in C.SINGLES:
        p = C.problem(name)
        d = p["dec"]
        if d["valid"].any():
            assert d["best"] >= E.MIN_SCORE and p["ref_block"]["status"] == 0, name
            assert p["report"]["solved"] and p["report"]["norm_usable"], name
        else:
            assert p["ref_block"]["status"] == 1, name
    for what, why in NOT_COVERED.items():
        print("not covered: %s -- %s" % (what, why))


# ---- the filter and the pose ---------------------------------------------------------------------------------------------------
def test_filter_cases_take_every_branch():
    c = C.filter_case("rules")
    out, n_out = c["expect"]
    print("filter rules: n_match %s n_inliers %s status %s min_inliers %d -> kept %s" %
          (c["n_match"].tolist(), c["n_inliers"].tolist(), c["status"].tolist(), c["min_inliers"], n_out.tolist()))
    assert set(np.unique(c["mask"][0])) == {0, 2, 255} and n_out[0] == np.count_nonzero(c["mask"][0])
    assert n_out[1] == 0 and not out[1].any()                                  # an all-zero mask is applied
    assert n_out[2] == 40 and np.array_equal(out[2, :40], c["match"][2, :40])   # n_inliers = min_inliers: filtered
    assert n_out[3] == 1025 and np.array_equal(out[3, :1025], c["match"][3, :1025]) and not out[3, 1025:].any()   # one below
    assert n_out[4] == 0 and 0 < n_out[5] < 1100 and n_out[6] == 64 and n_out[7] == 0
    full = C.filter_case("full4096")
    assert full["n_match"][0] == 4096 and 0 < full["expect"][1][0] < 4096


def test_pose_decisions_are_decided():
    c = C.pose_case()
    L = c["L"]
    want = []
    for k, (front, n_inl) in enumerate(C.POSE_ROWS):
        m = C.gathered(L, k)
        r = PR.two_view_pose(c["F"][k], c["mask"][k, :m.shape[0]], n_inl, 0, m, c["intr"][0])
        z = r["depth"][r["front"]]
        print("pose row %d: %d in the mask, n_inliers %d -> n_front %d counts %s status %d (least depth %.3g)" %
              (k, front, n_inl, r["n_front"], r["counts"].tolist(), r["status"], z.min()))
        assert r["n_front"] == front and sorted(r["counts"])[-2] == 0 and z.min() > 0.1
        want.append(r["status"])
    assert want == [2 if (f < 8 or 2 * f < n) else 0 for f, n in C.POSE_ROWS] == [2, 0, 0, 0, 2, 0, 0, 2]
