"""The cases of the exact epipolar tests: one table of problems (matches, seed, threshold), one of
launches (the operator's arrays) and the filter's and the pose's inputs, all from seeds.  tests/test_epipolar_exact_cpu.py
asserts on the CPU that every one of them is decided (tests/epipolar_ref.py `decisions`); tests/test_gpu_epipolar_exact.py
runs exactly these inputs on the device.  A random scene that is not decided is redrawn (scene seed + 1000 k, at most
REDRAWS times); none is dropped.  Everything here is computed once and shared: treat it as read-only."""
import functools

import numpy as np

from tests import epipolar_ref as E

SCENE_SEED, RANSAC_SEED, REDRAWS = 11, 211, 8
PIVOT_ACCEPTED, PIVOT_REFUSED, GAP = 1e-9, 1e-15, 1e-6     # the conditions of a decided case
SIZES = (7, 8, 9, 10, 63, 64, 65, 255, 256, 257, 511, 512, 513, 4095, 4096)
INTRINSICS = ((E.FOCAL, E.FOCAL, E.WIDTH / 2, E.HEIGHT / 2), (E.FOCAL2, E.FOCAL2, E.WIDTH / 2, E.HEIGHT / 2))

# ---- problems: name -> (kind, inliers, outliers, noise px, thresh, scene seed, RANSAC seed) -----------------------------------
PROBLEMS = {}
for _n in SIZES:            # about 30 % outliers, noise-free and with 0.5 px of noise
    PROBLEMS["n%d_clean" % _n] = ("scene", _n - (3 * _n) // 10, (3 * _n) // 10, 0.0, 1.0, SCENE_SEED, RANSAC_SEED)
    PROBLEMS["n%d_noisy" % _n] = ("scene", _n - (3 * _n) // 10, (3 * _n) // 10, 0.5, 1.0, SCENE_SEED, RANSAC_SEED)
for _k in (255, 256, 257):  # the inlier count on either side of 256 (a thread's second term), below and above 512 rows
    PROBLEMS["in%d_out100" % _k] = ("scene", _k, 100, 0.0, 1.0, SCENE_SEED, RANSAC_SEED)
    PROBLEMS["in%d_out300" % _k] = ("scene", _k, 300, 0.0, 1.0, SCENE_SEED, RANSAC_SEED)
PROBLEMS.update({
    "empty": ("scene", 0, 0, 0.0, 1.0, SCENE_SEED, RANSAC_SEED),
    "n12_clean": ("scene", 9, 3, 0.0, 1.0, SCENE_SEED, RANSAC_SEED),
    "thresh_0.25": ("scene", 150, 100, 0.5, 0.25, SCENE_SEED, RANSAC_SEED),
    "thresh_3": ("scene", 150, 100, 0.5, 3.0, SCENE_SEED, RANSAC_SEED),
    "launch300": ("scene", 210, 90, 0.5, 1.0, SCENE_SEED, RANSAC_SEED),
    # without the direct rule of 8 matches, hypothesis 0 of (seed 458, n = 8) would spend its 64 draws on 7 distinct matches
    # and hypothesis 1 would win (a search over the seeds 0 .. 458): the rule is distinguished by `winner`
    "n8_direct": ("scene", 6, 2, 0.0, 1.0, SCENE_SEED, 458),
    # the sampler: hypothesis 1267 of (seed 80, n = 9) spends its 64 draws (found by a search over the seeds 0 .. 80)
    "exhausted_seed80": ("scene", 9, 0, 0.0, 1.0, SCENE_SEED, 80),
    # ... and hypothesis 7 of (seed 4866, n = 9) does (a search over hypotheses 0 .. 11 of the seeds 0 .. 11999); with more
    # draws it would hold the matches 0 6 3 1 7 8 4 2.  Match 5 is a copy of match 1, the hypotheses 0 .. 6 hold both (an
    # exact zero pivot), so the winner is the first hypothesis after 7 that leaves 1 or 5 out; a sampler that drew on would
    # make 7 the winner: the path is distinguished by `winner`.
    "exhausted_first": ("exhausted_first", 9, 0, 0.0, 1.0, SCENE_SEED, 4866),
    # 12 matches and 4 copies of match 0: under seed 7 most samples hold two copies and are refused by a zero pivot
    "copies": ("copies", 12, 0, 0.0, 1.0, SCENE_SEED, 7),
    # a few outlier rows hold NaN, inf and 1e200: never inliers, and no sample that holds one is valid
    "nonfinite": ("nonfinite", 40, 16, 0.0, 1.0, SCENE_SEED, RANSAC_SEED),
    # all points on one plane: every 8x9 system has rank 6, every hypothesis is refused by the pivot rule, status 1
    "planar": ("planar", 48, 0, 0.0, 1.0, 4, 104),
})
NONFINITE_ROWS = ((np.nan, 10.0, 20.0, 30.0), (10.0, np.inf, 20.0, 30.0), (10.0, 20.0, -np.inf, 30.0), (10.0, 20.0, 30.0, np.nan),
                  (1e200, 20.0, 30.0, 40.0), (10.0, 20.0, 1e200, 1e200), (-1e200, 1e200, 30.0, 40.0), (np.inf, np.nan, 1e200, 5.0))
FIXED = ("exhausted_first", "copies", "nonfinite", "planar", "empty")    # decided by construction: never redrawn


def family(name):
    """The family whose measured ratio bounds F and err: the size class and whether the inliers carry noise."""
    n = sum(PROBLEMS[name][1:3]) + (4 if name == "copies" else 0)
    size = "small" if n <= 65 else ("large" if n >= 4095 else "mid")
    return size + ("_noisy" if PROBLEMS[name][3] > 0.0 else "_clean")


FAMILIES = ("small_clean", "small_noisy", "mid_clean", "mid_noisy", "large_clean", "large_noisy")
# The largest max(|dF|, |derr|) / max|F| of the device against the block-order restatement per family, as
# tools/measure_epipolar_exact.py measured it on the MI355X (profiles/epipolar_exact_measure.txt).
# Every family measured 0: the device's F and err are bit-identical to that restatement on every case, so the floor decides.
MEASURED = {"small_clean": 0.0, "small_noisy": 0.0, "mid_clean": 0.0, "mid_noisy": 0.0, "large_clean": 0.0, "large_noisy": 0.0}
FLOOR = 16.0 * 2.0 ** -53


def bound(name):
    """The bound on max(|dF|, |derr|) / max|F| against the block-order restatement: 4 x the family's measured ratio, never
    below 16 x 2^-53, never above the tolerance of the older tests."""
    return min(max(4.0 * MEASURED[family(name)], FLOOR), E.TOLERANCE)


def _matches(kind, n_in, n_out, noise, scene_seed):
    sc = E.make_scene(scene_seed, n_in, n_out, noise=noise, planar=kind == "planar")
    m, truth = sc["m"], sc["truth"]
    if kind == "exhausted_first":
        m = m.copy()
        m[5] = m[1]
    elif kind == "copies":
        m = np.concatenate([m, np.repeat(m[:1], 4, axis=0)])
        truth = np.concatenate([truth, np.ones(4, dtype=bool)])
    elif kind == "nonfinite":
        m = m.copy()
        rows = np.nonzero(~truth)[0][:len(NONFINITE_ROWS)]
        m[rows] = np.array(NONFINITE_ROWS)
    return np.ascontiguousarray(m), truth


def solve(m, seed, thresh):
    """The restatement of one problem: dec = decisions, ref / ref_pairwise / ref_block = ransac with its refit's sums in the
    three orders, report = the refit's margins (block order), spread = the largest difference of F or err between two orders."""
    dec = E.decisions(m, seed, thresh)
    w = (dec["winner"], dec["best"], dec["winner_F"])
    report = {}
    out = {"m": m, "seed": seed, "thresh": thresh, "dec": dec, "ref": E.ransac(m, seed, thresh, winner=w),
           "ref_pairwise": E.ransac(m, seed, thresh, pairwise=True, winner=w),
           "ref_block": E.ransac(m, seed, thresh, pairwise="block", winner=w, report=report), "report": report}
    refs = [out[k] for k in ("ref", "ref_pairwise", "ref_block")]
    out["spread"] = max(max(float(np.abs(a["F"] - b["F"]).max()), abs(a["err"] - b["err"])) for a in refs for b in refs)
    return out


def undecided(p):
    """Why the problem p (solve()) is not decided: a list of reasons, empty when it is."""
    dec, rep, why = p["dec"], p["report"], []
    refs = [p[k] for k in ("ref", "ref_pairwise", "ref_block")]
    if not dec["decided"]:
        why.append("winner: slack %s, %d ambiguous" % (dec["slack"], dec["ambiguous"][dec["winner"]]))
    if dec["pivot_least_accepted"] < PIVOT_ACCEPTED:
        why.append("accepted pivot %.3g" % dec["pivot_least_accepted"])
    if dec["pivot_largest_refused"] > PIVOT_REFUSED:
        why.append("refused pivot %.3g" % dec["pivot_largest_refused"])
    if any(r["status"] != refs[0]["status"] or r["winner"] != (dec["winner"] if r["status"] == 0 else -1) for r in refs):
        why.append("the summation orders disagree on status or winner")
    if refs[0]["status"] == 0:
        if not rep["norm_usable"] or not rep["solved"]:
            why.append("the refit's fallbacks")
        elif float(rep["pivots"].min()) < PIVOT_ACCEPTED:
            why.append("refit pivot %.3g" % rep["pivots"].min())
        if min(rep["gap_G"], rep["gap_Fd"]) < GAP:
            why.append("argmax gap %.3g / sign gap %.3g" % (rep["gap_G"], rep["gap_Fd"]))
    return why


@functools.lru_cache(maxsize=None)
def problem(name):
    """solve() of the named problem plus truth [n], redraws (how often the scene was drawn again) and name."""
    kind, n_in, n_out, noise, thresh, scene_seed, seed = PROBLEMS[name]
    why = None
    for k in range(1 if name in FIXED else REDRAWS + 1):
        m, truth = _matches(kind, n_in, n_out, noise, scene_seed + 1000 * k)
        p = solve(m, seed, thresh)
        why = undecided(p)
        if not why or name in FIXED:
            p.update(truth=truth, redraws=k, name=name, scene_seed=scene_seed + 1000 * k, why=why)
            return p
    raise AssertionError("%s is not decided after %d redraws (%s): redesign it" % (name, REDRAWS, why))


SINGLES = tuple(PROBLEMS)


# ---- launches: the operator's arrays -------------------------------------------------------------------------------------
def arrays(ms, cap, pair_stride=1, pt_stride=2, decoy_seed=SCENE_SEED, rng_seed=0, ends=False):
    """The operator's inputs for the matches ms (one [n,4] per pair): pts1, pts2 float64 [P * pair_stride, cap, pt_stride]
    (pair p at entry p * pair_stride), match float32 [P, cap, 3] with the b points scattered by a permutation, n_match.
    Every unused point row, every entry between the pairs and every match row past n holds a decoy: an exact inlier of the
    scenes' F at distance 0, which would raise n_inliers if it were read.  ends: match row 0 -> point rows (0, cap - 1) and the
    last match row -> (cap - 1, 0), the targets of the clamped indices."""
    P = len(ms)
    rng = np.random.RandomState(1000 * cap + 7 * pair_stride + 13 * pt_stride + rng_seed)
    pts1, pts2 = (rng.uniform(0, 300, (P * pair_stride, cap, pt_stride)) for _ in range(2))
    match = np.zeros((P, cap, 3), dtype=np.float32)
    n_match = np.zeros(P, dtype=np.int32)
    for e in range(P * pair_stride):
        live = e % pair_stride == 0
        p = e // pair_stride
        n = ms[p].shape[0] if live else 0
        assert n <= cap and (not ends or n == cap)
        d = E.make_scene(decoy_seed, cap + 1 + e, 0)["m"]
        order = n + rng.permutation(cap - n)                 # the decoys keep to the point rows n .. cap - 1 on both sides
        pts1[e, n:, :2], pts2[e, order, :2] = d[n:cap, :2], d[n:cap, 2:]
        if not live:
            continue
        match[p, n:, 0], match[p, n:, 1] = np.arange(n, cap), order
        m = ms[p]
        perm = rng.permutation(n)
        if ends:
            perm = np.concatenate([[cap - 1], rng.permutation(np.arange(1, cap - 1)), [0]])
        pts1[e, :n, :2], pts2[e, perm, :2] = m[:, :2], m[:, 2:]
        match[p, :n, 0], match[p, :n, 1], match[p, :n, 2] = np.arange(n), perm, rng.rand(n)
        n_match[p] = n
    return pts1, pts2, match, n_match


def gathered(L, p):
    """The matches pair p of the launch L holds: what the kernel stages (indices and count clamped)."""
    e = p * L["pair_stride"]
    return E.gather(L["pts1"][e], L["pts2"][e], L["match"][p], L["n_match"][p])


def _launch(names, cap, pair_stride=1, pt_stride=2, groups=0, thresh=1.0, ms=None, seeds=None, **kw):
    ps = [problem(nm) for nm in names]
    pts1, pts2, match, n_match = arrays([p["m"] for p in ps] if ms is None else ms, cap, pair_stride, pt_stride, **kw)
    return {"names": tuple(names), "pts1": pts1, "pts2": pts2, "match": match, "n_match": n_match, "cap": cap,
            "seeds": np.array([p["seed"] for p in ps] if seeds is None else seeds, dtype=np.int64), "pair_stride": pair_stride,
            "pt_stride": pt_stride, "groups": groups, "thresh": thresh, "same_as": tuple(names)}


CAPS = (300, 301, 1024, 4096)
GROUPS = (1, 2, 3, 7, 31, 32, 33, 50, 51, 63, 64)
BATCH9 = ("n9_clean", "n10_noisy", "n63_clean", "n64_noisy", "n65_clean", "n255_noisy", "n256_clean", "n257_noisy", "launch300")
MIXED = ("empty", "n7_clean", "n8_clean", "n9_clean", "n64_clean", "n257_clean", "launch300", "n12_clean")   # 0 7 8 9 64 257 300 12
CLAMPED_ROWS = ((0, -3.0), (0, None), (1, None))     # (column, value; None: see launch("clamped"))


@functools.lru_cache(maxsize=None)
def launch(name):
    """One call of the operator.  dict(pts1, pts2, match, n_match, seeds, cap, pair_stride, pt_stride, groups, thresh, names,
    same_as): pair p must equal, bit for bit, the single launch at cap = n of problem same_as[p] (None: a problem of its own,
    expected from solve(gathered()))."""
    if name.startswith("single:"):           # the launch every other one is compared with: one pair, cap = n, the library's groups
        return _launch((name[7:],), max(problem(name[7:])["m"].shape[0], 1), thresh=problem(name[7:])["thresh"])
    if name.startswith("cap"):
        return _launch(("launch300",), int(name[3:]))
    if name.startswith("groups"):
        return _launch(("launch300", "exhausted_first"), 300, groups=int(name[6:]))
    if name.startswith("stride"):            # stride_<pair_stride>_<pt_stride>
        a, b = (int(v) for v in name.split("_")[1:])
        return _launch(("launch300", "n64_noisy"), 320, pair_stride=a, pt_stride=b)
    if name == "batch9":
        return _launch(BATCH9, 320)
    if name == "batch8":
        return _launch(BATCH9[:8], 320)
    if name == "mixed":
        return _launch(MIXED, 301, pair_stride=2, pt_stride=3)
    if name == "one_row_n5":                    # one row is staged, status 1
        L = _launch(("n9_clean",), 1, ms=[problem("n9_clean")["m"][:1]])
        L["n_match"][:] = 5
        L["same_as"] = (None,)
        return L
    if name == "n_match_outside":            # cap + 37 reads cap rows (pair 1 lies behind them), -3 reads none
        L = _launch(("launch300", "launch300"), 300)
        L["n_match"][:] = (300 + 37, -3)
        for k in ("match", "pts1", "pts2"):      # pair 1 is pair 0 again: a count that is not clamped reads its first 37
            L[k][1] = L[k][0]                    # rows a second time, and a count of -3 that is read as 300 finds a model
        L["same_as"] = ("launch300", "empty")
        return L
    if name == "clamped":
        # three outlier rows of launch300 get an index outside the arrays: -3 (-> 0), cap (-> cap - 1) in column 0 and
        # cap + 100 (-> cap - 1) in column 1; the other column names the partner of the clamped row, which is an inlier, so
        # each row is an inlier when the index is clamped and an outlier when it wraps around
        p = problem("launch300")
        m, truth = p["m"].copy(), p["truth"]
        ins = np.nonzero(truth)[0]
        keep = np.concatenate([ins[:1], np.delete(np.arange(300), ins[[0, -1]]), ins[-1:]])    # inliers at both ends
        m, truth = m[keep], truth[keep]
        L = _launch(("launch300",), 300, ms=[m], ends=True)
        out = np.nonzero(~truth)[0][:3]
        L["match"][0, out[0], :2] = (-3.0, 299.0)       # (0, cap - 1) is match row 0
        L["match"][0, out[1], :2] = (300.0, 0.0)        # (cap - 1, 0) is the last match row
        L["match"][0, out[2], :2] = (0.0, 400.0)        # (0, cap - 1) again
        L["same_as"] = (None,)
        L["rows"] = out
        return L
    raise KeyError(name)


LAUNCHES = (tuple("cap%d" % c for c in CAPS) + tuple("groups%d" % g for g in GROUPS)
            + ("stride_1_2", "stride_1_5", "stride_3_2", "stride_3_5", "batch9", "batch8", "mixed", "one_row_n5", "n_match_outside",
               "clamped"))


@functools.lru_cache(maxsize=None)
def expected(name, p):
    """solve() of pair p of a launch."""
    L = launch(name)
    if L["same_as"][p] is not None:
        return problem(L["same_as"][p])
    return solve(gathered(L, p), int(L["seeds"][p]), L["thresh"])


# ---- ssp_op_filter_matches -------------------------------------------------------------------------------------------------
def filter_ref(match, n_match, mask, status, n_inliers, min_inliers):
    """match_filter_kernel: the rows whose mask byte is not 0, in order, zero rows behind them; every row of a pair with
    status != 0 or n_inliers < min_inliers."""
    P, cap = match.shape[:2]
    out, n_out = np.zeros_like(match), np.zeros(P, dtype=np.int32)
    for p in range(P):
        n = min(max(int(n_match[p]), 0), cap)
        keep = np.ones(n, dtype=bool) if (status[p] != 0 or n_inliers[p] < min_inliers) else mask[p, :n] != 0
        k = int(keep.sum())
        out[p, :k], n_out[p] = match[p, :n][keep], k
    return out, n_out


@functools.lru_cache(maxsize=None)
def filter_case(name):
    """dict(match, n_match, mask, status, n_inliers, min_inliers, expect = filter_ref of them)."""
    rng = np.random.RandomState(35)
    if name == "full4096":
        cap, ns, min_inl = 4096, [4096], 8
        status = [0]
    else:  # "rules": pair 0 mask bytes 2 and 255; 1 an all-zero mask that is applied; 2 n_inliers = min_inliers; 3 one below it;
        #           4 n_match = -3; 5 n_match = cap + 37; 6 status 1 with a mask; 7 an empty pair
        cap, ns, min_inl = 1100, [1100, 700, 1025, 1025, -3, 1137, 64, 0], 40
        status = [0, 0, 0, 0, 0, 0, 1, 0]
    P = len(ns)
    match = rng.rand(P, cap, 3).astype(np.float32) + 1.0          # no row is zero
    match[:, :, 0] = np.sort(rng.rand(P, cap).astype(np.float32), axis=1) * 4096.0
    mask = (rng.rand(P, cap) < 0.55).astype(np.uint8)
    n_inl = np.array([int(mask[p, :min(max(n, 0), cap)].sum()) for p, n in enumerate(ns)], dtype=np.int32)
    if name == "rules":
        mask[0] = mask[0] * np.where(rng.rand(cap) < 0.5, 2, 255).astype(np.uint8)
        mask[1], n_inl[1] = 0, 40
        mask[2, 40:] = 0
        mask[2, :40], n_inl[2] = 1, 40
        mask[3, 39:] = 0
        mask[3, :39], n_inl[3] = 1, 39
    c = {"match": match, "n_match": np.array(ns, dtype=np.int32), "mask": mask, "status": np.array(status, dtype=np.int32),
         "n_inliers": n_inl, "min_inliers": min_inl}
    c["expect"] = filter_ref(**c)
    return c


FILTERS = ("full4096", "rules")


# ---- the pose's decisions on the restatement's F and hand-made masks ----------------------------------------------------------
# (front, n_inliers): the mask holds `front` true inliers (all in front of both cameras under the true candidate) and n_inliers
# is given by hand: the status-2 rule n_front < 8 or 2 n_front < n_inliers on both sides of both boundaries.
POSE_ROWS = ((7, 8), (8, 8), (8, 15), (8, 16), (8, 17), (20, 39), (20, 40), (20, 41))
POSE_PROBLEM = "n64_clean"


@functools.lru_cache(maxsize=None)
def pose_case():
    """dict(L = a launch whose pairs all hold POSE_PROBLEM, F [P,3,3], mask [P,cap], n_inliers [P], status [P], intr)."""
    p = problem(POSE_PROBLEM)
    P, cap = len(POSE_ROWS), 80
    L = _launch((POSE_PROBLEM,) * P, cap, pt_stride=3)
    ins = np.nonzero(p["ref_block"]["mask"])[0]
    mask = np.zeros((P, cap), dtype=np.uint8)
    for k, (front, _) in enumerate(POSE_ROWS):
        mask[k, ins[k:k + front]] = 1
    return {"L": L, "F": np.repeat(p["ref_block"]["F"][None], P, axis=0), "mask": mask,
            "n_inliers": np.array([r[1] for r in POSE_ROWS], dtype=np.int32), "status": np.zeros(P, dtype=np.int32),
            "intr": np.array(INTRINSICS, dtype=np.float64)[None]}
