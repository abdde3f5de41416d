"""The cases of the exact tests of the evaluation kernels, all from seeds; numpy only.

Repeatability: a *call* is one launch of eval_repeat_kernel - dict(name, height, width, cap, pair_stride, n_pairs, pts1 /
pts2 [n_pairs * pair_stride, cap, 3], n1 / n2, H / H_inv [n_pairs,3,3], keep_k, thresh, pairs = the pairs' names).  Rows past a
count hold points that would repeat (confidence 2), and so do the decoy entries between the strides (count = cap).
Random pairs are redrawn (seed + 1000 k) until the restatement's decision margin is >= MARGIN; no case is dropped.

RANSAC: a *problem* is dict(name, m [n,4], seed, dist [n] float32); problems are redrawn the same way until no residual
lies within RESID_BAND of the threshold under any of the restatement's homographies (tests/eval_restatement.py)."""
import functools

import numpy as np

from tests import eval_restatement as ER
from tests import evaluation_ref as R

MARGIN = 1e-6
RESID_BAND = 1e-6
TRAP_CONF = 2.0


def _translation(tx, ty):
    return np.array([[1.0, 0, tx], [0, 1.0, ty], [0, 0, 1.0]])


def _perspective(rng, height, width):
    a, b, c, d = rng.uniform(-0.08, 0.08, 4)
    e, f = rng.uniform(-0.05, 0.05, 2) / max(height, width)
    return np.array([[1 + a, b, rng.uniform(-0.05, 0.05) * width], [c, 1 + d, rng.uniform(-0.05, 0.05) * height], [e, f, 1.0]])


def _conf(rng, n):
    return (rng.permutation(n) + 1.0) / (n + 7.0)


def _random_pair(rng, height, width, n1, n2, H, thresh):
    """n1 points over the image and a margin of 2 px around it; the first min(n1, n2) points of the other side are their
    images displaced by up to 2 thresh in a random direction, the rest are free; side 2 is shuffled."""
    def free(n):
        return np.stack([rng.uniform(-2, width + 2, n), rng.uniform(-2, height + 2, n)], 1)
    p1 = free(n1)
    p2 = free(n2)
    k = min(n1, n2)
    u, v = R.warp(H, p1[:k, 0], p1[:k, 1])
    r, t = rng.uniform(0, 2 * thresh, k), rng.uniform(0, 2 * np.pi, k)
    p2[:k] = np.stack([u + r * np.cos(t), v + r * np.sin(t)], 1)
    p2 = p2[rng.permutation(n2)]
    return (np.concatenate([p1, _conf(rng, n1)[:, None]], 1).reshape(-1, 3),
            np.concatenate([p2, _conf(rng, n2)[:, None]], 1).reshape(-1, 3))


def _traps(rng, height, width, H, n):
    """n pairs of rows that would repeat at distance 0 with a confidence above every real one."""
    x = np.stack([rng.uniform(0.2, 0.8, n) * width, rng.uniform(0.2, 0.8, n) * height], 1)
    u, v = R.warp(H, x[:, 0], x[:, 1])
    c = np.full((n, 1), TRAP_CONF)
    return np.concatenate([x, c], 1), np.concatenate([np.stack([u, v], 1), c], 1)


def _assemble(name, height, width, cap, stride, pairs, keep_k, thresh, seed):
    """pairs: list of (name, p1 [a,3], p2 [b,3], H, count1 or None, count2 or None); a count None is the number of rows."""
    rng = np.random.default_rng(seed + 77)
    P = len(pairs)
    pts1, pts2 = np.zeros((P * stride, cap, 3)), np.zeros((P * stride, cap, 3))
    n1, n2 = np.full(P * stride, cap, np.int32), np.full(P * stride, cap, np.int32)
    Hs = np.stack([p[3] for p in pairs]).astype(np.float64)
    for e in range(P * stride):
        t1, t2 = _traps(rng, height, width, Hs[e // stride], cap)
        pts1[e], pts2[e] = t1, t2
    for p, (_, p1, p2, _, c1, c2) in enumerate(pairs):
        e = p * stride
        assert len(p1) <= cap and len(p2) <= cap
        pts1[e, :len(p1)], pts2[e, :len(p2)] = p1, p2
        n1[e] = len(p1) if c1 is None else c1
        n2[e] = len(p2) if c2 is None else c2
    return dict(name=name, height=height, width=width, cap=cap, pair_stride=stride, n_pairs=P, pts1=pts1, pts2=pts2, n1=n1, n2=n2,
                H=Hs, H_inv=np.stack([np.linalg.inv(h) for h in Hs]), keep_k=keep_k, thresh=thresh, pairs=[p[0] for p in pairs])


def _search(build, seed):
    """build(seed) -> call; the first of seed, seed + 1000, ... whose margins all reach MARGIN."""
    for k in range(64):
        call = build(seed + 1000 * k)
        out, margins = R.repeatability_call(call)
        if margins.min() >= MARGIN:
            call["seed"], call["expect"], call["margins"] = seed + 1000 * k, out, margins
            return call
    raise AssertionError("no decided draw within 64 seeds")


# ---- hand-computable pairs (integer or eighth-pixel coordinates; the counts are worked out in test_evaluation_ref_cpu.py) ----
def threshold_pair():
    """37x53, H = translation (2, 1).  Warped side-1 points a0..a4 and side-2 points b0..b4 at distances 0, 3, 5 (3-4-5), 4 and
    a far one."""
    A = np.array([[5, 5], [20, 5], [35, 5], [5, 25], [25, 25]], float)
    B = np.array([[5, 5], [23, 5], [38, 9], [5, 29], [45, 30]], float)
    c = np.array([0.9, 0.8, 0.7, 0.6, 0.5])[:, None]
    return np.concatenate([A - [2, 1], c], 1), np.concatenate([B, c], 1), _translation(2, 1)


def border_pair():
    """12x16, H = identity: points exactly on x = 0, W - 1, W and y = 0, H - 1, H, one at x = -1, and on side 2 three more with
    negative or fractional sub-pixel coordinates for the float32 truncation of the matching-score count."""
    p = np.array([[0, 5], [15, 5], [16, 5], [4, 0], [4, 11], [4, 12], [-1, 3]], float)
    extra = np.array([[-0.5, 3.25], [3.25, -0.75], [11.625, 2.5]])
    c1 = (np.arange(len(p)) + 1.0)[:, None] / 16
    p2 = np.concatenate([p, extra])
    return np.concatenate([p, c1], 1), np.concatenate([p2, (np.arange(len(p2)) + 1.0)[:, None] / 16], 1), np.eye(3)


def tie_pair(signed_zero):
    """48x64, H = translation (3, 2), 12 points a side with ONE confidence (or -0.0 on rows 0..5 and +0.0 on rows 6..11): rows
    0..5 have a partner at distance 1, rows 6..11 have none within 9 px.  With keep_k = 6 the lower-index rule keeps the
    partnered rows (count1 = count2 = 6); the higher-index rule - or an order that puts +0.0 above -0.0 - keeps the others (0)."""
    A = np.array([[6 + 9 * k, 6] for k in range(6)] + [[6 + 9 * k, 30] for k in range(6)], float)
    B = np.array([[6 + 9 * k, 7] for k in range(6)] + [[6 + 9 * k, 42] for k in range(6)], float)
    c = np.where(np.arange(12) < 6, -0.0, 0.0)[:, None] if signed_zero else np.full((12, 1), 0.5)
    return np.concatenate([A - [3, 2], c], 1), np.concatenate([B, c], 1), _translation(3, 2)


def horizon_pair(rng):
    """48x64, w2 = 1 - x / 32: the horizon x = 32 crosses the cloud; (32, 7) lies exactly on it (u = v = inf) and (32, 0) gives
    v = 0 / 0.  Side 2 has (-32, 4) on the horizon of inv(H) (w2 = 1 + x / 32)."""
    H = np.array([[1.0, 0, 0], [0, 1.0, 0], [-1 / 32, 0, 1.0]])
    p1 = np.stack([rng.uniform(0, 64, 40), rng.uniform(0, 48, 40)], 1)
    p1[0], p1[1] = (32, 7), (32, 0)
    u, v = R.warp(H, p1[:, 0], p1[:, 1])
    p2 = np.stack([u, v], 1) + rng.uniform(-2.5, 2.5, (40, 2))
    p2[~np.isfinite(p2).all(1)] = (10, 10)
    p2[2] = (-32, 4)
    return np.concatenate([p1, _conf(rng, 40)[:, None]], 1), np.concatenate([p2, _conf(rng, 40)[:, None]], 1), H


def _keepk_data(seed):
    """48x64: 20 side-1 points whose image is inside and 6 outside it with the HIGHEST confidences (a top-k ahead of the filter
    would spend its places on them); side 2 likewise."""
    rng = np.random.default_rng(seed)
    H = _perspective(rng, 48, 64)
    x = np.stack([rng.uniform(12, 48, 20), rng.uniform(10, 33, 20)], 1)
    far = np.stack([rng.uniform(80, 90, 6), rng.uniform(5, 40, 6)], 1)
    u, v = R.warp(H, x[:, 0], x[:, 1])
    r, t = rng.uniform(0, 6, 20), rng.uniform(0, 2 * np.pi, 20)
    y = np.stack([u + r * np.cos(t), v + r * np.sin(t)], 1)
    c1 = np.concatenate([_conf(rng, 20), 1.5 + _conf(rng, 6)])
    c2 = np.concatenate([_conf(rng, 20), 1.5 + _conf(rng, 6)])
    o1, o2 = rng.permutation(26), rng.permutation(26)
    p1 = np.concatenate([np.concatenate([x, far]), c1[:, None]], 1)[o1]
    p2 = np.concatenate([np.concatenate([y, far + [0, 1]]), c2[:, None]], 1)[o2]
    return p1, p2, H


def _levels_data(seed):
    """48x64, H = translation (2, 1), 30 points a side well inside, side 2 = the images displaced by < 4 px with the SAME
    confidences drawn from 3 levels: keep_k = the number of points on the two upper levels, so every tie lies inside the kept set
    (or wholly outside it) and the result cannot depend on the tie rule."""
    rng = np.random.default_rng(seed)
    x = np.stack([rng.uniform(6, 54, 30), rng.uniform(6, 38, 30)], 1)
    c = np.array([0.25, 0.5, 0.75])[rng.integers(0, 3, 30)]
    y = x + [2, 1] + rng.uniform(-2.8, 2.8, (30, 2))
    o = rng.permutation(30)
    return np.concatenate([x, c[:, None]], 1), np.concatenate([y, c[:, None]], 1)[o], _translation(2, 1), int(np.sum(c >= 0.5))


@functools.lru_cache(maxsize=None)
def repeat_calls():
    """Every launch of the GPU test, with `expect` = the restatement's [P,8] and `margins`."""
    calls = []

    def counts_small(seed):
        rng = np.random.default_rng(seed)
        h, w, cap, th = 12, 16, 24, 3.0
        Hs = [_perspective(rng, h, w) for _ in range(6)]
        sizes = [(0, 5), (5, 0), (0, 0), (1, 1), (cap, cap), (cap, cap)]
        pairs = []
        for k, (a, b) in enumerate(sizes):
            p1, p2 = _random_pair(rng, h, w, a, b, Hs[k], th)
            over = k == 5
            pairs.append(("n%d_%d%s" % (a, b, "_over" if over else ""), p1, p2, Hs[k], cap + 37 if over else None, cap + 1 if over else None))
        return _assemble("counts_12x16_stride2", h, w, cap, 2, pairs, 1000, th, seed)
    calls.append(_search(counts_small, 3401))

    def counts_mid(seed):
        rng = np.random.default_rng(seed)
        h, w, cap, th = 37, 53, 257, 2.0
        pairs = []
        for a, b in ((255, 256), (256, 257), (257, 255)):
            H = _perspective(rng, h, w)
            p1, p2 = _random_pair(rng, h, w, a, b, H, th)
            pairs.append(("n%d_%d" % (a, b), p1, p2, H, None, None))
        return _assemble("counts_37x53_stride3", h, w, cap, 3, pairs, 100, th, seed)
    calls.append(_search(counts_mid, 3402))

    # thresholds: one hand pair at 3, one ulp below 3, 5, one ulp below 5, and 0
    p1, p2, H = threshold_pair()
    for nm, th in (("3", 3.0), ("3_below", np.nextafter(3.0, 0)), ("5", 5.0), ("5_below", np.nextafter(5.0, 0)), ("0", 0.0)):
        calls.append(_search(lambda s, th=th, nm=nm: _assemble("thresh_" + nm, 37, 53, 8, 1, [("hand", p1, p2, H, None, None)], 1000, th, s), 3403))

    def geometry(seed):
        rng = np.random.default_rng(seed)
        b1, b2, Hb = border_pair()
        o1, o2 = _random_pair(rng, 12, 16, 9, 9, np.eye(3), 3.0)
        o1[:, 0] = -1 - 4 * rng.uniform(size=9)  # every side-1 point left of the image
        o2[:, :2] = np.stack([rng.uniform(1, 15, 9), rng.uniform(1, 11, 9)], 1)
        return _assemble("geometry_12x16", 12, 16, 12, 2, [("border", b1, b2, Hb, None, None), ("side1_outside", o1, o2, np.eye(3), None, None)],
                         1000, 3.0, seed)
    calls.append(_search(geometry, 3404))

    def horizon(seed):
        rng = np.random.default_rng(seed)
        h1, h2, H = horizon_pair(rng)
        return _assemble("horizon_48x64", 48, 64, 40, 1, [("horizon", h1, h2, H, None, None)], 30, 3.0, seed)
    calls.append(_search(horizon, 3405))

    # keep_k: 1, 7 of 20, the inside count and its neighbours, >= cap - one data set, found at keep_k = 7
    base = _search(lambda s: _assemble("keepk_7", 48, 64, 26, 1, [("k20",) + _keepk_data(s) + (None, None)], 7, 3.0, s), 3406)
    assert base["expect"][0, 0] == 7 and R.repeatability_call(dict(base, keep_k=1000))[0][0, 0] == 20
    calls.append(base)
    for kk in (1, 19, 20, 21, 26, 1000):
        calls.append(_search(lambda s, kk=kk: _assemble("keepk_%d" % kk, 48, 64, 26, 1, [("k20",) + _keepk_data(base["seed"]) + (None, None)],
                                                         kk, 3.0, s), 3406))

    def levels(seed):
        p1, p2, H, kk = _levels_data(seed)
        return _assemble("ties_3levels", 48, 64, 32, 1, [("levels", p1, p2, H, None, None)], kk, 3.0, seed)
    calls.append(_search(levels, 3407))
    ties = [("straddle",) + tie_pair(False) + (None, None), ("signed_zero",) + tie_pair(True) + (None, None)]
    calls.append(_search(lambda s: _assemble("ties_straddle", 48, 64, 16, 2, ties, 6, 3.0, s), 3408))

    # 240x320, 2500 points a side, keep_k = 2048: at cap 4096 the launch needs 96 KB of LDS; the same data at cap = n
    def big(seed, cap):
        rng = np.random.default_rng(seed)
        H = _perspective(rng, 240, 320)
        p1, p2 = _random_pair(rng, 240, 320, 2500, 2500, H, 1.0)
        return _assemble("k2048_cap%d" % cap, 240, 320, cap, 1, [("n2500", p1, p2, H, None, None)], 2048, 1.0, seed)
    b4096 = _search(lambda s: big(s, 4096), 3409)
    calls.append(b4096)
    calls.append(_search(lambda s: big(b4096["seed"], 2500), 3409))

    # three integer-coordinate pairs whose distances and sums are exact in every order: the streamed round compares bit for bit
    exact = [("threshold",) + threshold_pair() + (None, None)] + ties
    calls.append(_search(lambda s: _assemble("stream_48x64", 48, 64, 16, 2, exact, 6, 3.0, s), 3410))
    assert tuple(c["name"] for c in calls) == REPEAT_NAMES
    return calls


REPEAT_NAMES = ("counts_12x16_stride2", "counts_37x53_stride3", "thresh_3", "thresh_3_below", "thresh_5", "thresh_5_below", "thresh_0",
                "geometry_12x16", "horizon_48x64", "keepk_7", "keepk_1", "keepk_19", "keepk_20", "keepk_21", "keepk_26", "keepk_1000",
                "ties_3levels", "ties_straddle", "k2048_cap4096", "k2048_cap2500", "stream_48x64")


def repeat_call(name):
    return repeat_calls()[REPEAT_NAMES.index(name)]


# ---- RANSAC ----
def _matches(rng, n, outliers, sigma):
    H = np.array([[1 + rng.uniform(-.1, .1), rng.uniform(-.1, .1), rng.uniform(-20, 20)],
                  [rng.uniform(-.1, .1), 1 + rng.uniform(-.1, .1), rng.uniform(-20, 20)],
                  [rng.uniform(-3e-4, 3e-4), rng.uniform(-3e-4, 3e-4), 1.0]])
    p = np.stack([rng.uniform(0, 320, n), rng.uniform(0, 240, n)], 1)
    u, v = R.warp(H, p[:, 0], p[:, 1])
    q = np.stack([u, v], 1) + rng.normal(0, 1, (n, 2)) * sigma
    out = np.zeros(n, bool)
    out[rng.permutation(n)[:int(round(outliers * n))]] = True
    q[out] = q[out] + rng.uniform(25, 80, (int(out.sum()), 2)) * rng.choice([-1, 1], (int(out.sum()), 2))
    return np.concatenate([p, q], 1), out


# name: (seed, n, outlier fraction, noise sigma, kind of the match distances)
RANSAC_SPECS = {
    "n5_clean": (4101, 5, 0.0, 0.0, "uniform"), "n5_noise": (4102, 5, 0.0, 0.5, "uniform"),
    "n6_clean": (4103, 6, 0.0, 0.0, "uniform"), "n6_out": (4104, 6, 0.3, 0.5, "uniform"),
    "n8_clean": (4105, 8, 0.0, 0.0, "uniform"), "n8_out": (4106, 8, 0.3, 0.0, "uniform"), "n8_out_noise": (4107, 8, 0.3, 0.5, "uniform"),
    "n255_clean": (4108, 255, 0.0, 0.0, "uniform"), "n255_out_noise": (4109, 255, 0.3, 0.5, "uniform"),
    "n256_out": (4110, 256, 0.3, 0.0, "uniform"), "n256_out60_noise": (4111, 256, 0.6, 0.5, "uniform"),
    "n257_noise": (4112, 257, 0.0, 0.5, "uniform"), "n257_out60": (4113, 257, 0.6, 0.0, "uniform"),
    "n4096_out_noise": (4114, 4096, 0.3, 0.5, "uniform"), "n4096_out60": (4115, 4096, 0.6, 0.0, "uniform"),
    "caps_n300": (4116, 300, 0.3, 0.5, "uniform"),
    "over_cap": (4117, 64, 0.3, 0.5, "uniform"),       # launched with n_match = 101 at cap 64
    "n40": (4118, 40, 0.3, 0.5, "uniform"),
    "n4": (4119, 4, 0.0, 0.0, "uniform"), "n3": (4120, 3, 0.0, 0.0, "uniform"), "n0": (4121, 0, 0.0, 0.0, "uniform"),
    "ap_3levels": (4122, 60, 0.4, 0.5, "levels"), "ap_all_inliers": (4123, 40, 0.0, 0.5, "uniform"),
    "ap_outliers_first": (4124, 50, 0.4, 0.0, "outliers_first"),
}
CAPS = (None, 1771, 1772, 2048, 3321, 3322, 4096)   # None: cap = n
BATCH = ("n0", "n3", "n4", "n5_noise", "n40", "n257_noise", "caps_n300", "n8_out")
FAMILIES = (("n<=8", 8), ("n~256", 400), ("n=4096", 4096))


def family_of(n):
    return next(name for name, top in FAMILIES if n <= top)


def _distances(rng, kind, n, out):
    if kind == "levels":
        return np.array([0.3, 0.6, 0.9], np.float32)[rng.integers(0, 3, n)]
    d = rng.uniform(0.1, 1.0, n).astype(np.float32)
    if kind == "outliers_first":
        d = np.where(out, 0.05 + 0.2 * d, 0.5 + 0.5 * d).astype(np.float32)
    return d


def residual_gap(ref, m):
    """The least |residual^2 - 9| of any match under the winner, the refit and the refit in lane order."""
    Hs = np.stack([ref[k].reshape(9) for k in ("H_best", "H", "H_lanes")])
    return float(np.abs(ER.resid2(Hs, m) - 9.0).min())


@functools.lru_cache(maxsize=None)
def ransac_problem(name):
    """-> dict(name, m, seed, dist, outliers, ref = ER.ransac's result, gap = residual_gap), redrawn until decided."""
    seed, n, frac, sigma, kind = RANSAC_SPECS[name]
    for k in range(64):
        s = seed + 1000 * k
        rng = np.random.default_rng(s)
        m, out = _matches(rng, n, frac, sigma) if n else (np.zeros((0, 4)), np.zeros(0, bool))
        dist = _distances(rng, kind, n, out)
        ref = ER.ransac(m, s, scores=dist)
        if n < 4:
            return dict(name=name, m=m, seed=s, dist=dist, outliers=out, ref=ref, gap=np.inf)
        if ref["status"] != 0:
            continue
        gap = residual_gap(ref, m)
        if gap >= RESID_BAND:
            return dict(name=name, m=m, seed=s, dist=dist, outliers=out, ref=ref, gap=gap)
    raise AssertionError("no decided draw within 64 seeds: " + name)


def ransac_call(names, cap=None, pair_stride=1, n_match=None, seed=0):
    """The device inputs of one launch over the named problems: pts1 / pts2 [P * stride, cap, 3] whose used entries hold
    the matched points under a random permutation of the rows (match row k = (i_k, j_k, dist_k)), decoy entries and unused rows
    hold random points, match rows past n hold valid indices and a distance of 0 (an AP that read them would move).
    n_match: overrides the counts (a count above cap)."""
    probs = [ransac_problem(n) for n in names]
    P = len(probs)
    cap = cap or max(1, max(p["m"].shape[0] for p in probs))
    rng = np.random.default_rng(9000 + seed)
    pts1, pts2 = rng.uniform(0, 300, (P * pair_stride, cap, 3)), rng.uniform(0, 300, (P * pair_stride, cap, 3))
    match = np.zeros((P, cap, 3), np.float32)
    match[:, :, :2] = rng.integers(0, cap, (P, cap, 2))
    nm = np.zeros(P, np.int32)
    for p, pr in enumerate(probs):
        n = pr["m"].shape[0]
        i, j = rng.permutation(cap)[:n], rng.permutation(cap)[:n]
        pts1[p * pair_stride, i, :2], pts2[p * pair_stride, j, :2] = pr["m"][:, :2], pr["m"][:, 2:]
        match[p, :n, 0], match[p, :n, 1], match[p, :n, 2] = i, j, pr["dist"]
        nm[p] = n
    if n_match is not None:
        nm[:] = n_match
    return dict(pts1=pts1, pts2=pts2, match=match, n_match=nm, seeds=np.array([p["seed"] for p in probs], np.int64), cap=cap,
                pair_stride=pair_stride, problems=probs)
