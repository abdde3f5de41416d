"""Inputs of the G16 evaluation fixtures (tools/make_golden_evaluation.py), regenerated from seeds.

Each case is a synthetic export pair at 240x320 in the layout of export.py's `<n>.npz` (image, warped_image, prob,
warped_prob, desc, warped_desc, homography).  Matches are unique by construction: every linked pair of points shares a
descriptor code (designed, distinct dots in [0.76, 0.99]) and is either an exact inlier (warped by the true homography) or a gross outlier (> 25 px);
unlinked points copy a linked code with heavy noise (dot ~0.7), so they are never a mutual nearest neighbour.  The
recorded homography is the true one followed by a shift of `offset` px, so the corner error of a good estimate is the
offset and each correctness threshold flips for some case."""
import numpy as np

H_IMG, W_IMG = 240, 320

# name, seed, inliers, outliers, unlinked points of the image / of the warped image, offset (px), kind
CASES = [
    ("border", 1601, 40, 10, 12, 12, 0.0, "border"),
    ("translate", 1602, 120, 30, 40, 40, 2.0, "translate"),
    ("persp_a", 1603, 200, 50, 60, 60, 0.0, "persp"),
    ("persp_b", 1604, 150, 150, 50, 50, 4.0, "persp"),
    ("outliers60", 1605, 120, 180, 30, 30, 7.0, "persp"),
    ("topk", 1606, 700, 100, 300, 300, 0.0, "persp"),
    ("persp_c", 1607, 300, 100, 100, 100, 15.0, "persp"),
    ("persp_d", 1608, 250, 60, 80, 80, 30.0, "persp"),
    ("persp_e", 1609, 180, 40, 40, 40, 60.0, "persp"),
    ("few", 1610, 12, 3, 5, 5, 0.5, "persp"),
    ("small_outl", 1611, 90, 60, 200, 200, 1.5, "translate"),
    ("dense", 1612, 500, 300, 200, 100, 0.0, "persp"),
]
EMPTY_CASE = ("empty_side", 1613, 0, 0, 50, 0, 0.0, "persp")  # compute_repeatability only: the reference's evaluate
# crashes on a pair without matches (findHomography returns no mask)

# (label, distance) vectors for average_precision_score, with ties: seed, length, distinct distance levels
AP_CASES = [(1701, 40, 5), (1702, 200, 17), (1703, 100, 100), (1704, 60, 3)]


def _warp(H, p):
    hp = np.concatenate([p, np.ones((p.shape[0], 1))], axis=1)
    w = np.dot(hp, np.transpose(H))
    return w[:, :2] / w[:, 2:]


def _unit(v):
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def true_homography(rng, kind):
    if kind in ("border", "translate"):
        return np.array([[1.0, 0, rng.integers(-6, 7)], [0, 1.0, rng.integers(-6, 7)], [0, 0, 1.0]])
    a, b, c, d = rng.uniform(-0.08, 0.08, 4)
    e, f = rng.uniform(-2e-4, 2e-4, 2)
    return np.array([[1 + a, b, rng.uniform(-12, 12)], [c, 1 + d, rng.uniform(-12, 12)], [e, f, 1.0]])


def case_pair(case):
    """-> (data dict in the npz layout, true homography, link dict with the inlier / outlier index ranges)."""
    name, seed, n_in, n_out, x1, x2, offset, kind = case
    rng = np.random.default_rng(seed)
    H = true_homography(rng, kind)
    integer = kind in ("border", "translate")

    def rand_pts(n, margin=6):
        p = np.stack([rng.uniform(margin, W_IMG - 1 - margin, n), rng.uniform(margin, H_IMG - 1 - margin, n)], 1)
        return np.round(p) if integer else np.round(p * 8) / 8

    p_in = rand_pts(n_in, 16)
    q_in = _warp(H, p_in)
    p_out = rand_pts(n_out)
    q_out = rand_pts(n_out)
    for k in range(n_out):  # gross outliers: > 25 px from the true image
        while np.linalg.norm(q_out[k] - _warp(H, p_out[k:k + 1])[0]) <= 25:
            q_out[k] = rand_pts(1)[0]
    e1, e2 = rand_pts(x1), rand_pts(x2)
    if kind == "border":
        # warped points exactly on the borders (x = 0, W - 1, W; y = 0, H - 1, H) and distances of exactly 3.0
        t = H[:2, 2]
        b2 = np.array([[0, 50], [W_IMG - 1, 60], [W_IMG, 70], [80, 0], [90, H_IMG - 1], [100, H_IMG], [-1, 30]], float)
        b1 = b2 - t
        p_in[:len(b1)] = b1
        q_in = _warp(H, p_in)
        e2[:4] = q_in[10:14] + np.array([[3.0, 0], [0, 3.0], [-3.0, 0], [0, -3.0]])
        e1[:2] = p_in[20:22] + np.array([[0, 3.0], [3.0, 0]])
    p1 = np.concatenate([p_in, p_out, e1])
    p2 = np.concatenate([q_in, q_out, e2])
    n_link = n_in + n_out
    # linked pairs: d2 = c d1 + sqrt(1 - c^2) n with n orthogonal to d1 and distinct designed dots c (spaced apart, so the
    # match distances of all three matchers rank alike); unlinked points: a linked d1 plus heavy noise
    base = _unit(rng.standard_normal((max(n_link, 1), 256))).astype(np.float64)
    nrm = rng.standard_normal((max(n_link, 1), 256))
    nrm = nrm - np.sum(nrm * base, 1, keepdims=True) * base
    nrm = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)
    cdot = (0.76 + 0.23 * (rng.permutation(max(n_link, 1)) + 0.5) / max(n_link, 1))[:, None]
    partner = cdot * base + np.sqrt(1 - cdot ** 2) * nrm
    d1 = np.concatenate([base[:n_link], base[rng.integers(0, max(n_link, 1), x1)] + 1.0 * _unit(rng.standard_normal((x1, 256)))])
    d2 = np.concatenate([partner[:n_link],
                         base[rng.integers(0, max(n_link, 1), x2)] + 1.0 * _unit(rng.standard_normal((x2, 256)))])
    # shuffle each side so that linked rows are not aligned by index
    o1, o2 = rng.permutation(len(p1)), rng.permutation(len(p2))

    def conf(n):
        return (rng.permutation(n) + 1).astype(np.float32) / np.float32(n + 7)

    prob = np.concatenate([p1, conf(len(p1))[:, None]], 1)[o1]
    wprob = np.concatenate([p2, conf(len(p2))[:, None]], 1)[o2]
    shift = np.array([[1.0, 0, offset], [0, 1.0, 0], [0, 0, 1.0]])
    data = {
        "image": np.zeros((H_IMG, W_IMG), np.float32),
        "warped_image": np.zeros((H_IMG, W_IMG), np.float32),
        "prob": prob.astype(np.float64),
        "warped_prob": wprob.astype(np.float64),
        "desc": _unit(d1.reshape(-1, 256))[o1] if len(p1) else np.zeros((0, 256), np.float32),
        "warped_desc": _unit(d2.reshape(-1, 256))[o2] if len(p2) else np.zeros((0, 256), np.float32),
        "homography": shift @ H,
    }
    return data, H


def ap_case(seed, n, levels):
    """(labels bool [n], distances float32 [n]) with tied distances."""
    rng = np.random.default_rng(seed)
    lv = np.sort(rng.uniform(0.05, 1.1, levels)).astype(np.float32)
    d = lv[rng.integers(0, levels, n)]
    labels = rng.uniform(size=n) < np.interp(d, [0.05, 1.1], [0.9, 0.2])
    labels[0] = True
    return labels, d


def ap_matches(labels, seed):
    """Matches whose RANSAC inlier set is `labels`: exact inliers of a mild homography and gross outliers."""
    rng = np.random.default_rng(seed)
    H = true_homography(rng, "persp")
    n = labels.size
    p = np.stack([rng.uniform(20, 300, n), rng.uniform(20, 220, n)], 1)
    q = _warp(H, p)
    for k in np.nonzero(~labels)[0]:
        q[k] = q[k] + rng.uniform(30, 60, 2) * rng.choice([-1, 1], 2)
    return p, q, H
