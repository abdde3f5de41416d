"""numpy restatement of the two kernels of the streamed descriptor metrics (csrc/eval_kernels.hip.h, DESIGN.md section
21) with explicit scalar operations: every product and every sum below is one rounded fp64 operation, in the kernels'
order, so the device results can be compared bit for bit."""
import numpy as np

ROW_WORDS = 16
STATE_WORDS = 16
THRESHOLDS = (1, 3, 5, 10, 20, 50)
F = np.float64


def mat3(a, b):
    """3x3 row-major product, every element ((a0*b0 + a1*b1) + a2*b2)."""
    c = np.zeros(9, F)
    for r in range(3):
        for k in range(3):
            c[3 * r + k] = (a[3 * r] * b[k] + a[3 * r + 1] * b[3 + k]) + a[3 * r + 2] * b[6 + k]
    return c


def pixel_homography(hn, height, width):
    """float32 normalised matrix [3,3] -> (M, inv M) float64 [3,3]: M = Tinv @ (Hn @ T), inv = adj(M) / det(M)."""
    W, H = F(width), F(height)
    T = np.array([F(2.0) / W, 0, -1, 0, F(2.0) / H, -1, 0, 0, 1], F)
    Ti = np.array([W * F(0.5), 0, W * F(0.5), 0, H * F(0.5), H * F(0.5), 0, 0, 1], F)
    h = np.asarray(hn, np.float32).astype(F).reshape(9)
    m = mat3(Ti, mat3(h, T))
    a = np.array([m[4] * m[8] - m[5] * m[7], m[2] * m[7] - m[1] * m[8], m[1] * m[5] - m[2] * m[4],
                  m[5] * m[6] - m[3] * m[8], m[0] * m[8] - m[2] * m[6], m[2] * m[3] - m[0] * m[5],
                  m[3] * m[7] - m[4] * m[6], m[1] * m[6] - m[0] * m[7], m[0] * m[4] - m[1] * m[3]], F)
    det = (m[0] * a[0] + m[1] * a[3]) + m[2] * a[6]
    with np.errstate(divide="ignore", invalid="ignore"):
        return m.reshape(3, 3), (a / det).reshape(3, 3)


def pixel_homographies(hn, height, width):
    out = [pixel_homography(h, height, width) for h in np.asarray(hn).reshape(-1, 3, 3)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def warp(M, x, y):
    M = np.asarray(M, F).reshape(9)
    x, y = F(x), F(y)
    w0 = (x * M[0] + y * M[1]) + M[2]
    w1 = (x * M[3] + y * M[4]) + M[5]
    w2 = (x * M[6] + y * M[7]) + M[8]
    with np.errstate(divide="ignore", invalid="ignore"):
        return w0 / w2, w1 / w2


def corner_distance(H, G, corner_h, corner_w):
    d = []
    for x, y in ((0, 0), (0, corner_h - 1), (corner_w - 1, 0), (corner_w - 1, corner_h - 1)):
        eu, ev = warp(H, x, y)
        gu, gv = warp(G, x, y)
        dx, dy = gu - eu, gv - ev
        d.append(np.sqrt(dx * dx + dy * dy))
    return (((d[0] + d[1]) + d[2]) + d[3]) / F(4.0)


def pair_row(number, rep=None, H=None, n_inl=None, status=None, ap=None, n1=None, hom=None, corner_shape=(240, 320),
             thresholds=THRESHOLDS):
    """The row of one pair.  rep: the 8 values of ssp_eval_repeatability or None; H .. hom: the RANSAC group or None."""
    r = np.zeros(ROW_WORDS, F)
    n_unw = F(0.0)
    if rep is not None:
        q = np.asarray(rep, F)
        c = int(q[2]) + int(q[3])
        if c == 0:
            r[1] = -1.0
        else:
            cd = F(c)
            r[0] = cd / F(int(q[0]) + int(q[1]))
            r[1] = (F(0.0) + q[4] / cd) + q[5] / cd
        n_unw = q[6]
    if H is not None:
        mean = F(np.inf)
        if int(status) == 0:
            mean = corner_distance(H, hom, corner_shape[0], corner_shape[1])
            for k, t in enumerate(thresholds):
                r[2 + k] = 1.0 if mean <= F(t) else 0.0
        den = F(int(n1) + int(n_unw))
        r[8] = F(2 * int(n_inl)) / den if den > 0 else 0.0
        r[9] = ap if ap > 0 else 0.0
        r[10], r[11], r[12], r[13], r[14] = status, n_inl, n1, n_unw, mean
    r[15] = number
    return r


def accumulate_rows(new_rows, rows, state, capacity=None):
    """Adds the rows of one call (their numbers in slot 15) into `state` in order and stores them in `rows`; both are
    updated in place.  One rounded addition per row and sum, as lane 0 of the kernel."""
    capacity = rows.shape[0] if capacity is None else capacity
    for r in new_rows:
        f = int(r[15])
        if f < capacity:
            rows[f] = r
        state[0] = state[0] + F(1.0)
        state[1] = state[1] + r[0]
        if r[1] > 0:
            state[2] = state[2] + r[1]
            state[3] = state[3] + F(1.0)
        for k in range(6):
            state[4 + k] = state[4 + k] + r[2 + k]
        state[10] = state[10] + r[8]
        state[11] = state[11] + r[9]
        if r[10] != 0:
            state[12] = state[12] + F(1.0)
        if f >= capacity:
            state[13] = state[13] + F(1.0)


def accumulate(first_pair, rows, state, rep=None, ransac=None, corner_shape=(240, 320), thresholds=THRESHOLDS):
    """ssp_eval_accumulate for one call.  rep: [P,8] or None; ransac: dict of arrays H [P,3,3], n_inliers, status, ap, n1
    (already strided: one per pair), hom [P,3,3], or None."""
    P = len(rep) if rep is not None else len(ransac["ap"])
    new = []
    for p in range(P):
        kw = {}
        if ransac is not None:
            kw = dict(H=ransac["H"][p], n_inl=ransac["n_inliers"][p], status=ransac["status"][p], ap=ransac["ap"][p],
                      n1=ransac["n1"][p], hom=ransac["hom"][p])
        new.append(pair_row(first_pair + p, rep=None if rep is None else rep[p], corner_shape=corner_shape,
                            thresholds=thresholds, **kw))
    accumulate_rows(new, rows, state)
    return np.stack(new)


def summary(state):
    """The means StreamingEvaluator.result() forms from a state block."""
    s = np.asarray(state, F)
    return {"pairs": int(s[0]), "repeatability": s[1] / s[0] if s[0] > 0 else F(0.0),
            "localization_err": s[2] / s[3] if s[3] > 0 else F("nan"), "loc_pairs": int(s[3]),
            "correctness": s[4:10] / s[0], "mscore": s[10] / s[0], "mAP": s[11] / s[0], "no_model": int(s[12]),
            "rows_dropped": int(s[13])}
