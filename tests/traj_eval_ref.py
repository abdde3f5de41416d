"""numpy restatement of the trajectory evaluation (csrc/traj_eval_kernels.hip.h): the validity of a frame,
the alignment (Umeyama from two passes of moments with the rotation from Jacobi sweeps on H^T H, or the first valid frame's pose),
the absolute and the relative pose errors, the KITTI devkit's segments and the statistics.  There is no evaluator installed here, so
this file is the specification the kernels are tested against; tests/test_traj_eval_cpu.py holds it against the textbook SVD form.
Everything is fp64 in the parenthesisation written here and every sum runs in the kernels' order: thread t of 256 takes the rows
t, t + 256, ..., then the xor butterfly of a wave from offset 32 down to 1, then the four waves in order (`block_sums`).  Every
function also runs in a second "way" (`WAY2`: numpy.longdouble), which is how the tolerance of the floating outputs is measured."""
import numpy as np

from tests import pose_ref

THREADS = 256
ROW_WORDS, GT_WORDS, SIM_WORDS, STATS_WORDS, INFO_WORDS = 16, 12, 16, 8, 4
FLAG_NO_POSE = 1
OK, FEW, COLLINEAR = 0, 1, 2
COLLINEAR_EPS = 1e-24
MODES = {"se3": 0, "sim3": 1, "origin": 2, "origin_scale": 3}
KITTI_LENGTHS = (100.0, 200.0, 300.0, 400.0, 500.0, 600.0, 700.0, 800.0)
WAY1 = np.float64
WAY2 = np.longdouble


def _dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def _mv(a, v):
    """a @ v for [..., 3, 3] and [..., 3]: every element (a0*v0 + a1*v1) + a2*v2"""
    return (a[..., :, 0] * v[..., None, 0] + a[..., :, 1] * v[..., None, 1]) + a[..., :, 2] * v[..., None, 2]


def _mm(a, b):
    """a @ b for [..., 3, 3]: mat3_mul"""
    return (a[..., :, 0, None] * b[..., None, 0, :] + a[..., :, 1, None] * b[..., None, 1, :]) + a[..., :, 2, None] * b[..., None, 2, :]


def _T(a):
    return np.swapaxes(a, -1, -2)


def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], dtype=a.dtype)


def block_sums(rows, dt=WAY1):
    """The kernels' sum of rows [n, N] (row r is thread r % 256's; a row of zeros for an item the kernel skips) -> [N]"""
    rows = np.asarray(rows, dtype=dt)
    n, N = rows.shape
    k = -(-max(n, 1) // THREADS)
    pad = np.zeros((k * THREADS, N), dtype=dt)
    pad[:n] = rows
    pad = pad.reshape(k, THREADS, N)
    acc = np.zeros((THREADS, N), dtype=dt)
    for j in range(k):
        acc = acc + pad[j]
    v = acc.reshape(THREADS // 64, 64, N)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lane ^ o]
    t = v[0, 0]
    for w in range(1, THREADS // 64):
        t = t + v[w, 0]
    return t


PI, PI_LO, PI_2 = 3.1415926535897931160e+00, 1.2246467991473531772e-16, 1.5707963267948966
ATAN_HI = (4.63647609000806093515e-01, 7.85398163397448278999e-01, 9.82793723247329054082e-01, 1.57079632679489655800e+00)
ATAN_LO = (2.26987774529616870924e-17, 3.06161699786838301793e-17, 1.39033110312309984516e-17, 6.12323399573676603587e-17)
ATAN_ODD = (3.33333333333329318027e-01, 1.42857142725034663711e-01, 9.09088713343650656196e-02, 6.66107313738753120669e-02,
            4.97687799461593236017e-02, 1.62858201153657823623e-02)
ATAN_EVEN = (-1.99999999998764832476e-01, -1.11111104054623557880e-01, -7.69187620504482999495e-02, -5.83357013379057348645e-02,
             -3.65315727442169155270e-02)


def atan_pos(t):
    """traj_atan_pos: atan(t) for t >= 0 in float64 operations written out (the reduction and the polynomial of fdlibm's s_atan.c)"""
    t = np.asarray(t, np.float64)
    with np.errstate(all="ignore"):
        band = (t >= 0.4375).astype(int) + (t >= 0.6875) + (t >= 1.1875) + (t >= 2.4375)   # 0: no reduction
        x = np.select([band == 4, band == 3, band == 2, band == 1], [-1.0 / t, (t - 1.5) / (1.0 + 1.5 * t), (t - 1.0) / (t + 1.0),
                                                                     (2.0 * t - 1.0) / (2.0 + t)], t)
        hi = np.select([band == k + 1 for k in range(4)], ATAN_HI, 0.0)
        lo = np.select([band == k + 1 for k in range(4)], ATAN_LO, 0.0)
        z = x * x
        w = z * z
        o, e = ATAN_ODD, ATAN_EVEN
        s1 = z * (o[0] + w * (o[1] + w * (o[2] + w * (o[3] + w * (o[4] + w * o[5])))))
        s2 = w * (e[0] + w * (e[1] + w * (e[2] + w * (e[3] + w * e[4]))))
        r = np.where(band == 0, x - x * (s1 + s2), hi - ((x * (s1 + s2) - lo) - x))
        r = np.where(t < 1.862645149230957e-09, t, r)
        return np.where(t >= 73786976294838206464.0, PI_2, r)


def atan2_pos(y, x):
    """traj_atan2_pos: atan2(y, x) for y >= 0"""
    y, x = np.asarray(y, np.float64), np.asarray(x, np.float64)
    with np.errstate(all="ignore"):
        z = atan_pos(y / np.abs(x))
        r = np.where(x > 0.0, z, PI - (z - PI_LO))
        r = np.where(x == 0.0, PI_2, r)
        return np.where(y == 0.0, np.where(x < 0.0, PI, 0.0), r)


def angle(E):
    """The angle of the rotations E [..., 3, 3] in radians.  float64: the written-out atan2 of the kernels; the second way: numpy's"""
    dt = E.dtype.type
    a, b, c = E[..., 2, 1] - E[..., 1, 2], E[..., 0, 2] - E[..., 2, 0], E[..., 1, 0] - E[..., 0, 1]
    sn = dt(0.5) * np.sqrt((a * a + b * b) + c * c)
    cs = dt(0.5) * (((E[..., 0, 0] + E[..., 1, 1]) + E[..., 2, 2]) - dt(1.0))
    return atan2_pos(sn, cs) if dt is np.float64 else np.arctan2(sn, cs)


def _deg(dt):
    return dt(57.29577951308232) if dt is np.float64 else dt(180.0) / dt(np.pi)


def frames(table, n_frames, gt, index=None, skip_flags=FLAG_NO_POSE):
    """(valid bool [capacity], g int [capacity]: the ground-truth row or -1) of one problem"""
    table, gt = np.asarray(table, np.float64), np.asarray(gt, np.float64)
    cap, n_gt = table.shape[0], gt.shape[0]
    nf = min(max(int(n_frames), 0), cap)
    g = np.arange(cap) if index is None else np.asarray(index).astype(np.int64)
    g = np.where((g >= 0) & (g < n_gt) & (np.arange(cap) < nf), g, -1)
    fl = table[:, 14]
    with np.errstate(invalid="ignore"):
        flag_ok = (fl >= 0.0) & (fl < 2147483648.0) & (fl == np.floor(fl))
        ints = np.where(flag_ok, fl, 0.0).astype(np.int64)
    flag_ok = flag_ok & ((ints & int(skip_flags)) == 0)
    fin = np.isfinite(table[:, :12]).all(axis=1) & np.isfinite(gt[np.maximum(g, 0)]).all(axis=1)
    return (g >= 0) & flag_ok & fin, g


def _unpack(table, gt, g, dt):
    """Rw [cap, 3, 3], C [cap, 3] of the estimate; Rg [cap, 3, 3], q [cap, 3] of the truth per frame (row 0 where there is none)"""
    table = np.asarray(table, np.float64).astype(dt)
    G = np.asarray(gt, np.float64).astype(dt)[np.maximum(g, 0)].reshape(-1, 3, 4)
    return table[:, :9].reshape(-1, 3, 3), table[:, 9:12], G[:, :, :3], G[:, :, 3]


def _zero_invalid(x, valid):
    """x with the rows of invalid frames at zero (no NaN of a skipped row reaches a sum)"""
    return np.where(valid.reshape((-1,) + (1,) * (x.ndim - 1)), x, x.dtype.type(0.0))


def align(table, n_frames, gt, index=None, mode="sim3", skip_flags=FLAG_NO_POSE, way=WAY1, margin=None):
    """sim [16] = (s, R [9], t [3], n_valid, status, sigma_p^2) in the way's number format.  margin: a list that receives the relative
    distance of the collinearity decision from its threshold."""
    dt, m = way, MODES[mode]
    valid, g = frames(table, n_frames, gt, index, skip_flags)
    Rw, C, Rg, q = _unpack(table, gt, g, dt)
    C, q = _zero_invalid(C, valid), _zero_invalid(q, valid)
    one = valid.astype(dt)[:, None]
    sim = np.zeros(SIM_WORDS, dtype=dt)
    ident = lambda nv, status, sig=dt(0.0): np.concatenate([[dt(1.0)], np.eye(3, dtype=dt).ravel(), np.zeros(3, dt), [nv, dt(status), sig]])
    with np.errstate(all="ignore"):
        if m <= 1:
            a = block_sums(np.concatenate([one, C, q], axis=1), dt)
            nv = a[0]
            mp, mq = a[1:4] / nv, a[4:7] / nv
            dp, dq = _zero_invalid(C - mp, valid), _zero_invalid(q - mq, valid)
            H = (dq[:, :, None] * dp[:, None, :]).reshape(-1, 9)
            b = block_sums(np.concatenate([H, _dot(dp, dp)[:, None], _dot(dq, dq)[:, None]], axis=1), dt)
            fin = bool(np.isfinite(b).all() and np.isfinite(mp).all() and np.isfinite(mq).all())
            if nv < 3 or not fin or not b[9] > 0.0:
                return ident(nv, FEW)
            sig = b[9] / nv
            H = b[:9].reshape(3, 3)
            G = np.array([[_dot(H[:, i], H[:, j]) for j in range(3)] for i in range(3)], dtype=dt)
            d, V = pose_ref.jacobi3(G, dt)
            k0 = 2 if d[2] > max(d[1], d[0]) else (1 if d[1] > d[0] else 0)
            ra, rb = (1 if k0 == 0 else 0), (1 if k0 == 2 else 2)
            k1 = rb if d[rb] > d[ra] else ra
            if margin is not None and d[k0] > 0:
                margin.append(float(abs(d[k1] / d[k0] - dt(COLLINEAR_EPS)) / max(d[k1] / d[k0], dt(COLLINEAR_EPS))))
            if not d[k1] > dt(COLLINEAR_EPS) * d[k0]:
                return ident(nv, COLLINEAR, sig)
            v0, v1 = V[:, k0].copy(), V[:, k1].copy()
            v2 = _cross(v0, v1)
            h0, h1 = _mv(H, v0), _mv(H, v1)
            u0 = h0 / np.sqrt(_dot(h0, h0))
            w = h1 - _dot(h1, u0) * u0
            u1 = w / np.sqrt(_dot(w, w))
            u2 = _cross(u0, u1)
            U, Vt = np.stack([u0, u1, u2], axis=1), np.stack([v0, v1, v2], axis=0)
            R = _mm(U, Vt)
            tr = _dot(R, H)
            s = ((tr[0] + tr[1]) + tr[2]) / b[9] if m == 1 else dt(1.0)
            t = mq - s * _mv(R, mp)
        else:
            nv = block_sums(one, dt)[0]
            if nv < (2 if m == 3 else 1):
                return ident(nv, FEW)
            f0 = int(np.flatnonzero(valid)[0])
            R = _mm(Rg[f0], Rw[f0])
            s, sig = dt(1.0), dt(0.0)
            if m == 3:
                r = _zero_invalid(_mv(R, C - C[f0]), valid)
                dq = _zero_invalid(q - q[f0], valid)
                c = block_sums(np.stack([_dot(dq, r), _dot(r, r)], axis=1), dt)
                s, sig = c[0] / c[1], c[1] / nv
            t = q[f0] - s * _mv(R, C[f0])
        if not (np.isfinite(s) and s > 0.0 and np.isfinite(t).all() and np.isfinite(R).all()):
            return ident(nv, FEW)
        sim[0], sim[1:10], sim[10:13], sim[13], sim[14], sim[15] = s, R.ravel(), t, nv, OK, (sig if np.isfinite(sig) else 0.0)
    return sim


def ape(table, n_frames, gt, sim, index=None, skip_flags=FLAG_NO_POSE, way=WAY1):
    """(err_t [capacity], err_r [capacity] in degrees, valid int32 [capacity])"""
    dt = way
    valid, g = frames(table, n_frames, gt, index, skip_flags)
    sim = np.asarray(sim).astype(dt)
    if sim[14] != 0.0:
        valid = np.zeros_like(valid)
    Rw, C, Rg, q = _unpack(table, gt, g, dt)
    s, R, t = sim[0], sim[1:10].reshape(3, 3), sim[10:13]
    with np.errstate(all="ignore"):
        e = q - (s * _mv(R, C) + t)
        et = np.sqrt(_dot(e, e))
        er = angle(_mm(_T(Rg), _mm(R, _T(Rw)))) * _deg(dt)
    return np.where(valid, et, dt(0.0)), np.where(valid, er, dt(0.0)), valid.astype(np.int32)


def rel_error(Rwa, Ca, Rga, qa, Rwb, Cb, Rgb, qb, s):
    """(|trans E|, the angle of rot E in radians) of E = (Pa^-1 Pb)^-1 (Qa^-1 Qb), batched"""
    RgaT = _T(Rga)
    Rq = _mm(RgaT, Rgb)
    dq = qb - qa
    dp = s * (Cb - Ca)
    Rp = _mm(Rwa, _T(Rwb))
    d = _mv(RgaT, dq) - _mv(Rwa, dp)
    RpT = _T(Rp)
    e = _mv(RpT, d)
    return np.sqrt(_dot(e, e)), angle(_mm(RpT, Rq))


def rpe_delta(table, n_frames, gt, index=None, delta=1, scale=1.0, skip_flags=FLAG_NO_POSE, way=WAY1):
    """(err_t [capacity], err_r [capacity] in degrees, valid int32 [capacity]): entry f is the error between f and f + delta"""
    dt = way
    valid, g = frames(table, n_frames, gt, index, skip_flags)
    cap = len(valid)
    Rw, C, Rg, q = _unpack(table, gt, g, dt)
    b = np.minimum(np.arange(cap) + delta, cap - 1)
    both = valid & (np.arange(cap) + delta < cap) & valid[b]
    with np.errstate(all="ignore"):
        et, ang = rel_error(Rw, C, Rg, q, Rw[b], C[b], Rg[b], q[b], dt(scale))
        er = ang * _deg(dt)
    return np.where(both, et, dt(0.0)), np.where(both, er, dt(0.0)), both.astype(np.int32)


def path_length(n_frames, gt, index, cap, way=WAY1):
    """dist [capacity]: thread t owns the frames [t K, (t + 1) K), K = cdiv(n_frames, 256); its steps in order, the totals of the
    threads before it in order, dist[f] = that base + its own running sum."""
    dt = way
    gt = np.asarray(gt, np.float64)
    n_gt = gt.shape[0]
    nf = min(max(int(n_frames), 0), cap)
    g = np.arange(cap) if index is None else np.asarray(index).astype(np.int64)
    centre = gt.astype(dt).reshape(-1, 3, 4)[:, :, 3]
    has = (g >= 0) & (g < n_gt)
    has = has & np.isfinite(gt.reshape(-1, 3, 4)[:, :, 3][np.where(has, g, 0)]).all(axis=1)
    K = -(-nf // THREADS)
    dist, part = np.zeros(cap, dtype=dt), np.zeros(THREADS, dtype=dt)
    local = np.zeros(cap, dtype=dt)
    last = None
    for f in range(nf):   # (the last centre before a thread's first frame is the last one seen: one walk serves all threads)
        if f % K == 0:
            run = dt(0.0)
        if has[f]:
            c = centre[g[f]]
            if last is not None:
                d = c - last
                run = run + np.sqrt(_dot(d, d))
            last = c
        local[f] = run
        part[f // K] = run
    base = dt(0.0)
    for t in range(THREADS):
        lo, hi = min(t * K, nf), min(t * K + K, nf)
        dist[lo:hi] = base + local[lo:hi]
        base = base + part[t]
    return dist


def rpe_segments(table, n_frames, gt, index=None, scale=1.0, lengths=KITTI_LENGTHS, step=10, skip_flags=FLAG_NO_POSE, way=WAY1,
                 margin=None):
    """(dist [capacity], seg [n_first, n_len, 4], summary [2 + 3 n_len], info int32 [4]).  margin: a list that receives, per segment
    with an end, the relative distance of dist[f1 - 1] and dist[f1] from dist[f0] + L."""
    dt = way
    valid, g = frames(table, n_frames, gt, index, skip_flags)
    cap = len(valid)
    nf = min(max(int(n_frames), 0), cap)
    Rw, C, Rg, q = _unpack(table, gt, g, dt)
    dist = path_length(n_frames, gt, index, cap, way)
    n_first, n_len = -(-cap // step), len(lengths)
    seg = np.zeros((n_first, n_len, 4), dtype=dt)
    info = np.zeros(INFO_WORDS, dtype=np.int32)
    with np.errstate(all="ignore"):
        for k in range(n_first):
            f0 = k * step
            for l, L in enumerate(lengths):
                L = dt(L)
                seg[k, l, 0] = -1.0
                if f0 >= nf:
                    continue
                target = dist[f0] + L
                lo = f0 + 1 + int(np.searchsorted(dist[f0 + 1:nf], target, side="right"))
                if lo >= nf:
                    info[2] += 1
                    continue
                seg[k, l, 0] = lo
                if margin is not None:
                    margin.append(float(min(dist[lo] - target, target - dist[lo - 1]) / target))
                if valid[f0] and valid[lo]:
                    et, ang = rel_error(Rw[f0], C[f0], Rg[f0], q[f0], Rw[lo], C[lo], Rg[lo], q[lo], dt(scale))
                    seg[k, l, 1:] = et / L, ang / L, L
                    info[0] += 1
                else:
                    info[1] += 1
    info[3] = -(-nf // step)
    summary = np.zeros(2 + 3 * n_len, dtype=dt)
    tot = np.zeros(3, dtype=dt)
    for l in range(n_len):
        on = seg[:, l, 3] > 0.0
        a = block_sums(np.stack([on.astype(dt), np.where(on, seg[:, l, 1], dt(0.0)), np.where(on, seg[:, l, 2], dt(0.0))], axis=1), dt)
        tot = tot + a
        summary[2 + 3 * l] = a[0]
        if a[0] > 0:
            summary[3 + 3 * l], summary[4 + 3 * l] = a[1] / a[0], a[2] / a[0]
    if tot[0] > 0:
        summary[0], summary[1] = tot[1] / tot[0], tot[2] / tot[0]
    return dist, seg, summary, info


def order_statistics(err, valid):
    """The order statistics (n - 1) // 2 and n // 2 of the valid entries (None, None for n = 0)"""
    x = np.sort(np.asarray(err)[np.asarray(valid) != 0])
    n = len(x)
    return (x[(n - 1) // 2], x[n // 2]) if n else (None, None)


def stats(err, valid, way=WAY1):
    """(n, rmse, mean, std, min, max, median, sse) of the valid entries of err [capacity]"""
    dt = way
    on = np.asarray(valid) != 0
    x = np.where(on, np.asarray(err).astype(dt), dt(0.0))
    a = block_sums(np.stack([on.astype(dt), x, x * x], axis=1), dt)
    out = np.zeros(STATS_WORDS, dtype=dt)
    if a[0] == 0:
        return out
    mean = a[1] / a[0]
    d = np.where(on, x - mean, dt(0.0))
    b = block_sums((d * d)[:, None], dt)
    lo, hi = order_statistics(x, on)
    out[:] = a[0], np.sqrt(a[2] / a[0]), mean, np.sqrt(b[0] / a[0]), x[on].min(), x[on].max(), dt(0.5) * (lo + hi), a[2]
    return out


# ---- the whole evaluation of one table, as TrajectoryEvaluator queues it ----
def evaluate(table, n_frames, gt, index=None, align_mode="sim3", skip_flags=FLAG_NO_POSE, lengths=KITTI_LENGTHS, step=10, deltas=(1,),
             way=WAY1):
    """dict(sim, ape = (err_t, err_r, valid), ate / ape_rot = stats, rpe = {delta: (err_t, err_r, valid, stats_t, stats_r)},
    dist, seg, summary, info)"""
    sim = align(table, n_frames, gt, index, align_mode, skip_flags, way)
    et, er, v = ape(table, n_frames, gt, sim, index, skip_flags, way)
    out = dict(sim=sim, ape=(et, er, v), ate=stats(et, v, way), ape_rot=stats(er, v, way), rpe={})
    for d in deltas:
        rt, rr, rv = rpe_delta(table, n_frames, gt, index, d, sim[0], skip_flags, way)
        out["rpe"][d] = (rt, rr, rv, stats(rt, rv, way), stats(rr, rv, way))
    out["dist"], out["seg"], out["summary"], out["info"] = rpe_segments(table, n_frames, gt, index, sim[0], lengths, step, skip_flags, way)
    return out


# ---- the textbook form, for tests/test_traj_eval_cpu.py ----
def umeyama_svd(p, q, with_scale=True):
    """(s, R, t) of q ~ s R p + t by numpy.linalg.svd with the determinant correction (Umeyama 1991)"""
    p, q = np.asarray(p, np.float64), np.asarray(q, np.float64)
    mp, mq = p.mean(axis=0), q.mean(axis=0)
    dp, dq = p - mp, q - mq
    H = dq.T @ dp / len(p)
    U, D, Vt = np.linalg.svd(H)
    S = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2, 2] = -1.0
    R = U @ S @ Vt
    s = float(np.trace(np.diag(D) @ S) / (dp * dp).sum() * len(p)) if with_scale else 1.0
    return s, R, mq - s * R @ mp
