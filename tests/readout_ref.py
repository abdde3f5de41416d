"""Plain restatement of the read-out kernels (csrc/export_kernels.hip.h, csrc/describe_kernels.hip.h) in numpy fp64: no torch, nothing
imported from the product.  Written from the reference's formulas:

  views / masks     datasets/Coco.py:258-292, utils/utils.py:347-385, 715-742   bilinear warp (zeros padding, align_corners=True) of one
                                                                              image under n matrices; nearest warp of ones
  flatten           utils/utils.py:515-560, utils/d2s.py:8-27, export.py:51    softmax over 65 channels, dustbin dropped, channel c ->
                                                                              pixel (c // 8, c % 8) of the cell, times the valid mask
  combine           export.py:49-60                                            bilinear un-warp of heat * mask and of mask, summed over the
                                                                              views, divided; 0 / 0 stays NaN
  soft_argmax5      models/model_wrap.py:212-249, utils/losses.py:53-91,138-142, torchgeometry contrib.SpatialSoftArgmax2d
  sample_desc       models/model_wrap.py:295-313                               grid_sample(bilinear, zeros, align_corners=True) at
                                                                              pts / (W / 2) - 1, divided by the L2 norm
  match_two_way     models/model_wrap.py:451-497                               sqrt(2 - 2 clip(D1^T D2)), mutual arg-min, strict threshold

Every stage returns its value and a per-element `base`: the quantity the fp32 roundings of the stage scale with, so that
|device - value| <= tau * base is a scale-free statement (tests/test_gpu_readout_exact.py).  Where a stage interpolates, the corner
weights carry the fp32 error of the COORDINATE, which is absolute (a fraction of a pixel) and not relative to a small weight: the base takes
every corner value with weight 1.  The image warp keeps the rule of the pair feed (tests/pairs_ref.py): 2 e_ref + 2^-23."""
import numpy as np

from tests import pairs_ref as P

F32 = np.float32
EPS = 2.0 ** -24


# ------------------------------------------------------------------------------------------------ bilinear taps, zeros padding
def bilinear_taps(plane, ix, iy):
    """The four corner values (nw, ne, sw, se) [4, ...] of `plane` [H, W] at unnormalised coordinates (ix, iy), their weights and
    `beyond` (all four corners in the zero padding, non-finite coordinates included)."""
    plane = np.asarray(plane, np.float64)
    H, W = plane.shape
    fin = np.isfinite(ix) & np.isfinite(iy)
    ix, iy = np.where(fin, ix, -9.0), np.where(fin, iy, -9.0)
    x0, y0 = np.floor(ix), np.floor(iy)
    ax, ay = ix - x0, iy - y0
    pad = np.zeros((H + 2, W + 2))
    pad[1:-1, 1:-1] = plane
    beyond = (x0 < -1) | (x0 > W - 1) | (y0 < -1) | (y0 > H - 1)
    xs = np.clip(x0, -1, W - 1).astype(np.int64) + 1
    ys = np.clip(y0, -1, H - 1).astype(np.int64) + 1
    vals = np.stack([pad[ys, xs], pad[ys, xs + 1], pad[ys + 1, xs], pad[ys + 1, xs + 1]])
    vals[:, beyond] = 0.0
    wts = np.stack([(1 - ax) * (1 - ay), ax * (1 - ay), (1 - ax) * ay, ax * ay])
    return vals, wts, beyond


def coord_error_bound(inv_h, H, W):
    """A-priori bound [H, W] on the distance between ANY fp32 evaluation of the source coordinates and the fp64 one, first order in
    2^-24: the grid carries 2 eps, a row of the 3x3 product 6 eps (|h0| + |h1| + |h2|), the division adds (d_sx + |u| d_sw) / |sw|,
    the unnormalisation 2 eps.  Doubled.  It grows without limit towards a horizon (sw -> 0), which is what it is for."""
    h = np.abs(np.asarray(inv_h, np.float64).reshape(3, 3))
    ix, iy, sw = P.source_coords64(inv_h, H, W)
    t = 6 * EPS * h.sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        u, v = 2 * ix / (W - 1) - 1, 2 * iy / (H - 1) - 1
        du = (t[0] + np.abs(u) * t[2]) / np.abs(sw) + EPS * np.abs(u)
        dv = (t[1] + np.abs(v) * t[2]) / np.abs(sw) + EPS * np.abs(v)
        dx = (du + 2 * EPS * (np.abs(u) + 1)) * (W - 1) / 2 + EPS * np.abs(ix)
        dy = (dv + 2 * EPS * (np.abs(v) + 1)) * (H - 1) / 2 + EPS * np.abs(iy)
    return 2 * np.maximum(dx, dy)


def tie_distance(inv_h, H, W):
    """distance [H, W] of the fp64 source coordinate from the nearest rounding tie (k + 1/2), the smaller of x and y"""
    ix, iy, _ = P.source_coords64(inv_h, H, W)
    with np.errstate(invalid="ignore"):
        return np.minimum(np.abs(ix - np.floor(ix) - 0.5), np.abs(iy - np.floor(iy) - 0.5))


# ------------------------------------------------------------------------------------------------ views and masks
def views_and_masks(img, inv_h):
    """img [H, W], inv_h [n, 3, 3] -> dict: views [n, H, W] (fp64), base (the same sum on absolute values), beyond (all four taps in the
    padding), masks (nearest warp of ones, half to even), ix, iy, sw (source coordinates), tie (distance from a rounding tie)."""
    img = np.asarray(img, np.float64)
    H, W = img.shape
    out = {k: [] for k in ("views", "base", "beyond", "masks", "ix", "iy", "sw", "tie")}
    for m in np.asarray(inv_h):
        with np.errstate(divide="ignore", invalid="ignore"):
            ix, iy, sw = P.source_coords64(m, H, W)
            vals, wts, beyond = bilinear_taps(img, ix, iy)
            rx, ry = np.rint(ix), np.rint(iy)
            out["masks"].append(((rx >= 0) & (rx <= W - 1) & (ry >= 0) & (ry <= H - 1)).astype(np.float64))
        out["views"].append((vals * wts).sum(0))
        out["base"].append((np.abs(vals) * wts).sum(0))
        out["beyond"].append(beyond)
        out["ix"].append(ix), out["iy"].append(iy), out["sw"].append(sw)
        out["tie"].append(tie_distance(m, H, W))
    return {k: np.stack(v) for k, v in out.items()}


# ------------------------------------------------------------------------------------------------ flatten
def depth_to_space(x):
    """[n, 64, Hc, Wc] -> [n, 8 Hc, 8 Wc]: channel c of cell (hc, wc) -> pixel (8 hc + c // 8, 8 wc + c % 8)"""
    n, _, Hc, Wc = x.shape
    return x.reshape(n, 8, 8, Hc, Wc).transpose(0, 3, 1, 4, 2).reshape(n, 8 * Hc, 8 * Wc)


def flatten(semi, mask=None, mag=None):
    """semi [n, 65, Hc, Wc] -> (heat [n, 8 Hc, 8 Wc], base).  mag: the magnitude the logits were formed at where they are the result of
    an affine y * scale + shift (|y * scale| + |shift|, [n, 65, Hc, Wc]); default |semi|.  Every term of a softmax is positive, so the expression on absolute values
    is the probability itself; the exponent's operand l - max is rounded in proportion to the logits, an absolute error of the
    operand and so a relative one of p: base = p (1 + max |l| of the cell).  A probability below the smallest normal fp32 number
    (2^-126) may be flushed to zero: the base carries that absolute step as 2^-102 (no tau is below 2^-24)."""
    l = np.asarray(semi, np.float64)
    e = np.exp(l - l.max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True)
    mag = np.abs(l) if mag is None else np.asarray(mag, np.float64)
    base = p * (1.0 + mag.max(axis=1, keepdims=True)) + 2.0 ** -102
    heat, base = depth_to_space(p[:, :64]), depth_to_space(base[:, :64])
    if mask is not None:
        m = np.asarray(mask, np.float64).reshape(heat.shape)
        heat, base = heat * m, base * np.abs(m)
    return heat, base


# ------------------------------------------------------------------------------------------------ combine
def combine(heat_masked, mask, unwarp_h, tau=0.0):
    """heat_masked, mask [n, H, W]; unwarp_h [n, 3, 3] -> dict:
      a, b        numerator and denominator, out = a / b with NaN exactly where b == 0
      base_a/b    the corner values of every view with weight 1 (see the module text)
      near        the NaN near-tie set: b has no corner weight that is firmly on (both of its factors above tau) but a live mask value
                  within tau of the coordinate - an fp32 coordinate may switch such a weight on or off"""
    heat_masked, mask = np.asarray(heat_masked, np.float64), np.asarray(mask, np.float64)
    n, H, W = mask.shape
    a, b, base_a, base_b = (np.zeros((H, W)) for _ in range(4))
    firm, reach = np.zeros((H, W)), np.zeros((H, W))
    for v in range(n):
        ix, iy, _ = P.source_coords64(unwarp_h[v], H, W)
        hv, wts, _ = bilinear_taps(heat_masked[v], ix, iy)
        mv, _, _ = bilinear_taps(mask[v], ix, iy)
        a += (hv * wts).sum(0)
        b += (mv * wts).sum(0)
        base_a += np.abs(hv).sum(0)
        base_b += np.abs(mv).sum(0)
        ax, ay = ix - np.floor(ix), iy - np.floor(iy)
        fx, fy = (1 - ax, ax, 1 - ax, ax), (1 - ay, 1 - ay, ay, ay)
        for k in range(4):
            firm += np.abs(mv[k]) * ((fx[k] > tau) & (fy[k] > tau))
        for sx in (-tau, 0.0, tau):
            for sy in (-tau, 0.0, tau):
                reach += np.abs(bilinear_taps(mask[v], ix + sx, iy + sy)[0]).sum(0)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = a / b
    out[b == 0] = np.nan
    return {"a": a, "b": b, "out": out, "base_a": base_a, "base_b": base_b, "near": (firm == 0) & (reach > 0)}


# ------------------------------------------------------------------------------------------------ soft-argmax
def soft_argmax5(heat, x, y):
    """5x5 patch of the zero-padded map around the integer pixel (x, y): q = patch / (sum + 1e-6), negatives -> 1e-6, l = log q,
    e = exp(l - max l), (sx, sy) = sum((column, row) e) / (sum e + 1e-6), coordinates 0..4.  -> (sx, sy, base_x, base_y); an
    exponential carries the rounding of its operand, (1 + |l| + |max l|) eps, into both sums: base_x = sum (column + sx) e
    (1 + |l| + |max l|) / (sum e + 1e-6).  A patch of zeros gives log 0 - log 0 = NaN, as in the reference."""
    heat = np.asarray(heat, np.float64)
    H, W = heat.shape
    pad = np.zeros((H + 4, W + 4))
    pad[2:-2, 2:-2] = heat
    p = pad[int(y):int(y) + 5, int(x):int(x) + 5].reshape(25)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = p / (p.sum() + 1e-6)
        q = np.where(q < 0, 1e-6, q)
        l = np.log(q)
        m = l.max()
        e = np.exp(l - m)
        inv = 1.0 / (e.sum() + 1e-6)
        col, row = np.arange(25) % 5, np.arange(25) // 5
        sx, sy = (col * e).sum() * inv, (row * e).sum() * inv
        amp = np.where(e > 0, 1.0 + np.abs(l) + abs(m), 0.0)
        bx, by = ((col + sx) * e * amp).sum() * inv, ((row + sy) * e * amp).sum() * inv
    return sx, sy, bx, by


# ------------------------------------------------------------------------------------------------ sparse descriptors
def sample_desc(desc, xy):
    """desc [256, Hc, Wc], xy [n, 2] pixels (x, y) -> (out [n, 256], base [n, 256]).  samp = x / (W / 2) - 1 in float64 with W = 8 Wc,
    rounded to fp32 (model_wrap.py:303-307); ATen's align_corners unnormalise (g + 1) (size - 1) / 2; four corner weights, zeros
    padding; division by the L2 norm with 0 / 0 kept.  base = (s + |out| |s|_2) / norm with s = the corner sum of |desc| at weight 1."""
    desc = np.asarray(desc, np.float64)
    D, Hc, Wc = desc.shape
    xy = np.asarray(xy, np.float64)
    xn = (xy[:, 0] / (8 * Wc / 2.0) - 1.0).astype(F32).astype(np.float64)
    yn = (xy[:, 1] / (8 * Hc / 2.0) - 1.0).astype(F32).astype(np.float64)
    ix, iy = (xn + 1) * ((Wc - 1) / 2.0), (yn + 1) * ((Hc - 1) / 2.0)
    v, s = np.zeros((len(xy), D)), np.zeros((len(xy), D))
    for c in range(D):
        vals, wts, _ = bilinear_taps(desc[c], ix, iy)
        v[:, c] = (vals * wts).sum(0)
        s[:, c] = np.abs(vals).sum(0)
    nrm = np.sqrt((v * v).sum(axis=1, keepdims=True))
    with np.errstate(divide="ignore", invalid="ignore"):
        out = v / nrm
        base = (s + np.abs(out) * np.sqrt((s * s).sum(axis=1, keepdims=True))) / nrm
    return out, base


# ------------------------------------------------------------------------------------------------ two-way matching
def match_distances(d1, d2):
    """d1 [n1, D], d2 [n2, D] -> (d [n1, n2] fp64 = sqrt(2 - 2 clip(dot, -1, 1)), delta [n1, n2], exact [n1, n2]: at most one
    non-zero product, so every fp32 evaluation gives the reference's bits).  delta propagates the fp32
    dot-product bound D 2^-24 sum |a_k b_k| (0 where at most one product is non-zero: adding zeros is exact in every order) through
    the fp32 difference (2^-23 on d^2) and the square root: with s = 2 dc + 2^-23, the larger of d - sqrt(max(d^2 - s, 0)) and
    sqrt(d^2 + s) - d, plus 2^-23 d."""
    a, b = np.asarray(d1, np.float64), np.asarray(d2, np.float64)
    dot = a @ b.T
    nz = (a != 0).astype(np.float64) @ (b != 0).astype(np.float64).T
    dc = np.where(nz > 1, a.shape[1] * EPS * (np.abs(a) @ np.abs(b).T), 0.0)
    d2_ = 2.0 - 2.0 * np.clip(dot, -1.0, 1.0)
    d = np.sqrt(d2_)
    slack = 2 * dc + np.where(nz > 1, 2.0 ** -23, 0.0)
    return d, np.maximum(d - np.sqrt(np.maximum(d2_ - slack, 0.0)), np.sqrt(d2_ + slack) - d) + 2.0 ** -23 * d, nz <= 1


def _first_of_equals(rows):
    """index of the first row bit-equal to each row"""
    first, seen = np.arange(len(rows)), {}
    for i, r in enumerate(rows):
        first[i] = seen.setdefault(np.asarray(r, F32).tobytes(), i)
    return first


def match_two_way(d1, d2, thr):
    """nn_match_two_way on unit rows d1 [n1, D], d2 [n2, D] (float32 data).  Decisions follow the reference's arithmetic on the exact
    dot product: the dot rounded to fp32, 2 - 2 clip and the square root in fp32, first index on ties, keep d < thr (strict).
    -> dict: matches [(i, j)] rows ascending, d / delta / exact (match_distances), d32 (the reference's fp32 distance of the exact dot), amb_rows [n1]: the match of row i may be decided by
    the fp32 summation order - its best and second-best distance (exact copies of the best column aside) are closer than the sum
    of their deltas, or the same for the column it picks, or its best distance is within delta of thr."""
    n1, n2 = len(d1), len(d2)
    if n1 == 0 or n2 == 0:
        return {"matches": [], "amb_rows": np.zeros(n1, bool), "d": np.zeros((n1, n2)), "delta": np.zeros((n1, n2))}
    d, delta, exact = match_distances(d1, d2)
    dot32 = (np.asarray(d1, np.float64) @ np.asarray(d2, np.float64).T).astype(F32)
    d32 = np.sqrt(F32(2) - F32(2) * np.clip(dot32, F32(-1), F32(1)))
    assert d32.dtype == F32
    rb, cb = d32.argmin(axis=1), d32.argmin(axis=0)
    thr32 = F32(thr)
    matches = [(i, int(rb[i])) for i in range(n1) if d32[i, rb[i]] < thr32 and cb[rb[i]] == i]

    def ambiguous(dm, dl, best, copies):
        out = np.zeros(len(dm), bool)
        for i in range(len(dm)):
            other = copies != copies[best[i]]
            if other.any():
                out[i] = (dm[i, other] - dl[i, other]).min() <= dm[i, best[i]] + dl[i, best[i]]
        return out
    row_amb = ambiguous(d, delta, rb, _first_of_equals(d2))
    col_amb = ambiguous(d.T, delta.T, cb, _first_of_equals(d1))
    best, bd = d[np.arange(n1), rb], delta[np.arange(n1), rb]
    near_thr = (np.abs(best - float(thr32)) <= bd) & ~exact[np.arange(n1), rb]
    return {"matches": matches, "amb_rows": row_amb | col_amb[rb] | near_thr, "d": d, "delta": delta, "d32": d32, "exact": exact}
