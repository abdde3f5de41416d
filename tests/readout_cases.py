"""Inputs shared by tests/test_readout_ref_cpu.py and tests/test_gpu_readout_exact.py, all generated from seeds on the CPU, and the
bounds of the GPU tests.  The CPU file shows for exactly these inputs that the shares the GPU tests may leave out stay inside their
caps and that every mutant of the restatement is rejected at these bounds."""
import functools

import numpy as np

from oracle import cpu_ref as C
from tests import pairs_cases as PC
from tests import pairs_ref as P
from tests import readout_ref as R

F32 = np.float32
SHAPES = ((37, 53), (40, 56))       # (37, 53): odd, H * W no multiple of a block; (40, 56): multiples of 8
BAND_CAP = 5e-3                     # nearest-mask tie band, share of a case
NEAR_CAP = 5e-3                     # NaN near-tie set of combine, share of a case
AMB_CAP = 2e-2                      # ambiguous rows of the matcher, share of a case
SW_MIN = 2.0 ** -10                 # horizon inside the frame: pixels with a smaller |sw| are not compared

# worst |device - fp64| / base per family on the MI355X (profiles/readout_exact_measure.txt); TAU = 4 x the value: room for another
# valid fp32 order.  tests/test_readout_ref_cpu.py prints the fp32 oracle's own ratios on the same cases beside them.
MEASURED = {
    "flatten_nchw": 1.13e-7,    # flatten_detection_kernel on a public NCHW tensor: 1.125e-7 (n 3, 5x7, N(0, 1) logits)
    "flatten_nhwc": 1.23e-7,    # the same kernel on the slot's NHWC convPb output with the bnPb affine: 1.221e-7 (n 3, 5x7, as drawn)
    "combine": 1.55e-6,         # combine_heatmap_kernel: 1.544e-6 (40x56, n 1): the fp32 un-warp coordinates, ~1e-6 px here
    "soft_argmax": 3.10e-8,     # soft_argmax5 (nms_points_kernel and soft_argmax_points_kernel): 3.100e-8 (signed_zeros_40x72, nms 0)
    "sample_nchw": 1.86e-7,     # sample_desc_kernel, NCHW, rows of 2 floats: 1.855e-7 (8x12)
    "sample_nhwc": 3.54e-7,     # sample_desc_kernel on the slot's NHWC rows, points in rows of 5 floats: 3.538e-7 (8x12, 3013 points)
}
TAU = {k: 4 * v for k, v in MEASURED.items()}


# ------------------------------------------------------------------------------------------------ views and masks
def _translation(tx, ty, H, W):
    return np.array([[1, 0, 2.0 * tx / (W - 1)], [0, 1, 2.0 * ty / (H - 1)], [0, 0, 1]])


@functools.lru_cache(maxsize=None)
def view_cases(H, W):
    """name -> inv_homographies float32 [n, 3, 3], n in {7, 4, 3, 1, 1}.  `horizon`: sw = 1 + 1.6 gx + 0.2 gy changes sign inside
    the frame (at gx = -0.625 on the middle row)."""
    w = PC.warp_cases(H, W)
    cases = {
        "n7": [np.eye(3), _translation(0.3, 0.25, H, W), w["scales_rotation"][0], w["scales_rotation"][1], w["scales_rotation"][2],
               w["warp11"][0], w["perspective"][0]],
        "n4": [w["warp11"][1], w["warp11"][2], w["perspective"][1], w["perspective"][2]],
        "n3": list(w["warp13"]),
        "n1": [_translation(-1.7, 2.4, H, W)],
        "horizon": [np.array([[1, 0, 0], [0, 1, 0], [1.6, 0.2, 1.0]])],
    }
    return {k: np.ascontiguousarray(np.stack(v), F32) for k, v in cases.items()}


def view_image(kind, H, W):
    """float32 [H, W]: white noise, or a linear ramp (bilinear interpolation is exact on it: the coordinates alone)"""
    return PC.images(kind, H, W, seed=7)[0, 0]


VIEW_KINDS = ("noise", "ramp")


@functools.lru_cache(maxsize=None)
def views_reference(H, W, name, kind):
    """Everything the views test needs, computed once: the restatement, the fp32 oracle's e_ref over the compared pixels, the tie
    band of the mask and the pixels that lie beyond the padding by more than any fp32 coordinate can stray.
    Regular cases: every pixel is compared, the band is tau = twice the measured fp32 - fp64 coordinate distance (the pair feed's
    rule).  `horizon`: pixels with |sw| >= SW_MIN are compared; the coordinate error grows towards the horizon, so the band is the
    a-priori bound of readout_ref.coord_error_bound pixel by pixel, among the pixels that it leaves within reach of the image."""
    import torch
    inv, img = view_cases(H, W)[name], view_image(kind, H, W)
    n = len(inv)
    r = R.views_and_masks(img, inv)
    with np.errstate(divide="ignore", invalid="ignore"):
        o = C.inv_warp_image_batch(torch.from_numpy(img).view(1, 1, H, W).repeat(n, 1, 1, 1), torch.from_numpy(inv)).numpy()[:, 0]
        om = C.compute_valid_mask((H, W), torch.from_numpy(inv)).numpy()
    ix, iy = r["ix"], r["iy"]
    if name == "horizon":
        compared = np.abs(r["sw"]) >= SW_MIN
        tol = np.stack([R.coord_error_bound(m, H, W) for m in inv])
        with np.errstate(invalid="ignore"):
            reach = (ix > -0.5 - tol) & (ix < W - 0.5 + tol) & (iy > -0.5 - tol) & (iy < H - 0.5 + tol)
        band = (r["tie"] <= tol) & reach & compared
    else:
        compared = np.ones(r["views"].shape, bool)
        tau, far = PC.nearest_tau(inv, H, W)
        assert far < 0.25, (name, far)
        tol = np.full(r["views"].shape, max(tau, 2 * far))
        band = r["tie"] <= tau
    with np.errstate(invalid="ignore"):
        far_beyond = compared & ((ix < -1 - tol) | (ix > W + tol) | (iy < -1 - tol) | (iy > H + tol))
    r.update(inv=inv, img=img, oracle=o, oracle_mask=om, compared=compared, band=band, far_beyond=far_beyond,
             e_ref=float(np.abs(o - r["views"])[compared].max()))
    return r


# ------------------------------------------------------------------------------------------------ flatten
FLATTEN_SHAPES = ((1, 3, 5), (3, 5, 7))     # (n, Hc, Wc): 15 cells (no multiple of the 4 cells of a block) and 105


@functools.lru_cache(maxsize=None)
def flatten_case(n, Hc, Wc, scale):
    """semi float32 [n, 65, Hc, Wc]: N(0, 1) * scale; cell (0, 0, 0) with a dominating dustbin (40 above the largest logit), the last
    cell with 65 equal logits; mask float32 [n, 1, 8 Hc, 8 Wc]: 0 / 1 with 30 % zeros and a few halves"""
    rs = np.random.RandomState(100 * n + Hc)
    semi = (rs.randn(n, 65, Hc, Wc) * scale).astype(F32)
    semi[0, 64, 0, 0] = semi[0, :, 0, 0].max() + F32(40)
    semi[n - 1, :, Hc - 1, Wc - 1] = F32(0.7) * scale
    mask = (rs.uniform(size=(n, 1, 8 * Hc, 8 * Wc)) > 0.3).astype(F32)
    mask[rs.uniform(size=mask.shape) < 0.05] = 0.5
    return semi, mask


# ------------------------------------------------------------------------------------------------ combine
COMBINE_N = (1, 2, 3, 4, 5, 7, 9)


@functools.lru_cache(maxsize=None)
def combine_case(H, W, n):
    """(heat float32 [n, H, W] in (0, 0.1), mask float32 [n, H, W], unwarp float32 [n, 3, 3]): WARP draws, none the identity.  Every
    mask is the nearest warp into its view of ONE map of the output frame with a zeroed block (n = 2: a zeroed half as well), so that
    no view covers that block: NaN inside, denominators down to ~1e-4 along its rim; each view also loses a block of its own."""
    seed = 300 + n
    hs, inv, _ = P.sample_homographies(seed, n, C.sample_homography, C.get_perspective_transform, **PC.f32_params(PC.WARP))
    unwarp, inv = np.ascontiguousarray(hs, F32), np.ascontiguousarray(inv, F32)
    rs = np.random.RandomState(seed)
    heat = rs.uniform(1e-3, 0.1, (n, H, W)).astype(F32)
    frame = np.ones((H, W))
    frame[H // 4:H // 2, W // 3:2 * W // 3] = 0
    if n == 2:
        frame[:, :W // 4] = 0
    mask = np.stack([P.warp_nearest64(frame, inv[v]) for v in range(n)])
    for v in range(n):
        y, x = rs.randint(0, H - 6), rs.randint(0, W - 8)
        mask[v, y:y + 6, x:x + 8] = 0
    return heat, mask.astype(F32), unwarp


def combine_tau(unwarp, H, W):
    """twice the largest fp32 - fp64 distance of the un-warp coordinates over the pixels that can read a view"""
    return 2.0 * max(P.coord_deviation(m, H, W)[0] for m in unwarp)


@functools.lru_cache(maxsize=None)
def combine_reference(H, W, n):
    """the restatement of one combine case (readout_ref.combine with the case's tau), with its inputs"""
    heat, mask, unwarp = combine_case(H, W, n)
    r = R.combine(heat.astype(np.float64) * mask, mask, unwarp, combine_tau(unwarp, H, W))
    r.update(heat=heat, mask=mask, unwarp=unwarp)
    return r


def combine_ratio(out, r):
    """|out b_ref - a_ref| / (base_a + |out| base_b) over the pixels with a finite out and b_ref > 0 outside the near-tie set: a small
    denominator does not hide a wrong numerator"""
    ok = np.isfinite(out) & (r["b"] > 0) & ~r["near"]
    o = np.where(ok, out, 0.0).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.abs(o * r["b"] - r["a"]) / (r["base_a"] + np.abs(o) * r["base_b"])
    return np.where(ok, q, 0.0)


def combine_nan_mismatch(out, r):
    """pixels outside the near-tie set whose NaN state differs from the restatement's (NaN exactly where b == 0)"""
    return (np.isnan(out) != (r["b"] == 0)) & ~r["near"]


# ------------------------------------------------------------------------------------------------ points
def point_maps():
    """(name, heat float32 [H, W], threshold) for nms_dist in {0, 9, 16}.  Sizes 8x8 (the smallest the export accepts), 32x32 (one
    tile), 40x72 (partial tiles).  Quantised maps tie inside every window and hold values exactly equal to the threshold."""
    rs = np.random.RandomState(77)
    out = []
    for (H, W) in ((8, 8), (32, 32), (40, 72)):
        out.append(("uniform_%dx%d" % (H, W), rs.uniform(0, 1, (H, W)).astype(F32), 0.3))
        out.append(("quantised_%dx%d" % (H, W), (np.round(rs.uniform(0, 1, (H, W)) * 8) / 8).astype(F32), 0.25))
        out.append(("constant_%dx%d" % (H, W), np.full((H, W), 0.25, F32), 0.25))
    z = (np.round(rs.uniform(0, 1, (40, 72)) * 4) / 4).astype(F32)
    z[z == 0] = np.where(rs.uniform(size=int((z == 0).sum())) < 0.5, F32(-0.0), F32(0.0))    # threshold 0 keeps -0.0 and +0.0 alike
    out.append(("signed_zeros_40x72", z, 0.0))
    return out


# ------------------------------------------------------------------------------------------------ soft-argmax
def soft_argmax_case():
    """(heat float32 [24, 40], xy float32 [n, 2]): corners, edges, a patch of zeros but for its centre, a flat patch, zeros inside a patch,
    a few negative values (set to 1e-6 after the normalisation), and a patch of zeros only (log 0 - log 0: NaN)."""
    H, W = 24, 40
    rs = np.random.RandomState(88)
    h = rs.uniform(0.01, 1, (H, W)).astype(F32)
    h[rs.uniform(size=(H, W)) < 0.1] = 0   # zeros inside patches
    h[8:15, 8:15] = 0
    h[11, 11] = 0.37                       # zero but for the centre
    h[8:15, 20:27] = 0.125                 # flat
    h[16:23, 28:35] = 0                    # zeros only around (31, 19)
    h[3, 30], h[4, 33], h[20, 5] = -0.05, -0.2, -0.01
    pts = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (1, 1), (W - 2, H - 2), (0, 10), (W - 1, 12), (17, 0), (19, H - 1),
           (11, 11), (23, 11), (31, 19), (30, 3), (32, 4), (5, 20), (12, 12), (10, 11)]
    pts += [(int(x), int(y)) for x, y in zip(rs.randint(0, W, 30), rs.randint(0, H, 30))]
    return h, np.array(pts, F32)


# ------------------------------------------------------------------------------------------------ sparse descriptors
SAMPLE_SHAPES = ((5, 7), (8, 12))


@functools.lru_cache(maxsize=None)
def sample_case(Hc, Wc):
    """(desc float32 [3, 256, Hc, Wc], xy float32 [3, cap, 2]): the four corners, cell boundaries, quarter-pixel offsets, the band
    (-8, 0) left of / above the first cell centre's reach, just beyond the last pixel, wholly outside (NaN rows), random points."""
    H, W = 8 * Hc, 8 * Wc
    rs = np.random.RandomState(10 * Hc + Wc)
    desc = rs.randn(3, 256, Hc, Wc).astype(F32)
    far_x, far_y = W * Wc / (Wc - 1.0) + 9, H * Hc / (Hc - 1.0) + 9
    pts = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (8, 8), (16, 24), (W - 8, H - 8), (7.5, 8), (10.25, 13.75), (3.75, 30.5),
           (W - 1.25, H - 1.75), (-3.5, 5), (5, -7.75), (-0.25, -0.25), (-7.5, -6), (W + 3, 7), (9, H + 2.5), (-20, 5), (far_x, 5),
           (5, far_y), (-30, -30), (4, 4), (12, 20)]
    cap = len(pts) + 9
    xy = np.zeros((3, cap, 2), F32)
    for b in range(3):
        xy[b, :len(pts)] = np.roll(np.array(pts, F32), b, axis=0)
        xy[b, len(pts):] = np.stack([rs.uniform(-8, W + 8, 9), rs.uniform(-8, H + 8, 9)], axis=1)
    return desc, xy


# ------------------------------------------------------------------------------------------------ matching
MATCH_CAP = 131
MATCH_SIZES = (((33, 65), (64, 129), (1, 31)), ((63, 32), (129, 64), (65, 1)), ((31, 33), (32, 63), (129, 129)))


def _unit(a):
    a = a.astype(F32)
    return (a / np.sqrt((a.astype(np.float64) ** 2).sum(axis=1, keepdims=True))).astype(F32)


def threshold_triple(near=0.7):
    """(thr, [c_below, c_at, c_above]): an fp32 threshold close to `near` and fp32 cosines whose reference distance sqrt(2 - 2 c),
    evaluated in fp32, is the fp32 number just below thr, thr itself and the one just above.  Consecutive cosines move the distance
    by about 1.4 ulp, so not every distance is reachable: the fp32 neighbours of 1 - near^2 / 2 are scanned for three in a row."""
    c = F32(1.0 - near ** 2 / 2)
    reach = {}
    for _ in range(400):
        reach.setdefault(np.sqrt(F32(2) - F32(2) * c), c)
        c = np.nextafter(c, F32(-2))
    for d in sorted(reach):
        lo, hi = np.nextafter(d, F32(0)), np.nextafter(d, F32(2))
        if lo in reach and hi in reach:
            return float(d), [reach[lo], reach[d], reach[hi]]
    raise AssertionError("no three consecutive distances")


MATCH_THR, THRESHOLD_COSINES = threshold_triple()


@functools.lru_cache(maxsize=None)
def match_case(n1, n2, seed):
    """(d1 float32 [n1, 256], d2 float32 [n2, 256]) unit rows: half of d2 are noisy copies of rows of d1 (noise spread so that the
    distances straddle the threshold), the rest distractors.  Where the sizes allow: exact duplicates on both sides, an antipodal
    pair, an identical pair, an axis pair of length 1 + 2^-23 (dot above 1), and three axis pairs d1 = e_2k, d2 = c e_2k + s e_2k+1 whose dot product c is exact in every order and
    whose fp32 distance is one ulp below, at and one ulp above the threshold."""
    rs = np.random.RandomState(seed)
    d1, d2 = _unit(rs.randn(n1, 256)), _unit(rs.randn(n2, 256))
    m = min(n1, n2) // 2
    if m:
        src, dst = rs.choice(n1, m, replace=False), rs.choice(n2, m, replace=False)
        d2[dst] = _unit(d1[src] + rs.uniform(0.01, 0.06, (m, 1)) * rs.randn(m, 256))
    if n1 >= 31 and n2 >= 31:
        d2[3] = _unit(d1[4:5] + 0.02 * rs.randn(1, 256))[0]
        d2[11], d2[5] = d2[3], d2[3]                 # duplicate columns: row 4 picks among 3, 5, 11 and takes 3
        d2[8] = _unit(d1[2:3] + 0.02 * rs.randn(1, 256))[0]
        d1[9] = d1[2]                                # duplicate rows: column 8 picks among 2 and 9 and takes 2
        d2[20] = -d1[6]                              # antipodal: dot -1, d = 2
        d2[21] = d1[7]                               # identical: the dot rounds to 1 or just beside it
        for k, c in enumerate(THRESHOLD_COSINES):
            d1[12 + k], d2[14 + k] = 0, 0
            d1[12 + k, 2 * k] = 1
            d2[14 + k, 2 * k], d2[14 + k, 2 * k + 1] = c, F32(np.sqrt(1.0 - float(c) ** 2))
        d1[15], d2[17] = 0, 0                        # dot = (1 + 2^-23)^2 > 1 in every order: only the clip gives d = 0
        d1[15, 6] = d2[17, 6] = np.nextafter(F32(1), F32(2))
    return d1, d2


def match_tensors(group, g):
    """numpy inputs of one call with 3 pairs at pair_stride 2: desc1, desc2 float32 [6, cap, 256] (NaN in every row past the counts and
    in the entries a stride of 2 skips), count1, count2 int32 [6] (the skipped entries hold cap + 5)."""
    d1 = np.full((6, MATCH_CAP, 256), np.nan, F32)
    d2 = np.full((6, MATCH_CAP, 256), np.nan, F32)
    c1 = np.full(6, MATCH_CAP + 5, np.int32)
    c2 = np.full(6, MATCH_CAP + 5, np.int32)
    pairs = []
    for p, (n1, n2) in enumerate(group):
        a, b = match_case(n1, n2, 500 + 10 * g + p)
        d1[2 * p, :n1], d2[2 * p, :n2], c1[2 * p], c2[2 * p] = a, b, n1, n2
        pairs.append((a, b))
    return d1, d2, c1, c2, pairs
