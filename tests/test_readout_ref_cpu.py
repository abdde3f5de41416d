"""CPU: pins tests/readout_ref.py, the fp64 restatement the read-out kernels are compared with (tests/test_gpu_readout_exact.py), to
oracle/cpu_ref.py, to the G8 / G15 fixtures and by mutants, on exactly the cases of the GPU tests (tests/readout_cases.py); prints the fp32
oracle's own ratio per family and case, and prints and asserts the shares the GPU tests may leave out:
  nearest-mask tie band <= 0.5 % of a case, NaN near-tie set of combine <= 0.5 %, ambiguous match rows <= 2 %.
A mutant is a wrong formula; each must move some element of some GPU case by more than the LARGEST bound its family uses (the larger tau
of the family's two layouts; for the views the largest 2 e_ref + 2^-23 of any case)."""
import numpy as np
import pytest
import torch

from oracle import cpu_ref as C
from tests import golden_util as G
from tests import pairs_ref as P
from tests import readout_cases as K
from tests import readout_ref as R
from tests.golden_descriptor import MATCH_CASES, match_case_inputs

TAU_FLATTEN = max(K.TAU["flatten_nchw"], K.TAU["flatten_nhwc"])
TAU_SAMPLE = max(K.TAU["sample_nchw"], K.TAU["sample_nhwc"])
F32 = np.float32


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


# ------------------------------------------------------------------------------------------------ views and masks
def _view_bound(r):
    return 2 * r["e_ref"] + 2.0 ** -23


@pytest.mark.parametrize("shape", K.SHAPES)
def test_views_restatement_against_oracle_and_band_caps(shape):
    """e_ref per case (printed); the oracle's nearest mask equals the restatement outside the tie band among the compared pixels;
    the band holds at most 0.5 % of a case; beyond the padding both are exactly 0."""
    H, W = shape
    for name in K.view_cases(H, W):
        for kind in K.VIEW_KINDS:
            r = K.views_reference(H, W, name, kind)
            cmp_ = r["compared"]
            share = float(r["band"].sum()) / max(int(cmp_.sum()), 1)
            bad = (r["oracle_mask"] != r["masks"]) & cmp_ & ~r["band"]
            print("views %dx%d %-8s %-5s n %d  compared %.4f  e_ref %.3g  band share %.5f  oracle mask mismatches outside %d, inside %d" %
                  (H, W, name, kind, len(r["inv"]), cmp_.mean(), r["e_ref"], share, int(bad.sum()),
                   int(((r["oracle_mask"] != r["masks"]) & r["band"]).sum())))
            assert share <= K.BAND_CAP, (name, share)
            assert not bad.any(), (name, np.argwhere(bad)[:5])
            assert not r["oracle"][r["far_beyond"]].any() and not r["views"][r["far_beyond"]].any()
            assert r["e_ref"] <= (2e-2 if name == "horizon" else 1e-3), (name, r["e_ref"])
            assert cmp_.mean() >= 0.99
            if name == "horizon":
                assert (r["sw"] > 0).any() and (r["sw"] < 0).any() and np.abs(r["sw"]).min() > 0    # the horizon IS inside


def _warp_mutant(img, m, kind):
    """a wrong bilinear warp of one image"""
    H, W = img.shape
    if kind == "transposed":
        m = np.asarray(m).T
    ix, iy, _ = P.source_coords64(m, H, W)
    if kind == "align_false":
        ix, iy = ((2 * ix / (W - 1) - 1 + 1) * W - 1) / 2, ((2 * iy / (H - 1) - 1 + 1) * H - 1) / 2
    if kind == "clamp":
        ix, iy = np.clip(ix, 0, W - 1), np.clip(iy, 0, H - 1)
    vals, wts, _ = R.bilinear_taps(img, ix, iy)
    out = (vals * wts).sum(0)
    if kind == "band_dropped":
        out[(ix < 0) | (ix > W - 1) | (iy < 0) | (iy > H - 1)] = 0
    return out


def test_views_mutants_are_rejected():
    bound = max(_view_bound(K.views_reference(H, W, name, kind)) for (H, W) in K.SHAPES for name in K.view_cases(H, W) for kind in K.VIEW_KINDS)
    H, W = K.SHAPES[0]
    r = K.views_reference(H, W, "n7", "noise")
    for kind in ("align_false", "clamp", "band_dropped", "transposed"):
        moved = max(float(np.abs(_warp_mutant(r["img"], r["inv"][v], kind) - r["views"][v]).max()) for v in range(len(r["inv"])))
        print("views mutant %-13s moves %.3g (largest bound in use %.3g)" % (kind, moved, bound))
        assert moved > bound, kind
    # floor instead of half-to-even in the mask: pixels outside the tie band change
    flo = np.stack([(np.floor(r["ix"][v]) >= 0) & (np.floor(r["ix"][v]) <= W - 1) & (np.floor(r["iy"][v]) >= 0) & (np.floor(r["iy"][v]) <= H - 1)
                    for v in range(len(r["inv"]))])
    assert ((flo != r["masks"]) & ~r["band"]).sum() > 0
    tr = R.views_and_masks(r["img"], np.transpose(r["inv"], (0, 2, 1)))["masks"]
    assert ((tr != r["masks"]) & ~r["band"]).sum() > 0


@pytest.mark.parametrize("name", ("sp_64x96_v6", "ssp_48x64_v5", "sp_120x160_v4"))
def test_restatement_reproduces_g8(name):
    """G8 (the real reference, fp32): views within the fp32 coordinate distance times the image's gradient (the pair feed's G7 bound),
    masks equal outside the tie band, per-view heat maps and the aggregate at fp32 rounding level of their bases."""
    g = G.load("g8_export_%s.npz" % name)
    img, inv = g["img"], g["inv_homographies"]
    H, W = img.shape
    r = R.views_and_masks(img, inv)
    tau = 2 * max(P.coord_deviation(m, H, W)[0] for m in inv)
    span = float(img.max() - img.min())
    assert np.abs(r["views"] - g["views"][:, 0]).max() <= 2 * tau * span + 2.0 ** -21
    masks = r["masks"] if int(g["erosion"]) == 0 else np.stack([P.erode(m, int(g["erosion"])) for m in r["masks"]])
    band = r["tie"] <= tau
    if int(g["erosion"]) == 0:
        assert not ((masks != g["valid_mask"][:, 0]) & ~band).any()
    else:
        assert (masks != g["valid_mask"][:, 0]).mean() <= K.BAND_CAP
    sd = C.to_torch(C.init_state_dict(str(g["arch"]), seed=int(g["seed"])))
    with torch.no_grad():
        semi = C.forward(sd, t(g["views"]), str(g["arch"]), train=True)["semi"].numpy()
    heat, base = R.flatten(semi)
    q = float((np.abs(heat - g["views_heatmap"][:, 0]) / base).max())
    ctau = K.combine_tau(g["homographies"], H, W)
    c = R.combine(g["views_heatmap"][:, 0].astype(np.float64) * g["valid_mask"][:, 0], g["valid_mask"][:, 0], g["homographies"], ctau)
    assert not K.combine_nan_mismatch(g["aggregate"], c).any()
    qc = float(K.combine_ratio(g["aggregate"], c).max())
    print("G8 %-14s flatten ratio %.3g  combine ratio %.3g" % (name, q, qc))
    # a corner weight (1 - ax)(1 - ay) moves by at most the coordinate distance in x plus that in y, and every corner enters the base at 1
    assert q <= 2.0 ** -20 and qc <= 2 * ctau + 2.0 ** -20
    pts = C.get_pts_from_heatmap(g["aggregate"], F32(float(g["thr"])), 4, 4)
    assert np.array_equal(pts, g["pts_nms"])
    sub = _soft_points(g["aggregate"], pts.T)
    k = g["pts"].shape[0]
    assert np.abs(sub[:k, :2] - g["pts"][:, :2]).max() < 1e-5


def _soft_points(heat, pts):
    """[N, 3] points moved by the restatement's soft-argmax: (x, y) + (sx, sy) - 2"""
    out = np.array(pts, np.float64)
    for i, p in enumerate(out):
        sx, sy, _, _ = R.soft_argmax5(heat, p[0], p[1])
        out[i, 0], out[i, 1] = p[0] + sx - 2, p[1] + sy - 2
    return out


# ------------------------------------------------------------------------------------------------ flatten
def _flatten_mutant(semi, mask, kind):
    l = np.asarray(semi, np.float64)
    e = np.exp(l - l.max(axis=1, keepdims=True))
    p = e / (e[:, :64].sum(axis=1, keepdims=True) if kind == "no_dustbin" else e.sum(axis=1, keepdims=True))
    n, _, Hc, Wc = l.shape
    x = p[:, :64].reshape(n, 8, 8, Hc, Wc)
    heat = (x.transpose(0, 3, 2, 4, 1) if kind == "swapped" else x.transpose(0, 3, 1, 4, 2)).reshape(n, 8 * Hc, 8 * Wc)
    return heat if kind == "no_mask" else heat * np.asarray(mask, np.float64)[:, 0]


def test_flatten_restatement_against_oracle_and_mutants():
    rejected = set()
    for (n, Hc, Wc) in K.FLATTEN_SHAPES:
        for scale in (1.0, 30.0):
            semi, mask = K.flatten_case(n, Hc, Wc, scale)
            heat, base = R.flatten(semi)
            o = C.flatten_detection(t(semi)).numpy()[:, 0]
            ratio = float((np.abs(o - heat) / base).max())
            print("flatten n %d %dx%d scale %g: oracle ratio %.3g, dustbin cell max p %.3g, equal cell p - 1/65 %.3g" %
                  (n, Hc, Wc, scale, ratio, heat[0, :8, :8].max(), np.abs(heat[n - 1, -8:, -8:] - 1 / 65.0).max()))
            assert ratio <= 2.0 ** -20
            assert heat[0, :8, :8].max() < 1e-15 and np.abs(heat[n - 1, -8:, -8:] - 1 / 65.0).max() < 1e-15
            hm, bm = R.flatten(semi, mask)
            assert np.array_equal(hm == 0, (mask[:, 0] == 0) | (heat == 0))
            for kind in ("no_dustbin", "swapped", "no_mask"):
                if (np.abs(_flatten_mutant(semi, mask, kind) - hm) > TAU_FLATTEN * np.maximum(bm, base * (kind == "no_mask"))).any():
                    rejected.add(kind)
    assert rejected == {"no_dustbin", "swapped", "no_mask"}, rejected
    # a hand vector: two channels at l, 63 at 0 -> p = e^l / (2 e^l + 63); channel 9 sits at pixel (1, 1) of the cell
    semi = np.zeros((1, 65, 1, 1))
    semi[0, 9], semi[0, 64] = 2.0, 2.0
    heat, _ = R.flatten(semi)
    assert abs(heat[0, 1, 1] - np.exp(2.0) / (2 * np.exp(2.0) + 63)) < 1e-15 and abs(heat[0, 0, 0] - 1 / (2 * np.exp(2.0) + 63)) < 1e-15


# ------------------------------------------------------------------------------------------------ combine
def _combine_mutant(r, kind):
    heat, mask, unwarp = r["heat"].astype(np.float64) * r["mask"], r["mask"].astype(np.float64), r["unwarp"]
    n, H, W = mask.shape
    if kind == "views_dropped":
        k = n // 4 * 4
        return R.combine(heat[:k], mask[:k], unwarp[:k])["out"] if k else np.full((H, W), np.nan)
    c = R.combine(heat, mask, unwarp)
    if kind == "divided_by_n":
        return c["a"] / n
    if kind == "zero_for_nan":
        return np.where(c["b"] == 0, 0.0, c["out"])
    assert kind == "mask_nearest"
    b = sum(P.warp_nearest64(mask[v], unwarp[v]) for v in range(n))
    with np.errstate(divide="ignore", invalid="ignore"):
        return c["a"] / b


@pytest.mark.parametrize("shape", K.SHAPES)
def test_combine_restatement_against_oracle_caps_and_mutants(shape):
    H, W = shape
    rejected = set()
    for n in K.COMBINE_N:
        r = K.combine_reference(H, W, n)
        o = C.combine_heatmap(t(r["heat"])[:, None], t(r["unwarp"]), t(r["mask"])[:, None]).numpy()[0]
        nan_bad = K.combine_nan_mismatch(o, r)
        ratio = K.combine_ratio(o, r)
        b_pos = r["b"][r["b"] > 0]
        print("combine %dx%d n %d: NaN pixels %d, near-tie share %.5f, smallest b %.3g, b < 1e-3: %d, oracle ratio %.3g, oracle NaN mismatches "
              "outside the near-tie set %d, inside %d" % (H, W, n, int((r["b"] == 0).sum()), r["near"].mean(), b_pos.min(),
                                                          int((b_pos < 1e-3).sum()), ratio.max(), int(nan_bad.sum()),
                                                          int(((np.isnan(o) != (r["b"] == 0)) & r["near"]).sum())))
        assert r["near"].mean() <= K.NEAR_CAP, (n, r["near"].mean())
        assert not nan_bad.any() and (r["b"] == 0).sum() >= 50
        assert ratio.max() <= 2 * K.combine_tau(r["unwarp"], H, W) + 2.0 ** -20       # see test_restatement_reproduces_g8
        assert not np.allclose(r["unwarp"], np.eye(3), atol=1e-3)
        for kind in ("divided_by_n", "mask_nearest", "zero_for_nan", "views_dropped"):
            m = _combine_mutant(r, kind)
            if K.combine_nan_mismatch(m, r).any() or (K.combine_ratio(m, r) > K.TAU["combine"]).any():
                rejected.add(kind)
    assert rejected == {"divided_by_n", "mask_nearest", "zero_for_nan", "views_dropped"}, rejected


def test_combine_small_denominators_occur():
    """denominators down to ~1e-4 are part of the cases (the rim of the uncovered block)"""
    smallest = min(K.combine_reference(H, W, n)["b"][K.combine_reference(H, W, n)["b"] > 0].min() for (H, W) in K.SHAPES for n in K.COMBINE_N)
    assert smallest < 1e-3, smallest


# ------------------------------------------------------------------------------------------------ points and soft-argmax
def test_point_cases_hold_what_they_claim():
    """the oracle on the GPU test's maps: values equal to the threshold are kept, kept points lie farther apart than nms_dist, ties go to the
    lower row-major index, -0.0 passes a threshold of 0"""
    for name, hm, thr in K.point_maps():
        for dist in (0, 9, 16):
            pts = C.get_pts_from_heatmap(hm, F32(thr), dist, 0)
            assert pts.shape[1] > 0, name
            xy = pts[:2].T.astype(np.int64)
            if dist and len(xy) > 1:
                d = np.abs(xy[:, None] - xy[None]).max(-1)
                np.fill_diagonal(d, 10 ** 6)
                assert d.min() > dist
            if dist == 0:
                assert pts.shape[1] == int((hm >= F32(thr)).sum())
                if name.startswith(("quantised", "constant")):
                    assert (pts[2] == F32(thr)).any()
            if name.startswith("constant"):
                assert tuple(pts[:2, 0]) == (0.0, 0.0)
        if name.startswith("signed"):
            assert np.signbit(hm[hm == 0]).any() and not np.signbit(hm[hm == 0]).all()


def _soft_mutant(heat, x, y, kind):
    heat = np.asarray(heat, np.float64)
    H, W = heat.shape
    pad = np.pad(heat, 2, mode="edge" if kind == "clamped" else "constant")
    p = pad[int(y):int(y) + 5, int(x):int(x) + 5].reshape(25)
    eps = 0.0 if kind == "no_eps" else 1e-6
    with np.errstate(divide="ignore", invalid="ignore"):
        q = p / (p.sum() + eps)
        q = np.where(q < 0, 1e-6, q)
        l = np.log(q)
        e = np.exp(l - l.max())
        inv = 1.0 / (e.sum() + eps)
        sx, sy = (np.arange(25) % 5 * e).sum() * inv, (np.arange(25) // 5 * e).sum() * inv
    return (sy, sx) if kind == "swapped" else (sx, sy)


def test_soft_argmax_restatement_against_oracle_and_mutants():
    heat, xy = K.soft_argmax_case()
    pts = np.concatenate([xy.astype(np.float64), np.ones((len(xy), 1))], axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        o = C.soft_argmax_points(heat, pts.T.copy()).T[:, :2] - pts[:, :2] + 2
    ref = np.array([R.soft_argmax5(heat, x, y) for x, y in xy])
    nan = np.isnan(ref[:, 0])
    assert nan.sum() == 1 and np.array_equal(np.isnan(o[:, 0]), nan)
    ratio = np.abs(o - ref[:, :2])[~nan] / ref[:, 2:][~nan]
    print("soft-argmax: %d points, oracle ratio %.3g, one NaN patch (zeros only)" % (len(xy), ratio.max()))
    assert ratio.max() <= 2.0 ** -18
    i = [tuple(p) for p in xy.tolist()].index((11.0, 11.0))
    assert abs(ref[i, 0] - 2 / (1 + 1e-6)) < 1e-12 and abs(ref[i, 1] - 2 / (1 + 1e-6)) < 1e-12           # zero but for the centre
    j = [tuple(p) for p in xy.tolist()].index((23.0, 11.0))
    assert abs(ref[j, 0] - 50 / (25 + 1e-6)) < 1e-12                                                       # flat: the centre, but for 1e-6
    for kind in ("no_eps", "clamped", "swapped"):
        m = np.array([_soft_mutant(heat, x, y, kind) for x, y in xy])
        moved = (np.abs(m - ref[:, :2]) / ref[:, 2:])[~nan]
        print("soft-argmax mutant %-8s largest |moved| / base %.3g (tau %.3g)" % (kind, moved.max(), K.TAU["soft_argmax"]))
        assert moved.max() > K.TAU["soft_argmax"], kind


# ------------------------------------------------------------------------------------------------ sparse descriptors
def _sample_oracle(desc, xy, H, W):
    """models/model_wrap.py:295-313 on torch's CPU grid sampler, fp32"""
    samp = np.array(xy, np.float64)
    samp[:, 0] = samp[:, 0] / (float(W) / 2.0) - 1.0
    samp[:, 1] = samp[:, 1] / (float(H) / 2.0) - 1.0
    grid = torch.from_numpy(samp).view(1, 1, -1, 2).float()
    d = torch.nn.functional.grid_sample(t(desc)[None], grid, align_corners=True).view(256, -1)
    return (d / torch.norm(d, dim=0, keepdim=True)).numpy().T


def _sample_mutant(desc, xy, kind):
    D, Hc, Wc = desc.shape
    xy = np.asarray(xy, np.float64)
    if kind == "coarse_norm":
        xn, yn = xy[:, 0] / (Wc / 2.0) - 1, xy[:, 1] / (Hc / 2.0) - 1
    else:
        xn, yn = xy[:, 0] / (8 * Wc / 2.0) - 1, xy[:, 1] / (8 * Hc / 2.0) - 1
    if kind == "align_false":
        ix, iy = ((xn + 1) * Wc - 1) / 2, ((yn + 1) * Hc - 1) / 2
    else:
        ix, iy = (xn + 1) * (Wc - 1) / 2, (yn + 1) * (Hc - 1) / 2
    v = np.stack([(lambda a: (a[0] * a[1]).sum(0))(R.bilinear_taps(desc[c], ix, iy)) for c in range(D)], axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return v if kind == "no_norm" else v / np.sqrt((v * v).sum(axis=1, keepdims=True))


@pytest.mark.parametrize("hw", K.SAMPLE_SHAPES)
def test_sample_restatement_against_oracle_and_mutants(hw):
    Hc, Wc = hw
    desc, xy = K.sample_case(Hc, Wc)
    for b in range(3):
        ref, base = R.sample_desc(desc[b], xy[b])
        with np.errstate(divide="ignore", invalid="ignore"):
            o = _sample_oracle(desc[b], xy[b], 8 * Hc, 8 * Wc)
        nan = np.isnan(ref).any(axis=1)
        assert nan.sum() >= 4 and np.array_equal(np.isnan(o).any(axis=1), nan) and np.isnan(ref[nan]).all()
        ratio = float((np.abs(o - ref) / base)[~nan].max())
        print("sample %dx%d image %d: %d rows, %d NaN rows (wholly in the padding), smallest norm before division %.3g, oracle ratio %.3g" %
              (Hc, Wc, b, len(ref), int(nan.sum()), 1.0 / np.nanmax(base), ratio))
        assert ratio <= 2.0 ** -18
        assert np.abs(np.sqrt((ref[~nan] ** 2).sum(axis=1)) - 1).max() < 1e-12
        for kind in ("align_false", "coarse_norm", "no_norm"):
            m = _sample_mutant(desc[b].astype(np.float64), xy[b], kind)
            both = ~nan & ~np.isnan(m).any(axis=1)
            assert (np.abs(m - ref)[both] > TAU_SAMPLE * base[both]).any() or not np.array_equal(np.isnan(m).any(axis=1), nan), kind


def test_sample_restatement_reproduces_g15():
    g = G.load("g15_descriptor_ssp_120x160.npz")
    for tag in ("", "warped_"):
        k = g[tag + "desc"].shape[0]
        ref, base = R.sample_desc(g["coarse_desc"][0] if tag == "" else g["coarse_desc"][0], g[tag + "pts_int"][:k, :2])
        if tag == "":
            q = float((np.abs(ref - g["desc"]) / base).max())
            print("G15 sampled descriptors: ratio %.3g" % q)
            assert q <= 2.0 ** -18
        sub = _soft_points(g[tag + "heatmap"], g[tag + "pts_int"])
        assert np.abs(sub[:, :2] - g[tag + "pts"][:, :2]).max() < 1e-5
        assert np.array_equal(C.get_pts_from_heatmap(g[tag + "heatmap"], F32(float(g["conf_thresh"])), int(g["nms"]), 4).T, g[tag + "pts_int"])


# ------------------------------------------------------------------------------------------------ matching
def _match_fp32(d1, d2, thr, kind="reference"):
    """models/model_wrap.py:451-497 in numpy fp32 on rows [n, 256] (the fp32 oracle), or a wrong variant of it"""
    if len(d1) == 0 or len(d2) == 0:
        return []
    dmat = np.asarray(d1, F32) @ np.asarray(d2, F32).T
    with np.errstate(invalid="ignore"):
        dmat = np.sqrt(2 - 2 * (dmat if kind == "no_clip" else np.clip(dmat, -1, 1)))
    if kind == "last_index":
        idx = dmat.shape[1] - 1 - np.argmin(dmat[:, ::-1], axis=1)
        idx2 = dmat.shape[0] - 1 - np.argmin(dmat[::-1], axis=0)
    else:
        idx, idx2 = np.argmin(dmat, axis=1), np.argmin(dmat, axis=0)
    scores = dmat[np.arange(dmat.shape[0]), idx]
    keep = scores <= F32(thr) if kind == "le" else scores < F32(thr)
    if kind != "one_way":
        keep = np.logical_and(keep, np.arange(len(idx)) == idx2[idx])
    return [(int(i), int(idx[i])) for i in np.nonzero(keep)[0]]


def _match_differs(a, b, amb):
    a, b = {i: j for i, j in a if not amb[i]}, {i: j for i, j in b if not amb[i]}
    return a != b


def test_match_restatement_caps_crafted_rows_and_mutants():
    rejected = set()
    for g, group in enumerate(K.MATCH_SIZES):
        for p, (a, b) in enumerate(K.match_tensors(group, g)[4]):
            r = R.match_two_way(a, b, K.MATCH_THR)
            share = float(r["amb_rows"].mean())
            o = _match_fp32(a, b, K.MATCH_THR)
            print("match group %d pair %d (%d x %d): %d matches, ambiguous rows %.4f, fp32 oracle differs outside them: %s" %
                  (g, p, len(a), len(b), len(r["matches"]), share, _match_differs(o, r["matches"], r["amb_rows"])))
            assert share <= K.AMB_CAP and not _match_differs(o, r["matches"], r["amb_rows"])
            m = dict(r["matches"])
            if len(a) >= 31 and len(b) >= 31:
                assert m.get(4) == 3 and m.get(2) == 8 and 9 not in m                  # duplicates: the first copy, on both sides
                assert m.get(7) == 21 and r["d32"][7, 21] < 1e-3                         # identical pair
                assert abs(r["d"][6, 20] - 2.0) < 1e-6 and 6 not in m                              # antipodal pair: d = 2
                assert m.get(12) == 14 and 13 not in m and 14 not in m                   # one ulp below thr / at thr / one ulp above
                t32 = F32(K.MATCH_THR)
                assert (r["d32"][12, 14], r["d32"][13, 15], r["d32"][14, 16]) == (np.nextafter(t32, F32(0)), t32, np.nextafter(t32, F32(2)))
                assert m.get(15) == 17 and r["d32"][15, 17] == 0                         # dot above 1: the clip
                assert not r["amb_rows"][[2, 4, 7, 12, 13, 14, 15]].any()
            for kind in ("one_way", "le", "last_index", "no_clip"):
                if _match_differs(_match_fp32(a, b, K.MATCH_THR, kind), r["matches"], r["amb_rows"]):
                    rejected.add(kind)
    assert rejected == {"one_way", "le", "last_index", "no_clip"}, rejected


@pytest.mark.parametrize("case", [c[0] for c in MATCH_CASES if c[0] != "cap"])
def test_match_restatement_reproduces_g15(case):
    name, seed, n1, n2, thr = next(c for c in MATCH_CASES if c[0] == case)
    ref = G.load("g15_match_cases.npz")[name + "/matches"]
    d1, d2 = match_case_inputs(name, seed, n1, n2)
    r = R.match_two_way(d1.T, d2.T, thr)
    amb = r["amb_rows"]
    assert not _match_differs([(int(i), int(j)) for i, j, _ in ref], r["matches"], amb)
    if n1 and n2:
        assert amb.mean() <= K.AMB_CAP
        for i, j, s in ref:
            assert abs(s - r["d"][int(i), int(j)]) <= r["delta"][int(i), int(j)], (i, j, s)
