"""GPU: the read-out kernels (csrc/export_kernels.hip.h: homoadapt_views, flatten_detection, combine_heatmap, nms_*, soft-argmax;
csrc/describe_kernels.hip.h: sample_desc, match_dist, match_compact) element by element against the fp64 restatement
tests/readout_ref.py, on the inputs of tests/readout_cases.py.

  views, masks   |view - ref| <= 2 e_ref + 2^-23 (e_ref: the fp32 oracle's deviation from the restatement on the same case), exactly 0
                 beyond the padding, masks equal outside the tie band; with the horizon inside the frame only pixels with
                 |sw| >= 2^-10 are compared, and every output is finite, every mask value 0 or 1
  flatten        NCHW (the public operator) and NHWC + bnPb affine (Engine.detector_heatmap after an eval forward, teacher-forced from
                 the stored raw convPb output and its scale / shift): |p - ref| <= tau base; with a mask: bit-equal to heat * mask
  combine        NaN exactly where the restatement has b == 0, outside the near-tie set; |out b_ref - a_ref| <= tau (base_a + |out| base_b)
  points         nms_dist 0, 9 and 16 (above 8 nms_points_kernel decides alone) bit-exact against cpu_ref.get_pts_from_heatmap; the
                 batched launch of Engine.describe_points bit for bit equal to single calls
  soft-argmax    |s - ref| <= tau base, NaN where the restatement has NaN (a patch of zeros)
  sampling       NCHW (the operator) and the slot's NHWC rows (describe_points): |d - ref| <= tau base, NaN rows where the sample lies wholly
                 in the padding, rows past the count untouched, a count above cap clamped
  matching       indices exact outside the ambiguous rows, scores within the propagated dot-product bound, crafted rows decided exactly

tau = 4 x the worst ratio measured on the MI355X (readout_cases.MEASURED, profiles/readout_exact_measure.txt); every figure is printed
before it is asserted.  tests/test_readout_ref_cpu.py pins the restatement and caps the shares left out."""
import numpy as np
import pytest
import torch

from oracle import cpu_ref as C
from tests import readout_cases as K
from tests import readout_ref as R
from tests.gate_util import _dev

pytestmark = pytest.mark.gpu
F32 = np.float32
ARCH = "SuperPointNet_gauss2"


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _note(family, case, ratio):
    print("MEASURE %-13s %-34s %.4e  (tau %.3e)" % (family, case, ratio, K.TAU[family]))
    assert ratio <= K.TAU[family], (family, case, ratio, K.TAU[family])


# ------------------------------------------------------------------------------------------------ 1 views and masks
@pytest.mark.parametrize("name", ("n7", "n4", "n3", "n1", "horizon"))
@pytest.mark.parametrize("shape", K.SHAPES)
def test_views_and_masks(shape, name):
    from semantic_superpoint_amd import lib as L
    H, W = shape
    for kind in K.VIEW_KINDS:
        r = K.views_reference(H, W, name, kind)
        views, masks = L.op_homoadapt_views(t(r["img"]).to(_dev()), t(r["inv"]))
        v, m = views.cpu().numpy()[:, 0], masks.cpu().numpy()[:, 0]
        assert v.shape == r["views"].shape and np.isfinite(v).all() and np.isin(m, (0.0, 1.0)).all()
        cmp_ = r["compared"]
        err, bound = float(np.abs(v - r["views"])[cmp_].max()), 2 * r["e_ref"] + 2.0 ** -23
        bad = (m != r["masks"]) & cmp_ & ~r["band"]
        print("MEASURE views         %dx%d %-8s %-5s e_ref %.3e  kernel %.3e  bound %.3e  mask mismatches outside the band %d, inside %d" %
              (H, W, name, kind, r["e_ref"], err, bound, int(bad.sum()), int(((m != r["masks"]) & r["band"]).sum())))
        assert err <= bound, (name, kind, err, bound)
        assert not v[r["far_beyond"]].any(), (name, kind)
        assert not bad.any(), (name, kind, np.argwhere(bad)[:5])


# ------------------------------------------------------------------------------------------------ 2 flatten
@pytest.mark.parametrize("scale", (1.0, 30.0))
@pytest.mark.parametrize("nhw", K.FLATTEN_SHAPES)
def test_flatten_public_nchw(nhw, scale):
    from semantic_superpoint_amd import lib as L
    n, Hc, Wc = nhw
    semi, mask = K.flatten_case(n, Hc, Wc, scale)
    ref, base = R.flatten(semi)
    d = t(semi).to(_dev())
    heat = L.op_flatten_detection(d)
    _note("flatten_nchw", "n %d %dx%d scale %g" % (n, Hc, Wc, scale), float((np.abs(heat.cpu().numpy()[:, 0] - ref) / base).max()))
    dm = t(mask).to(_dev())
    masked = L.op_flatten_detection(d, dm)
    assert torch.equal(masked, heat * dm) and not masked[dm == 0].any() and bool((dm == 0).any())


def _flatten_state(variant):
    sd = {k: np.array(v) for k, v in C.init_state_dict(ARCH, seed=5).items()}
    if variant == "large":
        sd["bnPb.weight"] = sd["bnPb.weight"] * F32(200)
    elif variant == "dustbin":
        sd["bnPb.bias"][64] += F32(40)
    elif variant == "equal":
        sd["bnPb.weight"][:] = 0
        sd["bnPb.bias"][:] = F32(0.7)
    return sd


@pytest.mark.parametrize("variant", ("plain", "large", "dustbin", "equal"))
@pytest.mark.parametrize("nhw", K.FLATTEN_SHAPES)
def test_flatten_engine_nhwc_affine(nhw, variant):
    """the form ssp_export_points, ssp_describe_points and ssp_detector_heatmap launch: NHWC logits with the bnPb affine applied
    inside the kernel.  Variants of the bnPb parameters: as drawn, gamma x 200 (logits of ~100: the max subtraction), the dustbin's beta + 40, gamma 0
    (65 equal logits in every cell)."""
    from semantic_superpoint_amd.lib import Engine
    n, Hc, Wc = nhw
    H, W = 8 * Hc, 8 * Wc
    e = Engine(ARCH, n, H, W, _dev(), with_grad=False)
    e.load_state_dict(_flatten_state(variant))
    x = t(np.random.RandomState(n + Hc).uniform(0, 1, (n, 1, H, W)).astype(F32)).to(_dev())
    e.forward(x, slot=0, train=False, want=())
    heat = e.detector_heatmap(0, n, H, W).cpu().numpy()[:, 0]
    y = e.debug_buffer(0, "Y9", (n, Hc, Wc, 80)).cpu().numpy().astype(np.float64)[..., :65]
    sc, sh = (e.debug_buffer(0, nm, (65,)).cpu().numpy().astype(np.float64) for nm in ("scale9", "shift9"))
    logits = (y * sc + sh).transpose(0, 3, 1, 2)
    ref, base = R.flatten(logits, mag=(np.abs(y * sc) + np.abs(sh)).transpose(0, 3, 1, 2))
    print("flatten nhwc %s: logits in [%.3g, %.3g], largest p %.3g" % (variant, logits.min(), logits.max(), ref.max()))
    if variant == "equal":
        assert np.abs(ref - 1 / 65.0).max() < 1e-12
    if variant == "dustbin":
        assert ref.max() < 1e-12
    if variant == "large":
        assert np.abs(logits).max() > 30
    _note("flatten_nhwc", "n %d %dx%d %s" % (n, Hc, Wc, variant), float((np.abs(heat - ref) / base).max()))


# ------------------------------------------------------------------------------------------------ 3 combine
@pytest.mark.parametrize("n", K.COMBINE_N)
@pytest.mark.parametrize("shape", K.SHAPES)
def test_combine(shape, n):
    from semantic_superpoint_amd import lib as L
    H, W = shape
    r = K.combine_reference(H, W, n)
    hm = t(r["heat"] * r["mask"])[:, None].to(_dev())
    out = L.op_combine_heatmap(hm, t(r["mask"])[:, None].to(_dev()), t(r["unwarp"])).cpu().numpy()
    bad = K.combine_nan_mismatch(out, r)
    print("combine %dx%d n %d: NaN pixels %d (restatement %d), near-tie set %d, NaN mismatches outside it %d" %
          (H, W, n, int(np.isnan(out).sum()), int((r["b"] == 0).sum()), int(r["near"].sum()), int(bad.sum())))
    assert not bad.any(), np.argwhere(bad)[:5]
    assert not np.isinf(out).any()
    _note("combine", "%dx%d n %d" % (H, W, n), float(K.combine_ratio(out, r).max()))


# ------------------------------------------------------------------------------------------------ 4 points
def _oracle_pts(hm, thr, dist, border):
    return C.get_pts_from_heatmap(hm, F32(thr), dist, border).T


@pytest.mark.parametrize("case", [c[0] for c in K.point_maps()])
def test_points_bit_exact(case):
    """(x, y, conf) and their order equal to the sequential oracle for nms_dist 0, 9 and 16, borders 0 and 3; top_k = 1 and above the
    count; border_remove = 0 with subpixel: the refined coordinates within the soft-argmax bound of the restatement."""
    from semantic_superpoint_amd import lib as L
    name, hm, thr = next(c for c in K.point_maps() if c[0] == case)
    d = t(hm).to(_dev())
    for dist in (0, 9, 16):
        for border in (0, 3):
            ref = _oracle_pts(hm, thr, dist, border)
            mine = L.op_heatmap_points(d, thr, dist, border)
            assert mine.shape == ref.shape and np.array_equal(mine, ref), (name, dist, border, mine.shape, ref.shape)
        ref = _oracle_pts(hm, thr, dist, 0)
        assert len(ref) >= 1
        assert np.array_equal(L.op_heatmap_points(d, thr, dist, 0, top_k=1), ref[:1]), (name, dist)
        assert np.array_equal(L.op_heatmap_points(d, thr, dist, 0, top_k=len(ref) + 5), ref), (name, dist)
        sub = L.op_heatmap_points(d, thr, dist, 0, subpixel=True)
        assert sub.shape == ref.shape and np.array_equal(sub[:, 2], ref[:, 2])
        worst = 0.0
        for p, q in zip(sub, ref):
            sx, sy, bx, by = R.soft_argmax5(hm, q[0], q[1])
            if np.isnan(sx):
                assert np.isnan(p[0]) and np.isnan(p[1])
                continue
            worst = max(worst, abs(p[0] - q[0] + 2 - sx) / bx, abs(p[1] - q[1] + 2 - sy) / by)
        _note("soft_argmax", "%s nms %d" % (name, dist), worst)


@pytest.mark.parametrize("dist", (0, 4, 9))
def test_points_batched_equals_single(dist):
    """Engine.describe_points over 3 images (blockIdx.y = image, points_work_of) == op_heatmap_points on each image of
    detector_heatmap, bit for bit in (x, y, conf, sx, sy): x + sx - 2 is exact in float64, so equal sums are equal offsets."""
    from semantic_superpoint_amd import lib as L
    from semantic_superpoint_amd.lib import Engine, points_to_numpy
    n, H, W = 3, 40, 72
    e = Engine(ARCH, n, H, W, _dev(), with_grad=False)
    e.load_state_dict(C.init_state_dict(ARCH, seed=6))
    x = t(np.random.RandomState(3).uniform(0, 1, (n, 1, H, W)).astype(F32)).to(_dev())
    e.forward(x, slot=0, train=False, want=())
    heat = e.detector_heatmap(0, n, H, W)
    thr = float(heat.median())
    out = e.describe_points(0, n, conf_thresh=thr, nms_dist=dist, subpixel=True, border_remove=0)
    counts = out["count"].cpu().numpy()
    assert (counts > 0).all()
    for i in range(n):
        single = L.op_heatmap_points(heat[i, 0].contiguous(), thr, dist, 0, 0, True)
        batched = points_to_numpy(out["pts"][i], out["count"][i:i + 1], True)
        assert batched.shape == single.shape and np.array_equal(batched, single, equal_nan=True), (dist, i)
        ref = _oracle_pts(heat[i, 0].cpu().numpy(), thr, dist, 0)
        assert np.array_equal(points_to_numpy(out["pts"][i], out["count"][i:i + 1], False), ref), (dist, i)
    print("batched points nms %d: counts %s" % (dist, counts.tolist()))


# ------------------------------------------------------------------------------------------------ 5 soft-argmax
def test_soft_argmax_points():
    from semantic_superpoint_amd import lib as L
    heat, xy = K.soft_argmax_case()
    out = L.op_soft_argmax_points(t(heat).to(_dev()), t(xy).to(_dev())).cpu().numpy().astype(np.float64)
    ref = np.array([R.soft_argmax5(heat, x, y) for x, y in xy])
    nan = np.isnan(ref[:, 0])
    assert nan.sum() == 1 and np.array_equal(np.isnan(out[:, 0]), nan) and np.array_equal(np.isnan(out[:, 1]), nan)
    ratio = np.abs(out - ref[:, :2])[~nan] / ref[:, 2:][~nan]
    for i in np.argsort(-ratio.max(axis=1))[:3]:
        print("soft-argmax point %s: ratio %.3e" % (xy[~nan][i].tolist(), ratio[i].max()))
    _note("soft_argmax", "crafted patches, %d points" % len(xy), float(ratio.max()))


# ------------------------------------------------------------------------------------------------ 6 sparse descriptors
SENTINEL = 777.25


@pytest.mark.parametrize("over", (0, 7))
@pytest.mark.parametrize("hw", K.SAMPLE_SHAPES)
def test_sample_public_nchw(hw, over):
    """counts (cap + over, 5, 0): a count above cap is clamped; the output starts as a sentinel and rows past the count keep it"""
    from semantic_superpoint_amd import lib as L
    Hc, Wc = hw
    desc, xy = K.sample_case(Hc, Wc)
    cap = xy.shape[1]
    counts = np.array([cap + over, 5, 0], np.int32)
    lib = L.load_library()
    dev = _dev()
    d, q, c = t(desc).to(dev), t(xy).to(dev), t(counts).to(dev)
    out = torch.full((3, cap, 256), SENTINEL, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        assert lib.ssp_op_sample_descriptors(L._ptr(d), 3, Hc, Wc, L._ptr(q), L._ptr(c), cap, L._ptr(out), L._stream()) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    worst, nan_rows = 0.0, 0
    for b in range(3):
        k = min(int(counts[b]), cap)
        assert (got[b, k:] == F32(SENTINEL)).all(), b
        if k == 0:
            continue
        ref, base = R.sample_desc(desc[b], xy[b, :k])
        nan = np.isnan(ref).any(axis=1)
        nan_rows += int(nan.sum())
        assert np.array_equal(np.isnan(got[b, :k]), np.isnan(ref)), b
        worst = max(worst, float((np.abs(got[b, :k] - ref) / base)[~nan].max()))
    assert nan_rows >= 4
    _note("sample_nchw", "%dx%d counts %s" % (Hc, Wc, counts.tolist()), worst)


@pytest.mark.parametrize("hw", K.SAMPLE_SHAPES)
def test_sample_slot_nhwc(hw):
    """the launch of ssp_describe_points: the slot's NHWC descriptor rows, points read from rows of 5 floats; teacher-forced from the stored
    normalised descriptor and the points the call itself returned (border_remove = 0: corners and edges are among them)"""
    from semantic_superpoint_amd.lib import Engine
    Hc, Wc = hw
    n, H, W = 3, 8 * Hc, 8 * Wc
    e = Engine(ARCH, n, H, W, _dev(), with_grad=False)
    e.load_state_dict(C.init_state_dict(ARCH, seed=7))
    x = t(np.random.RandomState(Hc).uniform(0, 1, (n, 1, H, W)).astype(F32)).to(_dev())
    e.forward(x, slot=0, train=False, want=())
    thr = float(e.detector_heatmap(0, n, H, W).median())
    out = e.describe_points(0, n, conf_thresh=thr, nms_dist=1, subpixel=True, border_remove=0)
    desc = e.debug_buffer(0, "desc", (n, Hc, Wc, 256)).cpu().numpy().transpose(0, 3, 1, 2)
    counts, pts, got = out["count"].cpu().numpy(), out["pts"].cpu().numpy(), out["desc"].cpu().numpy()
    worst, edge = 0.0, 0
    for b in range(n):
        k = int(counts[b])
        assert k > 20
        xy = pts[b, :k, :2]
        edge += int(((xy[:, 0] == 0) | (xy[:, 0] == W - 1) | (xy[:, 1] == 0) | (xy[:, 1] == H - 1)).sum())
        ref, base = R.sample_desc(desc[b], xy)
        assert np.isfinite(ref).all() and np.isfinite(got[b, :k]).all()
        worst = max(worst, float((np.abs(got[b, :k] - ref) / base).max()))
    assert edge > 0
    _note("sample_nhwc", "%dx%d, %d points, %d on the image's edge" % (Hc, Wc, int(counts.sum()), edge), worst)


# ------------------------------------------------------------------------------------------------ 7 matching
@pytest.mark.parametrize("g", range(len(K.MATCH_SIZES)))
def test_match_two_way(g):
    """3 pairs per call at pair_stride 2, cap 131 above every count, sizes around the 32 / 64 tile edges; NaN in every row past the
    counts and in the skipped entries, whose counts exceed cap"""
    from semantic_superpoint_amd import lib as L
    d1, d2, c1, c2, pairs = K.match_tensors(K.MATCH_SIZES[g], g)
    dev = _dev()
    match, nm = L.op_match_two_way(t(d1).to(dev), t(c1).to(dev), t(d2).to(dev), t(c2).to(dev), K.MATCH_THR, pair_stride=2, n_pairs=3)
    match, nm = match.cpu().numpy(), nm.cpu().numpy()
    for p, (a, b) in enumerate(pairs):
        r = R.match_two_way(a, b, K.MATCH_THR)
        rows = match[p, :int(nm[p])].astype(np.float64)
        assert np.isfinite(rows).all() and np.all(np.diff(rows[:, 0]) > 0)
        amb = r["amb_rows"]
        mine = {int(i): int(j) for i, j, _ in rows}
        assert all(0 <= i < len(a) and 0 <= j < len(b) for i, j in mine.items())
        ours = {i: j for i, j in mine.items() if not amb[i]}
        theirs = {i: j for i, j in r["matches"] if not amb[i]}
        worst = max([abs(s - r["d"][int(i), int(j)]) / r["delta"][int(i), int(j)] for i, j, s in rows if r["delta"][int(i), int(j)] > 0] or [0.0])
        print("match group %d pair %d (%d x %d): %d matches (restatement %d), ambiguous rows %d, largest score deviation / bound %.3f" %
              (g, p, len(a), len(b), len(rows), len(r["matches"]), int(amb.sum()), worst))
        assert amb.mean() <= K.AMB_CAP
        assert ours == theirs, (p, sorted(set(ours.items()) ^ set(theirs.items()))[:6])
        for i, j, s in rows:
            assert abs(s - r["d"][int(i), int(j)]) <= r["delta"][int(i), int(j)], (p, i, j, s)
            if r["exact"][int(i), int(j)]:   # an exact dot product: the reference's fp32 distance, bit for bit
                assert F32(s) == r["d32"][int(i), int(j)], (p, i, j, s, r["d32"][int(i), int(j)])
        if len(a) >= 31 and len(b) >= 31:
            score = {int(i): s for i, _, s in rows}
            assert mine.get(4) == 3 and mine.get(2) == 8 and 9 not in mine                 # duplicates: the first copy
            assert mine.get(7) == 21 and 6 not in mine                                     # identical / antipodal pair
            assert mine.get(12) == 14 and 13 not in mine and 14 not in mine                # one ulp below / at / one ulp above the threshold
            assert F32(score[12]) == np.nextafter(F32(K.MATCH_THR), F32(0))
            assert mine.get(15) == 17 and score[15] == 0.0                                 # dot above 1: the clip

