"""GPU: the kernels of the device pair feed (csrc/pair_kernels.hip.h: image / mask / class-id warps, erosion, homography sampler,
class-id finalisation, warpLabels(bilinear=True)) against the plain restatement tests/pairs_ref.py.

Every allowance is derived on the reference side, inside the test, on the CPU:
  e_ref   largest deviation of the fp32 oracle (C.inv_warp_image_batch) from the fp64 restatement on the same inputs; the kernel
          may deviate from the fp64 restatement by 2 e_ref + 2^-23 (another equally valid fp32 operation order, no more)
  tau     twice the largest distance between the fixed-order fp32 and the fp64 source coordinates; only pixels whose fp64
          coordinate is within tau of a rounding tie are left out of the exact comparison of the nearest warp
tests/test_pairs_ref_cpu.py pins the restatement and shows that the shares left out stay inside their caps for these inputs
(tests/pairs_cases.py).  Measured figures: profiles/pairs_exact_measure.txt."""
import numpy as np
import pytest
import torch

from oracle import cpu_ref as C
from tests import pairs_cases as K
from tests import pairs_ref as R

pytestmark = pytest.mark.gpu
CASES = ("warp11", "warp13", "identity_translations", "scales_rotation", "perspective")


def _dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _beyond_by(inv_h, H, W, tau):
    ix, iy, _ = R.source_coords64(inv_h, H, W)
    return (ix < -1 - tau) | (ix > W + tau) | (iy < -1 - tau) | (iy > H + tau)


# ------------------------------------------------------------------------------------------------ 1 bilinear warp
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("shape", K.SHAPES)
def test_bilinear_warp_against_fp64(shape, case):
    """op_warp_image (bilinear) on noise, on a linear ramp (bilinear interpolation is exact on it: the coordinates alone) and on
    a bright pixel in each corner: within 2 e_ref + 2^-23 of the fp64 restatement; pixels whose source lies beyond the zero
    padding (by more than the coordinate distance) are exactly 0."""
    from semantic_superpoint_amd import lib as L
    H, W = shape
    inv = K.warp_cases(H, W)[case]
    tau, far = K.nearest_tau(inv, H, W)
    for kind in ("noise", "ramp", "corners"):
        img = K.images(kind, H, W)
        ref, beyond = zip(*[R.warp_bilinear64(img[b, 0], inv[b]) for b in range(K.BATCH)])
        ref, beyond = np.stack(ref), np.stack(beyond)
        e_ref = float(np.abs(C.inv_warp_image_batch(t(img), t(inv)).numpy()[:, 0] - ref).max())
        out = L.op_warp_image(t(img).to(_dev()), t(inv).to(_dev())).cpu().numpy()[:, 0]
        err = float(np.abs(out - ref).max())
        print("bilinear %dx%d %-22s %-8s e_ref %.3g  kernel %.3g  bound %.3g" % (H, W, case, kind, e_ref, err, 2 * e_ref + 2.0 ** -23))
        assert err <= 2 * e_ref + 2.0 ** -23, (kind, err, e_ref)
        far_beyond = beyond & np.stack([_beyond_by(inv[b], H, W, max(tau, 2 * far)) for b in range(K.BATCH)])
        assert not out[far_beyond].any(), kind


# ------------------------------------------------------------------------------------------------ 2 nearest warp
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("shape", K.SHAPES)
def test_nearest_warp_every_pixel(shape, case):
    """op_warp_image (nearest) on class ids 0..133 and on ones: every pixel farther than tau from a rounding tie equals the
    fp64 restatement; the band holds at most 0.5 % of the case's pixels."""
    from semantic_superpoint_amd import lib as L
    H, W = shape
    inv = K.warp_cases(H, W)[case]
    tau, far = K.nearest_tau(inv, H, W)
    assert far < 0.25
    band = np.stack([R.tie_band(inv[b], H, W, tau) for b in range(K.BATCH)])
    assert band.mean() <= K.BAND_CAP
    for kind in ("classes", "ones"):
        img = K.images(kind, H, W)
        ref = np.stack([R.warp_nearest64(img[b, 0], inv[b]) for b in range(K.BATCH)])
        out = L.op_warp_image(t(img).to(_dev()), t(inv).to(_dev()), nearest=True).cpu().numpy()[:, 0]
        bad = (out != ref) & ~band
        print("nearest %dx%d %-22s %-8s tau %.3g  band %.5f  mismatches outside the band %d, inside %d" %
              (H, W, case, kind, tau, band.mean(), int(bad.sum()), int(((out != ref) & band).sum())))
        assert not bad.any(), (kind, np.argwhere(bad)[:5])


# ------------------------------------------------------------------------------------------------ 3 erosion
def _erosion_masks(H, W):
    """float32 [6, 1, H, W]: one zero in the middle; zeros in the four corners; a zero on each border; 5 % random zeros (twice);
    a float-valued mask"""
    rs = np.random.RandomState(H * 1000 + W)
    m = np.ones((6, 1, H, W), np.float32)
    m[0, 0, H // 2, W // 2] = 0
    m[1, 0, 0, 0] = m[1, 0, 0, W - 1] = m[1, 0, H - 1, 0] = m[1, 0, H - 1, W - 1] = 0
    m[2, 0, 0, W // 2] = m[2, 0, H - 1, W // 3] = m[2, 0, H // 2, 0] = m[2, 0, H // 3, W - 1] = 0
    m[3, 0] = rs.uniform(0, 1, (H, W)) > 0.05
    m[4, 0] = rs.uniform(0, 1, (H, W)) > 0.05
    m[5, 0] = rs.uniform(-1, 2, (H, W))
    return m


@pytest.mark.parametrize("r", range(0, 7))
def test_erosion_exact(r):
    """op_erode == the restatement (OpenCV's ellipse rows in fp64, sliding minimum that ignores pixels outside, anchor (r, r)),
    torch.equal, including images narrower or lower than the 2r element; a single zero gives exactly the REFLECTED
    footprint (out[y, x] = min of m[y + i - r, x + j - r]: the zero at c reaches c - (i - r, j - r))."""
    from semantic_superpoint_amd import lib as L
    for (H, W) in ((40, 56), (37, 53), (5, 9), (11, 3), (1, 1)):
        m = _erosion_masks(H, W)
        out = L.op_erode(t(m).to(_dev()), r).cpu().numpy()
        ref = np.stack([R.erode(m[b, 0], r) for b in range(m.shape[0])])[:, None]
        assert out.dtype == ref.dtype and np.array_equal(out, ref), (H, W, r, np.argwhere(out != ref)[:5])
        if H >= 14 and r > 0:   # the element fits around the middle: the zeros ARE the reflected element
            k = R.ellipse(2 * r)
            exp = np.ones((H, W), np.float32)
            for i in range(2 * r):
                for j in range(2 * r):
                    if k[i, j]:
                        exp[H // 2 - (i - r), W // 2 - (j - r)] = 0
            assert np.array_equal(out[0, 0], exp), (H, W, r)


# ------------------------------------------------------------------------------------------------ 4 homography sampler
@pytest.mark.parametrize("name", sorted(K.SAMPLER_CONFIGS))
def test_sampler_against_oracle_on_device_stream(name):
    """op_sample_homographies == C.sample_homography(DeviceStream(seed, n), shape=(2, 2), shift=-1, ...) matrix by matrix:
    |dev - ref| <= 2^-23 |ref| + 1e-10 max|ref| (one fp32 rounding of the entry + fp64 round-off through an 8x8 solve), for
    every matrix whose smallest decision margin is at least 1e-9 (at most 0.1 % are left out)."""
    from semantic_superpoint_amd import lib as L
    seed, cfg = K.SAMPLER_CONFIGS[name]
    hs_ref, inv_ref, mg = K.sampler_reference(name)
    B = len(mg)
    hs, inv = L.op_sample_homographies(B, seed, _dev(), **cfg)
    keep = mg >= K.MARGIN_MIN
    assert (~keep).mean() <= K.MARGIN_CAP
    worst = 0.0
    for dev_m, ref in ((hs, hs_ref), (inv, inv_ref)):
        d = np.abs(dev_m.cpu().numpy().astype(np.float64) - ref)
        bound = 2.0 ** -23 * np.abs(ref) + 1e-10 * np.abs(ref).max(axis=(1, 2), keepdims=True)
        worst = max(worst, float((d / bound)[keep].max()))
        bad = (d > bound).any(axis=(1, 2)) & keep
        assert not bad.any(), (name, int(bad.sum()), np.argwhere(bad)[:5].ravel(), float(d[keep].max()))
    eye = torch.eye(3, device=_dev()).expand(B, 3, 3)
    assert ((hs @ inv) - eye).abs().max() < 1e-3
    print("sampler %-15s %d of %d matrices compared, largest |dev - ref| / bound %.3f" % (name, int(keep.sum()), B, worst))


def test_sampler_refuses_what_it_would_clamp():
    """the kernel holds 16 scales and 63 angles: larger requests are refused, not clamped"""
    from semantic_superpoint_amd import lib as L
    L.op_sample_homographies(4, 1, _dev(), n_scales=16, n_angles=63)
    with pytest.raises(RuntimeError, match="n_scales"):
        L.op_sample_homographies(4, 1, _dev(), n_scales=17)
    with pytest.raises(RuntimeError, match="n_angles"):
        L.op_sample_homographies(4, 1, _dev(), n_angles=64)


# ------------------------------------------------------------------------------------------------ 5 class ids
def test_sem_finalize_direct():
    """crafted floats: integers k, k + 0.999999, k - 1e-6 and 0 (as the fp32 values they become) -> truncation toward zero;
    a pixel is invalid exactly where the mask is 0 (0.5 and -1 count as valid)"""
    from semantic_superpoint_amd import lib as L
    k = np.arange(0, 134, dtype=np.float64)
    v = np.concatenate([k, k + 0.999999, k[1:] - 1e-6, [0.0, 0.999999, 1e-6]]).astype(np.float32)
    v = np.tile(v, 3)[: 3 * 400].reshape(3, 20, 20)
    valid = np.ones_like(v)
    valid[0, ::3], valid[1, :, ::2], valid[2, 5:9] = 0.0, 0.5, -1.0
    valid[1, 7] = 0.0
    out = L.op_sem_finalize(t(v).to(_dev()), t(valid).to(_dev()), 133).cpu().numpy()
    assert out.dtype == np.int64 and np.array_equal(out, R.sem_finalize(v, valid, 133))
    assert (out[valid == 0] == 133).all() and out[valid != 0].max() <= 134


@pytest.mark.parametrize("case", ("warp11", "warp13"))
@pytest.mark.parametrize("shape", K.SHAPES)
def test_sem_chain_warp_then_finalize(shape, case):
    """bilinear warp of class ids, then finalize: every valid pixel whose fp64 warped value is farther than 2 e_ref from an
    integer has the truncated fp64 value; at most 1 % of the pixels are left out; invalid pixels are exactly n_classes."""
    from semantic_superpoint_amd import lib as L
    H, W = shape
    inv = K.warp_cases(H, W)[case]
    img = K.images("classes", H, W)
    ref = np.stack([R.warp_bilinear64(img[b, 0], inv[b])[0] for b in range(K.BATCH)])
    e_ref = float(np.abs(C.inv_warp_image_batch(t(img), t(inv)).numpy()[:, 0] - ref).max())
    vm = np.stack([R.erode(R.warp_nearest64(np.ones((H, W)), inv[b]), 3) for b in range(K.BATCH)]).astype(np.float32)
    near = (np.abs(ref - np.rint(ref)) <= 2 * e_ref) & (vm != 0)
    assert near.mean() <= K.SEM_CAP
    sw = L.op_warp_image(t(img).to(_dev()), t(inv).to(_dev()))
    out = L.op_sem_finalize(sw.view(K.BATCH, H, W), t(vm).to(_dev()), 133).cpu().numpy()
    want = R.sem_finalize(ref, vm, 133)
    bad = (out != want) & ~near
    print("class ids %dx%d %s: e_ref %.3g, left out %.5f, mismatches among the left-out %d, elsewhere %d" %
          (H, W, case, e_ref, near.mean(), int(((out != want) & near).sum()), int(bad.sum())))
    assert not bad.any(), np.argwhere(bad)[:5]
    assert (out[vm == 0] == 133).all() and (vm == 0).any()


# ------------------------------------------------------------------------------------------------ 6 label scatter
def _labels_ref(maps, hs, H, W):
    """the restatement on warped coordinates in the reference's own fp32 operations: pairs_ref.warp_points32 on the host-scaled
    pixel matrix, which tests/test_pairs_ref_cpu.py pins bit for bit to the oracle's warp_points and to G11 for these very
    inputs.  torch's own matrix product on THIS host may round the last bit otherwise (test_warp_labels_full_golden): the
    number of such coordinates is printed, the pinned form is what the kernel is held to."""
    from semantic_superpoint_amd import lib as L
    hpx = L.scaled_homographies(t(hs), H, W)
    lab, res, bi, c_res, c_bi, host_differs = [], [], [], 0, 0, 0
    for b in range(maps.shape[0]):
        pts = R.map_points(maps[b, 0])
        wp = R.warp_points32(hpx[b].numpy(), pts)
        host_differs += int((C.warp_points(t(pts), hpx[b]).numpy() != wp).sum())
        o = R.warp_labels_full(wp, H, W)
        lab.append(o[0][None]), res.append(o[1]), bi.append(o[2][None])
        c_res, c_bi = c_res + o[3], c_bi + o[4]
    print("labels: %d coordinates of this host's torch product differ from the pinned fp32 order" % host_differs)
    return np.stack(lab), np.stack(res), np.stack(bi), c_res, c_bi


def _assert_labels(maps, hs, H, W, tag):
    from semantic_superpoint_amd import lib as L
    lab_r, res_r, bi_r, c_res, c_bi = _labels_ref(maps, hs, H, W)
    d = t(maps).to(_dev())
    lab, res, bi = L.op_warp_labels_full(d, t(hs))
    lab2, res2, bi2 = L.op_warp_labels_full(d, t(hs))
    assert torch.equal(lab, lab2) and torch.equal(res, res2) and torch.equal(bi, bi2), tag   # two calls: bit-identical
    n = [int((a.cpu().numpy() != b).sum()) for a, b in ((lab, lab_r), (res, res_r), (bi, bi_r))]
    print("labels %s: %d / %d pixels with colliding res / bi; differing elements labels %d res %d bi %d" % (tag, c_res, c_bi, *n))
    assert n == [0, 0, 0], (tag, n)
    return (lab, res, bi), (c_res, c_bi)


@pytest.mark.parametrize("name", ("half", "warp"))
@pytest.mark.parametrize("shape", K.SHAPES)
def test_label_scatter_with_collisions(shape, name):
    """5 % key point maps under a scale of 0.5 and under WARP: all three outputs torch.equal to the restatement whose
    winners are defined by the reference's write order, and two calls bit-identical."""
    H, W = shape
    _, (c_res, c_bi) = _assert_labels(K.keypoint_maps(H, W, seed=0), K.label_homographies(H, W)[name], H, W, "%dx%d %s" % (H, W, name))
    assert c_res > 0 and c_bi > 0


def _pixel_affine(a, tx, ty, H, W):
    """normalised homography whose pixel form T^-1 h T is [[a, 0, tx], [0, a, ty], [0, 0, 1]]: x_n = 2 x / W - 1, so
    h = [[a, 0, a - 1 + 2 tx / W], [0, a, a - 1 + 2 ty / H], [0, 0, 1]] - exact in fp32 for power-of-two sizes, dyadic a, tx, ty"""
    return np.array([[a, 0, a - 1 + 2.0 * tx / W], [0, a, a - 1 + 2.0 * ty / H], [0, 0, 1]], np.float32)


def test_label_scatter_edge_inputs():
    """32 x 64 (powers of two: the pixel homography and every warped coordinate are exact, checked below), three images:
       0: x -> x / 2 - 0.75, y -> y / 2 - 0.25: points warp into the band (-1, 0), where truncation toward zero gives 0 and the
          weights 1 - rx exceed 1; the neighbour (x, y) = (0, 0) is inside although the point is not
       1: x -> x / 2: odd coordinates land on .5 ties (half to even: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2), colliding there
       2: x -> x + 53, y -> y + 26: (10, 5) lands exactly on (W - 1, H - 1), (11, 5) and (10, 6) just outside"""
    from semantic_superpoint_amd import lib as L
    H, W = 32, 64
    hs = np.stack([_pixel_affine(0.5, -0.75, -0.25, H, W), _pixel_affine(0.5, 0, 0, H, W), _pixel_affine(1.0, 53, 26, H, W)])
    maps = np.zeros((3, 1, H, W), np.float32)
    for (x, y) in ((0, 0), (1, 0), (0, 1), (2, 1), (3, 1), (1, 2), (5, 7), (0, 9), (63, 31)):
        maps[0, 0, y, x] = 1
    for (x, y) in ((1, 1), (3, 3), (5, 5), (5, 3), (3, 5), (7, 9), (9, 7), (2, 2), (63, 31), (0, 31), (63, 0), (21, 13)):
        maps[1, 0, y, x] = 1
    for (x, y) in ((10, 5), (11, 5), (10, 6), (9, 4), (0, 0), (9, 5), (10, 4)):
        maps[2, 0, y, x] = 1
    hpx = L.scaled_homographies(t(hs), H, W).numpy()
    assert np.array_equal(hpx[0], [[0.5, 0, -0.75], [0, 0.5, -0.25], [0, 0, 1]]) and np.array_equal(hpx[2], [[1, 0, 53], [0, 1, 26], [0, 0, 1]])
    wp0 = R.warp_points32(hpx[0], R.map_points(maps[0, 0]))
    assert np.array_equal(wp0[:2], [[-0.75, -0.25], [-0.25, -0.25]])                 # the band (-1, 0)
    wp1 = R.warp_points32(hpx[1], R.map_points(maps[1, 0]))
    assert np.array_equal(wp1[:3], [[31.5, 0], [0.5, 0.5], [1, 1]])                   # .5 ties
    wp2 = R.warp_points32(hpx[2], R.map_points(maps[2, 0]))
    assert [W - 1, H - 1] in wp2.tolist() and [W, H - 1] in wp2.tolist()             # exactly on / just beyond the last pixel
    (lab, res, bi), (c_res, c_bi) = _assert_labels(maps, hs, H, W, "edge inputs")
    assert c_res > 0 and c_bi > 0
    lab, res, bi = lab.cpu().numpy(), res.cpu().numpy(), bi.cpu().numpy()
    # (0, 9) -> (-0.75, 4.25): truncated to (0, 4) with rx = -0.75, so pixel (0, 4) holds (1 + 0.75) (1 - 0.25); (2, 1) -> (0.25, 0.25)
    assert bi[0, 0, 4, 0] == 1.75 * 0.75 and lab[0, 0, 0, 0] == 1 and lab[0, 0, 4, 0] == 0
    assert lab[1, 0, 2, 2] == 1 and lab[1, 0, 0, 0] == 1 and res[1, 0, 2, 2] == 0.5   # (5, 5) -> (2.5, 2.5) -> (2, 2), after (3, 3)
    assert lab[2, 0, H - 1, W - 1] == 1 and lab[2].sum() == 5                          # (11, 5) and (10, 6) fall outside


def test_label_scatter_null_outputs():
    """any of the three maps may be NULL at the C ABI: the others do not change"""
    from semantic_superpoint_amd import lib as L
    H, W = 37, 53
    d = t(K.keypoint_maps(H, W, seed=0)).to(_dev())
    hs = t(K.label_homographies(H, W)["half"])
    full = L.op_warp_labels_full(d, hs)
    for outputs in ((True, False, False), (False, True, False), (False, False, True), (True, False, True), (False, True, True)):
        part = L.op_warp_labels_full(d, hs, outputs=outputs)
        for want, a, b in zip(outputs, part, full):
            assert (a is None) if not want else torch.equal(a, b), outputs


def test_label_scatter_refuses_maps_beyond_the_key():
    """the scatter key holds the source index in 29 bits: h * w >= 2^29 is refused before any memory is touched"""
    from semantic_superpoint_amd import lib as L
    lib = L.load_library()
    d = torch.zeros(16, device=_dev())
    assert lib.ssp_op_warp_labels_full_px(L._ptr(d), L._ptr(d), L._ptr(d), None, None, 1, 1 << 15, 1 << 14, None) != 0
    assert b"2^29" in lib.ssp_last_error()


# ------------------------------------------------------------------------------------------------ 7 make_pairs
@pytest.mark.parametrize("deterministic", (False, True))
def test_make_pairs_is_repeatable_on_dense_labels(deterministic):
    """two calls on the same dense (5 %) random label map with the same seed: every key bit-identical"""
    from semantic_superpoint_amd import lib as L
    from semantic_superpoint_amd import pairs
    H, W = 120, 160
    dev = _dev()
    img = t(K.images("noise", H, W)).to(dev)
    lab = t(K.keypoint_maps(H, W, seed=1)).to(dev)
    sem = t(K.images("classes", H, W)[:, 0]).long().to(dev)
    L.set_deterministic(deterministic)
    try:
        a = pairs.make_pairs(img, lab, seed=9, warp_params=K.WARP, erosion_radius=3, semantic=sem)
        b = pairs.make_pairs(img, lab, seed=9, warp_params=K.WARP, erosion_radius=3, semantic=sem)
    finally:
        L.set_deterministic(False)
    assert sorted(a) == sorted(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k
