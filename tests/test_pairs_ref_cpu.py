"""CPU: pins tests/pairs_ref.py, the plain restatement the device pair feed is compared with (tests/test_gpu_pairs_exact.py),
against the reference's arrays (G7, G11), the oracle, hand-written vectors and scipy - and shows that the pixels and matrices
the GPU tests may leave out (tie bands, small decision margins, near-integer class values) stay inside their caps for the
seeds and shapes those tests use (tests/pairs_cases.py).  The shares are printed."""
import math

import numpy as np
import pytest
import torch

from oracle import cpu_ref as C
from tests import golden_util as G
from tests import pairs_cases as K
from tests import pairs_ref as R


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _oracle_points(pts, hn, H, W):
    """warped coordinates in the reference's own fp32 operations: the oracle's warp_points on the host-scaled pixel matrix.
    pairs_ref.warp_points32 restates that operation order without torch (torch's matrix product may differ in the last bit on
    another CPU); every caller of this helper thereby pins it bit for bit: G11's matrices and all label cases of the GPU tests."""
    from semantic_superpoint_amd import lib as L
    hpx = L.scaled_homographies(t(hn).view(1, 3, 3), H, W)[0]
    wp = C.warp_points(t(pts), hpx).numpy()
    assert len(pts) >= 12 and np.array_equal(R.warp_points32(hpx.numpy(), pts), wp)
    return wp


# ------------------------------------------------------------------------------------------------ image warps
def test_fp64_warp_reproduces_g7():
    """G7 holds inv_warp_image_batch / compute_valid_mask (erosion 0) of the real reference in fp32.
    mask: no pixel of G7 lies in the tie band, so the fp64 nearest warp must reproduce it exactly.
    warped: the fixture was computed from fp32 coordinates that stray from the fp64 ones by at most d (measured with the
    fixed-order fp32 form; another fp32 order is allowed twice that) - a coordinate error d moves a bilinear value by at most
    d (|dI/dx| + |dI/dy|) <= 2 d (max - min of the image) - plus the roundings of four products and three sums of values
    below 1 held in fp32 (8 * 2^-24).  Bound = 2 d * 2 (max - min) + 2^-21."""
    g = G.load("g7_warps.npz")
    inv = torch.inverse(t(g["H"])).numpy()
    H, W = g["img"].shape[2:]
    tau, far = K.nearest_tau(inv, H, W)
    assert far < 0.25
    worst = 0.0
    for b in range(inv.shape[0]):
        assert not R.tie_band(inv[b], H, W, tau).any()
        assert np.array_equal(R.warp_nearest64(np.ones((H, W)), inv[b]), g["mask"][b].astype(np.float64)), b
        w, _ = R.warp_bilinear64(g["img"][b, 0], inv[b])
        d = R.coord_deviation(inv[b], H, W)[0]
        bound = 2 * d * 2 * float(g["img"][b].max() - g["img"][b].min()) + 2.0 ** -21
        err = float(np.abs(w - g["warped"][b, 0]).max())
        worst = max(worst, err)
        assert err <= bound, (b, err, bound)
    print("G7: tau %.3g, 0 pixels in the tie band, bilinear fp64 vs fixture %.3g" % (tau, worst))


@pytest.mark.parametrize("shape", K.SHAPES)
def test_nearest_restatement_matches_oracle_outside_the_tie_band(shape):
    """C.inv_warp_image_batch(mode="nearest") on integer images == the fp64 restatement wherever the fp64 coordinate is
    farther than tau from a tie; the band holds at most 0.5 % of each case's pixels (the cap of the GPU test)."""
    H, W = shape
    for name, inv in K.warp_cases(H, W).items():
        tau, far = K.nearest_tau(inv, H, W)
        assert far < 0.25, (name, far)    # a pixel whose fp64 source is outside [-1, W] x [-1, H] cannot round into the image
        band = np.stack([R.tie_band(inv[b], H, W, tau) for b in range(K.BATCH)])
        print("nearest %dx%d %-22s tau %.3g  band share %.5f  coordinate distance beyond the image %.3g" % (H, W, name, tau, band.mean(), far))
        assert band.mean() <= K.BAND_CAP, name
        for kind in ("classes", "ones"):
            img = K.images(kind, H, W)
            o = C.inv_warp_image_batch(t(img), t(inv), mode="nearest").numpy()[:, 0]
            ref = np.stack([R.warp_nearest64(img[b, 0], inv[b]) for b in range(K.BATCH)])
            assert np.array_equal(o[~band], ref[~band]), (name, kind)


@pytest.mark.parametrize("shape", K.SHAPES)
def test_bilinear_restatement_and_class_shares(shape):
    """The fp32 oracle stays close to the fp64 bilinear restatement (e_ref, printed: what the GPU test scales its bound with),
    pixels beyond the padding are exactly 0 in both, and for the WARP seeds at most 1 % of the pixels are valid and within
    2 e_ref of an integer class value (the chain case of op_sem_finalize)."""
    H, W = shape
    for name, inv in K.warp_cases(H, W).items():
        for kind in ("noise", "ramp", "corners", "classes"):
            img = K.images(kind, H, W)
            o = C.inv_warp_image_batch(t(img), t(inv)).numpy()[:, 0]
            ref, beyond = zip(*[R.warp_bilinear64(img[b, 0], inv[b]) for b in range(K.BATCH)])
            ref, beyond = np.stack(ref), np.stack(beyond)
            e_ref = float(np.abs(o - ref).max())
            scale = float(np.abs(img).max())
            # fp32 coordinates off by ~1e-5 .. 1e-4 pixels times a gradient of at most 2 * scale per pixel
            assert e_ref <= 1e-3 * scale, (name, kind, e_ref)
            tau, far = K.nearest_tau(inv, H, W)
            far_beyond = beyond & np.stack([_beyond_by(inv[b], H, W, max(tau, 2 * far)) for b in range(K.BATCH)])
            assert not o[far_beyond].any()
            line = "bilinear %dx%d %-22s %-8s e_ref %.3g" % (H, W, name, kind, e_ref)
            if kind == "classes" and name.startswith("warp"):
                vm = np.stack([R.erode(R.warp_nearest64(np.ones((H, W)), inv[b]), 3) for b in range(K.BATCH)])
                near = (np.abs(ref - np.rint(ref)) <= 2 * e_ref) & (vm != 0)
                line += "  valid pixels within 2 e_ref of an integer: %.5f" % near.mean()
                assert near.mean() <= K.SEM_CAP, name
            print(line)


def _beyond_by(inv_h, H, W, tau):
    """pixels whose fp64 source is more than tau beyond the zero padding (x < -1 - tau, x > W + tau, likewise y); tau = twice
    the fp32 - fp64 coordinate distance, so an fp32 evaluation in any valid order puts them beyond the padding too"""
    ix, iy, _ = R.source_coords64(inv_h, H, W)
    return (ix < -1 - tau) | (ix > W + tau) | (iy < -1 - tau) | (iy > H + tau)


# ------------------------------------------------------------------------------------------------ erosion
def test_ellipse_hand_vectors():
    """OpenCV's row formula for a (2r, 2r) element: rows i = 0 .. 2r - 1, dy = i - r, dx = round(r sqrt(1 - dy^2 / r^2)),
    columns r - dx .. r + dx clipped to [0, 2r).
      r = 1: dy = -1: dx = 0 -> column 1;          dy = 0: dx = 1 -> columns 0..2 clipped to 0..1
      r = 2: dy = -2: dx = 0 -> column 2;          dy = -1, 1: 2 sqrt(3/4) = 1.73 -> 2 -> columns 0..3;   dy = 0: dx = 2
      r = 3: dy = -3: dx = 0 -> column 3;          dy = -2, 2: 3 sqrt(5/9) = 2.24 -> 2 -> columns 1..5;
             dy = -1, 1: 3 sqrt(8/9) = 2.83 -> 3 -> columns 0..5;                                          dy = 0: dx = 3
    The element is NOT symmetric: the row dy = -r exists, the row dy = +r does not, and column 0 is only reached where dx = r."""
    rows = lambda s: np.array([[int(c) for c in r] for r in s.split("/")], np.uint8)  # noqa: E731
    assert np.array_equal(R.ellipse(2), rows("01/11"))
    assert np.array_equal(R.ellipse(4), rows("0010/1111/1111/1111"))
    assert np.array_equal(R.ellipse(6), rows("000100/011111/111111/111111/111111/011111"))
    assert np.array_equal(R.ellipse(5, 5), rows("00100/11111/11111/11111/00100"))   # the element OpenCV's tutorial prints
    assert np.array_equal(C.structuring_element_ellipse(5, 5), rows("00100/11111/11111/11111/00100"))
    for r in range(1, 9):
        assert np.array_equal(R.ellipse(2 * r), C.ellipse_kernel(r)), r


def test_erosion_matches_oracle_and_scipy():
    rs = np.random.RandomState(7)
    masks = [(rs.uniform(0, 1, (23, 31)) > 0.05).astype(np.float32), (rs.uniform(0, 1, (9, 40)) > 0.2).astype(np.float32),
             rs.uniform(0, 1, (17, 12)).astype(np.float32)]
    for r in range(0, 9):
        for m in masks:
            assert np.array_equal(R.erode(m, r), C.erode_ellipse(t(m), r).numpy()), r
    ndi = pytest.importorskip("scipy.ndimage")
    for r in range(1, 9):
        for m in masks:
            ref = ndi.grey_erosion(m.astype(np.float64), footprint=R.ellipse(2 * r), mode="constant", cval=np.inf)
            assert np.array_equal(R.erode(m, r).astype(np.float64), ref), r


def test_kernel_fp32_ellipse_rows_equal_fp64():
    """erode_ellipse_kernel evaluates lrintf(r * sqrtf((r*r - dy*dy) / (r*r))) in fp32: the same dx as OpenCV's fp64 form
    for every radius up to 16 (the trainer uses 3)."""
    for r in range(1, 17):
        assert R.ellipse_rows_dx_kernel32(r) == R.ellipse_rows_dx(r), r


# ------------------------------------------------------------------------------------------------ label scatter
def test_label_scatter_restatement_matches_g11_and_oracle():
    g = G.load("g11_pair_labels.npz")
    for k in range(3):
        H, W = g["labels%d" % k].shape[1:]
        lab = np.zeros((H, W), np.float32)
        pts = g["pts%d" % k].astype(np.int64)
        lab[pts[:, 1], pts[:, 0]] = 1
        pts = R.map_points(lab)
        lab_r, res_r, bi_r, c_res, c_bi = R.warp_labels_full(_oracle_points(pts, g["H%d" % k], H, W), H, W)
        assert c_res == 0 and c_bi == 0                          # G11 has no collisions
        assert np.array_equal(lab_r, g["labels%d" % k][0]) and np.array_equal(res_r, g["res%d" % k]), k
        assert np.array_equal(bi_r, g["bi%d" % k][0]), k
        o_lab, o_res, o_bi = C.warp_labels_full(t(pts), H, W, t(g["H%d" % k]))
        assert np.array_equal(lab_r, o_lab.numpy()[0]) and np.array_equal(res_r, o_res.numpy()) and np.array_equal(bi_r, o_bi.numpy()[0])


def test_label_scatter_hand_made_collision():
    """Three points, warped coordinates given directly (x, y), map 4 x 6, in row-major order of the source map:
         p0 -> (2.25, 1.25)   truncates to (2, 1), rounds to (2, 1)
         p1 -> (1.75, 1.50)   truncates to (1, 1), rounds to (2, 2)     (1.5 -> 2, half to even)
         p2 -> (2.40, 0.75)   truncates to (2, 0), rounds to (2, 1)
       labels / res: pixel (2, 1) is claimed by p0 and p2 -> p2, the later point, wins: res = (0.40, -0.25); (2, 2) is p1's.
       labels_bi, lists in the order (x, y), (x, y+1), (x+1, y), (x+1, y+1):
         pixel (2, 1): list 0 of p0, list 1 of p2, list 2 of p1                  -> list 2 wins: p1's rx (1 - ry) = 0.75 * 0.5
         pixel (2, 2): list 1 of p0, list 3 of p1                                -> list 3: p1's rx ry = 0.75 * 0.5
         pixel (3, 1): list 2 of p0, list 3 of p2                                -> list 3: p2's rx ry = 0.4 * 0.75
         pixel (3, 2): list 3 of p0 only: 0.25 * 0.25;  (1, 1): list 0 of p1: 0.25 * 0.5;  (1, 2): list 1 of p1: 0.25 * 0.5
         pixel (2, 0): list 0 of p2: 0.6 * 0.25;        (3, 0): list 2 of p2: 0.4 * 0.25"""
    f = np.float32
    wp = np.array([[2.25, 1.25], [1.75, 1.5], [2.4, 0.75]], f)
    lab, res, bi, c_res, c_bi = R.warp_labels_full(wp, 4, 6)
    exp_lab = np.zeros((4, 6), f)
    exp_lab[1, 2] = exp_lab[2, 2] = 1
    assert np.array_equal(lab, exp_lab) and c_res == 1 and c_bi == 3
    rx2 = f(2.4) - f(2)
    assert res[0, 1, 2] == rx2 and res[1, 1, 2] == f(-0.25) and res[0, 2, 2] == f(-0.25) and res[1, 2, 2] == f(-0.5)
    assert np.count_nonzero(res) == 4
    one = f(1)
    exp_bi = np.zeros((4, 6), f)
    exp_bi[1, 2] = f(0.75) * f(0.5)
    exp_bi[2, 2] = f(0.75) * f(0.5)
    exp_bi[1, 3] = rx2 * f(0.75)
    exp_bi[2, 3] = f(0.25) * f(0.25)
    exp_bi[1, 1] = f(0.25) * f(0.5)
    exp_bi[2, 1] = f(0.25) * f(0.5)
    exp_bi[0, 2] = (one - rx2) * f(0.25)
    exp_bi[0, 3] = rx2 * f(0.25)
    assert np.array_equal(bi, exp_bi)


@pytest.mark.parametrize("shape", K.SHAPES)
def test_label_scatter_cases_collide(shape):
    """Every 5 % map of the GPU test has collisions in labels_bi and in res under both homographies; on the collision-free
    part the restatement equals the oracle (whose indexed assignment is only defined there)."""
    H, W = shape
    for name, hs in K.label_homographies(H, W).items():
        maps = K.keypoint_maps(H, W, seed=0)
        for b in range(K.BATCH):
            pts = R.map_points(maps[b, 0])
            lab, res, bi, c_res, c_bi = R.warp_labels_full(_oracle_points(pts, hs[b], H, W), H, W)
            print("labels %dx%d %-5s image %d: %d points, %d pixels with colliding res, %d with colliding bi" % (H, W, name, b, len(pts), c_res, c_bi))
            assert c_res > 0 and c_bi > 0, (name, b)
            o_lab, o_res, o_bi = C.warp_labels_full(t(pts), H, W, t(hs[b]))
            assert np.array_equal(lab, o_lab.numpy()[0])


# ------------------------------------------------------------------------------------------------ sampler
def test_device_stream_first_uniforms():
    """uniform() number c of stream (seed, n) is (mix(mix(seed ^ n << 32) ^ c * 0xD1342543DE82EF95) >> 11) / 2^53 with
         mix(x): x += 0x9E3779B97F4A7C15; x = (x ^ x >> 30) * 0xBF58476D1CE4E5B9; x = (x ^ x >> 27) * 0x94D049BB133111EB; x ^ x >> 31
       (mod 2^64).  (seed 0, n 0): key = mix(0) = 0xE220A8397B1DCDAF (the first output of splitmix64 seeded with 0, a
       published test vector); draw 0 = mix(key ^ 0) >> 11 and draw 1 = mix(key ^ 0xD1342543DE82EF95) >> 11 are evaluated
       below step by step with Python integers, independently of pairs_ref.mix.  (seed 7, n 3): key = mix(7 ^ 3 << 32)."""
    def mix_steps(x):
        m = (1 << 64) - 1
        x = (x + 0x9E3779B97F4A7C15) & m
        x ^= x >> 30
        x = (x * 0xBF58476D1CE4E5B9) & m
        x ^= x >> 27
        x = (x * 0x94D049BB133111EB) & m
        x ^= x >> 31
        return x
    assert mix_steps(0) == 0xE220A8397B1DCDAF == R.mix(0)
    for seed, n in ((0, 0), (7, 3)):
        key = mix_steps(seed ^ (n << 32))
        st = R.DeviceStream(seed, n)
        for c in range(3):
            want = (mix_steps(key ^ ((c * 0xD1342543DE82EF95) & ((1 << 64) - 1))) >> 11) / 2.0 ** 53
            assert st.uniform() == want and 0.0 <= want < 1.0
    assert R.DeviceStream(0, 0).uniform() == (mix_steps(0xE220A8397B1DCDAF) >> 11) / 2.0 ** 53


def test_device_stream_moments():
    """20000 normals: mean within 4 sigma / sqrt(N), variance within 4 sqrt(2 / N), P(|v| <= 2) = erf(sqrt 2) = 0.9545
    within 4 binomial deviations; randint(5) stays in range and hits every value."""
    st = R.DeviceStream(5, 1)
    v = np.array([st.randn() for _ in range(20000)])
    n = len(v)
    assert abs(v.mean()) < 4 / math.sqrt(n) and abs(v.var() - 1) < 4 * math.sqrt(2.0 / n)
    p = math.erf(math.sqrt(2.0))
    assert abs((np.abs(v) <= 2).mean() - p) < 4 * math.sqrt(p * (1 - p) / n)
    assert st.normals == n and st.ctr == 2 * n
    k = [st.randint(5) for _ in range(2000)]
    assert set(k) == {0, 1, 2, 3, 4}
    u = [st.uniform(-2.0, 3.0) for _ in range(2000)]
    assert min(u) >= -2.0 and max(u) < 3.0 and abs(np.mean(u) - 0.5) < 4 * 5 / math.sqrt(12 * 2000)


@pytest.mark.parametrize("name", sorted(K.SAMPLER_CONFIGS))
def test_sampler_reference_margins(name):
    """The oracle's geometry on the device stream for every configuration of the GPU test: at most 0.1 % of the matrices
    rest on a decision closer than 1e-9; sample_homographies itself asserts that its fp64 walk casts to the oracle's matrix."""
    hs, inv, mg = K.sampler_reference(name)
    small = float((mg < K.MARGIN_MIN).mean())
    print("sampler %-15s matrices with a margin below 1e-9: %d of %d (smallest margin %.3g)" % (name, int((mg < K.MARGIN_MIN).sum()), len(mg), mg.min()))
    assert small <= K.MARGIN_CAP
    assert np.abs(hs @ inv - np.eye(3)).max() < 1e-9
    if name == "tight":   # no artifacts: every corner of the patch stays inside the unit square
        w = inv @ np.array([[-1.0, -1, 1], [-1, 1, 1], [1, 1, 1], [1, -1, 1]]).T
        assert np.abs(w[:, :2] / w[:, 2:]).max() <= 1.0 + 1e-12
