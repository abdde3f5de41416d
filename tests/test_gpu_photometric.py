"""GPU: photometric augmentation on the device (csrc/photo_kernels.hip.h).  The arithmetic of
`ssp_op_photometric_apply` is tested exactly against the numpy restatement tests/photometric_ref.py on hand-made rows of
draws; the per-pixel noise and `ssp_op_photometric_draw` are tested here through their statistics (the device RNG stream differs
from numpy's by construction) and value by value in tests/test_gpu_draws_exact.py; pairs.make_pairs is tested for its three new
arguments."""
import json
import os

import numpy as np
import pytest
import torch

from tests import photometric_ref as R

pytestmark = pytest.mark.gpu
SHADE_TOL = 5e-5   # derived: two separable fp32 passes of <= 351 terms, weights summing to 1, values <= 255:
#                    351 * 2^-24 * 255 = 5.3e-3 per pass on the 255 scale, * |t| <= 0.8 / 255 = 1.7e-5 per pass, two passes


def _dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _aug(golden_dir):
    with open(os.path.join(golden_dir, "g17_photometric_config.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("hw", [(240, 320), (67, 93), (388, 16)])
def test_apply_matches_the_restatement(hw):
    """Stages 1-7 exactly (multiples of 1/255) outside the helper's tie set, which must stay under 0.1 % of the pixels and
    may differ by one level; the shade at SHADE_TOL absolute."""
    from semantic_superpoint_amd import lib as L
    H, W = hw
    img = R.case_image(H, W)
    cases = R.exact_cases(H, W)
    rows = torch.from_numpy(np.stack([r for _, r in cases])).to(_dev())
    x = torch.from_numpy(img).view(1, 1, H, W).repeat(len(cases), 1, 1, 1).contiguous().to(_dev())
    got = L.op_photometric_apply(x, rows).cpu().numpy()[:, 0]
    for i, (name, row) in enumerate(cases):
        ref, may = R.apply(img, row)
        frac = float(may.mean())
        err = np.abs(got[i].astype(np.float64) - ref)
        shade = row[R.KSIZE] > 0
        print("%dx%d %-22s tie fraction %.5f  max err outside ties %.3g  inside %.3g" %
              (H, W, name, frac, err[~may].max(), err[may].max() if may.any() else 0.0))
        assert frac < 1e-3, (name, frac)
        if shade:
            assert err[~may].max() <= SHADE_TOL, (name, err[~may].max())
            assert (err[may] <= 1.5 / 255 + SHADE_TOL).all(), name     # one level, scaled by 1 - t * M <= 1.5
        else:
            assert np.array_equal(got[i][~may], ref.astype(np.float32)[~may]), (name, err[~may].max())
            assert (err[may] <= 1 / 255 + 1e-7).all(), name
            assert np.array_equal(np.rint(got[i] * 255).astype(np.float32) / np.float32(255), got[i]), name   # multiples of 1/255


def test_all_primitives_off_equals_label_quantize():
    from semantic_superpoint_amd import lib as L
    g = torch.Generator().manual_seed(3)
    x = torch.rand(5, 1, 67, 93, generator=g)
    x[0, 0, 0, :4] = torch.tensor([0.0, 1.0, 128 / 255, 1 / 255])
    x = x.to(_dev())
    rows = torch.from_numpy(np.stack([R.make_row(key=k) for k in range(5)])).to(_dev())
    assert torch.equal(L.op_photometric_apply(x, rows), L.op_label_quantize(x))


def _noise_residual(L, sigma=0.0, p=0.0, key0=1234567891011):
    B, H, W = 8, 240, 320
    x = torch.full((B, 1, H, W), 128 / 255, dtype=torch.float32, device=_dev())
    rows = torch.from_numpy(np.stack([R.make_row(sigma=sigma, impulse_p=p, key=key0 + 7919 * k) for k in range(B)])).to(_dev())
    base = L.op_label_quantize(x)
    out = L.op_photometric_apply(x, rows)
    assert torch.equal(out, L.op_photometric_apply(x, rows))                      # same key, same bits
    res = ((out - base) * 255).double().cpu().numpy()[:, 0]
    assert np.abs(res - np.rint(res)).max() < 1e-3                                 # 8-bit values
    return np.rint(res), float(np.rint(float(base.flatten()[0]) * 255)), (x, rows, out, L)


def test_gaussian_noise_statistics():
    from semantic_superpoint_amd import lib as L
    sigma = 10.0
    res, _, (x, rows, out, _) = _noise_residual(L, sigma=sigma)
    n = res.size
    sd = np.sqrt(sigma ** 2 + 1 / 12)
    print("noise: mean %.4f (4 se = %.4f)  std %.4f (model %.4f)" % (res.mean(), 4 * sd / np.sqrt(n), res.std(), sd))
    assert abs(res.mean()) < 4 * sd / np.sqrt(n)
    assert abs(res.std() / sd - 1) < 0.02
    assert not np.array_equal(res[0], res[1])                                      # another image index, another noise
    rows2 = rows.clone()
    rows2[:, R.KEY] = rows[:, R.KEY] + 1
    assert not torch.equal(L.op_photometric_apply(x, rows2), out)                  # another key, another noise
    same = rows.clone()
    same[1] = rows[0]
    assert torch.equal(L.op_photometric_apply(x, same)[1], out[0])                 # a pure function of image and row


def test_impulse_noise_statistics():
    from semantic_superpoint_amd import lib as L
    p = 0.0035
    res, base, _ = _noise_residual(L, p=p)
    n = res.size
    frac = float((res != 0).mean())
    se = np.sqrt(p * (1 - p) / n)
    print("impulse: replaced fraction %.6f (p %.6f, 4 se %.6f)" % (frac, p, 4 * se))
    assert abs(frac - p) < 4 * se
    vals = res[res != 0] + base
    assert (vals < 128).any() and (vals > 128).any() and vals.min() >= 0 and vals.max() <= 255
    # Beta(1/2, 1/2): half of the replacements fall outside [255 * sin^2(pi/8), 255 * cos^2(pi/8)] = [37.3, 217.7]
    outer = float(((vals < 37.3) | (vals > 217.7)).mean())
    assert abs(outer - 0.5) < 4 * np.sqrt(0.25 / vals.size)
    assert not np.array_equal(res[0], res[1])


def _chi2_uniform(counts, weights=None):
    """chi-square statistic of bin counts against a uniform law (weights: the share of each bin; equal bins by default)"""
    w = np.full(counts.size, 1.0 / counts.size) if weights is None else np.asarray(weights, np.float64)
    e = counts.sum() * w
    return float(((counts - e) ** 2 / e).sum())


def test_draw_statistics(golden_dir):
    from semantic_superpoint_amd import lib as L
    B, H, W = 4096, 240, 320
    aug = _aug(golden_dir)
    d = L.op_photometric_draw(B, H, W, 20241016, aug, _dev())
    assert torch.equal(d, L.op_photometric_draw(B, H, W, 20241016, aug, _dev()))
    assert not torch.equal(d, L.op_photometric_draw(B, H, W, 20241017, aug, _dev()))
    d = d.cpu().numpy().astype(np.float64)
    assert d.shape == (B, R.STRIDE)
    br, ct, sg, ip, fl = (d[:, i] for i in (R.BRIGHTNESS, R.CONTRAST, R.SIGMA, R.IMPULSE_P, R.BLUR_FLAG))
    assert np.array_equal(br, np.rint(br)) and br.min() >= -50 and br.max() <= 50 and br.min() < -45 and br.max() > 45
    assert ct.min() >= 0.5 and ct.max() <= 1.5 and sg.min() >= 0 and sg.max() <= 10 and ip.min() >= 0 and ip.max() <= 0.0035
    assert set(np.unique(fl)) == {0.0, 1.0} and abs(fl.mean() - 0.5) < 4 * np.sqrt(0.25 / B)
    w = d[:, R.BLUR_W:R.BLUR_W + 9]
    assert np.abs(w.sum(axis=1) - 1).max() < 1e-6 and w.min() >= 0
    assert np.abs(w[:, 4] - w[:, 4].mean()).max() > 1e-3                                     # rotated / skewed kernels, not one kernel
    ell = d[:, R.ELLIPSES:R.ELLIPSES + 5 * R.MAX_ELLIPSES].reshape(B, R.MAX_ELLIPSES, 5)
    used, unused = ell[:, :20], ell[:, 20:]
    assert (unused[..., 2] < 0).all()
    cx, cy, ax, ay, ang = (used[..., i] for i in range(5))
    min_dim = min(H, W) / 4
    assert np.array_equal(ax, np.floor(ax)) and ax.min() >= int(min_dim / 5) and ax.max() <= min_dim and ay.min() >= int(min_dim / 5) and ay.max() <= min_dim
    rad = np.maximum(ax, ay)
    assert (cx >= rad).all() and (cx < W - rad).all() and (cy >= rad).all() and (cy < H - rad).all()
    assert np.array_equal(cx, np.floor(cx)) and np.array_equal(cy, np.floor(cy))
    assert ang.min() >= 0 and ang.max() < 90
    t, ks = d[:, R.TRANSPARENCY], d[:, R.KSIZE]
    assert t.min() >= -0.5 and t.max() <= 0.5
    assert np.array_equal(ks % 2, np.ones(B)) and ks.min() >= 101 and ks.max() <= 149 + 1
    key = d[:, R.KEY:R.KEY + 4]
    assert np.array_equal(key, np.floor(key)) and key.min() >= 0 and key.max() <= 65535
    assert len({tuple(k) for k in key}) == B
    # chi-square over 10 bins, 9 degrees of freedom: p > 1e-3 <=> statistic < 27.88
    edges = np.linspace(-50.5, 50.5, 11)                                               # 101 integers: 10 or 11 per bin
    c_br = np.histogram(br, bins=edges)[0].astype(np.float64)
    w_br = np.histogram(np.arange(-50, 51), bins=edges)[0] / 101.0
    c_t = np.histogram(t, bins=np.linspace(-0.5, 0.5, 11))[0].astype(np.float64)
    print("chi2 brightness %.2f  transparency %.2f" % (_chi2_uniform(c_br, w_br), _chi2_uniform(c_t)))
    assert _chi2_uniform(c_br, w_br) < 27.88 and _chi2_uniform(c_t) < 27.88


def test_draw_rejects_unknown_struct_size_and_repeated_primitives(golden_dir):
    from semantic_superpoint_amd import lib as L
    p = L.photometric_params_from_config(_aug(golden_dir))
    p.struct_size += 4
    with pytest.raises(RuntimeError, match="struct_size"):
        L.op_photometric_draw(2, 64, 96, 1, p, _dev())
    aug = _aug(golden_dir)
    aug["photometric"]["params"]["motion_blur"] = {"max_kernel_size": 5}
    with pytest.raises(RuntimeError, match="twice"):
        L.op_photometric_draw(2, 64, 96, 1, aug, _dev())


def _pair_inputs(B=4, H=64, W=96):
    g = torch.Generator().manual_seed(0)
    img = torch.rand(B, 1, H, W, generator=g).to(_dev())
    # keypoints 8 pixels apart (chosen when colliding keypoints still made warped_labels_bi depend on thread order; the scatter is
    # order-defined now: tests/test_gpu_pairs_exact.py); these tests compare two calls bit for bit
    lab = torch.zeros(B, 1, H, W)
    lab[:, :, 4::8, 4::8] = (torch.rand(B, 1, H // 8, W // 8, generator=g) < 0.3).float()
    sem = torch.randint(0, 134, (B, H, W), generator=g).to(_dev())
    return img, lab.to(_dev()), sem


WARP = dict(translation=True, rotation=True, scaling=True, perspective=True, scaling_amplitude=0.2,
            perspective_amplitude_x=0.2, perspective_amplitude_y=0.2, patch_ratio=0.85, max_angle=1.57, allow_artifacts=True)


def test_make_pairs_defaults_are_unchanged():
    from semantic_superpoint_amd import pairs
    img, lab, sem = _pair_inputs()
    a = pairs.make_pairs(img, lab, seed=5, warp_params=WARP, erosion_radius=3, semantic=sem)
    b = pairs.make_pairs(img, lab, seed=5, warp_params=WARP, erosion_radius=3, semantic=sem, photometric=None,
                         homographies=None, photometric_draws=None)
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(a["image"], img)


def test_make_pairs_given_homographies_and_draws(golden_dir):
    from semantic_superpoint_amd import lib as L
    from semantic_superpoint_amd import pairs
    img, lab, sem = _pair_inputs()
    B, _, H, W = img.shape
    hs, _ = L.op_sample_homographies(B, 11, _dev(), **WARP)
    s = pairs.make_pairs(img, lab, seed=5, warp_params=WARP, semantic=sem, homographies=hs)
    assert torch.equal(s["homographies"], hs)
    assert torch.equal(s["warped_img"], L.op_warp_image(img, s["inv_homographies"]))
    eye = torch.eye(3, device=_dev()).expand(B, 3, 3)
    assert ((s["homographies"] @ s["inv_homographies"]) - eye).abs().max() < 1e-4
    draws = tuple(L.op_photometric_draw(B, H, W, 100 + v, _aug(golden_dir), _dev()) for v in (0, 1))
    t = pairs.make_pairs(img, lab, seed=5, warp_params=WARP, semantic=sem, homographies=hs, photometric_draws=draws)
    assert torch.equal(t["image"], L.op_photometric_apply(img, draws[0]))
    assert torch.equal(t["warped_img"], L.op_photometric_apply(L.op_warp_image(img, t["inv_homographies"]), draws[1]))   # the warp reads the RAW image
    for k in ("labels_2D", "warped_labels", "warped_valid_mask", "warped_sem", "warped_res"):
        assert torch.equal(s[k], t[k]), k
    # photometric= draws by itself, independently for the two views, and only when enabled
    u = pairs.make_pairs(img, lab, seed=5, warp_params=WARP, homographies=hs, photometric=_aug(golden_dir))
    assert not torch.equal(u["image"], img) and float(u["image"].min()) >= 0 and float(u["image"].max()) <= 1
    off = _aug(golden_dir)
    off["photometric"]["enable"] = False
    assert torch.equal(pairs.make_pairs(img, lab, seed=5, warp_params=WARP, homographies=hs, photometric=off)["image"], img)
    # uint8 image / narrow semantic: widened on the device
    u8 = (img * 255).to(torch.uint8)
    v = pairs.make_pairs(u8, lab, seed=5, warp_params=WARP, semantic=sem.to(torch.uint8), homographies=hs)
    wv = pairs.make_pairs((u8.cpu().float() / 255.0).to(_dev()), lab, seed=5, warp_params=WARP, semantic=sem, homographies=hs)
    for k in wv:
        assert torch.equal(v[k], wv[k]), k
    assert v["semantic"].dtype == torch.int64
