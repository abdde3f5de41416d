"""CPU: the host side of the photometric augmentation: the numpy restatement's Gaussian weights, the
config parser `lib.photometric_params_from_config` on the shipped COCO block (settings-only fixture g17, values of
configs/superpoint_coco_train_wsem_heatmap.yaml:24-38) with the reference's max_kernel_size quirk, and the preconditions
of the exact GPU test (tests/test_gpu_photometric.py): tie sets under the cap, ellipse edges away from pixel centres."""
import copy
import ctypes
import json
import os

import numpy as np
import pytest

from tests import photometric_ref as R


def _cfg(golden_dir):
    with open(os.path.join(golden_dir, "g17_photometric_config.json")) as f:
        return json.load(f)


def test_gaussian_weights_and_sigma():
    for k, sigma in ((101, 15.5), (151, 23.0), (351, 53.0)):
        assert abs(R.gaussian_sigma(k) - (0.3 * ((k - 1) * 0.5 - 1) + 0.8)) < 1e-12
        assert abs(R.gaussian_sigma(k) - sigma) < 1e-9
        w = R.gaussian_weights(k)
        assert w.shape == (k,) and abs(w.sum() - 1.0) < 1e-12
        assert np.allclose(w, w[::-1]) and w.argmax() == (k - 1) // 2
        assert abs(w[(k - 1) // 2 + 1] / w[(k - 1) // 2] - np.exp(-0.5 / sigma ** 2)) < 1e-12


def test_params_from_shipped_config(golden_dir):
    from semantic_superpoint_amd import lib as L
    p = L.photometric_params_from_config(_cfg(golden_dir))
    assert p.struct_size == ctypes.sizeof(L.SspPhotometricParams) and p.struct_size > 0
    assert L.SspPhotometricParams._fields_[0][0] == "struct_size"
    assert [p.random_brightness, p.random_contrast, p.additive_gaussian_noise, p.additive_speckle_noise, p.motion_blur,
            p.additive_shade] == [1, 1, 1, 1, 1, 1]
    assert p.brightness_max_abs_change == 50
    assert (p.contrast_lo, p.contrast_hi) == (0.5, 1.5)
    assert (p.noise_std_lo, p.noise_std_hi) == (0.0, 10.0)
    assert p.impulse_prob_lo == 0.0 and abs(p.impulse_prob_hi - 0.0035) < 1e-9
    assert p.shade_nb_ellipses == 20                      # additive_shade's own default
    assert (p.shade_transparency_lo, p.shade_transparency_hi) == (-0.5, 0.5)
    assert (p.shade_kernel_lo, p.shade_kernel_hi) == (100, 150)
    off = copy.deepcopy(_cfg(golden_dir))
    off["photometric"]["enable"] = False
    q = L.photometric_params_from_config(off)
    assert q.struct_size == p.struct_size
    assert [q.random_brightness, q.random_contrast, q.additive_gaussian_noise, q.additive_speckle_noise, q.motion_blur,
            q.additive_shade] == [0] * 6


@pytest.mark.parametrize("size", [5, 2])
def test_max_kernel_size_quirk(golden_dir, size):
    """utils/photometric.py:51-57: max_kernel_size != 3 assigns no augmenter; the previous one is appended a second time"""
    from semantic_superpoint_amd import lib as L
    cfg = _cfg(golden_dir)
    cfg["photometric"]["params"]["motion_blur"] = {"max_kernel_size": size}
    p = L.photometric_params_from_config(cfg)
    assert p.motion_blur == 0 and p.additive_speckle_noise == 2        # the last primitive before motion_blur in parse order
    assert [p.random_brightness, p.random_contrast, p.additive_gaussian_noise] == [1, 1, 1]
    del cfg["photometric"]["params"]["additive_speckle_noise"]
    p = L.photometric_params_from_config(cfg)
    assert p.additive_gaussian_noise == 2 and p.additive_speckle_noise == 0 and p.motion_blur == 0
    only = {"photometric": {"enable": True, "params": {"motion_blur": {"max_kernel_size": size}, "additive_shade": False}}}
    with pytest.raises(NameError):
        L.photometric_params_from_config(only)
    only["photometric"]["params"]["motion_blur"]["max_kernel_size"] = 3
    assert L.photometric_params_from_config(only).motion_blur == 1


def test_gaussian_blur_primitive_is_rejected(golden_dir):
    from semantic_superpoint_amd import lib as L
    cfg = _cfg(golden_dir)
    cfg["photometric"]["params"]["GaussianBlur"] = {"sigma": 0.2}
    with pytest.raises(ValueError, match="GaussianBlur"):
        L.photometric_params_from_config(cfg)


def test_row_layout_matches_the_library_constants():
    from semantic_superpoint_amd import lib as L
    assert (R.BRIGHTNESS, R.CONTRAST, R.SIGMA, R.IMPULSE_P, R.BLUR_FLAG, R.BLUR_W, R.ELLIPSES, R.TRANSPARENCY, R.KSIZE, R.KEY,
            R.STRIDE) == (L.PHOTO_BRIGHTNESS, L.PHOTO_CONTRAST, L.PHOTO_SIGMA, L.PHOTO_IMPULSE_P, L.PHOTO_BLUR_FLAG, L.PHOTO_BLUR_W,
                          L.PHOTO_ELLIPSES, L.PHOTO_TRANSPARENCY, L.PHOTO_KSIZE, L.PHOTO_KEY, L.PHOTO_DRAW_STRIDE)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "ssp_hip.h")).read()
    for name in ("BRIGHTNESS", "CONTRAST", "SIGMA", "IMPULSE_P", "BLUR_FLAG", "BLUR_W", "ELLIPSES", "TRANSPARENCY", "KSIZE", "KEY"):
        assert "SSP_PHOTO_%s = %d" % (name, getattr(R, name)) in hdr, name
    assert "SSP_PHOTO_DRAW_STRIDE = %d" % R.STRIDE in hdr


def test_all_primitives_off_is_the_quantisation():
    rs = np.random.RandomState(0)
    x = rs.rand(37, 53).astype(np.float32)
    x[0, :4] = [0.0, 1.0, 128 / 255, 1 / 255]
    out, may = R.apply(x, R.make_row())
    ref = np.floor(x * np.float32(255.0)).astype(np.float32) / np.float32(255.0)
    assert np.array_equal(out.astype(np.float32), ref) and not may.any()


def test_motion_blur_weights():
    for ang, d in ((0.0, 0.0), (90.0, -1.0), (45.0, 0.3), (200.0, 1.0)):
        w = R.motion_blur_weights(ang, d)
        assert abs(w.sum() - 1.0) < 1e-12 and (w >= 0).all()
    assert np.allclose(R.motion_blur_weights(0.0, 0.0)[:, 1], 1 / 3) and np.allclose(R.motion_blur_weights(90.0, -1.0)[1], [2 / 3, 1 / 3, 0])


@pytest.mark.parametrize("hw", [(240, 320), (67, 93), (388, 16)])
def test_exact_cases_meet_their_conditions(hw):
    """The conditions the exact GPU comparison rests on, checked on the helper itself: fewer than 0.1 % of the pixels within
    1e-3 of a rounding tie, and no pixel centre within 2e-5 of an ellipse's edge in f = (x'/ax)^2 + (y'/ay)^2 (the fp32
    evaluation of f is good to about 1e-6, so the device's mask is the helper's)."""
    img = R.case_image(*hw)
    assert img.min() == 0.0 and img.max() == 1.0
    for name, row in R.exact_cases(*hw):
        if name.startswith("shade_351") and hw == (240, 320):
            _, margin = R.ellipse_mask(row, *hw)   # (the float64 351-tap blur is the slow part: the tie set does not depend on it)
            assert margin > 2e-5, name
            continue
        out, may = R.apply(img, row)
        assert may.mean() < 1e-3, (name, may.mean())
        assert out.min() >= 0.0 and out.max() <= 1.0
        if row[R.KSIZE] > 0:
            assert R.ellipse_mask(row, *hw)[1] > 2e-5, name


def test_tile_case_height_is_read_from_the_header():
    """The (388, 16) case of the exact tests stands for the 16-column tile of ssp_op_photometric_apply: 388 is the smallest height
    whose shade strip exceeds 64 KiB at 32 columns, by the header's own photo_shade_lds_bytes (its return expression, evaluated
    here), and it fits at 16 columns."""
    import re
    from semantic_superpoint_amd import lib as L
    with open(os.path.join(os.path.dirname(L.__file__), "csrc", "photo_kernels.hip.h")) as f:
        src = f.read()
    body = re.search(r"size_t photo_shade_lds_bytes\(int H, int tx\) \{\s*return (.*?);", src, re.S).group(1).replace("(size_t)", "")
    ext = re.search(r"int photo_ext_width\(int tx\) \{ return (.*?); \}", src).group(1)
    names = {"PHOTO_MAX_KSIZE": L.PHOTO_MAX_KSIZE, "PHOTO_MAX_ELLIPSES": L.PHOTO_MAX_ELLIPSES, "PHOTO_HALO": (L.PHOTO_MAX_KSIZE - 1) // 2,
             "PHOTO_BAND": int(re.search(r"PHOTO_BAND = (\d+)", src).group(1))}
    names["photo_ext_width"] = lambda tx: eval(ext, dict(names, tx=tx))
    lds = lambda H, tx: eval("(%s)" % body, dict(names, H=H, tx=tx))  # noqa: E731
    tall = [hw for hw in R.SHADE_ELLIPSES if lds(hw[0], 32) > 65536]
    assert tall == [(388, 16)] and lds(387, 32) <= 65536 < lds(388, 32) and lds(388, 16) <= 65536
    assert all(lds(hw[0], 32) <= 65536 for hw in R.SHADE_ELLIPSES if hw != (388, 16))
