"""Synthetic Shapes without a GPU: the config parser, the facts the numpy restatement (tests/shapes_ref.py) rests on, and the
precondition of the exact GPU test (tests/test_gpu_shapes.py) on the committed scene tables."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

from semantic_superpoint_amd import lib as L
from tests import shapes_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def cfg():
    with open(os.path.join(HERE, "golden", "g18_shapes_config.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def tables():
    return np.load(os.path.join(HERE, "golden", "g18_shapes_tables.npz"))


def test_config_parser_merges_the_class_defaults(cfg):
    p = L.shapes_params_from_config(cfg["data"])
    assert p.struct_size == ctypes.sizeof(L.SspShapesParams)
    assert (p.gen_h, p.gen_w, p.out_h, p.out_w, p.blur_size) == (960, 1280, 120, 160, 21)
    # SyntheticDataset_gaussian.default_config["generation"]["params"] (:63-72) over synthetic_dataset.py's keyword defaults
    assert (p.bg_min_kernel, p.bg_max_kernel, p.bg_nb_blobs) == (150, 500, 100)
    assert (p.bg_min_rad_ratio, p.bg_max_rad_ratio) == (np.float32(0.02), np.float32(0.031))
    assert tuple(p.stripes_transform) == (np.float32(0.1), np.float32(0.1)) and tuple(p.checker_transform) == (np.float32(0.05), np.float32(0.15))
    assert (p.multi_kernel_lo, p.multi_kernel_hi, p.multi_nb_blobs, p.multi_nb_polygons) == (50, 100, 3000, 30)
    w = np.array(list(p.weights), np.float32)
    assert np.array_equal(w, np.array([1, 1, 1, 0.3, 1, 1, 0.2, 1, 0.1], np.float32))
    assert abs(float(w.sum()) - 6.6) < 1e-6
    assert np.array_equal(np.array(list(p.gauss_w)[:21], np.float32), R.gaussian_weights(21)) and list(p.gauss_w)[21:] == [0.0] * 42
    assert (p.resize_scale_y, p.resize_scale_x) == (8.0, 8.0)
    q = L.shapes_params_from_config(dict(cfg["data"], primitives=["draw_cube", "draw_star"]))
    assert list(q.weights) == [0, 0, 0, 0, 1, 0, 0, 1, 0]
    with pytest.raises(ValueError):
        L.shapes_params_from_config(dict(cfg["data"], primitives=["draw_circle"]))


def test_restatement_facts():
    assert R.gaussian_sigma(21) == 3.5
    w = R.gaussian_weights(21)
    assert w.dtype == np.float32 and abs(float(w.astype(np.float64).sum()) - 1) < 1e-6 and np.array_equal(w, w[::-1]) and w.argmax() == 10
    y0, y1, f = R.resize_taps(120, 960)  # an 8x reduction reads exactly the 2x2 block at 8 d + 3, 8 d + 4 with weight 1/2
    assert np.array_equal(y0, 8 * np.arange(120) + 3) and np.array_equal(y1, 8 * np.arange(120) + 4) and (f == 0.5).all()
    y0, y1, f = R.resize_taps(7, 5)      # enlarging clamps at both borders
    assert y0[0] == 0 and f[0] == 0 and y1[-1] == 4 and y0.max() <= 4
    assert R.reflect101(np.arange(-6, 11), 5).tolist() == [2, 3, 4, 3, 2, 1, 0, 1, 2, 3, 4, 3, 2, 1, 0, 1, 2]
    assert R.reflect101(np.array([-1, 7]), 1).tolist() == [0, 0]
    img = np.zeros((5, 6), np.int64)
    img[2, 3] = 90
    b = R.box_blur(img, 3)
    assert b[1:4, 2:5].tolist() == [[10] * 3] * 3 and b.sum() == 90   # (90 + 4) // 9
    assert R.box_blur(np.full((4, 4), 7, np.int64), 9).tolist() == [[7] * 4] * 4  # a window wider than the image reflects repeatedly


def test_integer_coverage_of_a_triangle_and_a_thick_segment():
    tri = R.poly_mask(np.array([[1, 1], [6, 1], [1, 6]]), 8, 8).astype(int)
    assert tri.tolist() == [[0, 0, 0, 0, 0, 0, 0, 0],
                            [0, 1, 1, 1, 1, 1, 1, 0],
                            [0, 1, 1, 1, 1, 1, 0, 0],
                            [0, 1, 1, 1, 1, 0, 0, 0],
                            [0, 1, 1, 1, 0, 0, 0, 0],
                            [0, 1, 1, 0, 0, 0, 0, 0],
                            [0, 1, 0, 0, 0, 0, 0, 0],
                            [0, 0, 0, 0, 0, 0, 0, 0]]
    seg = R.seg_mask(2, 3, 6, 3, 3, 7, 9).astype(int)   # thickness 3: |dy| <= 1.5 and round caps of radius 1.5
    assert seg.tolist() == [[0, 0, 0, 0, 0, 0, 0, 0, 0],
                            [0, 0, 0, 0, 0, 0, 0, 0, 0],
                            [0, 1, 1, 1, 1, 1, 1, 1, 0],
                            [0, 1, 1, 1, 1, 1, 1, 1, 0],
                            [0, 1, 1, 1, 1, 1, 1, 1, 0],
                            [0, 0, 0, 0, 0, 0, 0, 0, 0],
                            [0, 0, 0, 0, 0, 0, 0, 0, 0]]
    assert R.seg_mask(1, 1, 4, 4, 1, 6, 6).astype(int).tolist() == np.eye(6, dtype=int).tolist()[:1] * 0 + [
        [0, 0, 0, 0, 0, 0], [0, 1, 0, 0, 0, 0], [0, 0, 1, 0, 0, 0], [0, 0, 0, 1, 0, 0], [0, 0, 0, 0, 1, 0], [0, 0, 0, 0, 0, 0]]
    bow = R.poly_mask(np.array([[0, 0], [4, 4], [4, 0], [0, 4]]), 5, 5)   # a self-crossing quad: even-odd, edges included
    assert bow[2, 2] and bow[1, 0] and not bow[0, 2] and bow[2, 3]


def test_fixture_tables_obey_the_rules_and_keep_the_flip_set_small(cfg, tables):
    """The precondition of test_gpu_shapes.test_render_is_exact: on the committed tables the output pixels whose value could flip
    (a Gaussian value within 1e-3 of a rounding boundary in their footprint, an inexactly computed bilinear value within 1e-3 of
    one, or an ellipse pixel centre within 1e-3 of the boundary) are at most 1 %.  A bilinear value that fp32 computes exactly
    (dyadic fractions: every integer reduction) is a tie for every implementation and is not counted."""
    p = L.shapes_params_from_config(R.small_config(cfg["data"]))
    assert sorted(tables.files) == sorted(["prim%d" % k for k in range(9)] + list(R.FIXTURE_SEEDS))
    n_flip = n_pix = 0
    for k in tables.files:
        t = tables[k]
        assert t.dtype == np.int32 and t.shape[1] == L.SHAPES_ROW == R.ROW
        for row in t:
            if k.startswith("prim"):
                assert int(row[R.PRIM]) == int(k[4:])
            R.check_row(row, p)
            img, flip, pts = R.render(row, (192, 256), (24, 32), 5, R.SMALL_TEX_BLOBS)
            assert img.shape == (24, 32) and img.dtype == np.uint8 and 0 < img.std()
            n_flip += int(flip.sum())
            n_pix += flip.size
    print("flip set: %d of %d output pixels" % (n_flip, n_pix))
    assert n_flip <= 0.01 * n_pix


def test_new_exports_are_declared_and_listed():
    with open(os.path.join(os.path.dirname(HERE), "include", "ssp_hip.h")) as f:
        header = f.read()
    for name in ("ssp_shapes_workspace_bytes", "ssp_op_shapes_draw", "ssp_op_shapes_render", "ssp_op_warp_points_scatter"):
        assert re.search(r"\b%s\(" % name, header) and name in L.EXPORTS
    for c in ("ROW", "CMDS", "VERTS", "TEX", "POINTS", "BLOBS"):
        assert int(re.search(r"SSP_SHAPES_%s = (\d+)" % c, header).group(1)) == getattr(L, "SHAPES_" + c) == getattr(R, c)
