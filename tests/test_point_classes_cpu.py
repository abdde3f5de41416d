"""No GPU: the numpy restatement of the semantic-keypoint operators (tests/point_classes_ref.py) against hand-computed cases,
lib.class_mask, the host-side argument checks of the new C entry points, and the matcher seeds of tests/test_gpu_point_classes.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import point_classes_ref as R


def test_class_mask_bit_layout_and_errors():
    from semantic_superpoint_amd import lib as L
    assert L.CLASS_NONE == R.CLASS_NONE == 255
    m = L.class_mask(keep=[0, 31, 32, 132], n_classes=133)
    assert len(m) == 8 and m == (0x80000001, 0x1, 0, 0, 0x10, 0, 0, 0)
    d = L.class_mask(drop=[0, 31, 32, 132], n_classes=133)
    full = [(1 << 32) - 1] * 4 + [(1 << 5) - 1, 0, 0, 0]           # classes 0 .. 132
    assert d == tuple(f & ~k for f, k in zip(full, m))
    assert L.class_mask(drop=[], n_classes=5) == (0x1f, 0, 0, 0, 0, 0, 0, 0)
    assert L.class_mask(keep=[], n_classes=5) == (0,) * 8
    assert L.class_mask(keep=[254], n_classes=255)[7] == 1 << 30
    assert L.class_mask(keep=[3, 3], n_classes=5) == (8, 0, 0, 0, 0, 0, 0, 0)
    assert np.array_equal(np.nonzero(R.mask_bits(m))[0], [0, 31, 32, 132])
    with pytest.raises(ValueError, match="exactly one"):
        L.class_mask(n_classes=5)
    with pytest.raises(ValueError, match="exactly one"):
        L.class_mask(keep=[1], drop=[2], n_classes=5)
    for bad in ([5], [-1], [0, 133]):
        with pytest.raises(ValueError, match="outside"):
            L.class_mask(keep=bad, n_classes=5)
        with pytest.raises(ValueError, match="outside"):
            L.class_mask(drop=bad, n_classes=5)
    with pytest.raises(ValueError, match="n_classes"):
        L.class_mask(keep=[0], n_classes=256)


def test_python_argument_errors_need_no_device():
    from semantic_superpoint_amd import lib as L
    from semantic_superpoint_amd.export import PointTracker
    d, c = torch.zeros(1, 4, 256), torch.zeros(1, dtype=torch.int32)
    with pytest.raises(ValueError, match="both or neither"):
        L.op_match_two_way(d, c, d, c, 0.7, cls1=torch.zeros(1, 4, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="HIP device"):    # no CPU fallback
        L.op_point_classes(torch.zeros(1, 5, 2, 2), torch.zeros(1, 4, 2), c)
    with pytest.raises(RuntimeError, match="HIP device"):
        L.op_filter_points(torch.zeros(1, 4, 5), c, d, torch.zeros(1, 4, dtype=torch.uint8), L.class_mask(drop=[], n_classes=5))
    tr = PointTracker(3, 0.7, device="cuda:0", class_consistent=True)
    with pytest.raises(ValueError, match="cls"):
        tr.update_device(torch.zeros(4, 2), c, d[0])
    with pytest.raises(RuntimeError, match="HIP device"):
        tr.update_device(torch.zeros(4, 2), c, d[0], cls=torch.zeros(4, dtype=torch.uint8))


def test_c_abi_rejects_bad_arguments_before_any_launch():
    """every documented error case returns -1 with a message (the pointers below are never dereferenced)"""
    import ctypes
    import semantic_superpoint_amd as ssp
    lib = ssp.load_library()
    p, q, null = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x2000), None
    mask = (ctypes.c_uint32 * 8)()

    def err(fn, *a):
        assert fn(*a) == -1
        return lib.ssp_last_error().decode()
    pc = lib.ssp_op_point_classes
    #                  sout cs  b  h   w   C    pts stride count cap cls stream
    assert "multiples of 8" in err(pc, p, 136, 1, 60, 96, 133, p, 5, p, 10, p, null)
    assert "n_classes" in err(pc, p, 256, 1, 64, 96, 256, p, 5, p, 10, p, null)      # 255 is SSP_CLASS_NONE
    assert "n_classes" in err(pc, p, 136, 1, 64, 96, 0, p, 5, p, 10, p, null)
    assert "n_classes" in err(pc, p, 132, 1, 64, 96, 133, p, 5, p, 10, p, null)
    assert "cap" in err(pc, p, 136, 1, 64, 96, 133, p, 5, p, 0, p, null)
    assert "cap" in err(pc, p, 136, 1, 64, 96, 133, p, 1, p, 10, p, null)
    assert "null" in err(pc, p, 136, 1, 64, 96, 133, null, 5, p, 10, p, null)
    assert "not bound" in err(lib.ssp_point_classes, null, 0, 1, p, 5, p, 10, p, null)
    fp = lib.ssp_op_filter_points
    #                 pts count desc cls mask n cap  pts_out count_out desc_out cls_out ws stream
    assert "null" in err(fp, p, p, p, p, mask, 1, 10, q, q, q, null, q, null)
    assert "in place" in err(fp, p, p, p, p, mask, 1, 10, q, q, p, q, q, null)
    assert "cap" in err(fp, p, p, p, p, mask, 1, 0, q, q, q, q, q, null)
    assert "aligned" in err(fp, p, p, ctypes.c_void_p(0x1004), p, mask, 1, 10, q, q, q, q, q, null)
    assert lib.ssp_filter_workspace_bytes(0, 10) == 0 and lib.ssp_filter_workspace_bytes(3, 1500) >= 3 * 2 * 4
    mc = lib.ssp_match_two_way_classes
    #                   d1 c1 d2 c2 cls1 cls2 cap P stride thresh ws match n_match stream
    assert "class" in err(mc, p, p, p, p, p, null, 10, 1, 1, 0.7, p, p, p, null)
    assert "nn_thresh" in err(mc, p, p, p, p, p, p, 10, 1, 1, -1.0, p, p, p, null)
    assert "cap" in err(mc, p, p, p, p, p, p, 4097, 1, 1, 0.7, p, p, p, null)


# ---- the restatement against hand-computed cases ----

def test_upsample_restatement_hand_cases_and_torch():
    """A 2x2-cell map: weights (2 i + 1) / 16 between the cell centres, the clamp outside them."""
    s = np.zeros((1, 2, 2, 2))
    s[0, 0] = [[0.0, 16.0], [32.0, 48.0]]
    s[0, 1] = [[20.0, 20.0], [20.0, 20.0]]
    # corners and borders: the cell value itself (both cells of an axis coincide)
    assert R.logits_at(s, 0, 0, 0)[0] == 0.0 and R.logits_at(s, 0, 15, 0)[0] == 16.0
    assert R.logits_at(s, 0, 0, 15)[0] == 32.0 and R.logits_at(s, 0, 15, 15)[0] == 48.0
    assert R.logits_at(s, 0, 3, 2)[0] == 0.0                      # x, y <= 3: still inside the clamp of the first cell
    assert R.logits_at(s, 0, 4, 0)[0] == 16.0 * 1 / 16            # x = 4: weight 1/16 of the right cell
    assert R.logits_at(s, 0, 11, 0)[0] == 16.0 * 15 / 16
    assert R.logits_at(s, 0, 12, 0)[0] == 16.0                    # x >= 12: the clamp of the last cell
    assert R.logits_at(s, 0, 0, 7)[0] == 32.0 * 7 / 16
    assert R.logits_at(s, 0, 5, 9)[0] == (5 / 16) * (13 / 16 * 0 + 3 / 16 * 16) + (11 / 16) * (13 / 16 * 32 + 3 / 16 * 48)
    # the whole image against torch's fp64 interpolation
    rng = np.random.default_rng(0)
    s = rng.standard_normal((2, 3, 2, 3))
    up = F.interpolate(torch.from_numpy(s), size=(16, 24), mode="bilinear", align_corners=False).numpy()
    got = np.array([[[R.logits_at(s, k, x, y) for x in range(24)] for y in range(16)] for k in range(2)])
    assert np.abs(got.transpose(0, 3, 1, 2) - up).max() < 1e-14


def test_point_classes_restatement_ties_counts_and_clamp():
    s = np.zeros((2, 3, 2, 2))
    s[0, 1, 0, 0] = 16.0          # class 1 owns the first cell of image 0 ...
    s[0, 2, 0, 1] = 16.0          # ... class 2 the one right of it: along y = 0 they cross between x = 7 and x = 8
    s[1, 2] = 1.0
    pts = np.zeros((2, 6, 5), dtype=np.float32)
    pts[0, :, 0] = [0, 7, 8, 15, 40, -3]
    pts[0, 4, 1] = 99             # (40, 99) is clamped to (15, 15): all zero there -> tie of three -> class 0
    cls = R.point_classes(s, pts, [6, 2])
    assert cls.dtype == np.uint8
    assert list(cls[0]) == [1, 1, 2, 2, 0, 1]       # x = 7: 9 vs 7, x = 8: 7 vs 9; (-3, 0) clamps to (0, 0)
    assert list(cls[1]) == [2, 2, 255, 255, 255, 255]
    # an exact tie between classes 1 and 2 goes to the lower one; n_classes hides a louder padding channel
    t = np.zeros((1, 4, 1, 1))
    t[0, 1:3] = 5.0
    t[0, 3] = 1e9
    one = np.zeros((1, 1, 2), dtype=np.float32)
    assert R.point_classes(t, one, [1], n_classes=3)[0, 0] == 1 and R.point_classes(t, one, [1])[0, 0] == 3
    assert R.point_classes(t, one, [0])[0, 0] == 255 and R.point_classes(t, one, [7])[0, 0] == 3   # count clamped to cap


def test_filter_restatement_is_stable():
    from semantic_superpoint_amd import lib as L
    cls = np.array([[2, 0, 1, 2, 2, 1], [1, 1, 1, 1, 1, 1]], dtype=np.uint8)
    pts = np.arange(2 * 6 * 5, dtype=np.float32).reshape(2, 6, 5)
    desc = np.arange(2 * 6 * 256, dtype=np.float32).reshape(2, 6, 256)
    po, no, do, co = R.filter_points(pts, [5, 6], desc, cls, L.class_mask(keep=[2, 0], n_classes=3))
    assert list(no) == [4, 0]                       # rows 2 and 5 of image 0 are class 1 (5 is past the count too); image 1 holds class 1 only
    assert np.array_equal(po[0, :4], pts[0, [0, 1, 3, 4]]) and np.array_equal(do[0, :4], desc[0, [0, 1, 3, 4]])
    assert list(co[0]) == [2, 0, 2, 2, 255, 255] and list(co[1]) == [255] * 6
    assert list(R.filter_points(pts, [3, 6], desc, cls, L.class_mask(keep=[2, 0], n_classes=3))[1]) == [2, 0]   # the count cuts
    po, no, do, co = R.filter_points(pts, [5, 6], desc, cls, L.class_mask(drop=[], n_classes=3))
    assert list(no) == [5, 6] and np.array_equal(po[1], pts[1]) and np.array_equal(co[0, :5], cls[0, :5]) and co[0, 5] == 255


def test_masked_matcher_restatement_hand_case():
    e = np.eye(256, dtype=np.float32)
    d1 = np.stack([e[0], e[1], e[2]])
    a = np.float32(np.sqrt(0.5))
    d2 = np.stack([e[0], a * (e[1] + e[2]), e[3]])    # row 1 and row 2 of d1 are equally near column 1: the tie
    same = [0, 0, 0]
    m = R.match_two_way_classes(d1, d2, same, same, 1.0)
    assert m[:, :2].tolist() == [[0, 0], [1, 1]]     # np.argmin: column 1 takes the first of its two nearest rows
    m = R.match_two_way_classes(d1, d2, [0, 1, 0], [0, 0, 0], 1.0)
    assert m[:, :2].tolist() == [[0, 0], [2, 1]]     # row 1 has no candidate, so column 1 goes to row 2
    assert abs(m[1, 2] - np.sqrt(2 - np.sqrt(2))) < 1e-7
    assert len(R.match_two_way_classes(d1, d2, [0, 0, 0], [1, 1, 1], 1.0)) == 0      # disjoint classes
    assert len(R.match_two_way_classes(d1[:0], d2, [], same, 1.0)) == 0               # an empty side
    assert R.match_two_way_classes(d1, d2, same, same, 0.5)[:, :2].tolist() == [[0, 0]]   # the threshold still applies


def test_matcher_seeds_of_the_gpu_test_are_decided_by_a_wide_margin():
    """tests/test_gpu_point_classes.py compares indices with this restatement: every row's and column's best / second-best gap,
    and every row minimum's distance from the threshold, must exceed 1e-5 (the fp32 distances of the device differ from fp64 by
    ~1e-7) for its fixed seeds - asserted there too, never skipped."""
    from tests.test_gpu_point_classes import MATCH_SEEDS, MATCH_THRESH, _decided, match_case
    assert len(MATCH_SEEDS) == 3
    for seed in MATCH_SEEDS:
        d1, d2, c1, c2 = match_case(seed)
        assert d1.shape == (70, 256) and d2.shape == (130, 256) and set(c1.tolist()) == set(c2.tolist()) == {0, 1, 2}
        _decided(d1, d2, c1, c2, MATCH_THRESH)
        want = R.match_two_way_classes(d1, d2, c1, c2, MATCH_THRESH)
        plain = R.match_two_way_classes(d1, d2, c1 * 0, c2 * 0, MATCH_THRESH)
        assert len(want) > 20 and (c1[plain[:, 0].astype(int)] != c2[plain[:, 1].astype(int)]).any()
    d1, d2, c1, c2 = match_case(MATCH_SEEDS[0])           # the one-sided class of test_class_matcher_edge_cases
    _decided(d1, d2, c1, np.where(c2 == 2, 1, c2).astype(np.uint8), MATCH_THRESH)
