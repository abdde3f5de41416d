"""Descriptor export (export.py:66-190) without a GPU: the C ABI is declared and exported, the drop-in names import,
the G15 fixtures load with their keys."""
import os
import re

import numpy as np

from tests import golden_util as G
from tests.golden_descriptor import MATCH_CASES, descriptor_case_images, match_case_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ssp_describe_workspace_bytes", "ssp_describe_points", "ssp_op_sample_descriptors", "ssp_match_workspace_bytes",
       "ssp_match_two_way")


def test_symbols_declared_and_exported():
    from semantic_superpoint_amd import lib
    with open(os.path.join(ROOT, "include", "ssp_hip.h")) as f:
        hdr = f.read()
    for n in NEW:
        assert re.search(r"\b%s\(" % n, hdr), n
        assert n in lib.EXPORTS, n
    assert re.search(r"#define SSP_MATCH_MAX_POINTS %d\b" % lib.MATCH_MAX_POINTS, hdr)


def test_dropin_names_import():
    from semantic_superpoint_amd.Val_model_heatmap import Val_model_heatmap
    from semantic_superpoint_amd.export import (DescriptorExporter, PointTracker, SuperPointFrontend_torch,
                                                export_descriptor)
    assert issubclass(Val_model_heatmap, SuperPointFrontend_torch)
    assert callable(export_descriptor) and callable(DescriptorExporter)
    for m in ("nn_match_two_way", "update", "get_matches", "get_mscores", "clear_desc"):
        assert hasattr(PointTracker, m)
    for m in ("loadModel", "run", "heatmap_to_pts", "desc_to_sparseDesc", "soft_argmax_points"):
        assert hasattr(Val_model_heatmap, m)


def test_point_tracker_refuses_short_tracks_and_negative_threshold():
    import pytest
    from semantic_superpoint_amd.export import PointTracker
    with pytest.raises(ValueError):
        PointTracker(max_length=1, nn_thresh=0.7, device="cpu")
    t = PointTracker(max_length=2, nn_thresh=0.7, device="cpu")
    d = np.eye(256, 3, dtype=np.float32)
    with pytest.raises(ValueError):  # checked before any device work, as in the reference
        t.nn_match_two_way(d, d, -0.1)
    # an empty side returns before the threshold check (models/model_wrap.py:472-475)
    assert t.nn_match_two_way(np.zeros((256, 0)), d, -0.1).shape == (3, 0)


def test_g15_goldens_load():
    g = G.load("g15_descriptor_ssp_120x160.npz")
    for k in ("homography", "matches", "mscores", "conf_thresh", "nn_thresh", "seed", "desc_rows", "coarse_desc"):
        assert k in g, k
    assert g["coarse_desc"].shape == (1, 256, 15, 20)
    img, warped, hom = descriptor_case_images(int(g["seed"]))
    assert img.shape == warped.shape == (120, 160) and np.array_equal(hom, g["homography"])
    for t in ("", "warped_"):
        n = g[t + "pts"].shape[0]
        assert g[t + "heatmap"].shape == (120, 160)
        assert g[t + "pts_int"].shape == (n, 3) and g[t + "pts"].shape == (n, 3)
        assert g[t + "desc"].shape == (min(n, int(g["desc_rows"])), 256) and g[t + "desc"].dtype == np.float32
        assert 100 <= n <= 1000
    assert g["matches"].shape[1] == 4 and g["mscores"].shape == (g["matches"].shape[0], 3)
    m = G.load("g15_match_cases.npz")
    for name, seed, n1, n2, thr in MATCH_CASES:
        assert list(m[name + "/seed"]) == [seed, n1, n2]
        assert m[name + "/matches"].shape[1] == 3
        d1, d2 = match_case_inputs(name, seed, n1, n2)
        assert d1.shape == (256, n1) and d2.shape == (256, n2)
