"""G15 fixtures of the descriptor export (export.py:66-190), produced by the REAL reference on the CPU.

  g15_descriptor_ssp_120x160.npz   Val_model_heatmap (eval mode, subpixel on, nms 4) on an image and its warped copy
                                   (regenerated from the seed: tests/golden_descriptor.py), then
                                   PointTracker(max_length=2, nn_thresh=1.0).update twice: both heatmaps, the image's coarse
                                   desc (NCHW), integer and subpixel points, the sparse descriptors of the DESC_ROWS most
                                   confident points of each image, matches and mscores
  g15_match_cases.npz              PointTracker.nn_match_two_way on descriptor sets regenerated from numpy seeds
                                   (tests/golden_descriptor.py): the seeds and the outputs only

Needs the reference checkout (oracle/ref_harness.py); run from the repository root:  python tools/make_golden_descriptor.py
"""
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import cpu_ref as C  # noqa: E402
from oracle import ref_harness as R  # noqa: E402
from tests.golden_descriptor import DESC_H, DESC_W, MATCH_CASES, descriptor_case_images, match_case_inputs  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
ARCH, H, W, SEED, THR, NN = "SuperPointNet_gauss2_ssmall", DESC_H, DESC_W, 15, 0.0157, 1.0
DESC_ROWS = 96  # sparse descriptors stored per image (the fixture stays small; the points are all stored)


def descriptor_case():
    R.install()
    from Val_model_heatmap import Val_model_heatmap
    from models.model_wrap import PointTracker
    img, warped, hom = descriptor_case_images(SEED)
    sd = C.init_state_dict(ARCH, seed=SEED)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "w.pth")
        torch.save({k: torch.as_tensor(np.array(v)) for k, v in sd.items()}, path)
        cfg = {"name": ARCH, "params": {}, "pretrained": path, "nms": 4, "detection_threshold": THR, "nn_thresh": NN}
        agent = Val_model_heatmap(cfg, device="cpu")
        agent.loadModel()
    tracker = PointTracker(max_length=2, nn_thresh=agent.nn_thresh)
    out = {}
    for tag, im in (("", img), ("warped_", warped)):
        x = torch.from_numpy(im)[None, None]
        heat = agent.run(x)                       # export.py:126-142 get_pts_desc_from_agent
        pts = agent.heatmap_to_pts()
        pts_int = pts[0].copy()
        pts = agent.soft_argmax_points(pts, patch_size=5)
        desc = agent.desc_to_sparseDesc()
        tracker.update(pts[0], desc[0])
        conf = pts_int[2]
        assert len(np.unique(conf.astype(np.float32))) == len(conf), "G15: tie among kept points, pick another seed"
        hm = heat[0, 0]
        cand = np.sort(hm[hm >= np.float32(THR)])
        gap = np.min(np.diff(cand)) if len(cand) > 1 else 1.0
        margin = float(np.min(np.abs(hm - np.float32(THR))))
        # equal-confidence candidates only matter to the greedy order when they can suppress each other (as G8)
        cm = np.where(hm >= np.float32(THR), hm, -1.0)
        for dy in range(-4, 5):
            for dx in range(-4, 5):
                if (dy, dx) > (0, 0):
                    a = cm[max(dy, 0):H + min(dy, 0), max(dx, 0):W + min(dx, 0)]
                    b = cm[max(-dy, 0):H + min(-dy, 0), max(-dx, 0):W + min(-dx, 0)]
                    assert not np.any((a == b) & (a > 0)), "G15: tie inside an NMS window, pick another seed"
        print("  %simage: %d candidates, %d kept, threshold margin %.3g, min candidate gap %.3g"
              % (tag, len(cand), pts_int.shape[1], margin, gap))
        out[tag + "heatmap"] = hm.astype(np.float32)
        if tag == "":
            out["coarse_desc"] = agent.outs["desc"].detach().numpy().astype(np.float32)
        out[tag + "pts_int"] = pts_int.T.copy()
        out[tag + "pts"] = pts[0].T.copy()
        out[tag + "desc"] = desc[0].T[:DESC_ROWS].astype(np.float32)
    out["matches"] = tracker.get_matches().T.copy()
    out["mscores"] = tracker.get_mscores().T.copy()
    print("  %d matches" % out["matches"].shape[0])
    np.savez_compressed(os.path.join(OUT, "g15_descriptor_ssp_120x160.npz"), arch=ARCH, seed=SEED, conf_thresh=THR,
                        nms=4, nn_thresh=NN, desc_rows=DESC_ROWS, homography=hom, **out)


def match_cases():
    R.install()
    from models.model_wrap import PointTracker
    out = {}
    for name, seed, n1, n2, thr in MATCH_CASES:
        d1, d2 = match_case_inputs(name, seed, n1, n2)
        m = PointTracker(max_length=2, nn_thresh=thr).nn_match_two_way(d1, d2, thr)
        if name == "dup":  # the duplicated columns of d2 never win over their first copy (np.argmin: first index)
            for b in (17, 40, 9, 61):
                assert not np.any(m[1] == b), "G15 dup: a later duplicate won"
        print("  %s: %d x %d -> %d matches" % (name, n1, n2, m.shape[1]))
        out[name + "/seed"] = np.array([seed, n1, n2])
        out[name + "/nn_thresh"] = np.float64(thr)
        out[name + "/matches"] = m.T.copy()
    np.savez_compressed(os.path.join(OUT, "g15_match_cases.npz"), **out)


if __name__ == "__main__":
    torch.manual_seed(0)
    descriptor_case()
    match_cases()
