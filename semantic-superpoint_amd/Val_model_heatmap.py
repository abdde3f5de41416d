"""Drop-in for the reference's Val_model_heatmap.py:33-186 (the `front_end_model` of export_descriptor, export.py:117-123):
eval-mode forward, keypoints, sparse descriptors on the MI355X.

The reference loads it by name: `get_module("", config["front_end_model"])` imports a top-level module
`Val_model_heatmap` (utils/loader.py:157-164); a stub next to export.py re-exports this class.

  run(images)           forward in eval mode (BatchNorm running statistics) + flattenDetection -> numpy [B,1,H,W]
  heatmap_to_pts()      getPtsFromHeatmap per image -> list of float64 [3,N] (x, y, conf)
  soft_argmax_points    inherited (SuperPointFrontend_torch): the first image's points, 5x5 soft-argmax
  desc_to_sparseDesc()  sample_desc_from_points per image -> list of float32 [256,N] unit columns

heatmap_to_pts and desc_to_sparseDesc come from ONE ssp_describe_points launch sequence over the batch; image k samples
its own descriptor map.  (The reference's grid_sample call has batch 1 and fails for a batch > 1: an extension.)
"""
import importlib

import numpy as np
import torch

from .export import SuperPointFrontend_torch


class Val_model_heatmap(SuperPointFrontend_torch):
    def __init__(self, config, device="cpu", verbose=False):
        # (the reference does not call the base constructor either: `config` is the model section of the yaml)
        self.config = config
        self.model = config["name"]
        self.params = config.get("params", {}) or {}
        self.weights_path = config.get("pretrained")
        self.device = torch.device(device)
        self.name = "SuperPoint"
        self.nms_dist = config["nms"]
        self.conf_thresh = config["detection_threshold"]
        self.nn_thresh = config["nn_thresh"]  # L2 descriptor distance for good match
        self.cell = 8
        self.cell_size = 8
        self.border_remove = 4
        self.subpixel = True  # soft_argmax_points is the caller's choice (export.py:131-132)
        self.sparsemap = None
        self._heatmap = None  # np [batch, 1, H, W]
        self.pts = None
        self.pts_subpixel = None
        self.pts_nms_batch = None
        self.desc_sparse_batch = None
        self.patches = None
        self.outs = None
        self.net = None
        self._described = None

    def loadModel(self):
        """Val_model_heatmap.py:62-106: the named network, .eval(), then `model_state_dict` of a full checkpoint or a bare
        state dict (the sener-style fallback of the reference is not supported)."""
        mod = importlib.import_module(__package__ + ".models." + self.model)
        self.net = getattr(mod, self.model)(**self.params)
        self.net.eval()
        if self.weights_path:
            ckpt = torch.load(self.weights_path, map_location="cpu")
            self.net.load_state_dict(ckpt["model_state_dict"] if "model_state_dict" in ckpt else ckpt)
        self.net = self.net.to(self.device)
        self.net.eval()

    def _engine(self, n, h, w):
        if self.device.type != "cuda":
            raise RuntimeError("Val_model_heatmap needs a HIP device: there is no CPU fallback")
        return self.net.engine(n, h, w, self.device)

    def run(self, images):
        """Val_model_heatmap.py:123-148: images [B,1,H,W] -> numpy heatmap [B,1,H,W]; self.outs = {"semi", "desc"}."""
        x = torch.as_tensor(images).to(self.device, torch.float32).contiguous()
        n, _, h, w = x.shape
        eng = self._engine(n, h, w)
        with torch.no_grad():
            self.outs = eng.forward(x, slot=0, train=False, want=("semi", "desc"))
            heat = eng.detector_heatmap(0, n, h, w)
        self._described = None
        self.heatmap = heat.cpu().numpy()
        return self.heatmap

    def _describe(self):
        if self._described is None:
            if self.heatmap is None:
                raise RuntimeError("run(images) first")
            n = self.heatmap.shape[0]
            o = self.net.engine().describe_points(0, n, conf_thresh=self.conf_thresh, nms_dist=self.nms_dist,
                                                  subpixel=False, border_remove=self.border_remove)
            counts = o["count"].cpu().numpy()
            self._described = (o, counts)
        return self._described

    def heatmap_to_pts(self):
        """Val_model_heatmap.py:151-156: getPtsFromHeatmap of every image -> list of float64 [3,N]."""
        o, counts = self._describe()
        pts = o["pts"].cpu().numpy()
        self.pts_nms_batch = [pts[k, :c, :3].astype(np.float64).T.copy() for k, c in enumerate(counts)]
        return self.pts_nms_batch

    def desc_to_sparseDesc(self):
        """Val_model_heatmap.py:181-185: the descriptors of the integer points of heatmap_to_pts -> list of float32
        [256,N]; image k is sampled from its own descriptor map."""
        o, counts = self._describe()
        self.desc_sparse_batch = [o["desc"][k, :c].cpu().numpy().T.copy() for k, c in enumerate(counts)]
        return self.desc_sparse_batch
