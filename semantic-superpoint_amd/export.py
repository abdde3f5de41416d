"""Drop-in for the homography-adaptation branch of the reference's export.py.

Same names as the reference so that its call sites read unchanged:
  combine_heatmap(heatmap, inv_homographies, mask_2D, device)        export.py:49-60
  SuperPointFrontend_torch(...).run / getPtsFromHeatmap / nms_fast / soft_argmax_points
                                                                     models/model_wrap.py:60-293
  export_detector_homoAdapt_gpu(config, output_dir, args)            export.py:192-352
plus `HomoAdaptExporter`, the fused MI355X path the loop uses: one ssp_export_points call per pair of images
(forward of the detector head over the views in train-mode BatchNorm, softmax -> depth-to-space, masked un-warp
accumulation, greedy NMS, soft-argmax refinement, top-k) with no host round trip before the final point list.

The descriptor export (keypoints, sparse descriptors and two-way matches of image pairs):
  PointTracker(max_length, nn_thresh).nn_match_two_way / update / get_matches / get_mscores / clear_desc / get_tracks /
  get_offsets (2 <= max_length <= 16; plus update_device / track_points)          models/model_wrap.py:426-615
  SequenceTracker: forward -> points / descriptors -> match -> track update per frame, all on the device
  (both live in tracker.py and are re-exported here)
  export_descriptor(config, output_dir, args)                        export.py:66-190
with `Val_model_heatmap` (Val_model_heatmap.py) as the per-image front end and `DescriptorExporter`, the fused path the
loop uses: ONE eval forward over the 2P images of P pairs, keypoints + sparse descriptors (ssp_describe_points) and the
matcher (ssp_match_two_way) on the device, then one read of the counts and sized copies.
  evaluate_descriptor(config, args): the same loop feeding evaluation.StreamingEvaluator: the metrics, no files.

Every arithmetic step runs in libssp_hip.so; tensors must live on a HIP device (no CPU fallback).  The dense-descriptor
branch of SuperPointFrontend_torch.run (`onlyHeatmap=False`) is not provided and raises.
"""
import logging
import os
from pathlib import Path

import numpy as np
import torch

from . import lib as L
from .tracker import PointTracker, SequenceTracker, _image_2d, _matches_to_numpy  # noqa: F401 (re-exported)


def _dev_f32(t, device):
    t = torch.as_tensor(t)
    return t.to(device=device, dtype=torch.float32).contiguous()


def combine_heatmap(heatmap, inv_homographies, mask_2D, device="cpu"):
    """export.py:49-60.  heatmap, mask_2D: [N,1,H,W]; inv_homographies: [1,N,3,3] (the reference indexes [0]).
    Returns the [1,H,W] aggregate sum(unwarp(heatmap*mask)) / sum(unwarp(mask)) on the tensors' HIP device."""
    dev = heatmap.device
    mask = _dev_f32(mask_2D, dev)
    heat = (heatmap.to(torch.float32) * mask).contiguous()
    hm = inv_homographies[0] if inv_homographies.dim() == 4 else inv_homographies
    return L.op_combine_heatmap(heat, mask, _dev_f32(hm, dev)).unsqueeze(0)


class SuperPointFrontend_torch(object):
    """The subset of models/model_wrap.py:SuperPointFrontend_torch that the homography-adaptation export uses."""

    def __init__(self, config, weights_path, nms_dist, conf_thresh, nn_thresh, cuda=False, trained=False, device="cpu",
                 grad=False, load=True):
        self.config = config
        self.name = "SuperPoint"
        self.nms_dist, self.conf_thresh, self.nn_thresh = nms_dist, conf_thresh, nn_thresh
        self.cell, self.border_remove = 8, 4  # models/model_wrap.py:69-70
        self.device = torch.device(device)
        self.subpixel = bool(config["model"]["subpixel"]["enable"])
        self.sparsemap = self.pts = self.pts_subpixel = self.patches = None
        self._heatmap = None
        self.net = None
        if load:
            self.loadModel(weights_path)

    @property
    def heatmap(self):
        return self._heatmap

    @heatmap.setter
    def heatmap(self, heatmap):
        self._heatmap = heatmap

    def loadModel(self, weights_path):
        """models/model_wrap.py:84-121: config['model']['name'](**params) + checkpoint['model_state_dict'];
        the network stays in TRAIN mode (the reference never calls .eval() here)."""
        import importlib
        name = self.config["model"]["name"]
        mod = importlib.import_module(__package__ + ".models." + name)
        self.net = getattr(mod, name)(**self.config["model"].get("params", {}))
        if weights_path:
            ckpt = torch.load(weights_path, map_location="cpu")
            self.net.load_state_dict(ckpt["model_state_dict"] if "model_state_dict" in ckpt else ckpt)
        self.net = self.net.to(self.device)

    def net_parallel(self):
        """nn.DataParallel in the reference (models/model_wrap.py:123-125).  Here: one process per GPU, images
        sharded across ranks by export_detector_homoAdapt_gpu -- nothing to wrap."""
        return None

    def run(self, inp, onlyHeatmap=False, train=True):
        """models/model_wrap.py:338-372 up to `if onlyHeatmap: return heatmap`."""
        if not onlyHeatmap:
            raise NotImplementedError("descriptor export is outside the MI355X hot path (SURVEY.md section 8)")
        inp = inp.to(self.device)
        if train:
            semi = self.net(inp)["semi"]
        else:
            with torch.no_grad():
                semi = self.net(inp)["semi"]
        self.heatmap = L.op_flatten_detection(semi.contiguous())
        return self.heatmap

    def getPtsFromHeatmap(self, heatmap):
        """models/model_wrap.py:266-293: [H,W] heatmap (numpy or tensor, any device) -> float64 3xN (x, y, conf)."""
        hm = _dev_f32(heatmap, self.device).squeeze()
        self.sparsemap = (hm >= float(np.float32(self.conf_thresh))).cpu().numpy()
        return L.op_heatmap_points(hm, self.conf_thresh, self.nms_dist, self.border_remove).T

    def nms_fast(self, in_corners, H, W, dist_thresh):
        """models/model_wrap.py:129-192 for corners at distinct integer pixels: returns (3xN kept corners by
        descending confidence, their indices into in_corners)."""
        n = in_corners.shape[1]
        if n == 0:
            return np.zeros((3, 0)).astype(int), np.zeros(0).astype(int)
        rc = in_corners[:2].round().astype(np.int64)
        flat = rc[1] * W + rc[0]
        if len(np.unique(flat)) != n:
            raise ValueError("nms_fast: corners must round to distinct pixels")
        conf = in_corners[2].astype(np.float32)
        # order-preserving remap to (0, 1]: the device kernel ranks by the fp32 value itself
        grid = torch.full((H * W,), float("nan"))
        grid[torch.from_numpy(flat)] = torch.from_numpy(conf)
        out = L.op_heatmap_points(grid.view(H, W).to(self.device), -np.inf, dist_thresh, 0)
        inds = np.full(H * W, -1, np.int64)
        inds[flat] = np.arange(n)
        keep = inds[(out[:, 1] * W + out[:, 0]).astype(np.int64)]
        return in_corners[:, keep], keep

    def soft_argmax_points(self, pts, patch_size=5):
        """models/model_wrap.py:212-249: pts = [3xN]; returns [3xN] with (x, y) moved by the 5x5 soft-argmax of
        self.heatmap."""
        assert patch_size == 5, "the device kernel implements the 5x5 patch the reference uses"
        p = pts[0].transpose().copy()
        hm = _dev_f32(self.heatmap, self.device).squeeze()
        xy = torch.from_numpy(np.ascontiguousarray(p[:, :2]).astype(np.float32)).to(self.device)
        d = L.op_soft_argmax_points(hm, xy).cpu().numpy()
        p[:, :2] = p[:, :2] + d - patch_size // 2
        self.pts_subpixel = [p.transpose().copy()]
        return self.pts_subpixel.copy()


class HomoAdaptExporter:
    """Fused export of image PAIRS on one GPU.  `net` is one of this package's model drop-ins (its Engine is created
    for n_views x H x W on first use)."""

    def __init__(self, net, device, conf_thresh, nms_dist, top_k, subpixel, border_remove=4):
        self.net, self.device = net, torch.device(device)
        self.args = dict(conf_thresh=conf_thresh, nms_dist=nms_dist, top_k=top_k, subpixel=subpixel,
                         border_remove=border_remove)

    def __call__(self, samples, want_heatmap=False):
        """samples: 1 or 2 dicts with "image" [n,1,H,W] (the warped views), "valid_mask" [n,1,H,W] and
        "homographies" [n,3,3] (the un-warp matrices, see combine_heatmap).  Returns one float64 [N,3] array per
        sample (+ the aggregated heatmaps when asked)."""
        views = [_dev_f32(s["image"], self.device) for s in samples]
        masks = [_dev_f32(s["valid_mask"], self.device) for s in samples]
        hms = [_dev_f32(s["homographies"], self.device) for s in samples]
        n, _, h, w = views[0].shape
        eng = self.net.engine(n, h, w, self.device)
        outs = eng.export_points(views, masks, hms, want_heatmap=want_heatmap, **self.args)
        pts = [L.points_to_numpy(o["pts"], o["count"], self.args["subpixel"]) for o in outs]
        return (pts, [o["heatmap"] for o in outs]) if want_heatmap else pts


def export_detector_homoAdapt_gpu(config, output_dir, args):
    """export.py:192-352: pseudo ground truth by homography adaptation, one `<name>.npz {"pts": [N,3]}` per image.
    The data loader is the HOST repository's (`utils.loader.dataLoader_test`, as in the reference); images are
    sharded over ranks when torch.distributed is initialised (replaces nn.DataParallel)."""
    from utils.loader import dataLoader_test as dataLoader  # the reference's own loader (export.py:236-239)

    task = config["data"]["dataset"]
    export_task = config["data"]["export_folder"]
    if not torch.cuda.is_available():
        raise RuntimeError("export_detector_homoAdapt_gpu needs a HIP device: there is no CPU fallback")
    rank, world = 0, 1
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        rank, world = torch.distributed.get_rank(), torch.distributed.get_world_size()
    device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", 0)))
    mcfg = config["model"]
    save_output = Path(output_dir) / "predictions" / export_task
    os.makedirs(Path(output_dir) / "checkpoints", exist_ok=True)
    os.makedirs(save_output, exist_ok=True)

    fe = SuperPointFrontend_torch(config=config, weights_path=config["pretrained"], nms_dist=mcfg["nms"],
                                  conf_thresh=mcfg["detection_threshold"], nn_thresh=0.7, cuda=False, device=device)
    fe.net_parallel()
    exporter = HomoAdaptExporter(fe.net, device, fe.conf_thresh, fe.nms_dist, mcfg["top_k"], fe.subpixel,
                                 fe.border_remove)
    if rank == 0:
        with open(save_output / "export.txt", "a") as f:
            f.write("load model: %s\n" % config["pretrained"])
            f.write("homography adaptation: %s\n" % config["data"]["homography_adaptation"]["num"])

    test_loader = dataLoader(config, dataset=task, export_task=export_task)["test_loader"]
    pending, count = [], 0

    def flush():
        nonlocal count
        if not pending:
            return
        for (name, scene), pts in zip([p[0] for p in pending], exporter([p[1] for p in pending])):
            if scene is not None:
                os.makedirs(Path(save_output, scene), exist_ok=True)
            np.savez_compressed(Path(save_output, "{}.npz".format(name)), pts=pts)
            count += 1
        pending.clear()

    for i, sample in enumerate(test_loader):
        if i % world != rank:
            continue
        name = sample["name"][0]
        if Path(save_output, "{}.npz".format(name)).exists():
            logging.info("file %s exists. skip the sample.", name)
            continue
        # loader batch of 1: image [1,n,H,W] -> [n,1,H,W]; the un-warp matrices are sample["homographies"]
        # (export.py:281-284 binds them to the name inv_homographies before combine_heatmap)
        s = {"image": sample["image"].transpose(0, 1), "valid_mask": sample["valid_mask"].transpose(0, 1),
             "homographies": sample["homographies"][0]}
        pending.append(((name, sample["scene_name"][0] if "scene_name" in sample else None), s))
        if len(pending) == 2:
            flush()
    flush()
    logging.info("output pseudo ground truth: %d", count)
    if rank == 0:
        with open(save_output / "export.txt", "a") as f:
            f.write("output pairs: %d\n" % count)
    return count


class DescriptorExporter:
    """Fused descriptor export of image PAIRS on one GPU.  `net` is one of this package's model drop-ins (its Engine
    is created / grown for 2 x batch_pairs x H x W on first use).  Eval-mode BatchNorm computes every image on its own,
    but the engine picks its convolution kernels by batch size (last-bit differences in the heatmap move points that sit
    at the threshold), so the forward always runs over 2 x batch_pairs images, zero-padded: a pair's result does not
    depend on how many pairs share its call."""

    def __init__(self, net, device, conf_thresh, nms_dist, subpixel, nn_thresh, border_remove=4, batch_pairs=16, classes=False):
        if nn_thresh < 0.0:
            raise ValueError("'nn_thresh' should be non-negative")
        if classes and not hasattr(net, "convSout"):
            raise ValueError("classes=True needs a model with a segmentation head")
        self.classes = bool(classes)  # run_device adds "cls": uint8 [2P,cap], the class at each keypoint
        self.net, self.device = net, torch.device(device)
        self.conf_thresh, self.nms_dist, self.subpixel = conf_thresh, nms_dist, bool(subpixel)
        self.nn_thresh, self.border_remove = nn_thresh, border_remove
        self.batch_pairs = int(batch_pairs)

    def run_device(self, pairs):
        """pairs: list of (image, warped_image), each [H,W] / [1,H,W] / [1,1,H,W].  Returns the device tensors of the
        batch: {"pts": [2P,cap,5], "count": [2P], "desc": [2P,cap,256], "match": [P,cap,3], "n_match": [P]} (image
        2p = pair p's image, 2p + 1 its warped image); no host synchronisation."""
        if not 1 <= len(pairs) <= self.batch_pairs:
            raise ValueError("1 to %d pairs per call (got %d)" % (self.batch_pairs, len(pairs)))
        ims = []
        for a, b in pairs:
            ims += [_image_2d(a), _image_2d(b)]
        n = len(ims)
        h, w = ims[0].shape
        x = torch.zeros(2 * self.batch_pairs, 1, h, w, dtype=torch.float32, device=self.device)
        x[:n, 0] = torch.stack([t.to(self.device, torch.float32) for t in ims])
        eng = self.net.engine(x.shape[0], h, w, self.device)
        with torch.no_grad():
            eng.forward(x, slot=0, train=False, want=())
        o = eng.describe_points(0, n, conf_thresh=self.conf_thresh, nms_dist=self.nms_dist, subpixel=self.subpixel,
                                border_remove=self.border_remove, classes=self.classes)
        o["match"], o["n_match"] = L.op_match_two_way(o["desc"], o["count"], o["desc"][1:], o["count"][1:],
                                                      self.nn_thresh, pair_stride=2, n_pairs=len(pairs))
        return o

    def __call__(self, pairs, homographies=None):
        """Returns one `pred` dict per pair with the keys and layouts of export.py:145-183: image, warped_image,
        prob / warped_prob (float64 [N,3], subpixel when enabled), desc / warped_desc (float32 [N,256], sampled at the
        integer points), matches (float64 [L,4] = x0, y0, x1, y1) and homography when given."""
        o = self.run_device(pairs)
        counts = o["count"].cpu().numpy()
        n_match = o["n_match"].cpu().numpy()
        preds = []
        for p, (a, b) in enumerate(pairs):
            pred = {}
            probs = []
            for k, tag in ((2 * p, ""), (2 * p + 1, "warped_")):
                c = int(counts[k])
                prob = L.points_to_numpy(o["pts"][k], torch.tensor(c), self.subpixel)
                pred[tag + "prob"] = prob
                pred[tag + "desc"] = o["desc"][k, :c].cpu().numpy()
                probs.append(prob)
            pred["image"] = _image_2d(a).detach().cpu().numpy()
            pred["warped_image"] = _image_2d(b).detach().cpu().numpy()
            m = _matches_to_numpy(o["match"][p], int(n_match[p]))
            idx0, idx1 = m[0].astype(int), m[1].astype(int)
            pred["matches"] = np.concatenate((probs[0][idx0, :2], probs[1][idx1, :2]), axis=1)
            if homographies is not None:
                pred["homography"] = np.asarray(homographies[p])
            preds.append(pred)
        return preds


def export_descriptor(config, output_dir, args, test_loader=None, pairs_per_flush=16):
    """export.py:66-190: keypoints, descriptors and matches of (image, warped_image) pairs, one `<count>.npz` per pair
    under output_dir/checkpoints/../predictions.  The front end is `Val_model_heatmap` of this package (config["model"]:
    name, params, pretrained, nms, detection_threshold, nn_thresh, subpixel.enable).  test_loader: any iterable of
    samples with "image", "warped_image" ([1,1,H,W]) and "homography"; default = the HOST repository's
    utils.loader.dataLoader_test, as in the reference.  Pairs are batched `pairs_per_flush` at a time and sharded over
    ranks when torch.distributed is initialised (rank r writes the pairs i with i % world == r, named by i)."""
    import yaml
    from .Val_model_heatmap import Val_model_heatmap

    if not torch.cuda.is_available():
        raise RuntimeError("export_descriptor needs a HIP device: there is no CPU fallback")
    rank, world = 0, 1
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        rank, world = torch.distributed.get_rank(), torch.distributed.get_world_size()
    device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", 0)))
    os.makedirs(output_dir, exist_ok=True)
    if rank == 0:
        with open(os.path.join(output_dir, "config.yml"), "w") as f:
            yaml.dump(config, f, default_flow_style=False)
    save_path = Path(output_dir) / "checkpoints"
    os.makedirs(save_path, exist_ok=True)
    save_output = save_path / "../predictions"
    os.makedirs(save_output, exist_ok=True)

    mcfg = config["model"]
    subpixel = bool(mcfg.get("subpixel", {}).get("enable", False))
    patch_size = mcfg.get("subpixel", {}).get("patch_size", 5)
    if subpixel and patch_size != 5:
        raise ValueError("the device soft-argmax implements the 5x5 patch of the reference configs")
    if test_loader is None:
        from utils.loader import dataLoader_test as dataLoader  # the reference's own loader (export.py:100-104)
        test_loader = dataLoader(config, dataset=config["data"]["dataset"])["test_loader"]
    agent = Val_model_heatmap(mcfg, device=device)
    agent.loadModel()
    exporter = DescriptorExporter(agent.net, device, agent.conf_thresh, agent.nms_dist, subpixel, agent.nn_thresh,
                                  agent.border_remove, batch_pairs=pairs_per_flush)
    pending, count = [], 0

    def flush():
        nonlocal count
        if not pending:
            return
        preds = exporter([(s["image"], s["warped_image"]) for _, s in pending],
                         homographies=[_squeeze_np(s["homography"]) for _, s in pending])
        for (i, _), pred in zip(pending, preds):
            np.savez_compressed(Path(save_output, "{}.npz".format(i)), **pred)
            count += 1
        pending.clear()

    for i, sample in enumerate(test_loader):
        if i % world != rank:
            continue
        pending.append((i, sample))
        if len(pending) == pairs_per_flush:
            flush()
    flush()
    logging.info("output pairs: %d", count)
    return count


def evaluate_descriptor(config, args, test_loader=None, pairs_per_flush=16):
    """export_descriptor's loop feeding an evaluation.StreamingEvaluator instead of writing `.npz` files: the -r -homo
    metrics of the reference's `evaluation.py` over the loader's pairs with no export on disk and one host read at the
    end.  Same config and loader as export_descriptor.  args: `repeatibility` / `homography` as evaluation.evaluate
    reads them (both on when args is None or lacks them).  Returns StreamingEvaluator.result(); under torch.distributed
    each rank evaluates the pairs i with i % world == rank and returns the summary of that shard (its pairs are
    numbered in the shard's own order)."""
    from .Val_model_heatmap import Val_model_heatmap
    from .evaluation import StreamingEvaluator

    if not torch.cuda.is_available():
        raise RuntimeError("evaluate_descriptor needs a HIP device: there is no CPU fallback")
    rank, world = 0, 1
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        rank, world = torch.distributed.get_rank(), torch.distributed.get_world_size()
    device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", 0)))
    mcfg = config["model"]
    subpixel = bool(mcfg.get("subpixel", {}).get("enable", False))
    if subpixel and mcfg.get("subpixel", {}).get("patch_size", 5) != 5:
        raise ValueError("the device soft-argmax implements the 5x5 patch of the reference configs")
    if test_loader is None:
        from utils.loader import dataLoader_test as dataLoader  # the reference's own loader (export.py:100-104)
        test_loader = dataLoader(config, dataset=config["data"]["dataset"])["test_loader"]
    if not hasattr(test_loader, "__len__"):
        test_loader = list(test_loader)
    agent = Val_model_heatmap(mcfg, device=device)
    agent.loadModel()
    exporter = DescriptorExporter(agent.net, device, agent.conf_thresh, agent.nms_dist, subpixel, agent.nn_thresh,
                                  agent.border_remove, batch_pairs=pairs_per_flush)
    rep_on, homo_on = bool(getattr(args, "repeatibility", True)), bool(getattr(args, "homography", True))
    capacity = max(1, (len(test_loader) + world - 1 - rank) // world)
    ev, pending = None, []

    def flush():
        nonlocal ev
        if not pending:
            return
        if ev is None:
            h, w = _image_2d(pending[0]["image"]).shape
            ev = StreamingEvaluator(h, w, device, capacity, repeatability=rep_on, homography=homo_on)
        o = exporter.run_device([(s["image"], s["warped_image"]) for s in pending])
        ev.update_device(o, np.stack([_squeeze_np(s["homography"]) for s in pending]), subpixel=subpixel)
        pending.clear()

    for i, sample in enumerate(test_loader):
        if i % world != rank:
            continue
        pending.append(sample)
        if len(pending) == pairs_per_flush:
            flush()
    flush()
    if ev is None:
        raise ValueError("the loader gave this rank no pair")
    res = ev.result()
    logging.info("evaluated pairs: %d", res["pairs"])
    return res


def _squeeze_np(t):
    return (t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)).squeeze()
