"""Detector evaluation against ground-truth corners on the device: the true / false positives, the precision-recall curve, mAP
and the localisation error of the reference's evaluations/detector_evaluation.py:15-136 (compute_tp_fp, compute_pr,
compute_mAP, compute_loc_error), the numbers of the SuperPoint paper's Synthetic Shapes table.  The rules, the tie rule and
what is exact against what are DESIGN.md section 19.

  DetectorEvaluator   streams a validation set batch by batch (dense heat maps or the exporter's point lists); nothing is
                      copied to the host until the curve is asked for, and then only the small state block.
  compute_tp_fp, compute_pr, compute_mAP, compute_loc_error   drop-ins under the reference's names for its per-image .npz
                      layout (`prob`, optional `prob_nms`, `keypoint_map`); a directory stands where the reference takes an
                      experiment name under its EXPER_PATH.
  evaluate_detector   a net or an Engine over a loader of `image` / `labels_2D` batches (shapes.SyntheticShapes(cfg, "val")).

Order of equal probabilities (numpy's argsort leaves it undefined, so does the reference): descending probability, among
equals the later record first, np.argsort(kind="stable")[::-1]; a record's index is image order, then the row-major pixel
index (the list position for point lists)."""
import glob
import os
import warnings

import numpy as np
import torch

from . import lib as L


class DetectorEvaluator:
    """Accumulates compute_tp_fp records of images of one size on `device`.  capacity: the largest number of records
    (predictions above remove_zero) the whole set may hold; they cost 8 bytes each (reserve() grows it).
    prob_thresh >= remove_zero: the localisation error is measured on candidates, which are the predictions above remove_zero.
    Synchronisation: update() makes none.  The first compute_pr() / compute_loc_error() / result() after an update reads the
    small state block once; compute_mAP() / result() read one more scalar, the sum the curve kernel left, once."""

    def __init__(self, height, width, device, capacity, remove_zero=1e-4, distance_thresh=2, prob_thresh=0.5, simplified=False):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("DetectorEvaluator needs a HIP device (got %s): no CPU fallback exists" % self.device)
        self.height, self.width, self.capacity = int(height), int(width), int(capacity)
        if not 1 <= self.capacity < 2 ** 31:
            raise ValueError("1 <= capacity < 2^31 records required (got %d)" % self.capacity)
        self.remove_zero, self.prob_thresh = float(remove_zero), float(prob_thresh)
        if not np.float32(self.prob_thresh) >= np.float32(self.remove_zero) >= 0:
            raise ValueError("prob_thresh >= remove_zero >= 0 required (got prob_thresh %r, remove_zero %r): predictions at or "
                             "below remove_zero are no candidates, so compute_loc_error could not count them"
                             % (prob_thresh, remove_zero))
        self.distance_thresh, self.simplified = distance_thresh, bool(simplified)
        self.r2 = L.detector_eval_r2(distance_thresh)
        if not 0 <= self.r2 <= L.DET_EVAL_MAX_R2:
            raise ValueError("distance_thresh %r is outside the supported range (0 <= squared radius <= %d)"
                             % (distance_thresh, L.DET_EVAL_MAX_R2))
        self.keys = torch.empty(self.capacity, dtype=torch.int64, device=self.device)
        self.state = L.detector_eval_state(self.device)
        self._ws = None
        self._final = None

    def reset(self):
        self.state.zero_()
        self._final = None

    def reserve(self, capacity):
        """Grow the record buffer to `capacity` records and keep what was fed (a device copy, no synchronisation)."""
        capacity = int(capacity)
        if capacity <= self.capacity:
            return
        if capacity >= 2 ** 31:
            raise ValueError("1 <= capacity < 2^31 records required (got %d)" % capacity)
        keys = torch.empty(capacity, dtype=torch.int64, device=self.device)
        keys[:self.capacity].copy_(self.keys)
        self.keys, self.capacity = keys, capacity
        self._final = None

    def _kw(self):
        return dict(remove_zero=self.remove_zero, r2=self.r2, prob_thresh=self.prob_thresh, simplified=self.simplified, ws=self._ws)

    def update(self, prob=None, labels=None, pts=None, count=None):
        """One batch: update(prob=[B,H,W] or [B,1,H,W] float32, labels=...) or update(pts=[B,cap,5] float32, count=[B] int32,
        labels=...); labels float32 or uint8, nonzero = ground truth.  No host copy, no synchronisation."""
        if labels is None or (prob is None) == (pts is None):
            raise ValueError("update(prob=, labels=) or update(pts=, count=, labels=)")
        if tuple(labels.shape[-2:]) != (self.height, self.width):
            raise ValueError("labels are %s, the evaluator was made for %dx%d" % (tuple(labels.shape), self.height, self.width))
        self._final = None
        labels = labels.contiguous()
        if prob is not None:
            self._ws = L.op_detector_tp_fp(prob.contiguous(), labels, self.keys, self.state, **self._kw())
        else:
            if count is None:
                raise ValueError("update(pts=...) needs count")
            self._ws = L.op_detector_tp_fp_points(pts.contiguous(), count.contiguous(), labels, self.keys, self.state, **self._kw())

    def _finalize(self):
        if self._final is None:
            st = self.state.cpu().numpy()  # the state read: records, n_gt, overflow flag, rows outside, d2 histogram
            n = int(st[0])
            if st[2] != 0 or n > self.capacity:
                raise RuntimeError("DetectorEvaluator: %d records were fed but capacity is %d: make the evaluator with a larger "
                                   "capacity (reset() empties this one)" % (n, self.capacity))
            out = L.op_detector_pr_curve(torch.sort(self.keys[:n], descending=True).values, self.state)
            out["n_gt"] = int(st[1])
            out["outside_points"] = int(st[L.DET_EVAL_OUTSIDE])
            if out["outside_points"]:
                warnings.warn("DetectorEvaluator: %d point-list rows lie outside the %dx%d image and were skipped: are the "
                              "points in the labels' pixel units?" % (out["outside_points"], self.height, self.width))
            hist = st[L.DET_EVAL_HIST:L.DET_EVAL_HIST + L.DET_EVAL_MAX_R2 + 1].astype(np.float64)
            d = np.sqrt(np.arange(L.DET_EVAL_MAX_R2 + 1, dtype=np.float64))
            out["loc_error"] = np.float64(np.nan) if hist.sum() == 0 else np.float64((hist * d).sum() / hist.sum())
            self._final = out
        return self._final

    def compute_pr(self):
        """(precision float64 [n+2], recall float64 [n+2], prob float32 [n]) as device tensors (the reference's shapes and dtypes)."""
        f = self._finalize()
        return f["precision"], f["recall"], f["prob"]

    def compute_mAP(self):
        f = self._finalize()
        if not isinstance(f["mAP"], float):
            f["mAP"] = float(f["mAP"].item())  # read once, then kept
        return f["mAP"]

    def compute_loc_error(self):
        """Mean distance to the nearest ground-truth point of the predictions above prob_thresh that have one within
        distance_thresh (nan without any), from the device's integer d2 histogram."""
        return float(self._finalize()["loc_error"])

    def result(self):
        f = self._finalize()
        return {"precision": f["precision"], "recall": f["recall"], "prob": f["prob"], "tp": f["tp"], "n_gt": f["n_gt"],
                "outside_points": f["outside_points"], "mAP": self.compute_mAP(), "loc_error": self.compute_loc_error()}


# ---- drop-ins under the reference's names ----
def _paths(exper_name_or_dir):
    d = str(exper_name_or_dir)
    if not os.path.isdir(d):
        raise FileNotFoundError("%r is not a directory of per-image .npz files (prob, optional prob_nms, keypoint_map)" % d)
    return sorted(glob.glob(os.path.join(d, "*.npz")))


def _feed(ev, probs, kps, batch=64):
    for i in range(0, len(probs), batch):
        p = torch.from_numpy(np.stack(probs[i:i + batch]).astype(np.float32)).to(ev.device)
        k = torch.from_numpy((np.stack(kps[i:i + batch]) != 0).astype(np.uint8)).to(ev.device)
        ev.update(prob=p, labels=k)


def _evaluator(probs, device, **kw):
    shapes = {p.shape for p in probs}
    if len(shapes) != 1:
        raise ValueError("the files hold maps of different sizes: %s" % sorted(shapes))
    h, w = probs[0].shape
    kw.setdefault("prob_thresh", max(0.5, float(kw.get("remove_zero", 1e-4))))  # (unused where no localisation error is asked for)
    return DetectorEvaluator(h, w, device, max(len(probs) * h * w, 1), **kw)


def compute_tp_fp(data, remove_zero=1e-4, distance_thresh=2, simplified=False, device="cuda"):
    """The reference's compute_tp_fp for one image (`data`: a loaded .npz or a dict): tp, fp, prob, n_gt as numpy."""
    keys = data.files if hasattr(data, "files") else data.keys()
    prob = np.asarray(data["prob_nms"] if "prob_nms" in keys else data["prob"])
    ev = _evaluator([prob], device, remove_zero=remove_zero, distance_thresh=distance_thresh, simplified=simplified)
    _feed(ev, [prob], [np.asarray(data["keypoint_map"])])
    r = ev.result()
    tp = r["tp"].cpu().numpy().astype(bool)
    return tp, np.logical_not(tp), r["prob"].cpu().numpy(), r["n_gt"]


def compute_pr(exper_name_or_dir, device="cuda", **kwargs):
    """The reference's compute_pr over the .npz files of a directory: precision, recall, prob as numpy."""
    data = [np.load(p) for p in _paths(exper_name_or_dir)]
    probs = [np.asarray(d["prob_nms"] if "prob_nms" in d.files else d["prob"]) for d in data]
    if not probs:
        return np.zeros(2), np.array([0.0, 1.0]), np.zeros(0, np.float32)
    ev = _evaluator(probs, device, **kwargs)
    _feed(ev, probs, [np.asarray(d["keypoint_map"]) for d in data])
    precision, recall, prob = ev.compute_pr()
    return precision.cpu().numpy(), recall.cpu().numpy(), prob.cpu().numpy()


def compute_mAP(precision, recall):
    """The reference's compute_mAP (numpy arrays or tensors of compute_pr)."""
    if torch.is_tensor(precision):
        return float((precision[1:] * torch.diff(recall)).sum().item())
    return (np.asarray(precision)[1:] * np.diff(np.asarray(recall))).sum()


def compute_loc_error(exper_name_or_dir, prob_thresh=0.5, distance_thresh=2, device="cuda"):
    """The reference's compute_loc_error over the .npz files of a directory (it reads `prob`, never `prob_nms`)."""
    data = [np.load(p) for p in _paths(exper_name_or_dir)]
    probs = [np.asarray(d["prob"]) for d in data]
    if not probs:
        return np.float64(np.nan)
    # only predictions above prob_thresh enter the histogram: the record buffer needs no more than those above it
    ev = _evaluator(probs, device, remove_zero=max(float(prob_thresh), 0.0), prob_thresh=prob_thresh, distance_thresh=distance_thresh)
    _feed(ev, probs, [np.asarray(d["keypoint_map"]) for d in data])
    ev._finalize()
    return np.float64(ev.compute_loc_error())


def evaluate_detector(net_or_engine, loader, nms_dist=None, conf_thresh=0.015, remove_zero=1e-4, distance_thresh=2, prob_thresh=0.5,
                      simplified=False, max_batches=None, capacity=None, border_remove=4):
    """Detector mAP / localisation error of a model over a loader of {"image": [B,1,H,W], "labels_2D": [B,1,H,W]} device batches
    (shapes.SyntheticShapes(cfg, "val"), or any loader of such dicts): the eval-mode forward, flattenDetection
    (Engine.detector_heatmap) and DetectorEvaluator.update per batch.  With nms_dist the predictions are the points of the
    existing NMS path instead (Engine.describe_points: conf_thresh, nms_dist, border_remove), the reference's `prob_nms` case.
    capacity: records of the whole set (default: every pixel of every batch of a sized loader / of max_batches).
    Returns DetectorEvaluator.result()."""
    ev = None
    eng = net_or_engine if isinstance(net_or_engine, L.Engine) else None
    for j, sample in enumerate(loader):
        if max_batches is not None and j >= max_batches:
            break
        img, lab = sample["image"], sample["labels_2D"]
        if not img.is_cuda:
            raise RuntimeError("evaluate_detector reads device batches: the MI355X path has no CPU fallback")
        img = L.u8_to_unit_float(img) if img.dtype == torch.uint8 else img.float()
        img = img.contiguous()
        B, _, H, W = img.shape
        e = eng if eng is not None else net_or_engine.engine(B, H, W, img.device)
        if ev is None:
            if capacity is None:
                nb = max_batches if max_batches is not None else len(loader)
                capacity = nb * B * H * W
            ev = DetectorEvaluator(H, W, img.device, capacity, remove_zero=remove_zero, distance_thresh=distance_thresh,
                                   prob_thresh=prob_thresh, simplified=simplified)
        lab = lab if lab.dtype in (torch.float32, torch.uint8) else lab.float()
        if nms_dist is None:
            e.forward(img, slot=0, train=False, want=("semi",))
            ev.update(prob=e.detector_heatmap(0, B, H, W), labels=lab)
        else:
            e.forward(img, slot=0, train=False, want=("semi", "desc"))
            d = e.describe_points(0, B, conf_thresh=conf_thresh, nms_dist=nms_dist, subpixel=False, border_remove=border_remove)
            ev.update(pts=d["pts"], count=d["count"], labels=lab)
    if ev is None:
        raise ValueError("evaluate_detector: the loader gave no batch")
    return ev.result()
