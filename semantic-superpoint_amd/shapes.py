"""Synthetic Shapes on the device: the data of the MagicPoint stage.

`SyntheticShapes(config, task)` stands where the reference's `DataLoader(SyntheticDataset_gaussian(...))` stands
(datasets/SyntheticDataset_gaussian.py, datasets/synthetic_dataset.py): every batch is drawn (`ssp_op_shapes_draw`), rendered
(`ssp_op_shapes_render`) and augmented (`pairs.make_single_view`) in HBM; no dataset, no tar cache, no host image work.

The RNG streams differ from numpy's and cv2's, so this is a distribution-level equivalent of the reference generator (like
pairs.py and synth.py); the raster, blur and rounding rules are this project's own and are stated in DESIGN.md section 15 -
"same as cv2" is argued there, not measured (cv2 is not available to compare against)."""
import torch

from . import lib as L
from . import pairs, parallel

_TASKS = {"train": 0, "training": 0, "val": 1, "validation": 1}


def generate(B, seed, config=None, device="cuda", params=None, return_table=False):
    """The raw product: (image uint8 [B,1,h,w], points float32 [B, lib.SHAPES_MAX_POINTS, 2] (x, y), counts int32 [B]) of B
    images from `seed`.  config: the `data:` dict of a MagicPoint yaml (None: the class defaults); params: a ready
    lib.SspShapesParams instead."""
    p = params if params is not None else L.shapes_params_from_config(config)
    table = L.op_shapes_draw(B, seed, p, device)
    out = L.op_shapes_render(table, p)
    return out + (table,) if return_table else out


def batch_seed(seed, index, rank, task):
    """One 64-bit seed per (seed, batch index, rank, task): ranks and splits never share a stream."""
    m = (1 << 64) - 1
    x = (int(seed) * 0x9E3779B97F4A7C15 + 0x632BE59BD9B4E019) & m
    for v in (int(index), int(rank), _TASKS[task]):
        x = ((x ^ (x >> 31)) * 0xBF58476D1CE4E5B9 + v + 1) & m
        x = ((x ^ (x >> 29)) * 0x94D049BB133111EB) & m
    return x


class SyntheticShapes:
    """Iterable of device-resident single-view batches.  config: the whole yaml dict (its `data:` and `model:` blocks are read)
    or the `data:` block alone; task "train" | "val"; length: batches per epoch (None: generation.split_sizes of the task
    times the truncate shares, divided by the batch size: the reference's epoch).  Training epochs continue the stream, the
    validation pass repeats its own.  `trainer.train_loader = SyntheticShapes(cfg, "train")` is the whole
    integration."""

    def __init__(self, config, task="train", device="cuda", seed=0, length=None, batch_size=None):
        if task not in _TASKS:
            raise ValueError("task must be 'train' or 'val'")
        data = config.get("data", config)
        model = config.get("model") or {}
        self.task = "train" if _TASKS[task] == 0 else "val"
        self.device = torch.device(device)
        self.seed = int(seed)
        self.params = L.shapes_params_from_config(data)
        self.batch_size = int(batch_size or model.get("batch_size" if self.task == "train" else "eval_batch_size", 1))
        aug = data.get("augmentation") or {}
        key = "enable_train" if self.task == "train" else "enable_val"
        ph, ho = aug.get("photometric") or {}, aug.get("homographic") or {}
        # (a stage the reference's parser doubles is applied once: lib.photometric_params_single_pass)
        self.photo_params = L.photometric_params_single_pass({"photometric": dict(ph, enable=True)}) if ph.get(key, False) else None
        self.photometric = self.photo_params is not None
        self.homographic = ho if ho.get(key, False) else None
        if length is None:
            sizes = dict({"training": 10000, "validation": 200}, **((data.get("generation") or {}).get("split_sizes") or {}))
            # the reference's epoch: the union of the per-primitive splits, each truncated to its share
            n = sum(int(w * sizes["training" if self.task == "train" else "validation"]) for w in self.params.weights)
            length = max(n // self.batch_size, 1)
        self.length = int(length)
        self.epoch = 0

    def __len__(self):
        return self.length

    def batch(self, index):
        s = batch_seed(self.seed, index, parallel.rank(), self.task)
        img, pts, cnt = generate(self.batch_size, s, device=self.device, params=self.params)
        draws = None
        if self.photo_params is not None:
            draws = L.op_photometric_draw(self.batch_size, self.params.out_h, self.params.out_w, s ^ 0x70686F746F, self.photo_params, self.device)
        return pairs.make_single_view(img, pts, cnt, s >> 1, homographic=self.homographic, photometric_draws=draws)

    def __iter__(self):
        base = self.epoch * self.length
        if self.task == "train":  # the validation set is fixed: every pass sees the same images, as the reference's does
            self.epoch += 1
        for i in range(self.length):
            yield self.batch(base + i)
