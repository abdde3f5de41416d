"""Synthetic Shapes on the GPU: the render against the numpy restatement, the draw against the
reference generator's rules, the single-view feed, determinism and the way through the trainer."""
import json
import os

import numpy as np
import pytest
import torch

from semantic_superpoint_amd import lib as L
from semantic_superpoint_amd import pairs, shapes
from tests import shapes_ref as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DEV = "cuda:0"


@pytest.fixture(scope="module")
def cfg():
    with open(os.path.join(HERE, "golden", "g18_shapes_config.json")) as f:
        return json.load(f)


def _small_cfg(cfg, batch=8):
    c = {"data": R.small_config(cfg["data"]), "model": dict(cfg["model"], batch_size=batch, eval_batch_size=batch)}
    return c


def _compare(table, p, gen_hw, out_hw, blur, tex_blobs):
    img, pts, cnt = L.op_shapes_render(torch.from_numpy(table).to(DEV), p)
    img, pts, cnt = img.cpu().numpy(), pts.cpu().numpy(), cnt.cpu().numpy()
    for b, row in enumerate(table):
        ref, flip, rp = R.render(row, gen_hw, out_hw, blur, tex_blobs)
        d = np.abs(ref.astype(int) - img[b, 0].astype(int))
        print("primitive %d: %d differing pixels, %d in the flip set of %d" % (row[0], (d > 0).sum(), ((d > 0) & flip).sum(), flip.sum()))
        assert np.array_equal(ref[~flip], img[b, 0][~flip])
        assert d.max() <= 1
        assert cnt[b] == len(rp) and (np.abs(rp - pts[b, :cnt[b]]).max() <= 1e-5 if len(rp) else True)
        assert not pts[b, cnt[b]:].any()


def test_render_is_exact_on_the_fixture_and_on_fresh_tables(cfg):
    p = L.shapes_params_from_config(R.small_config(cfg["data"]))
    z = np.load(os.path.join(HERE, "golden", "g18_shapes_tables.npz"))
    for k in z.files:
        _compare(z[k], p, (192, 256), (24, 32), 5, R.SMALL_TEX_BLOBS)
    # drawn on the spot: the fixture's own seeds give the fixture's tables, a new seed gives new ones
    for k, seed in R.FIXTURE_SEEDS.items():
        assert np.array_equal(L.op_shapes_draw(4, seed, p, DEV).cpu().numpy(), z[k])
    for k, name in enumerate(L.SHAPES_PRIMITIVES):
        q = L.shapes_params_from_config(R.small_config(cfg["data"], name))
        assert np.array_equal(L.op_shapes_draw(1, 100 + k, q, DEV).cpu().numpy(), z["prim%d" % k])
    _compare(L.op_shapes_draw(6, 977, p, DEV).cpu().numpy(), p, (192, 256), (24, 32), 5, R.SMALL_TEX_BLOBS)


def test_render_is_exact_at_the_shipped_size(cfg):
    p = L.shapes_params_from_config(cfg["data"])
    _compare(L.op_shapes_draw(4, 31, p, DEV).cpu().numpy(), p, (960, 1280), (120, 160), 21, 3000)


def test_draw_obeys_the_reference_rules(cfg):
    """2048 tables at the shipped size: every rule of shapes_ref.check_row, and the primitive frequencies within 5 binomial
    standard deviations of N w / 6.6."""
    p = L.shapes_params_from_config(cfg["data"])
    N = 2048
    t = torch.cat([L.op_shapes_draw(256, 1000 + i, p, DEV) for i in range(N // 256)]).cpu().numpy()
    for row in t:
        R.check_row(row, p)
    prim = t[:, R.PRIM]
    n_pts = t[:, R.NPOINTS]
    assert (n_pts[(prim == 3) | (prim == 8)] == 0).all() and (n_pts[prim == 7] <= 7).all()
    w = np.array(list(p.weights), np.float64)
    counts = np.bincount(prim, minlength=9)
    print("primitive counts", counts.tolist())
    for k in range(9):
        q = w[k] / w.sum()
        assert abs(counts[k] - N * q) <= 5 * np.sqrt(N * q * (1 - q)), (k, counts[k], N * q)


def _labels_from_points(pts, cnt, H, W):
    out = torch.zeros(len(cnt), 1, H, W)
    for b in range(len(cnt)):
        q = pts[b, :cnt[b]]
        q = q[(q[:, 0] >= 0) & (q[:, 0] <= W - 1) & (q[:, 1] >= 0) & (q[:, 1] <= H - 1)]
        r = torch.min(q.round().long(), torch.tensor([[W - 1, H - 1]]))
        out[b, 0, r[:, 1], r[:, 0]] = 1
    return out


def test_single_view_labels_mask_and_image(cfg):
    data = cfg["data"]
    H, W = 24, 32
    for name in L.SHAPES_PRIMITIVES:
        p = L.shapes_params_from_config(R.small_config(data, name))
        img, pts, cnt = shapes.generate(4, 7, params=p, device=DEV)
        s = pairs.make_single_view(img, pts, cnt, seed=3)
        assert torch.equal(s["labels_2D"].cpu(), _labels_from_points(pts.cpu(), cnt.cpu(), H, W))
        assert torch.equal(s["valid_mask"], torch.ones_like(s["valid_mask"]))
        assert torch.equal(s["image"].cpu(), img.cpu().float() / 255.0)      # load_as_float
        assert torch.equal(s["labels_2D_gaussian"], L.op_label_quantize(s["labels_2D"]))
    p = L.shapes_params_from_config(R.small_config(data))
    img, pts, cnt = shapes.generate(16, 9, params=p, device=DEV)
    ho = data["augmentation"]["homographic"]
    hs, inv = L.op_sample_homographies(16, 5, DEV, **ho["params"])
    draws = L.op_photometric_draw(16, H, W, 77, L.photometric_params_from_config(
        {"photometric": dict(data["augmentation"]["photometric"], params=dict(data["augmentation"]["photometric"]["params"], motion_blur={"max_kernel_size": 3},
                                                                               additive_shade={"transparency_range": [-0.5, 0.8], "kernel_size_range": [5, 11]}))}), DEV)
    s = pairs.make_single_view(img, pts, cnt, seed=3, homographic=ho, homographies=hs, photometric_draws=draws)
    inv2 = torch.inverse(hs.cpu()).to(DEV)
    f = (torch.arange(256, dtype=torch.float32) / 255.0).to(DEV)[img.long()]
    assert torch.equal(s["image"], L.op_warp_image(L.op_photometric_apply(f, draws), inv2))
    assert torch.equal(s["valid_mask"], L.op_erode(L.op_warp_image(torch.ones_like(f), inv2, nearest=True), ho["valid_border_margin"]))
    # warp_points + filter_points + round (utils/utils.py:303-343): fma(p1, y, p0 x) + p2 per row in fp32, restated in float64
    hpx = L.scaled_homographies(hs, H, W).double()
    ref = torch.zeros(16, 1, H, W)
    for b in range(16):
        q = pts[b, :cnt[b]].cpu()
        q = q[(q[:, 0] >= 0) & (q[:, 0] <= W - 1) & (q[:, 1] >= 0) & (q[:, 1] <= H - 1)].double()
        m = hpx[b]
        rows = [(((m[r, 0].float() * q[:, 0].float()).double() + m[r, 1] * q[:, 1]).float() + m[r, 2].float()) for r in range(3)]
        wq = torch.stack([rows[0] / rows[2], rows[1] / rows[2]], 1)
        wq = wq[(wq[:, 0] >= 0) & (wq[:, 0] <= W - 1) & (wq[:, 1] >= 0) & (wq[:, 1] <= H - 1)]
        r = torch.min(wq.round().long(), torch.tensor([[W - 1, H - 1]]))
        ref[b, 0, r[:, 1], r[:, 0]] = 1
    assert torch.equal(s["labels_2D"].cpu(), ref) and ref.sum() > 0


def test_determinism_and_streams(cfg):
    c = _small_cfg(cfg)
    a = shapes.SyntheticShapes(c, "train", device=DEV, seed=5, length=2)
    b = shapes.SyntheticShapes(c, "train", device=DEV, seed=5, length=2)
    x, y = a.batch(1), b.batch(1)
    assert all(torch.equal(x[k], y[k]) for k in x)
    L.set_deterministic(True)
    try:
        y = b.batch(1)
        assert all(torch.equal(x[k], y[k]) for k in x)
    finally:
        L.set_deterministic(False)
    base = shapes.batch_seed(5, 1, 0, "train")
    others = [shapes.batch_seed(6, 1, 0, "train"), shapes.batch_seed(5, 2, 0, "train"), shapes.batch_seed(5, 1, 1, "train"), shapes.batch_seed(5, 1, 0, "val")]
    assert len({base, *others}) == 5
    t0 = L.op_shapes_draw(8, base, a.params, DEV)
    for s in others:
        assert not torch.equal(t0, L.op_shapes_draw(8, s, a.params, DEV))
    v = shapes.SyntheticShapes(c, "val", device=DEV, seed=5, length=1)
    assert not v.photometric and v.homographic is None and a.photometric and a.homographic is not None
    img, pts, cnt = shapes.generate(v.batch_size, shapes.batch_seed(5, 0, 0, "val"), params=v.params, device=DEV)
    s = v.batch(0)
    assert torch.equal(s["image"].cpu(), img.cpu().float() / 255.0) and torch.equal(s["valid_mask"], torch.ones_like(s["image"]))


def _agent(cfg, tmp_path, B):
    from semantic_superpoint_amd.Train_model_heatmap_all import Train_model_heatmap_all as T
    c = {"data": dict(cfg["data"], gaussian_label={"enable": True}), "model": dict(cfg["model"], batch_size=B, eval_batch_size=B, real_batch_size=B, multi_task_loss=False),   # the keys train4.py reads that the yaml lacks
         "validation_interval": 10 ** 9, "tensorboard_interval": 10 ** 9, "retrain": True, "reset_iter": True}
    torch.manual_seed(0)
    a = T(c, save_path=str(tmp_path), device=DEV)
    a.loadModel()
    a.dataParallel()
    return a, c


def test_trainer_takes_device_batches(cfg, tmp_path):
    """The same scalars from a device-resident batch and from host copies of it; then K = 60 steps from the loader with every
    yielded tensor on the device, and the mean loss_det of the last tenth below that of the first tenth."""
    B, K = 16, 60
    a1, c = _agent(cfg, tmp_path / "a", B)
    a2, _ = _agent(cfg, tmp_path / "b", B)
    a2.net.load_state_dict(a1.net.state_dict())
    loader = shapes.SyntheticShapes(c, "train", device=DEV, seed=1, length=K)
    s = loader.batch(0)
    a1.train_val_sample(s, n_iter=1, train=True)
    a2.train_val_sample({k: v.cpu() for k, v in s.items()}, n_iter=1, train=True)
    assert a1.scalar_dict == a2.scalar_dict and np.isfinite(a1.scalar_dict["loss"])
    a1.train_loader = loader
    det = []
    for it, s in enumerate(a1.train_loader):
        assert all(v.is_cuda for v in s.values())
        a1.train_val_sample(s, n_iter=2 + it, train=True)
        det.append(a1.scalar_dict["loss_det"])
    first, last = float(np.mean(det[:K // 10])), float(np.mean(det[-(K // 10):]))
    print("loss_det first tenth %.4f last tenth %.4f (K = %d)" % (first, last, K))
    assert len(det) == K and last < first
