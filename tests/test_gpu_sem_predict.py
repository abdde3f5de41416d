"""GPU: the segmentation head read-out - fused bilinear upsample x8 + argmax + confusion matrix
(ssp_op_sem_predict / ssp_sem_predict), Engine.sem_predict and the trainer's `ssp_sem_metrics`.

The yardstick is torch.nn.functional.interpolate(sout.double(), (h, w), mode="bilinear", align_corners=False) on the host.
Tolerance of the random-logit checks: tol = 8 * 2^-24 * max|sout| - the kernel's value of a class is four products and three
sums of magnitude <= max|sout| in fp32 (<= 1 ulp each), and the winner is compared with the true maximum (twice that error)."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import cpu_ref as C

pytestmark = pytest.mark.gpu
ARCH = "SuperPointNet_gauss2_ssmall"
NC = 133


def _dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _up64(sout):
    return F.interpolate(sout.double().cpu(), size=(sout.shape[2] * 8, sout.shape[3] * 8), mode="bilinear", align_corners=False)


def _first_argmax(l64):
    c = l64.shape[1]
    at_max = l64 == l64.max(1, keepdim=True).values
    return torch.where(at_max, torch.arange(c).view(1, c, 1, 1), c).min(1).values


def _criterion(pred, l64, maxabs, what=""):
    """every pixel: l64[pred] >= max - tol; wherever the top two classes are more than 2 tol apart (>= 99 % of the image, asserted
    on the fp64 values alone): pred == argmax."""
    tol = 8.0 * 2.0 ** -24 * float(maxabs)
    pred = pred.cpu().long()
    assert pred.shape == (l64.shape[0],) + l64.shape[2:]
    assert int(pred.max()) < l64.shape[1]
    top = l64.topk(2, dim=1)
    gap = top.values[:, 0] - top.values[:, 1]
    clear = gap > 2 * tol
    share = float(clear.double().mean())
    chosen = l64.gather(1, pred.unsqueeze(1)).squeeze(1)
    worst = float((top.values[:, 0] - chosen).max())
    print("%s tol %.3e  clear share %.6f  worst shortfall %.3e  mismatches on clear pixels %d"
          % (what, tol, share, worst, int((pred != top.indices[:, 0])[clear].sum())))
    assert share >= 0.99
    assert bool((chosen >= top.values[:, 0] - tol).all()), worst
    assert torch.equal(pred[clear], top.indices[:, 0][clear])


def _bincount_conf(labels, pred, c):
    lab, p = labels.cpu().reshape(-1), pred.cpu().long().reshape(-1)
    ok = (lab >= 0) & (lab < c)
    return torch.bincount(lab[ok] * c + p[ok], minlength=c * c).view(c, c), int(ok.sum())


@pytest.fixture(scope="module")
def random_case():
    """3 randn logits, 133 classes, B = 2 at 40x56 (5x7 cells), the fp64 upsample and the kernel's class map: shared, never modified"""
    from semantic_superpoint_amd import lib as L
    g = torch.Generator().manual_seed(11)
    sout = 3.0 * torch.randn(2, NC, 5, 7, generator=g)
    pred, none = L.op_sem_predict(sout.to(_dev()))
    assert none is None and pred.dtype == torch.uint8 and tuple(pred.shape) == (2, 40, 56)
    return {"sout": sout, "l64": _up64(sout), "pred": pred}


@pytest.mark.parametrize("hc,wc", [(2, 3), (5, 7)])
def test_integer_logits_first_index_wins_every_tie(hc, wc):
    """Logits are integers in [-8, 8] (17 values over 133 classes: ties at almost every pixel); every interpolated value is a
    multiple of 2^-8 below 16, exact in fp32 in any order, so the class map must EQUAL the first-occurrence argmax of the fp64
    upsample.  16x24: every tile touches a border clamp; 40x56: interior, edges, odd cell counts."""
    from semantic_superpoint_amd import lib as L
    g = torch.Generator().manual_seed(5 + hc)
    sout = torch.randint(-8, 9, (2, NC, hc, wc), generator=g).float()
    l64 = _up64(sout)
    want = _first_argmax(l64)
    ties = float(((l64 == l64.max(1, keepdim=True).values).sum(1) > 1).double().mean())
    pred, _ = L.op_sem_predict(sout.to(_dev()))
    print("share of pixels with an exact tie at the top: %.3f, mismatches %d" % (ties, int((pred.cpu().long() != want).sum())))
    assert ties > 0.05
    assert torch.equal(pred.cpu().long(), want)


def test_random_logits(random_case):
    _criterion(random_case["pred"], random_case["l64"], random_case["sout"].abs().max(), "random 133")


@pytest.mark.parametrize("n_classes,cs,poison", [(5, 8, False), (21, None, False), (133, 136, False), (150, None, False), (256, None, False),
                                                 (21, 24, True), (22, 25, True)])
def test_class_counts_and_padding(n_classes, cs, poison):
    """All logits negative: a zero padding channel scanned by mistake would win everywhere.  poison: cs = n_classes + 3 with 1e9 in
    the padding channels (24: 16-byte loads, 25: 4-byte loads).  256 classes: class 255 must come out of the uint8 map, and the
    confusion matrix (65536 counters) is right."""
    from semantic_superpoint_amd import lib as L
    g = torch.Generator().manual_seed(n_classes)
    B, hc, wc = 2, 3, 5
    sout = 3.0 * torch.randn(B, n_classes, hc, wc, generator=g) - 20.0
    sout[:, n_classes - 1, 0, 0] = 5.0   # the last class wins around the first cell
    labels = torch.randint(0, n_classes + 1, (B, hc * 8, wc * 8), generator=g).to(_dev())
    if poison:
        assert cs == n_classes + 3
        x = torch.cat([sout, torch.full((B, 3, hc, wc), 1e9)], 1).to(_dev())
        pred, conf = L.op_sem_predict(x, labels=labels, confusion=True, n_classes=n_classes)
    else:
        pred, conf = L.op_sem_predict(sout.to(_dev()), labels=labels, confusion=True, cs=cs)
    assert int(pred[:, 0, 0].min()) == n_classes - 1 and int(pred.max()) == n_classes - 1
    _criterion(pred, _up64(sout), sout.abs().max(), "C=%d cs=%s" % (n_classes, cs))
    want, n_ok = _bincount_conf(labels, pred, n_classes)
    assert tuple(conf.shape) == (n_classes, n_classes) and torch.equal(conf.cpu(), want) and int(conf.sum()) == n_ok


def _labels(kind, g, B, hc, wc):
    if kind == "blocks":     # constant on the 8x8 cells (coherent), some cells ignored
        cells = torch.randint(0, NC, (B, hc, wc), generator=g)
        cells[0, 0, 0], cells[0, 1, 2], cells[1, 2, 3] = 133, -1, 10 ** 6
        return cells.repeat_interleave(8, 1).repeat_interleave(8, 2).contiguous()
    lab = torch.randint(0, NC + 1, (B, hc * 8, wc * 8), generator=g)   # uniformly random (133 = the reference's ignore label)
    lab[:, ::7, ::5] = -1
    lab[:, 3::11, 1::9] = 10 ** 6
    return lab


@pytest.mark.parametrize("kind", ["blocks", "random"])
def test_confusion_matrix_is_exact(random_case, kind):
    from semantic_superpoint_amd import lib as L
    sout, pred = random_case["sout"].to(_dev()), random_case["pred"]
    labels = _labels(kind, torch.Generator().manual_seed(3), 2, 5, 7)
    want, n_ok = _bincount_conf(labels, pred, NC)
    assert 0 < n_ok < labels.numel()
    lab = labels.to(_dev())
    p2, conf = L.op_sem_predict(sout, labels=lab, confusion=True)                  # both
    assert torch.equal(p2, pred) and conf.dtype == torch.int64
    assert torch.equal(conf.cpu(), want) and int(conf.sum()) == n_ok
    p3, conf3 = L.op_sem_predict(sout, labels=lab, want_pred=False, confusion=True)  # confusion only
    assert p3 is None and torch.equal(conf3, conf)
    p4, same = L.op_sem_predict(sout, labels=lab, want_pred=False, confusion=conf)   # accumulates: a second call doubles it
    assert same is conf and torch.equal(conf.cpu(), 2 * want)
    p5, none = L.op_sem_predict(sout, labels=lab)                                  # class map only (labels are not needed for it)
    assert none is None and torch.equal(p5, pred)


def test_confusion_single_cell_contention():
    """every pixel carries the same (label, prediction) pair: all counts land in one cell"""
    from semantic_superpoint_amd import lib as L
    B, hc, wc = 2, 5, 7
    sout = torch.zeros(B, NC, hc, wc)
    sout[:, 7] = 4.0
    labels = torch.full((B, hc * 8, wc * 8), 3, dtype=torch.int64)
    pred, conf = L.op_sem_predict(sout.to(_dev()), labels=labels.to(_dev()), confusion=True)
    assert bool((pred == 7).all())
    want = torch.zeros(NC, NC, dtype=torch.int64)
    want[3, 7] = labels.numel()
    assert torch.equal(conf.cpu(), want)


def test_error_cases_raise(random_case):
    from semantic_superpoint_amd import lib as L
    sout = random_case["sout"].to(_dev())
    lab = torch.zeros(2, 40, 56, dtype=torch.int64, device=_dev())
    with pytest.raises(ValueError, match="labels"):
        L.op_sem_predict(sout, confusion=True)
    with pytest.raises(ValueError, match="neither"):
        L.op_sem_predict(sout, labels=lab, want_pred=False)
    with pytest.raises(ValueError, match="int64"):
        L.op_sem_predict(sout, labels=lab.int(), confusion=True)
    with pytest.raises(ValueError, match="int64"):
        L.op_sem_predict(sout, labels=lab, confusion=torch.zeros(NC, NC + 1, dtype=torch.int64, device=_dev()))
    with pytest.raises(RuntimeError, match="n_classes"):
        L.op_sem_predict(torch.zeros(1, 257, 2, 2, device=_dev()))


# ---- engine ----

def _engine(arch, B, H, W, algo):
    from semantic_superpoint_amd.lib import Engine
    e = Engine(arch, B, H, W, _dev())
    e.set_conv_algo(algo)
    e.load_state_dict(C.init_state_dict(arch, seed=1))
    return e


def _slot_logits(eng, slot, B, H, W):
    """convSout of the last forward in `slot` as public NCHW logits (the engine's NHWC map has channel stride 136)"""
    cs = (NC + 3) // 4 * 4
    y = eng.debug_buffer(slot, "Y13", (B, H // 8, W // 8, cs))
    return y[..., :NC].permute(0, 3, 1, 2).contiguous(), cs


@pytest.mark.parametrize("algo", [1, 12])
def test_engine_sem_predict(algo):
    from semantic_superpoint_amd import lib as L
    B, H, W = 2, 64, 96
    eng = _engine(ARCH, B, H, W, algo)
    with pytest.raises(RuntimeError, match="no forward"):
        eng.sem_predict(1, B, H, W)
    sample = C.make_synthetic_pair(B, H, W, seed=2, kp_prob=0.01, semantic=True)
    dev = {k: v.to(_dev()).contiguous() for k, v in sample.items()}
    out = eng.forward(dev["image"], train=False, want=("semi", "desc", "sem"))
    pred, none = eng.sem_predict(0, B, H, W)
    assert none is None and pred.dtype == torch.uint8 and tuple(pred.shape) == (B, H, W)
    logits, cs = _slot_logits(eng, 0, B, H, W)
    _criterion(pred, out["sem"].double().cpu(), logits.abs().max(), "engine forward, algo %d" % algo)
    with pytest.raises(ValueError, match="multiples of 8"):
        eng.sem_predict(0, B, 60, W)
    for train in (True, False):
        eng.zero_grad()
        eng.pair_step(dev, seed=4, train=train)
        for slot, key in ((0, "semantic"), (1, "warped_sem")):
            p, conf = eng.sem_predict(slot, B, H, W, labels=dev[key], confusion=True)
            logits, cs = _slot_logits(eng, slot, B, H, W)
            p_op, conf_op = L.op_sem_predict(logits, labels=dev[key], confusion=True, cs=cs)
            assert torch.equal(p, p_op) and torch.equal(conf, conf_op), (train, slot)
            want, n_ok = _bincount_conf(dev[key], p, NC)
            assert torch.equal(conf.cpu(), want) and n_ok > 0
    assert not torch.equal(eng.sem_predict(0, B, H, W)[0], eng.sem_predict(1, B, H, W)[0])  # the two views differ


def test_engine_without_segmentation_head_is_refused():
    B, H, W = 1, 64, 96
    eng = _engine("SuperPointNet_gauss2", B, H, W, 1)
    eng.forward(torch.rand(B, 1, H, W, device=_dev()), train=False)
    with pytest.raises(RuntimeError, match="segmentation head"):
        eng.sem_predict(0, B, H, W)


# ---- trainer ----

def _cfg(B, sem_metrics):
    cfg = {"data": {"semantic": True, "gaussian_label": {"enable": True}, "warped_pair": {"enable": True}},
           "model": {"name": ARCH, "params": {}, "batch_size": B, "real_batch_size": B, "learning_rate": 1e-3,
                     "lambda_loss": 1, "multi_task_loss": True, "dense_loss": {"enable": False},
                     "detector_loss": {"loss_type": "softmax"},
                     "sparse_loss": {"enable": True, "params": {"num_matching_attempts": 600,
                                                                "num_masked_non_matches_per_match": 100, "lamda_d": 1}}},
           "validation_interval": 1000, "tensorboard_interval": 1, "retrain": True, "reset_iter": True, "ssp_seed": 3}
    if sem_metrics:
        cfg["ssp_sem_metrics"] = True
    return cfg


def _agent(cfg, tmp_path):
    from semantic_superpoint_amd.Train_model_heatmap_all import Train_model_heatmap_all as T
    agent = T(copy.deepcopy(cfg), save_path=tmp_path, device="cuda:0")
    agent.loadModel()
    sd = C.init_state_dict(ARCH, seed=6)
    agent.net.load_state_dict({k: torch.as_tensor(np.array(v)) for k, v in sd.items()})
    agent.dataParallel()
    return agent


NEW_SCALARS = ("sem_pixel_acc", "sem_miou", "sem_pixel_acc_warp", "sem_miou_warp")


def test_trainer_sem_metrics(tmp_path):
    from semantic_superpoint_amd import lib as L
    B, H, W = 2, 64, 96
    sample = C.make_compact_pair(B, H, W, seed=9, semantic=True, kp_prob=0.01)
    L.set_deterministic(True)   # same-seed steps of two trainers agree bit for bit
    try:
        on, off = _agent(_cfg(B, True), tmp_path), _agent(_cfg(B, False), tmp_path)
        loss_on = on.train_val_sample(sample, n_iter=0, train=True)
        sc_on, im_on = dict(on.scalar_dict), dict(on.images_dict)
        loss_off = off.train_val_sample(sample, n_iter=0, train=True)
        sc_off, im_off = dict(off.scalar_dict), dict(off.images_dict)
    finally:
        L.set_deterministic(False)
    # option off: none of the new keys, and the step is the same step
    assert not any(k in sc_off for k in NEW_SCALARS) and "sem_class" not in im_off and "warp_sem_class" not in im_off
    assert "sem_pred" not in im_on and "sem_pred" not in im_off
    assert off.sem_confusion_val is None
    assert loss_on == loss_off
    assert set(sc_on) == set(sc_off) | set(NEW_SCALARS)
    diff = {k: (sc_on[k], sc_off[k]) for k in sc_off if not np.array_equal(sc_on[k], sc_off[k], equal_nan=True)}
    assert not diff, diff
    assert torch.equal(on.net.engine().params, off.net.engine().params)
    # option on: scalars, class maps
    print({k: sc_on[k] for k in NEW_SCALARS})
    assert all(np.isfinite(sc_on[k]) and 0.0 <= sc_on[k] <= 1.0 for k in NEW_SCALARS)
    assert on.sem_confusion_val is None   # a training step does not touch the validation matrix
    eng = on.net.engine()
    for slot, key, suffix, img_key in ((0, "semantic", "", "sem_class"), (1, "warped_sem", "_warp", "warp_sem_class")):
        a = im_on[img_key]
        assert a.dtype == np.uint8 and a.shape == (B, 1, H, W)
        pred, _ = eng.sem_predict(slot, B, H, W)
        assert np.array_equal(a[:, 0], pred.cpu().numpy())
        want, n_ok = _bincount_conf(sample[key], pred, NC)
        met = L.sem_metrics(want)
        assert n_ok > 0 and met["n_pixels"] == n_ok
        assert sc_on["sem_pixel_acc" + suffix] == met["pixel_acc"] and sc_on["sem_miou" + suffix] == met["miou"]
    # validation: the device matrix sums both views of every step until it is reset
    total = torch.zeros(NC, NC, dtype=torch.int64)
    for it in range(2):
        on.train_val_sample(sample, n_iter=1 + it, train=False)
        for slot, key in ((0, "semantic"), (1, "warped_sem")):
            total += _bincount_conf(sample[key], eng.sem_predict(slot, B, H, W)[0], NC)[0]
        assert on.sem_confusion_val.dtype == torch.int64 and on.sem_confusion_val.is_cuda
        assert torch.equal(on.sem_confusion_val.cpu(), total)
    assert int(total.sum()) > 0
    on.reset_sem_confusion()
    assert int(on.sem_confusion_val.abs().sum()) == 0
