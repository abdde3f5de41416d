"""GPU: BASELINE configs[0] - the SINGLE-VIEW training step of `data.warped_pair.enable: false`
(Train_model_heatmap_all.py:207,237-262,330-332,346-353; the branch the shipped configs/magicpoint_shapes_pair.yaml takes)
through the drop-in trainer and the C ABI, against the G13 fixtures generated from the real reference."""
import copy

import numpy as np
import pytest
import torch

from oracle import cpu_ref as C
from tests import golden_util as G

pytestmark = pytest.mark.gpu
ARCH = "SuperPointNet_gauss2"

# the keys of configs/magicpoint_shapes_pair.yaml the trainer reads (data: the yaml ships warped_pair.enable false,
# lambda_loss 0, gaussian labels off, softmax detector loss, sparse_loss enabled) + the keys it lacks (oracle/make_goldens.py:
# magicpoint_config: real_batch_size, data.semantic, multi_task_loss), batch 64 -> 2 as BASELINE configs[0] states
MAGICPOINT = {
    "data": {"dataset": "SyntheticDataset_gaussian", "gaussian_label": {"enable": False}, "semantic": False,
             "preprocessing": {"resize": [120, 160]}, "warped_pair": {"enable": False, "valid_border_margin": 3}},
    "front_end_model": "Train_model_heatmap_all",
    "model": {"name": ARCH, "params": {}, "detector_loss": {"loss_type": "softmax"}, "batch_size": 2, "eval_batch_size": 2,
              "real_batch_size": 2, "learning_rate": 0.001, "detection_threshold": 0.001, "nms": 4, "lambda_loss": 0,
              "dense_loss": {"enable": False, "params": {"descriptor_dist": 4, "lambda_d": 800}},
              "sparse_loss": {"enable": True, "params": {"num_matching_attempts": 1000, "num_masked_non_matches_per_match": 100,
                                                         "lamda_d": 1, "dist": "cos", "method": "2d"}}},
    "retrain": True, "reset_iter": True, "train_iter": 200000, "tensorboard_interval": 1000, "save_interval": 2000,
    "validation_interval": 1000, "validation_size": 10, "seed": 0,
}


def _dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X (run through gpurun)"
    return torch.device("cuda:0")


def _agent(cfg, sd, tmp_path):
    from semantic_superpoint_amd.Train_model_heatmap_all import Train_model_heatmap_all as T
    agent = T(cfg, save_path=tmp_path, device="cuda:0")
    agent.loadModel()
    agent.net.load_state_dict({k: torch.as_tensor(np.array(v)) for k, v in sd.items()})
    agent.dataParallel()
    return agent


@pytest.mark.parametrize("tag", ["uniform", "kendall"])
@pytest.mark.parametrize("algo", [1, 10, 0])
def test_single_view_trainer_steps_golden(tag, algo, tmp_path):
    """Two optimizer steps + one validation call of the drop-in trainer on the G13 inputs: the reference's scalar_dict
    (incl. the post-step eta it logs), running variances and parameter slices after Adam."""
    g = G.load("g13_single_view_%s_120x160.npz" % tag)
    sample = G.g13_sample(g)
    cfg = copy.deepcopy(MAGICPOINT)
    cfg["model"]["multi_task_loss"] = tag == "kendall"
    sd = C.init_state_dict(ARCH, seed=37)
    agent = _agent(cfg, sd, tmp_path)
    agent.net.engine(2, 120, 160, _dev()).set_conv_algo(algo)
    for it in range(2):
        loss = agent.train_val_sample(sample, n_iter=it + 1, train=True)
        for k, v in g.items():
            if k.startswith("step%d/" % it):
                ref = float(v)
                assert abs(agent.scalar_dict[k[6:]] - ref) < 1e-3 * max(1.0, abs(ref)), (it, k, agent.scalar_dict[k[6:]], ref)
        assert abs(loss - float(g["step%d/loss" % it])) < 1e-3 * max(1.0, abs(loss))
        assert agent.scalar_dict["loss_det_warp"] == 0.0 and agent.scalar_dict["loss_desc"] == 0.0
        assert agent.scalar_dict["positive_dist"] == 0.0 and agent.scalar_dict["loss_sem_warp"] == 0.0
    eng = agent.net.engine()
    assert (eng.eta.cpu() - torch.from_numpy(g["post/eta"])).abs().max() < 1e-5
    st = agent.net.state_dict()
    for k, v in g.items():
        if k.startswith("post_state/"):  # running_var after two train-mode forwards
            ref = torch.from_numpy(v)
            assert (st[k[11:]].cpu() - ref).abs().max() < 1e-3 * float(ref.abs().max()) + 1e-7, k  # (second forward runs on post-Adam weights; measured 1e-4)
        if k.startswith("post_slice/"):
            # two Adam steps move every element by ~2 lr = 2e-3 whatever the size of its gradient: an element whose gradient is
            # 1e-3 of the tensor's largest carries the tensor's absolute rounding noise at a relative size of O(1) (the
            # generator's own oracle-vs-reference check, close_adam, allows 2.2 lr for the same reason).  Measured on the
            # GPU box: median 5e-5, max 4.9e-4
            d = (st[k[11:]].cpu().reshape(-1)[:64] - torch.from_numpy(v)).abs()
            assert float(d.max()) <= 2.2e-3 and float(d.median()) < 1.5e-4 and float((d > 5e-4).float().mean()) < 0.05, \
                (k, float(d.max()), float(d.median()))
    for k in ("convDa.weight", "bnDb.weight", "convDb.bias"):  # the descriptor head is not in the graph: untouched
        assert torch.equal(st[k].cpu(), torch.as_tensor(np.array(sd[k]))), k
    # validation call: forward under no_grad + the logging branch (precision / recall of the un-warped view only)
    v = agent.train_val_sample(sample, n_iter=7, train=False)
    for k in ("loss", "loss_det", "loss_det_warp", "precision", "recall"):
        ref = float(g["val/" + k])
        # precision / recall count thresholded points (0.015) of a model two noise-amplified Adam steps away from the
        # reference's: one or two of the ~150 label points may change sides (measured: recall 0.7289 vs 0.7355 = one point)
        tol = 0.02 if k in ("precision", "recall") else 2e-3 * max(1.0, abs(ref))
        assert abs(agent.scalar_dict[k] - ref) < tol, (k, agent.scalar_dict[k], ref)
    assert abs(v - float(g["val/loss"])) < 2e-3 * max(1.0, abs(v))
    assert "heatmap_warp_nms_batch" not in agent.images_dict and "original_nms_overlap" in agent.images_dict


@pytest.mark.parametrize("tag", ["uniform", "kendall"])
@pytest.mark.parametrize("algo", [1, 10, 12])
def test_single_view_gradients_golden(tag, algo):
    """Gradients of the first single-view step against the reference's (norms + 64-element slices); algorithm 12 (bf16
    path) at its own tolerance against the same fp32 numbers."""
    from semantic_superpoint_amd.lib import Engine, SCALAR_NAMES
    g = G.load("g13_single_view_%s_120x160.npz" % tag)
    sample = {k: v.to(_dev()).contiguous() for k, v in G.g13_sample(g).items()}
    sd = C.init_state_dict(ARCH, seed=37)
    e = Engine(ARCH, 2, 120, 160, _dev())
    e.load_state_dict(sd)
    e.set_conv_algo(algo)
    e.zero_grad()
    mt = tag == "kendall"
    sc = e.pair_step(sample, train=True, lambda_loss=0.0, multi_task=mt, gaussian=False)
    torch.cuda.synchronize()
    sc = dict(zip(SCALAR_NAMES, sc.cpu().tolist()))
    # step0/* were logged AFTER Adam: only the eta_* entries differ from the pre-step values
    tol = 3e-2 if algo == 12 else 1e-3
    for name in ("loss", "loss_det"):
        ref = float(g["step0/" + name])
        assert abs(sc[name] - ref) < tol * max(1.0, abs(ref)), (name, sc[name], ref)
    assert sc["loss_det_warp"] == 0.0 and sc["loss_desc"] == 0.0 and sc["negative_dist"] == 0.0
    gd = e.grad_dict()
    noisy = {c + ".bias" for c, bn, _, _, _ in C.layer_table(ARCH) if bn is not None}
    worst = 0.0
    for k in C.param_keys(ARCH):
        mine = gd[k].cpu().reshape(-1)
        if ("grad_norm/" + k) not in g:  # descriptor head: no gradient in the reference, zero here
            assert k.startswith(("convD", "bnD")) and float(mine.abs().max()) == 0.0, k
            continue
        if k in noisy:
            continue
        n_ref = float(g["grad_norm/" + k])
        sl = torch.from_numpy(g["grad_slice/" + k])
        err = float((mine[:64] - sl).abs().max()) / (float(mine.abs().max()) + 1e-30)
        worst = max(worst, err)
        if algo == 12:
            assert abs(float(mine.norm()) - n_ref) < 0.15 * n_ref + 1e-6, (k, float(mine.norm()), n_ref)
        else:
            assert abs(float(mine.norm()) - n_ref) < 5e-3 * n_ref + 1e-6, (k, float(mine.norm()), n_ref)
            # ReLU / max-pool gate flips (tests/test_gpu_model.py tolerance note): a BatchNorm beta gradient of a 30x40 map is a
            # sum of 2400 dY values and one flipped gate moves it by O(max|dY|); measured 8.1e-3 (down2 conv.1.bias)
            assert err < 2e-2, (k, err)
    print("G13 %s algo %d: worst 64-element slice error %.2e of max|grad|" % (tag, algo, worst))
    if mt:
        assert (gd["eta"].cpu() - torch.from_numpy(g["grad/eta"])).abs().max() < (3e-2 if algo == 12 else 1e-3)
    else:
        assert float(gd["eta"].abs().max()) == 0.0


def test_single_view_gradient_differences_are_gate_flips_only():
    """The 8e-3 slice differences above are ReLU / max-pool gate flips: against the oracle evaluated with the HIP path's own
    gates every gradient tensor of the single-view step agrees to 1e-4 (tests/test_gpu_fullsize.py::_gate_flip_case)."""
    from tests.gate_util import _gate_flip_case
    g = G.load("g13_single_view_kendall_120x160.npz")
    sample = G.g13_sample(g)
    sd = C.init_state_dict(ARCH, seed=37)
    kw = dict(lambda_loss=0.0, multi_task=True, gaussian=False)
    tr = C.Trainer(ARCH, sd, lr=1e-3, warped_pair=False, **kw)
    tr.real_batch_size = 10 ** 9
    tr.train_val_sample(sample, n_iter=1, train=True)
    plain = {k: (v if v is not None else torch.zeros_like(tr.sd[k])) for k, v in tr.last_grads.items() if k != "eta"}
    for algo in (1, 10):
        _gate_flip_case(ARCH, 2, 120, 160, sd, sample, None, algo, kw, plain, plain_tol=1e-2)


def test_single_view_semantic_step_vs_oracle():
    """The same branch with the segmentation head (data.semantic: true): loss_sem of the image only, loss_sem_warp = 0."""
    from semantic_superpoint_amd.lib import Engine, SCALAR_NAMES
    arch, B, H, W = "SuperPointNet_gauss2_ssmall", 2, 64, 96
    sd = C.init_state_dict(arch, seed=3)
    full = C.make_synthetic_pair(B, H, W, seed=5, semantic=True, kp_prob=0.01)
    sample = {k: full[k] for k in ("image", "labels_2D", "labels_2D_gaussian", "valid_mask", "semantic")}
    tr = C.Trainer(arch, sd, lr=1e-3, lambda_loss=0.0, multi_task=True, warped_pair=False)
    tr.real_batch_size = 10 ** 9
    tr.train_val_sample(sample, n_iter=0, train=True)
    e = Engine(arch, B, H, W, _dev())
    e.load_state_dict(sd)
    e.zero_grad()
    sc = e.pair_step({k: v.to(_dev()).contiguous() for k, v in sample.items()}, train=True, lambda_loss=0.0, multi_task=True)
    torch.cuda.synchronize()
    sc = dict(zip(SCALAR_NAMES, sc.cpu().tolist()))
    for k in ("loss", "loss_det", "loss_sem"):
        assert abs(sc[k] - tr.scalar_dict[k]) < 1e-3 * max(1.0, abs(tr.scalar_dict[k])), (k, sc[k], tr.scalar_dict[k])
    assert sc["loss_sem_warp"] == 0.0 and sc["loss_det_warp"] == 0.0
    gd = e.grad_dict()
    assert (gd["eta"].cpu() - tr.last_grads["eta"]).abs().max() < 1e-3
    noisy = {c + ".bias" for c, bn, _, _, _ in C.layer_table(arch) if bn is not None}
    for k in C.param_keys(arch):
        ref = tr.last_grads[k]
        if ref is None:
            assert float(gd[k].abs().max()) == 0.0, k
        elif k not in noisy:
            mine = gd[k].cpu().double().reshape(-1)
            r = ref.double().reshape(-1)
            assert float((mine - r).norm() / (r.norm() + 1e-30)) < 1.5e-2, k


def test_single_view_split_phases_equal_the_whole_step():
    """ssp_pair_step_phase(1) + (2) (the data-parallel overlap form) of a single-view step = phase 0."""
    from semantic_superpoint_amd.lib import Engine
    g = G.load("g13_single_view_kendall_120x160.npz")
    sample = {k: v.to(_dev()).contiguous() for k, v in G.g13_sample(g).items()}
    sd = C.init_state_dict(ARCH, seed=37)
    grads = []
    for phases in ((0,), (1, 2)):
        e = Engine(ARCH, 2, 120, 160, _dev())
        e.load_state_dict(sd)
        e.zero_grad()
        for ph in phases:
            e.pair_step(sample, train=True, lambda_loss=0.0, multi_task=True, gaussian=False, phase=ph)
        torch.cuda.synchronize()
        grads.append(e.grads.clone())
    d = (grads[0] - grads[1]).abs().max() / grads[0].abs().max()
    assert float(d) < 1e-5, float(d)


def test_single_view_error_behaviour(tmp_path):
    """lambda_loss > 0 without a pair: the reference asserts "need a pair of images" (:343); detector_loss.loss_type l2:
    the reference raises a RuntimeError (65 logits vs its 64-channel target; recorded in G13); any other value:
    UnboundLocalError (:168-178)."""
    from semantic_superpoint_amd.lib import Engine
    g = G.load("g13_single_view_uniform_120x160.npz")
    assert "must match the size" in str(g["l2_raises"])
    sample = G.g13_sample(g)
    sd = C.init_state_dict(ARCH, seed=37)
    cfg = copy.deepcopy(MAGICPOINT)
    cfg["model"]["multi_task_loss"] = False
    cfg["model"]["lambda_loss"] = 1
    with pytest.raises(AssertionError, match="need a pair of images"):
        _agent(cfg, sd, tmp_path).train_val_sample(sample, n_iter=1, train=True)
    for lt, exc in (("l2", RuntimeError), ("huber", UnboundLocalError)):
        cfg = copy.deepcopy(MAGICPOINT)
        cfg["model"]["multi_task_loss"] = False
        cfg["model"]["detector_loss"]["loss_type"] = lt
        with pytest.raises(exc):
            _agent(cfg, sd, tmp_path).train_val_sample(sample, n_iter=1, train=True)
    e = Engine(ARCH, 2, 120, 160, _dev())
    dev = {k: v.to(_dev()).contiguous() for k, v in sample.items()}
    with pytest.raises(AssertionError, match="need a pair of images"):
        e.pair_step(dev, train=True, lambda_loss=1.0, gaussian=False)


@pytest.mark.parametrize("algo", [1, 12])
def test_single_view_step_at_240x320_vs_oracle(algo):
    """The single-view step at the benchmark resolution (240x320, B = 4; default fp32 kernels incl. conv_wino4 on the large maps, and
    the bf16 path): scalars and the flat gradient against the oracle's single-view leg (bf16: against its bf16 leg)."""
    from semantic_superpoint_amd.lib import Engine, SCALAR_NAMES
    B, H, W = 4, 240, 320
    sd = C.init_state_dict(ARCH, seed=41)
    full = C.make_synthetic_pair(B, H, W, seed=42, kp_prob=0.003)
    sample = {k: full[k] for k in ("image", "labels_2D", "labels_2D_gaussian", "valid_mask")}
    kw = dict(lambda_loss=0.0, multi_task=True, gaussian=True)
    tr = C.Trainer(ARCH, sd, lr=1e-3, warped_pair=False, operand_dtype=torch.bfloat16 if algo == 12 else None, **kw)
    tr.real_batch_size = 10 ** 9
    tr.train_val_sample(sample, n_iter=0, train=True)
    e = Engine(ARCH, B, H, W, _dev())
    e.set_conv_algo(algo)
    e.load_state_dict(sd)
    e.zero_grad()
    sc = e.pair_step({k: v.to(_dev()).contiguous() for k, v in sample.items()}, train=True, **kw)
    torch.cuda.synchronize()
    sc = dict(zip(SCALAR_NAMES, sc.cpu().tolist()))
    tol = 2e-3 if algo == 12 else 2e-4
    for k in ("loss", "loss_det"):
        assert abs(sc[k] - tr.scalar_dict[k]) < tol * max(1.0, abs(tr.scalar_dict[k])), (k, sc[k], tr.scalar_dict[k])
    assert sc["loss_det_warp"] == 0.0 and sc["loss_desc"] == 0.0
    gd = e.grad_dict()
    noisy = {c + ".bias" for c, bn, _, _, _ in C.layer_table(ARCH) if bn is not None}
    keys = [k for k in C.param_keys(ARCH) if k not in noisy and tr.last_grads[k] is not None]
    mine = torch.cat([gd[k].cpu().double().flatten() for k in keys])
    ref = torch.cat([tr.last_grads[k].double().flatten() for k in keys])
    rel = float((mine - ref).norm() / ref.norm())
    cos = float(mine @ ref / (mine.norm() * ref.norm()))
    print("single view 240x320 algo %d: flat gradient rel-L2 %.2e cosine %.5f" % (algo, rel, cos))
    # fp32: gate flips only (5e-3 as at 120x160 and above); bf16: the accumulation-order floor of this size (1.1e-1 at B = 4 in
    # tests/test_gpu_bf16_path.py::test_bf16_path_at_the_benchmark_size) x 2
    assert rel < (0.22 if algo == 12 else 5e-3) and cos > (0.97 if algo == 12 else 0.9999), (rel, cos)
    for k in C.param_keys(ARCH):
        if tr.last_grads[k] is None:
            assert float(gd[k].abs().max()) == 0.0, k
