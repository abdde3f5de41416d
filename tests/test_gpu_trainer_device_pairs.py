"""GPU: the trainer's device feed (`ssp_device_pairs: true`): the plugin builds the pair from the loader's raw
`image`, `labels_2D` and `semantic` with pairs.make_pairs instead of receiving it from the host."""
import copy
import json
import os

import numpy as np
import pytest
import torch

from oracle import cpu_ref as C

pytestmark = pytest.mark.gpu
ARCH = "SuperPointNet_gauss2_ssmall"
WARP = dict(translation=True, rotation=True, scaling=True, perspective=True, scaling_amplitude=0.2,
            perspective_amplitude_x=0.2, perspective_amplitude_y=0.2, patch_ratio=0.85, max_angle=1.57, allow_artifacts=True)


def _dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _cfg(B, device_pairs, photometric=None):
    cfg = {"data": {"semantic": True, "gaussian_label": {"enable": True},
                    "warped_pair": {"enable": True, "params": dict(WARP), "valid_border_margin": 3}},
           "model": {"name": ARCH, "params": {}, "batch_size": B, "real_batch_size": B, "learning_rate": 1e-3,
                     "lambda_loss": 1, "multi_task_loss": True, "dense_loss": {"enable": False},
                     "detector_loss": {"loss_type": "softmax"},
                     "sparse_loss": {"enable": True, "params": {"num_matching_attempts": 600,
                                                                "num_masked_non_matches_per_match": 100, "lamda_d": 1}}},
           "validation_interval": 1000, "tensorboard_interval": 1, "retrain": True, "reset_iter": True, "ssp_seed": 3}
    if device_pairs:
        cfg["ssp_device_pairs"] = True
    if photometric is not None:
        cfg["data"]["augmentation"] = photometric
    return cfg


def _agent(cfg, tmp_path):
    from semantic_superpoint_amd.Train_model_heatmap_all import Train_model_heatmap_all as T
    agent = T(cfg, save_path=tmp_path, device="cuda:0")
    agent.loadModel()
    sd = C.init_state_dict(ARCH, seed=6)
    agent.net.load_state_dict({k: torch.as_tensor(np.array(v)) for k, v in sd.items()})
    agent.dataParallel()
    return agent


def _raw(B, H, W, seed=0, spaced=False):
    g = torch.Generator().manual_seed(seed)
    img = (torch.rand(B, 1, H, W, generator=g) * 255).to(torch.uint8)          # what an image decoder yields
    lab = (torch.rand(B, 1, H, W, generator=g) < 0.01).float()
    if spaced:  # keypoints at least 8 pixels apart: no two of them scatter into one pixel of the warped maps
        lab = torch.zeros(B, 1, H, W)
        lab[:, :, 4::8, 4::8] = (torch.rand(B, 1, H // 8, W // 8, generator=g) < 0.3).float()
    sem = torch.randint(0, 134, (B, H, W), generator=g)
    return img, lab, sem


def _aug(golden_dir):
    with open(os.path.join(golden_dir, "g17_photometric_config.json")) as f:
        return json.load(f)


class _NoCopy:
    """stands for a loader product that must stay on the host"""

    def to(self, *a, **k):
        raise AssertionError("a key other than image / labels_2D / semantic was copied to the device")

    def __getattr__(self, name):
        raise AssertionError("a key other than image / labels_2D / semantic was touched (%s)" % name)


def _run(agent, samples):
    losses = [agent.train_val_sample(s, n_iter=it, train=True) for it, s in enumerate(samples)]
    eng = agent.net.engine()
    torch.cuda.synchronize()
    return losses, dict(agent.scalar_dict), eng.params.clone(), eng.bn_running.clone()


def _host_fed_and_device_fed(tmp_path, spaced):
    """Two optimiser steps: trainer A is fed host dicts built by make_pairs and moved to the CPU, trainer B the raw image,
    labels and semantic with the same matrices in sample["homographies"] / ["inv_homographies"] (the sampler's inverse pair;
    re-inverting in fp32 would change the last bit of the warp).  Both hand the engine the same arrays: losses and every
    parameter are equal bit for bit under deterministic accumulation.  Variants of B: uint8 image + uint8 semantic (the
    reduced wire format) against float / int64, and every other key of the loader's dict poisoned.
    spaced: keypoints 8 pixels apart, so that no two of them claim one pixel of the warped maps; unspaced: a random 1 % map,
    where they do - the label scatter picks its winners by the reference's write order, not by thread order
    (ssp_op_warp_labels_full), so the two feeds agree there as well."""
    from semantic_superpoint_amd import lib as L
    from semantic_superpoint_amd import pairs
    B, H, W = 4, 120, 160
    L.set_deterministic(True)
    try:
        host, dev_f, dev_u8 = [], [], []
        for it in range(2):
            img, lab, sem = _raw(B, H, W, seed=it, spaced=spaced)
            imgf = img.float() / 255.0
            s = pairs.make_pairs(imgf.to(_dev()), lab.to(_dev()), seed=40 + it, warp_params=WARP, erosion_radius=3, semantic=sem.to(_dev()))
            host.append({k: v.cpu() for k, v in s.items()})
            geo = {"homographies": s["homographies"].cpu(), "inv_homographies": s["inv_homographies"].cpu()}
            dev_f.append(dict(geo, image=imgf, labels_2D=lab, semantic=sem))
            dev_u8.append(dict(geo, image=img, labels_2D=lab, semantic=sem.to(torch.uint8), warped_img=_NoCopy(), warped_labels=_NoCopy(),
                               valid_mask=_NoCopy(), warped_valid_mask=_NoCopy(), name=["a"] * B))
        la, sa, pa, ra = _run(_agent(_cfg(B, False), tmp_path), host)
        lb, sb, pb, rb = _run(_agent(_cfg(B, True), tmp_path), dev_f)
        lc, sc, pc, rc = _run(_agent(_cfg(B, True), tmp_path), dev_u8)
    finally:
        L.set_deterministic(False)
    print("losses host %r device %r device-uint8 %r" % (la, lb, lc))
    assert la == lb and sa == sb, (la, lb)
    assert torch.equal(pa, pb) and torch.equal(ra, rb)
    assert la == lc and sa == sc and torch.equal(pa, pc) and torch.equal(ra, rc)
    assert np.isfinite(la).all() and la[0] != la[1]


def test_host_fed_and_device_fed_steps_are_bit_identical(tmp_path):
    _host_fed_and_device_fed(tmp_path, spaced=True)


def test_host_fed_and_device_fed_steps_are_bit_identical_unspaced(tmp_path):
    """the same on random label maps whose keypoints collide in warped_labels_bi / warped_res"""
    _host_fed_and_device_fed(tmp_path, spaced=False)


def test_photometric_runs_in_training_only(tmp_path, golden_dir):
    B, H, W = 2, 64, 96
    img, lab, sem = _raw(B, H, W)
    sample = {"image": img, "labels_2D": lab, "semantic": sem.to(torch.int16)}
    agent = _agent(_cfg(B, True, photometric=_aug(golden_dir)), tmp_path)
    raw = (img.float() / 255.0).to(_dev())
    assert np.isfinite(agent.train_val_sample(sample, n_iter=0, train=False))
    assert torch.equal(agent.sample_dev["image"], raw)                               # enable_photo_val = False
    assert np.isfinite(agent.train_val_sample(sample, n_iter=0, train=True))
    d = agent.sample_dev
    assert not torch.equal(d["image"], raw) and float(d["image"].min()) >= 0 and float(d["image"].max()) <= 1
    assert d["image"].shape == raw.shape and d["warped_img"].shape == raw.shape
    first = d["image"].clone()
    agent.train_val_sample(sample, n_iter=1, train=True)
    assert not torch.equal(agent.sample_dev["image"], first)                         # the seed follows n_iter
    assert "original_nms_overlap" in agent.images_dict and "warped_nms_overlap" in agent.images_dict
    off = _aug(golden_dir)
    off["photometric"]["enable"] = False
    agent2 = _agent(_cfg(B, True, photometric=off), tmp_path)
    agent2.train_val_sample(sample, n_iter=0, train=True)
    assert torch.equal(agent2.sample_dev["image"], raw)


def test_reference_sampler_in_device_mode(tmp_path):
    """ssp_sampler "reference" draws the sparse-loss indices on the host from the homographies sampled on the device"""
    B, H, W = 2, 64, 96
    img, lab, sem = _raw(B, H, W)
    cfg = _cfg(B, True)
    cfg["ssp_sampler"] = "reference"
    agent = _agent(cfg, tmp_path)
    np.random.seed(1); torch.manual_seed(2)
    assert np.isfinite(agent.train_val_sample({"image": img, "labels_2D": lab, "semantic": sem}, n_iter=0, train=True))


def test_device_pairs_needs_warped_pair(tmp_path):
    from semantic_superpoint_amd.Train_model_heatmap_all import Train_model_heatmap_all as T
    cfg = copy.deepcopy(_cfg(2, True))
    cfg["data"]["warped_pair"]["enable"] = False
    cfg["model"]["lambda_loss"] = 0
    with pytest.raises(ValueError) as e:
        agent = T(cfg, save_path=tmp_path, device="cuda:0")
        agent.loadModel()
        agent.dataParallel()
        img, lab, sem = _raw(2, 64, 96)
        agent.train_val_sample({"image": img, "labels_2D": lab, "semantic": sem}, n_iter=0, train=True)
    assert "ssp_device_pairs" in str(e.value) and "warped_pair.enable" in str(e.value)
