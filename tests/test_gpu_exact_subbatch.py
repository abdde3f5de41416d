"""GPU: the layer-exact chains on calls SMALLER than the engine: a pair step of B < max_batch right after a full batch, and
Engine.forward below the configured size right after a full-size forward on the same slot.

What the larger call leaves behind - pooled copies, the replicas of the BatchNorm statistics, deferred weight-gradient slabs,
corner lists, the tails of every activation buffer - must be read by nothing in the smaller one:

  * test_step_below_max_batch_after_a_full_batch: an engine of (3, 88, 72) runs one pair step at B = 3, then one at B = 2 on other
    seeds; the forward and backward chains of the dtype (tests/test_gpu_layer_exact.py, test_gpu_backward_exact.py; bf16:
    test_gpu_bf16_path.py, test_gpu_bf16_backward_exact.py) hold on the second step under their committed TAU tables, with the
    route record asserted for B = 2.  Then, under set_deterministic(True), the same two steps against a FRESH engine of the same
    configured size that only runs the second: scalars, every gradient tensor, every BatchNorm running statistic and
    num_batches_tracked are torch.equal (same configuration, same dispatch, same workspace: a difference is left-over state).
    The running statistics are torch-owned state, not workspace: they are put back to their initial values between the steps.
  * test_forward_below_the_configured_size: an engine of (2, 64, 96); forward(slot 0, train=True) at full size, then at 2x8x8 (level
    maps down to 1x1, n = 2 per channel), 1x8x16 and 2x40x64; the forward chain (one view per launch: nprob = 1) holds on each.
    ssp_forward accepts every multiple of 8 up to the configured size, 8x8 included: nothing is refused.  At 2x8x8 and 1x8x16 the
    cell maps hold n = 2 values per channel: the fp32 path's one-pass variance (fp32 squares) is then off by up to 3.2e-5 of
    max |scale| against the chain's 1e-5; _Chain(one_pass_stats=True) adds 4 x the error of a numpy restatement of that
    accumulation per channel (tests/test_gpu_layer_exact.py).  The bf16 path holds under the unchanged bound."""
import os
import time

import pytest
import torch

from tests import test_gpu_backward_exact as BE
from tests import test_gpu_bf16_backward_exact as BB
from tests import test_gpu_bf16_path as BP
from tests import test_gpu_layer_exact as LE
from tests.gate_util import _dev

pytestmark = pytest.mark.gpu

SUBBATCH_ENGINE = ("ssp", 3, 88, 72)   # tag, max_batch, H, W
SUBBATCH_B = 2
FORWARD_ENGINE = ("ssp", 2, 64, 96)
FORWARD_SHAPES = [(2, 8, 8), (1, 8, 16), (2, 40, 64)]   # n, h, w


def _make_engine(algo, arch, B, H, W, sd):
    if algo == 12:
        return BP._engine(arch, B, H, W, sd)
    e = LE._engine(arch, B, H, W, sd)
    if algo != 1:
        e.set_conv_algo(algo)
    return e


def _two_steps(algo, arch, sd, B0, H, W, first, second, taps):
    """engine of (B0, H, W); the pair step `first` (None: skipped), the initial running statistics put back, then `second`"""
    e = _make_engine(algo, arch, B0, H, W, sd)
    running, nbt = e.bn_running.clone(), e.nbt.clone()
    if taps:
        e.debug_backward_taps(BE.TAP_LAYERS)
    if first is not None:
        e.zero_grad()
        e.pair_step(first, indices=None, seed=7, train=True)
        torch.cuda.synchronize()
        e.bn_running.copy_(running)
        e.nbt.copy_(nbt)
    e.zero_grad()
    sc = e.pair_step(second, indices=None, seed=8, train=True).clone()
    torch.cuda.synchronize()
    return e, sc


@pytest.mark.parametrize("algo", [1, 12])
def test_step_below_max_batch_after_a_full_batch(algo, monkeypatch):
    from semantic_superpoint_amd import lib as L
    from semantic_superpoint_amd import synth
    torch.set_num_threads(min(int(os.environ.get("OMP_NUM_THREADS", "16")), 16))
    monkeypatch.setenv("SSP_BF16_FUSE_APPLY", "1")
    t0 = time.perf_counter()
    tag, B0, H, W = SUBBATCH_ENGINE
    B = SUBBATCH_B
    arch, sd, first = LE._inputs(tag, B0, H, W, flip_gamma=True)
    BE._edit_gammas(arch, sd)
    second = synth.make_pair(B, H, W, _dev(), seed=101, semantic=True)
    # the chains on the second step
    e, _ = _two_steps(algo, arch, sd, B0, H, W, first, second, taps=True)
    xs = [second[k].cpu() for k in ("image", "warped_img")]
    if algo == 12:
        for v in range(2):
            BP._forward_chain(e, arch, sd, xs[v], v, list(range(B)))
        BB._check_backward(e, arch, sd, tag, B, H, W, 1, second, t0)
    else:
        ch = LE._Chain(e, arch, sd, B, H, W, algo, list(range(B)))
        for v in range(2):
            ch.view(v, xs[v])
        print("%s B=%d of %d %dx%d algo %d forward: worst |Y - Y64| / bound per family: %s" % (
            tag, B, B0, H, W, algo, ", ".join("%s %.3e [%s]" % (f, r, where) for f, (r, where) in sorted(ch.worst.items()))))
        BE._check_backward(e, arch, sd, tag, B, H, W, algo, second, t0)
    del e
    torch.cuda.empty_cache()
    # bit equality with an engine that never ran the larger step
    L.set_deterministic(True)
    try:
        got = []
        for prior in (first, None):
            e, sc = _two_steps(algo, arch, sd, B0, H, W, prior, second, taps=False)
            got.append((sc.cpu(), {k: v.cpu().clone() for k, v in e.grad_dict().items()}, e.bn_running.cpu().clone(), e.nbt.cpu().clone()))
            del e
            torch.cuda.empty_cache()
    finally:
        L.set_deterministic(False)
    (s0, g0, r0, n0), (s1, g1, r1, n1) = got
    assert torch.equal(s0, s1), ("scalars", s0, s1)
    diff = [k for k in g1 if not torch.equal(g0[k], g1[k])]
    assert not diff, ("gradient tensors that differ from the fresh engine's", diff)
    assert torch.equal(r0, r1), "BatchNorm running statistics"
    assert torch.equal(n0, n1) and int(n1.min()) > 0, ("num_batches_tracked", n0, n1)
    print("B=%d after B=%d on one engine, algo %d: scalars, %d gradient tensors, running statistics bit-identical to a fresh engine (%.1f s)"
          % (B, B0, algo, len(g1), time.perf_counter() - t0))


@pytest.mark.parametrize("n,h,w", FORWARD_SHAPES, ids=["%dx%dx%d" % s for s in FORWARD_SHAPES])
@pytest.mark.parametrize("algo", [1, 12])
def test_forward_below_the_configured_size(algo, n, h, w):
    torch.set_num_threads(min(int(os.environ.get("OMP_NUM_THREADS", "16")), 16))
    t0 = time.perf_counter()
    tag, B0, H, W = FORWARD_ENGINE
    arch, sd = LE._weights(tag, flip_gamma=True)
    e = _make_engine(algo, arch, B0, H, W, sd)
    g = torch.Generator().manual_seed(11)
    full = torch.rand(B0, 1, H, W, generator=g)
    x = torch.rand(n, 1, h, w, generator=g)
    e.forward(full.to(_dev()), slot=0, train=True, want=())
    xd = x.to(_dev())
    e.forward(xd, slot=0, train=True, want=())
    torch.cuda.synchronize()
    if algo == 12:
        BP._forward_chain(e, arch, sd, x, 0, list(range(n)))
        print("forward %dx%dx%d on an engine of %dx%dx%d, algo 12: holds (%.1f s)" % (n, h, w, B0, H, W, time.perf_counter() - t0))
    else:
        ch = LE._Chain(e, arch, sd, n, h, w, algo, list(range(n)), nprob=1, one_pass_stats=n * (h // 8) * (w // 8) < 8)
        ch.view(0, x)
        print("forward %dx%dx%d on an engine of %dx%dx%d, algo %d: worst |Y - Y64| / bound per family: %s (%.1f s)" % (
            n, h, w, B0, H, W, algo, ", ".join("%s %.3e [%s]" % (f, r, where) for f, (r, where) in sorted(ch.worst.items())),
            time.perf_counter() - t0))
