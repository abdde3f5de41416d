"""GPU: the bf16 path (conv algorithm 12, BASELINE configs[3] "bf16 compute / fp32 master") through the Engine against the
ORACLE evaluated with the same rounding points (oracle/cpu_ref.py, operand_dtype=torch.bfloat16: bf16 matrix-core operands,
bf16 stored activations / activation gradients, fp32 accumulation, BatchNorm, losses, master weights).  The reference is
fp32-only (models/unet_parts.py:14-21), so the anchor chain is: reference == fp32 oracle (goldens), fp32 oracle -> bf16 oracle by
the rounding functions alone, bf16 oracle == HIP bf16 path (here).

What "==" can mean.  A network that re-quantises every activation to 8 significant bits is NOT a continuous function of its
fp32 summation order: an accumulation that lands within fp32 noise of a bf16 rounding boundary stores the other neighbour
(one bf16 ulp = 2^-8), the next layer sums 576 - 2304 such inputs, re-quantises, and after ten layers two correct
implementations are decorrelated at the level of the quantisation noise itself.  Measured on the ORACLE ALONE (the same bf16
network with fp32- vs fp64-accumulated convolutions, 64x96): logits rel-L2 1.5e-2, max 0.09 of a scale of 6.6 - the "noise floor"
every test below computes for itself.  Hence:
  * LAYER-EXACT parity, teacher-forced: every layer of the HIP forward is re-evaluated on the CPU from the HIP path's own
    stored input of that layer; the stored output must equal bf16(exact) up to one bf16 ulp on boundary cases
    (test_bf16_forward_chain_teacher_forced; the kernels alone: tests/test_gpu_bf16_ops.py);
  * END-TO-END parity against the bf16 oracle within 2x the oracle's own accumulation-order floor, and both at the same
    distance from the fp32 oracle (forward, losses, every gradient tensor)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import cpu_ref as C
from tests.exact_sweep_cases import SWEEP_CASES

pytestmark = pytest.mark.gpu
ARCHS = ("SuperPointNet_gauss2", "SuperPointNet_gauss2_ssmall")
BF16 = torch.bfloat16


def _dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X (run through gpurun)"
    return torch.device("cuda:0")


def _engine(arch, B, H, W, sd, **kw):
    from semantic_superpoint_amd.lib import Engine
    e = Engine(arch, B, H, W, _dev(), **kw)
    e.set_conv_algo(12)
    e.load_state_dict(sd)
    return e


def _to_dev(sample):
    return {k: v.to(_dev()).contiguous() for k, v in sample.items()}


def _idx_to_dev(idx, Wc):
    ma = torch.stack([(i["uv_a"][:, 0] + i["uv_a"][:, 1] * Wc) for i in idx]).to(torch.int32)
    mb = torch.stack([(i["uv_b"][:, 0] + i["uv_b"][:, 1] * Wc) for i in idx]).to(torch.int32)
    nm = torch.stack([i["nm_b"] for i in idx]).to(torch.int32)
    return ma.to(_dev()).contiguous(), mb.to(_dev()).contiguous(), nm.to(_dev()).contiguous()


def _rel_l2(a, b):
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    return float((a - b).norm() / (b.norm() + 1e-30))


def _bf(x):
    return x.to(BF16).to(torch.float32)


def _np(v):
    """a state-dict entry (numpy array or tensor) as a CPU tensor"""
    return v.detach().cpu() if torch.is_tensor(v) else torch.from_numpy(np.asarray(v))


class _Fp64Convs:
    """The oracle's convolutions accumulated in fp64 instead of fp32: a second CORRECT evaluation of the same bf16 network, used
    to measure how far two correct evaluations are apart (the noise floor of the end-to-end comparisons)."""

    def __enter__(self):
        self.orig = F.conv2d
        orig = self.orig

        def conv64(i, w, b=None, **kw):
            return orig(i.double(), w.double(), None if b is None else b.double(), **kw).to(i.dtype)
        F.conv2d = conv64

    def __exit__(self, *a):
        F.conv2d = self.orig


def _ulp_bad(stored_bf16, exact_f64, noise):
    """elements of a stored bf16 tensor further than one bf16 ulp (+ accumulation noise) from the exact value"""
    err = (stored_bf16.double() - exact_f64).abs()
    return int((err > exact_f64.abs() * 2.0 ** -7 + noise).sum())


SWEEP_ARCH = {"sp": ARCHS[0], "ssp": ARCHS[1]}
# the tile-edge sweep (tests/exact_sweep_cases.py; what each case adds: its table), with negative BatchNorm scales on every third
# channel below B = 32 (the min branch of the raw pooled copies); B >= 32: the convolutions on the images [0, 1, B/2, B-2, B-1]
SWEEP_FORWARD_CASES = [(SWEEP_ARCH[tag], H, W, B) for tag, B, H, W in SWEEP_CASES]
FORWARD_CASES = [(ARCHS[1], 64, 96, 2), (ARCHS[1], 120, 160, 2), (ARCHS[0], 240, 320, 2)]


def _flip_gammas(arch, sd):
    for _, bn, _, _, _ in C.layer_table(arch):
        if bn is not None:
            g = np.array(sd[bn + ".weight"], copy=True)
            g[::3] = -g[::3]
            sd[bn + ".weight"] = g


@pytest.mark.parametrize("arch,H,W,B", FORWARD_CASES + SWEEP_FORWARD_CASES)
def test_bf16_forward_chain_teacher_forced(arch, H, W, B):
    """Every layer of the HIP bf16 forward, re-evaluated from the HIP path's OWN stored input of that layer: operand =
    bf16(relu(fma(y_prev, scale, shift))) (2x2 max-pooled where the reference pools), exact fp64 products and sums of bf16(weights),
    + bias -> the stored bf16 (fp32 for the pointwise heads) output must be the correctly rounded value up to one ulp; the
    BatchNorm affine the engine derived from the stored tensor must be that tensor's batch statistics."""
    import os
    import time
    torch.set_num_threads(min(int(os.environ.get("OMP_NUM_THREADS", "16")), 16))
    t0 = time.perf_counter()
    sweep = (arch, H, W, B) in SWEEP_FORWARD_CASES
    sd = C.init_state_dict(arch, seed=5)
    if sweep and B < 32:
        _flip_gammas(arch, sd)
    x = torch.rand(B, 1, H, W, generator=torch.Generator().manual_seed(3))
    e = _engine(arch, B, H, W, sd, with_grad=False)
    e.forward(x.to(_dev()), slot=0, train=True, want=())
    torch.cuda.synchronize()
    _forward_chain(e, arch, sd, x, 0, [0, 1, B // 2, B - 2, B - 1] if B >= 32 else list(range(B)))
    print("bf16 forward chain %s B=%d %dx%d: %.1f s" % (arch, B, H, W, time.perf_counter() - t0))


def test_bf16_forward_chain_teacher_forced_at_the_benchmark_size():
    """The same layer-by-layer check at the shape bench.py --dtype bf16 measures (B = 32, 240x320, SSp, bench.py's weights and
    inputs), both views of one pair step: the forward whose stored tensors the backward is teacher-forced from
    (tests/test_gpu_bf16_backward_exact.py).  BatchNorm statistics over the whole stored tensors, the convolutions on the images
    [0, 1, B/2, B-2, B-1] (bounded fp64 CPU work)."""
    import os
    from semantic_superpoint_amd import synth
    from semantic_superpoint_amd.lib import layer_table
    torch.set_num_threads(min(int(os.environ.get("OMP_NUM_THREADS", "16")), 16))
    arch = ARCHS[1]
    B, H, W = 32, 240, 320
    sd = synth.default_init_state_dict(layer_table(arch), seed=0)
    sample = synth.make_pair(B, H, W, _dev(), seed=100, semantic=True)
    e = _engine(arch, B, H, W, sd)
    e.zero_grad()
    e.pair_step(sample, indices=None, seed=7, train=True)
    torch.cuda.synchronize()
    for v, k in enumerate(("image", "warped_img")):
        _forward_chain(e, arch, sd, sample[k].cpu(), v, [0, 1, B // 2, B - 2, B - 1])


def _forward_chain(e, arch, sd, x, slot, imgs):
    """The checks of test_bf16_forward_chain_teacher_forced on view `slot` (input image x) of the engine's last forward:
    BatchNorm statistics and pooled copies over the whole batch, the convolutions on the images `imgs`."""
    B, _, H, W = x.shape
    t = C.layer_table(arch)
    nheads = 3 if arch.endswith("ssmall") else 2
    hcs = 256 * nheads
    Hc, Wc = H // 8, W // 8

    def res(l):
        s = 0 if l < 2 else 1 if l < 4 else 2 if l < 6 else 3
        return H >> s, W >> s

    def affine_check(l, y_nchw):
        conv, bn, cin, cout, k = t[l]
        yd = y_nchw.double()
        mean, var = yd.mean(dim=(0, 2, 3)), yd.var(dim=(0, 2, 3), unbiased=False)
        invstd = (var + 1e-5).rsqrt()
        sc = _np(sd[bn + ".weight"]).double() * invstd
        sh = _np(sd[bn + ".bias"]).double() - mean * sc
        msc = e.debug_buffer(slot, "scale%d" % l, (cout,)).cpu().double()
        msh = e.debug_buffer(slot, "shift%d" % l, (cout,)).cpu().double()
        assert (msc - sc).abs().max() <= 1e-5 * float(sc.abs().max()), ("scale", l)
        assert (msh - sh).abs().max() <= 1e-5 * max(1.0, float(sh.abs().max())), ("shift", l)
        return msc.float(), msh.float()

    def operand(y_nchw, sc, sh):  # one fp32 fma per element, ReLU, rounded to bf16
        z = (y_nchw.double() * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1)).float()
        return _bf(F.relu(z))

    # layer 0: fp32 arithmetic on the fp32 image
    y0 = e.debug_buffer(slot, "Y0", (B, H, W, 64), BF16).cpu().float().permute(0, 3, 1, 2)
    ex = F.conv2d(x[imgs].double(), _np(sd[t[0][0] + ".weight"]).double(), _np(sd[t[0][0] + ".bias"]).double(), padding=1)
    assert _ulp_bad(y0[imgs], ex, 1e-5 * float(ex.abs().max())) == 0, "layer 0"
    prev = y0
    for l in range(1, 8):
        conv, bn, cin, cout, k = t[l]
        sc, sh = affine_check(l - 1, prev)
        a = operand(prev, sc, sh)
        if l in (2, 4, 6):
            a = F.max_pool2d(a, 2)
            # the engine's raw pooled copy: per-channel max / min (sign of gamma) of the stored tensor, BatchNorm + ReLU on load
            hp, wp = res(l)
            raw = e.debug_buffer(slot, "A%d" % (l - 1), (B, hp, wp, cin), BF16).cpu().float().permute(0, 3, 1, 2)
            gam = _np(sd[t[l - 1][1] + ".weight"]).view(1, -1, 1, 1)
            want = torch.where(gam >= 0, F.max_pool2d(prev, 2), -F.max_pool2d(-prev, 2))
            assert torch.equal(raw, want), ("pooled copy", l - 1)
            assert torch.equal(operand(raw, sc, sh), a), ("pooled operand", l - 1)
        hl, wl = res(l)
        y = e.debug_buffer(slot, "Y%d" % l, (B, hl, wl, cout), BF16).cpu().float().permute(0, 3, 1, 2)
        ex = F.conv2d(a[imgs].double(), _bf(_np(sd[conv + ".weight"])).double(), _np(sd[conv + ".bias"]).double(), padding=1)
        nbad = _ulp_bad(y[imgs], ex, 1e-4 * float(ex.abs().max()))
        assert nbad == 0, ("layer", l, nbad)
        prev = y
    sc7, sh7 = affine_check(7, prev)
    x4 = operand(prev, sc7, sh7)
    yh = e.debug_buffer(slot, "Y8", (B, Hc, Wc, hcs), BF16).cpu().float().permute(0, 3, 1, 2)   # [Pa | Da | DS] raw outputs
    for hk, (l3, l1) in enumerate(((8, 9), (10, 11), (12, 13))[:nheads]):
        conv, bn, cin, cout, k = t[l3]
        ex = F.conv2d(x4[imgs].double(), _bf(_np(sd[conv + ".weight"])).double(), _np(sd[conv + ".bias"]).double(), padding=1)
        y = yh[:, 256 * hk:256 * hk + 256]
        assert _ulp_bad(y[imgs], ex, 1e-4 * float(ex.abs().max())) == 0, ("head", conv)
        sc, sh = affine_check(l3, y)
        a = operand(y, sc, sh)
        c1, b1, cin1, cout1, _ = t[l1]
        cs = {65: 80, 256: 256}.get(cout1, (cout1 + 3) // 4 * 4)
        o = e.debug_buffer(slot, "Y%d" % l1, (B, Hc, Wc, cs)).cpu().permute(0, 3, 1, 2)[imgs, :cout1]
        ex = F.conv2d(a[imgs].double(), _bf(_np(sd[c1 + ".weight"])).double(), _np(sd[c1 + ".bias"]).double())
        assert (o.double() - ex).abs().max() <= 2e-5 * float(ex.abs().max()), ("pointwise", c1)   # fp32 output, fp32 accumulation


@pytest.mark.parametrize("arch,H,W,B", [(ARCHS[0], 64, 96, 2), (ARCHS[1], 120, 160, 2)])
def test_bf16_forward_vs_bf16_oracle(arch, H, W, B):
    """semi / desc (/ sem) of a train-mode forward against the bf16 oracle: within 2x the oracle's own accumulation-order floor, and
    as far from the fp32 oracle as the bf16 oracle is; running statistics at 1e-2."""
    sd = C.init_state_dict(arch, seed=5)
    x = torch.rand(B, 1, H, W, generator=torch.Generator().manual_seed(3))
    tsd = C.to_torch(sd)
    with torch.no_grad():
        ref = C.forward(tsd, x, arch, train=True, operand_dtype=BF16)
        r32 = C.forward(C.to_torch(sd), x, arch, train=True)
        with _Fp64Convs():
            r64 = C.forward(C.to_torch(sd), x, arch, train=True, operand_dtype=BF16)
    e = _engine(arch, B, H, W, sd, with_grad=False)
    want = ("semi", "desc", "sem") if arch.endswith("ssmall") else ("semi", "desc")
    out = e.forward(x.to(_dev()), slot=0, train=True, want=want)
    torch.cuda.synchronize()
    for k in want:
        r, m = ref[k], out[k].cpu()
        floor, d32_ref, d32_hip = _rel_l2(r64[k], r), _rel_l2(r, r32[k]), _rel_l2(m, r32[k])
        err = _rel_l2(m, r)
        print("%s %dx%d %s: HIP vs bf16 oracle %.2e (oracle's own floor %.2e); distance to the fp32 oracle: HIP %.2e, bf16 oracle %.2e"
              % (arch, H, W, k, err, floor, d32_hip, d32_ref))
        assert err <= 2.0 * floor + 1e-4, (k, err, floor)
        assert d32_hip <= 1.5 * d32_ref + 1e-4, (k, d32_hip, d32_ref)
    st = e.state_dict()
    for k in ("inc.conv.conv.1.running_mean", "inc.conv.conv.4.running_var", "down2.mpconv.1.conv.4.running_var", "bnPa.running_var",
              "bnDb.running_mean"):
        assert (st[k].cpu() - tsd[k]).abs().max() <= 1e-2 * max(1.0, float(tsd[k].abs().max())), k


@pytest.mark.parametrize("arch", ARCHS)
def test_bf16_pair_step_vs_bf16_oracle(arch):
    """One pair step at 120x160, B = 2 against the bf16 oracle with the oracle's own sampled indices: the scalars, every gradient
    tensor (rel-L2 within 2x the oracle's accumulation-order floor of that tensor, cosine >= 0.97), the eta gradient."""
    from semantic_superpoint_amd.lib import SCALAR_NAMES
    B, H, W = 2, 120, 160
    semantic = arch.endswith("ssmall")
    sd = C.init_state_dict(arch, seed=9)
    sample = C.make_synthetic_pair(B, H, W, seed=4, semantic=semantic, kp_prob=0.005)
    tr = C.Trainer(arch, sd, lr=0.001, operand_dtype=BF16)
    np.random.seed(50)
    torch.manual_seed(60)
    tr.train_val_sample(sample, n_iter=0, train=True)
    used = tr.aux["indices"]
    tr64 = C.Trainer(arch, sd, lr=0.001, operand_dtype=BF16)
    with _Fp64Convs():
        tr64.train_val_sample(sample, n_iter=0, train=True, indices=used)
    idx = _idx_to_dev(used, W // 8)
    e = _engine(arch, B, H, W, sd)
    e.zero_grad()
    sc = e.pair_step(_to_dev(sample), indices=idx, train=True)
    torch.cuda.synchronize()
    sc = dict(zip(SCALAR_NAMES, sc.cpu().tolist()))
    for name in ("loss", "loss_det", "loss_det_warp", "positive_dist", "negative_dist", "loss_sem", "loss_sem_warp"):
        ref, r64 = tr.scalar_dict[name], tr64.scalar_dict[name]
        assert abs(sc[name] - ref) < 2.0 * abs(r64 - ref) + 1e-3 * max(1.0, abs(ref)), (name, sc[name], ref, r64)
    gd = e.grad_dict()
    noisy = {c + ".bias" for c, bn, _, _, _ in C.layer_table(arch) if bn is not None}  # conv bias under BatchNorm: exactly 0 + noise
    worst = (0.0, None, 0.0)
    for k in C.param_keys(arch):
        if k in noisy:
            continue
        g, r, r64 = gd[k].cpu(), tr.last_grads[k], tr64.last_grads[k]
        err, floor = _rel_l2(g, r), _rel_l2(r64, r)
        cos = float((g.double().flatten() @ r.double().flatten()) / (g.double().norm() * r.double().norm() + 1e-30))
        if err > worst[0]:
            worst = (err, k, floor)
        assert err <= 2.0 * floor + 2e-3, (k, err, floor)
        assert cos >= 0.97, (k, cos)
    print("bf16 path vs bf16 oracle, 120x160 %s: worst per-tensor gradient rel-L2 %.2e (%s; the oracle's own floor there %.2e)"
          % (arch, worst[0], worst[1], worst[2]))
    assert (gd["eta"].cpu() - tr.last_grads["eta"]).abs().max() < 2e-3
    e.adam_step(0.001)
    torch.cuda.synchronize()
    assert (e.eta.cpu() - tr.eta.detach()).abs().max() < 1e-4


@pytest.mark.parametrize("arch,B,H,W", [("SuperPointNet_gauss2_ssmall", 2, 120, 160), ("SuperPointNet_gauss2", 2, 240, 320),
                                        ("SuperPointNet_gauss2", 1, 72, 104)])
def test_bf16_apply_pass_fused_into_the_weight_gradient_equals_the_separate_pass(arch, B, H, W, monkeypatch):
    """Pass 2 (APPLY) of every encoder layer's BatchNorm + ReLU (+ MaxPool) backward rides the layer's weight gradient
    (wgrad_bf16_kernel<.., FUSE>, SSP_BF16_FUSE_APPLY, default on); bn_bwd_kernel<true, POOL, true, uint16_t> is the separate pass.
    Same inputs, same engine, the switch toggled between steps, under the bit-reproducible accumulation (so that two steps of ONE
    form are bit-identical - asserted - and the comparison sees the forms, not the order of the atomics).  dY = gs (dZ - S1/n -
    xhat S2/n) is evaluated as gs dZ + (P y + Q) in the fused form: single bf16 values of dY round to the other neighbour, and
    every layer below re-quantises what it inherits - a relative difference eps in a gradient tensor flips eps / ulp of its elements
    by one ulp when it is stored as bf16, i.e. leaves sqrt(eps ulp) behind, which converges to the ulp (4e-3) within a few layers however
    small it starts.  Bound per gradient tensor: 2e-2 rel-L2 and cosine >= 0.9999 (measured 9e-4 .. 8e-3 on the first layers; the
    path's own accumulation-order floor is 1e-2, module docstring); the scalars are identical (forward and losses do not depend on the switch).  72x104: ragged tiles
    (4.5 x 6.5), odd 9x13 maps under the plain form; 240x320: interior tiles of the staging path without bounds."""
    from semantic_superpoint_amd import lib as L
    semantic = arch.endswith("ssmall")
    sd = C.init_state_dict(arch, seed=12)
    sample = C.make_synthetic_pair(B, H, W, seed=6, semantic=semantic, kp_prob=0.005)
    L.set_deterministic(True)
    try:
        e = _engine(arch, B, H, W, sd)
        idx = e.sample_indices(_to_dev(sample)["homographies"], seed=5)
        out = []
        for mode in ("1", "0", "1"):
            monkeypatch.setenv("SSP_BF16_FUSE_APPLY", mode)
            e.zero_grad()
            sc = e.pair_step(_to_dev(sample), indices=idx, train=True)
            torch.cuda.synchronize()
            out.append((sc.cpu().clone(), {k: v.cpu().clone() for k, v in e.grad_dict().items()}))
        del e
    finally:
        L.set_deterministic(False)
    assert torch.equal(out[0][0], out[1][0])
    for k, g in out[0][1].items():
        assert torch.equal(g, out[2][1][k]), k   # the fused form twice: bit-identical
    worst = (0.0, None)
    for k, g in out[0][1].items():
        r = out[1][1][k]
        if float(r.abs().max()) < 1e-6 and float(g.abs().max()) < 1e-6:   # conv bias under BatchNorm: 0 + noise
            continue
        err = _rel_l2(g, r)
        cos = float((g.double().flatten() @ r.double().flatten()) / (g.double().norm() * r.double().norm() + 1e-30))
        if err > worst[0]:
            worst = (err, k)
        assert err < 2e-2 and cos >= 0.9999, (k, err, cos)
    print("fused vs separate APPLY pass, %s %dx%d: worst per-tensor gradient rel-L2 %.2e (%s)" % (arch, H, W, worst[0], worst[1]))


def test_bf16_path_at_the_benchmark_size():
    """B = 32, 240x320, SSp - the shape bench.py --dtype bf16 measures, bench.py's inputs and device-sampled indices: the scalars
    against the bf16 oracle fed with the SAME indices (one oracle step ~ 30 s on the GPU host), the flat gradient's direction, and ten
    optimizer steps that stay finite and lower the loss like the fp32 path's."""
    import os
    from semantic_superpoint_amd import synth
    from semantic_superpoint_amd.lib import layer_table, SCALAR_NAMES
    arch = ARCHS[1]
    B, H, W = 32, 240, 320
    sd = synth.default_init_state_dict(layer_table(arch), seed=0)
    sample = synth.make_pair(B, H, W, _dev(), seed=100, semantic=True)
    e = _engine(arch, B, H, W, sd)
    e.zero_grad()
    sc = e.pair_step(sample, indices=None, seed=7, train=True).clone()
    torch.cuda.synchronize()
    ma, mb, nm = (t.cpu().long() for t in e._last_idx)
    Wc = W // 8
    idx = [{"uv_a": torch.stack((ma[b] % Wc, ma[b] // Wc), 1), "uv_b": torch.stack((mb[b] % Wc, mb[b] // Wc), 1), "nm_b": nm[b]} for b in range(B)]
    torch.set_num_threads(min(os.cpu_count() or 1, 32))
    tr = C.Trainer(arch, {k: np.asarray(v) for k, v in sd.items()}, lr=0.001, operand_dtype=BF16)
    tr.real_batch_size = 10 ** 9
    tr.train_val_sample({k: v.cpu() for k, v in sample.items() if k != "cell_homographies"}, n_iter=0, train=True, indices=idx)
    sc = dict(zip(SCALAR_NAMES, sc.cpu().tolist()))
    for name in ("loss", "loss_det", "loss_det_warp", "positive_dist", "negative_dist", "loss_sem", "loss_sem_warp"):
        ref = tr.scalar_dict[name]
        assert abs(sc[name] - ref) < 2e-3 * max(1.0, abs(ref)), (name, sc[name], ref)
    gd = e.grad_dict()
    noisy = {c + ".bias" for c, bn, _, _, _ in C.layer_table(arch) if bn is not None}
    keys = [k for k in C.param_keys(arch) if k not in noisy]

    def flat(d):
        return torch.cat([(d[k].cpu() if d[k].is_cuda else d[k]).double().flatten() for k in keys])
    mine, ref = flat(gd), flat(tr.last_grads)
    cos = float(mine @ ref / (mine.norm() * ref.norm()))
    rel = float((mine - ref).norm() / ref.norm())
    # The calibration of that number: the accumulation-order floor of the flat gradient AT THIS RESOLUTION - the bf16 oracle with
    # fp32- vs fp64-accumulated convolutions on the first 4 pairs of the same batch with the same indices (B = 4: the fp64 leg
    # takes ~2 min on the GPU host) - and the HIP path on those 4 pairs against the same oracle.
    s4 = {k: v[:4].contiguous() for k, v in sample.items()}
    idx4 = tuple(t[:4].contiguous() for t in e._last_idx)
    c4 = {k: v.cpu() for k, v in s4.items() if k != "cell_homographies"}
    tr4 = C.Trainer(arch, {k: np.asarray(v) for k, v in sd.items()}, lr=0.001, operand_dtype=BF16)
    tr4.real_batch_size = 10 ** 9
    tr4.train_val_sample(c4, n_iter=0, train=True, indices=idx[:4])
    tr64 = C.Trainer(arch, {k: np.asarray(v) for k, v in sd.items()}, lr=0.001, operand_dtype=BF16)
    tr64.real_batch_size = 10 ** 9
    with _Fp64Convs():
        tr64.train_val_sample(c4, n_iter=0, train=True, indices=idx[:4])
    e.load_state_dict(sd)
    e.zero_grad()
    e.pair_step(s4, indices=idx4, train=True)
    torch.cuda.synchronize()
    r4, r64, m4 = flat(tr4.last_grads), flat(tr64.last_grads), flat(e.grad_dict())
    floor4 = float((r64 - r4).norm() / r4.norm())
    rel4 = float((m4 - r4).norm() / r4.norm())
    print("bf16 path, 240x320 flat gradient vs the bf16 oracle: B = 32 rel-L2 %.2e (cosine %.5f); B = 4 rel-L2 %.2e, the oracle's own "
          "fp32- vs fp64-accumulation floor there %.2e" % (rel, cos, rel4, floor4))
    assert rel4 <= 2.0 * floor4, (rel4, floor4)
    assert cos > 0.99 and rel <= 2.0 * floor4, (cos, rel, floor4)  # (a B = 32 gradient averages 8x the pairs: below the B = 4 floor)
    e.load_state_dict(sd)
    e.zero_grad()
    e.pair_step(sample, indices=None, seed=7, train=True)
    first = sc["loss"]
    for it in range(10):
        e.adam_step(0.001)
        e.zero_grad()
        sc2 = e.pair_step(sample, indices=None, seed=8 + it, train=True)
    torch.cuda.synchronize()
    last = float(sc2.cpu()[0])
    assert bool(torch.isfinite(e.params).all()) and last < first, (first, last)


@pytest.mark.parametrize("case", ["zero", "negative"])
def test_bf16_pooled_layers_with_zero_or_negative_gamma(case):
    """The raw pooled copy takes the per-channel MIN of a window when gamma < 0, and a channel with gamma == 0 gets its BatchNorm-backward
    sum S2 from the scan over the un-pooled tensor (the pooled value does not determine xhat there): forward and backward of a net
    whose pooled layers (1, 3, 5) carry such channels against the bf16 oracle."""
    arch = ARCHS[0]
    B, H, W = 2, 64, 96
    sd = C.init_state_dict(arch, seed=13)
    for bn in ("inc.conv.conv.4", "down1.mpconv.1.conv.4", "down2.mpconv.1.conv.4"):
        w = sd[bn + ".weight"].copy()
        if case == "zero":
            w[[1, 6, 7, 33]] = 0.0
            sd[bn + ".bias"][[1, 7]] = 0.3   # relu(beta) > 0: the degenerate channel is alive
        else:
            w[::3] *= -1.0
        sd[bn + ".weight"] = w
    x = torch.rand(B, 1, H, W, generator=torch.Generator().manual_seed(5))
    tsd = C.to_torch(sd, requires_grad=True)
    ref = C.forward(tsd, x, arch, train=True, operand_dtype=BF16)
    g = torch.Generator().manual_seed(6)
    gs = {k: torch.randn(ref[k].shape, generator=g) for k in ref}
    sum((ref[k] * gs[k]).sum() for k in ref).backward()
    with _Fp64Convs():
        tsd64 = C.to_torch(sd, requires_grad=True)
        r64 = C.forward(tsd64, x, arch, train=True, operand_dtype=BF16)
        sum((r64[k] * gs[k]).sum() for k in r64).backward()
    e = _engine(arch, B, H, W, sd)
    out = e.forward(x.to(_dev()), slot=0, train=True, want=("semi", "desc"))
    e.zero_grad()
    e.backward(0, gs["semi"].to(_dev()), gs["desc"].to(_dev()), None)
    torch.cuda.synchronize()
    for k in ("semi", "desc"):
        assert _rel_l2(out[k].cpu(), ref[k].detach()) <= 2.0 * _rel_l2(r64[k].detach(), ref[k].detach()) + 1e-3, k
    gd = e.grad_dict()
    for k in ("inc.conv.conv.4.weight", "inc.conv.conv.4.bias", "down1.mpconv.1.conv.4.weight", "down2.mpconv.1.conv.4.weight",
              "inc.conv.conv.3.weight", "down1.mpconv.1.conv.0.weight", "inc.conv.conv.0.weight"):
        err, floor = _rel_l2(gd[k].cpu(), tsd[k].grad), _rel_l2(tsd64[k].grad, tsd[k].grad)
        assert err <= 2.5 * floor + 5e-3, (k, err, floor)
