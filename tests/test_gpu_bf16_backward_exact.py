"""GPU: layer-exact, teacher-forced checks of the bf16 BACKWARD of a training pair step (conv algorithm 12, bench.py --dtype bf16).

After one eager pair step with the backward taps on (Engine.debug_backward_taps; dOut = the gradient wrt a layer's (pooled)
activation as it enters its BatchNorm backward, dY = the gradient wrt its conv output after the APPLY pass, bf16 tensors on this
path except Pb / Db dY), every stage is recomputed in fp64 from the step's OWN stored tensors.  The roots dsemi / ddesc / dsout
are taken as given: tests/test_gpu_loss_exact.py pins them element by element, under this algorithm too.  The semantics are those
of oracle/cpu_ref.py with operand_dtype=torch.bfloat16:

  * Operands.  The forward operand of layer l is bf16(relu(fma_fp32(Y_{l-1}, scale, shift))) from the stored bf16 Y_{l-1} and
    the engine's own affine, 2x2 max-pooled after layers 1, 3, 5 (the materialised act[] and the raw pooled copies hold the same
    values: test_bf16_forward_chain_teacher_forced).  Weights enter as bf16(W) (round to nearest even, pack_bf16); the fp32 dY
    of the pointwise heads enters their weight and data gradients as bf16(dY).
  * APPLY.  G = route(dOut) [z > 0], dY = gamma invstd (G - S1/n - xhat S2/n), S1 = sum G, S2 = sum G xhat per view over the
    STORED bf16 tensors (the kernels sum stored values).  The pooled gradient goes to the FIRST arg-max of relu(z) in window scan
    order (torch's max_pool2d indices on the fp32 relu(z)); the rule is asserted exactly, ties included: a non-winner element of a
    window carries only -S1/n - xhat S2/n, and bf16 ties are common (printed per layer).  gamma < 0 routes to the raw minimum;
    gamma == 0 (z == beta in the whole window) to the first element when beta > 0 (the pool_fix scan), to nothing otherwise.
    Bound: tau |gamma| invstd (|G| + sum|G| / n + |xhat| sum|G xhat| / n).  The fused APPLY (wgrad_bf16_kernel<.., FUSE>) and
    layer 0 (bn_bwd_apply_l0_kernel) evaluate xhat S2/n as y P + Q (P = -gs invstd S2/n) / as fma(y, invstd, -mean invstd): their
    bound adds the term those forms round, tau |gamma| invstd^2 (|y| + |mean|) |S2| / n, instead of a larger tau.
  * BatchNorm parameters: grad gamma = sum_v S2_v, grad beta = sum_v S1_v; the conv bias of a BatchNorm-fed conv = sum_v sum of the
    fp64 dY (0 up to rounding: the kernels form it from the sums), bound tau * the sum of the elements' APPLY bounds (the bf16 dY
    taps themselves are pinned element by element above; their own rounding, 2^-9 |dY|, would swamp a sum of them); Sout's bias =
    the column sums of dsout.
  * Weight gradients: dW = sum_v conv2d_weight(A_v, dY_v) (dY_v the bf16 tap, products exact, fp32 accumulation), bound
    tau * sum_v conv2d_weight(|A_v|, |dY_v|).  Layer 0: A = the fp32 image, dY = the fp64 APPLY result from the dOut_0 tap (dY_0
    is never stored), bound from the APPLY bound.  At B = 32 a listed subset of output channels.
  * Data gradients: the dOut tap of the layer below = bf16(conv2d_input(bf16(W), dY)) (the 3x3 heads: one sum over the
    concatenated channels; the pointwise heads: into the [cells][256 heads] tensor), on the images [0, 1, B/2, B-2, B-1] at B = 32.

Acceptance.  An fp32 output must satisfy |got - ref| <= tau * base per element (base: the same operation on absolute values).
A bf16 output must lie in [bf16(ref - e), bf16(ref + e)], e = tau * base, bf16 = round to nearest even: it is the correctly
rounded value unless ref lies within e of a rounding midpoint.  The ratio reported for it is the smallest e / base that admits
the stored value.

Every case also asserts the route record of every layer against a mirror of the dispatch predicates, and that taps on / off
give bit-identical results with equal launch counts under set_deterministic(True)."""
import os
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import cpu_ref as C
from tests.exact_sweep_cases import SWEEP_CASES
from tests.test_gpu_backward_exact import L_DA, L_DB, L_DS, L_PA, L_PB, L_SOUT, POOLED, TAP_LAYERS, _Back, _edit_gammas, _nchw, _res
from tests.test_gpu_bf16_path import _engine
from tests.test_gpu_layer_exact import _inputs, _sd_tensor

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16

# tau per family: 4 x the worst ratio |got - fp64| / bound (bf16 outputs: the smallest admitting e / bound) measured on the
# MI355X over every case of this module (both views)
TAU = {
    "apply_bf16": 4 * 4.94e-8,       # bn_bwd_kernel<.., uint16_t> (SSP_BF16_FUSE_APPLY=0): measured 3.004e-8 / 4.937e-8 in two runs
    "apply_fused": 4 * 4.76e-8,      # wgrad_bf16_kernel<.., FUSE 1 / 2>, bound with the y P + Q term: measured 4.753e-8 (layer 1)
    "apply_plain": 4 * 1.76e-7,      # bn_bwd_kernel<false, false, .., float>, Pb / Db (fp32 dY): measured 1.754e-7 (convPb)
    "bn_sums": 4 * 4.75e-7,          # grad gamma / beta / conv bias / Sout's column sums: measured 2.115e-7 / 4.744e-7 in two runs
                                     # (convSout.bias: colsum_kernel's fp32 atomics, their order)
    "dx_bf16_ws": 4 * 2.10e-7,       # conv_bf16_ws_kernel (3x3 data gradients): measured 2.094e-7 (the 3x3 heads' 768-channel sum)
    "dx_bf16": 4 * 5.25e-8,          # conv_bf16_kernel<1, 0, true, false> (pointwise heads, fp32 dY rounded on load): measured 5.248e-8
    "dw_bf16": 4 * 2.08e-7,          # wgrad_bf16_kernel + the deferred slab reductions: measured 2.078e-7 (convPb, 1x1)
    "dw_l0": 4 * 8.85e-9,            # bn_bwd_apply_l0_kernel<uint16_t> (bound from the APPLY bound, not |dY_0|): measured 8.847e-9
}

WG = {6: "l0", 7: "bf16"}
DG = {6: "bf16", 7: "bf16_ws"}


def _decode(r):
    """(bsums_fused, apply_fused, sums_lazy, act_input, wgrad kernel, dgrad kernel)"""
    return (bool(r & 1), bool(r & 2), bool(r & 4), bool(r & 8), WG.get((r >> 4) & 15), DG.get((r >> 8) & 15))


def _is_ws(cin):
    """launch_conv_bf16_is_ws of a 3x3 data gradient with dense bf16 tensors (bf16_host.hip.h): cin in whole, paired 32-chunks"""
    nchunks = -(-cin // 32)
    return os.environ.get("SSP_CONVB_WS", "1") != "0" and cin % 32 == 0 and nchunks >= 2 and nchunks % 2 == 0


def _predict_routes(arch, B, H, W, fuse):
    """Mirror of csrc/ssp.hip (encoder_backward_bf16, heads_backward_bf16): bit 0 = the bnr copy-out of the data gradient above
    (conv_bf16_ws_kernel for the encoder and layer 7, the generic kernel's for the 3x3 heads), fuse_apply, act_valid of the
    weight-gradient input (SSP_ACT7: 1 = the heads only, 2 = also layers 6, 7), launch_conv_bf16_is_ws."""
    t = C.layer_table(arch)
    nheads = 3 if arch.endswith("ssmall") else 2
    bnr = os.environ.get("SSP_BF16_BNR", "1") != "0"
    act_env = int(os.environ.get("SSP_ACT7", "1"))
    out = {}
    # pass 1 of layer l: fused when the data gradient of the layer above (its input channels = t[l][3]) ran wave-specialised
    above_ws = {l: _is_ws(t[l + 1][3]) for l in range(7)}
    above_ws[7] = _is_ws(256 * nheads)
    out[0] = (bnr and above_ws[0], False, False, False, "l0", None)
    for l in range(1, 8):
        hl, wl = _res(l, H, W)
        cout = t[l][3]
        apply = fuse and cout % 8 == 0 and (l not in POOLED or (hl | wl) & 1 == 0)
        act = l in (6, 7) and act_env >= 2
        out[l] = (bnr and above_ws[l], apply, False, act, "bf16", "bf16_ws" if _is_ws(cout) else "bf16")
    heads_dg = "bf16_ws" if _is_ws(256 * nheads) else "bf16"
    for l in (L_PA, L_DA, L_DS)[:nheads]:
        out[l] = (bnr, fuse, False, act_env != 0, "bf16", heads_dg)
    for l in (L_PB, L_DB, L_SOUT)[:nheads]:
        out[l] = (False, False, False, False, "bf16", "bf16")
    return out


def _bf(x):
    return x.to(BF16).to(torch.float32)


def _bf16_mag(m):
    """bf16 magnitude bit patterns (int32) -> their values (fp64)"""
    return (m << 16).view(torch.float32).double()


def _bf16_ratio(got, ref, base):
    """For a stored bf16 tensor: the smallest e / base with got in [bf16(ref - e), bf16(ref + e)], i.e. the distance from ref
    to the rounding interval of got (midpoints to its two neighbours) over base; base == 0 admits only the correctly rounded
    value.  (ratio, flat index)"""
    assert bool(torch.isfinite(got).all()), "non-finite bf16 gradient"
    b = got.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF
    m, neg = b & 0x7FFF, b >= 0x8000
    g = _bf16_mag(m)
    away = (g + _bf16_mag(m + 1)) / 2   # midpoints in magnitude: towards larger and towards smaller |value|
    toward = torch.where(m > 0, (g + _bf16_mag((m - 1).clamp_min(0))) / 2, -_bf16_mag(torch.ones_like(m)) / 2)
    hi = torch.where(neg, -toward, away)
    lo = torch.where(neg, -away, toward)
    e = torch.maximum(lo - ref, ref - hi).clamp_min(0.0)
    r = torch.where(base > 0, e / base.clamp_min(1e-300), torch.where(e > 0, torch.full_like(e, float("inf")), torch.zeros_like(e)))
    i = int(r.reshape(-1).argmax())
    return float(r.reshape(-1)[i]), i


class _BackB(_Back):
    def __init__(self, *a):
        super().__init__(*a)
        self.fails = []
        self.ties = {}

    def note(self, fam, r, where):
        """records the worst ratio per family; the case asserts once every stage has been measured"""
        self.worst[fam] = max(self.worst.get(fam, (0.0, "")), (r, where))
        if not r <= TAU[fam]:
            self.fails.append((fam, where, r, TAU[fam]))

    # ---- APPLY ----
    def apply_b(self, v, l, y, dout, dy, relu, pool, fam, wide, cb=None):
        """y [B,H,W,C] the stored conv output (bf16, or fp32 for Pb / Db), dout the gradient wrt the (pooled) activation, dy the dY
        tap (bf16, fp32 for Pb / Db; None: layer 0).  wide: the bound of the y P + Q forms (module docstring).  Returns the
        per-channel S1, S2, sum |G|, sum |G xhat| of this view and the sums of the fp64 dY and of its bounds.  cb(b0, b1, ref,
        base) sees the fp64 dY per chunk."""
        C_ = y.shape[-1]
        sc, sh, mean, invstd = self.stats(v, l, C_)
        gam = self.gamma(l)
        n = y.shape[0] * y.shape[1] * y.shape[2]
        ties = 0

        def g_of(b0, b1, count=False):
            nonlocal ties
            yc = y[b0:b1].double()
            z = (yc * sc + sh).float()   # fma in fp32: exact product, one rounding
            d = dout[b0:b1].double()
            if pool:
                a = _nchw(F.relu(z))
                m, idx = F.max_pool2d(a, 2, return_indices=True)
                if count:   # windows whose maximum is shared (routing decided by scan order) and carries a gradient
                    cnt = F.avg_pool2d((a == F.interpolate(m, scale_factor=2, mode="nearest")).double(), 2) * 4
                    ties += int(((cnt > 1) & (m > 0) & (_nchw(d) != 0)).sum())
                d = F.max_unpool2d(_nchw(d).contiguous(), idx, 2, output_size=a.shape[-2:]).permute(0, 2, 3, 1)
            g = d * (z > 0) if relu else d
            return g, (yc - mean) * invstd, yc

        S1, S2, A1, A2 = (torch.zeros(C_, dtype=torch.float64) for _ in range(4))
        for b0 in range(0, y.shape[0], self.chunk):
            g, xh, _ = g_of(b0, b0 + self.chunk, count=True)
            gx = g * xh
            S1 += g.sum((0, 1, 2)); S2 += gx.sum((0, 1, 2)); A1 += g.abs().sum((0, 1, 2)); A2 += gx.abs().sum((0, 1, 2))
        if pool:
            self.ties["%s v%d" % (self.t[l][0], v)] = ties
        k = gam * invstd
        R, RB = torch.zeros(C_, dtype=torch.float64), torch.zeros(C_, dtype=torch.float64)
        worst = (0.0, None)
        for b0 in range(0, y.shape[0], self.chunk):
            g, xh, yc = g_of(b0, b0 + self.chunk)
            ref = k * (g - S1 / n - xh * (S2 / n))
            base = k.abs() * (g.abs() + A1 / n + xh.abs() * (A2 / n))
            if wide:
                base = base + k.abs() * invstd * (yc.abs() + mean.abs()) * (S2.abs() / n)
            R += ref.sum((0, 1, 2)); RB += base.sum((0, 1, 2))
            if dy is not None:
                got = dy[b0:b0 + self.chunk]
                r, i = _bf16_ratio(got, ref, base) if got.dtype == BF16 else self.ratio(got, ref, base)
                if r > worst[0]:
                    worst = (r, np.unravel_index(i, ref.shape))
            if cb is not None:
                cb(b0, b0 + self.chunk, ref, base)
        if dy is not None:
            (b, yy, xx, c) = worst[1] if worst[1] is not None else (0, 0, 0, 0)
            self.note(fam, worst[0], "%s view %d APPLY dY[%d,%d,%d,c%d]" % (self.t[l][0], v, b, yy, xx, c))
        return S1, S2, A1, A2, R, RB

    def bn_params_b(self, l, sums):
        """sums: per view (S1, S2, A1, A2, sum dY, sum bound of dY)"""
        conv, bn = self.t[l][0], self.t[l][1]
        S1, S2, A1, A2, R, RB = (sum(s[j] for s in sums) for j in range(6))
        C_ = S1.shape[0]
        for key, ref, base in ((bn + ".weight", S2, A2), (bn + ".bias", S1, A1), (conv + ".bias", R, RB)):
            r, i = self.ratio(self.grad[key][:C_], ref, base)
            self.note("bn_sums", r, "%s[%d]" % (key, i))

    # ---- data gradient ----
    def dx_check_b(self, v, name, target, dy, w, pad, fam):
        """target [n,H,W,Cin] (the bf16 dOut tap below), dy [n,H,W,Cout] (bf16 values), w [Cout,Cin,k,k] fp32: target =
        bf16(conv2d_input(bf16(w), dy))"""
        dyd, wd = _nchw(dy).double(), _bf(w).double()
        ref = F.conv_transpose2d(dyd, wd, padding=pad)
        mag = F.conv_transpose2d(dyd.abs(), wd.abs(), padding=pad)
        r, i = _bf16_ratio(_nchw(target), ref, mag)
        b, c, yy, xx = np.unravel_index(i, ref.shape)
        self.note(fam, r, "%s view %d dX[img %d,%d,%d,c%d]" % (name, v, self.imgs[b], yy, xx, c))

    def operand(self, v, l, y):
        """NCHW fp64 forward operand of layer l + 1: bf16(relu(fma(Y_l, scale, shift))), 2x2 max-pooled after layers 1, 3, 5,
        from y = (images of) the stored bf16 Y_l and the engine's affine"""
        cout = self.t[l][3]
        sc, sh = [self.e.debug_buffer(v, "%s%d" % (n, l), (cout,)).cpu().double() for n in ("scale", "shift")]
        a = _nchw(_bf(F.relu((y.cpu().double() * sc + sh).float())))
        return (F.max_pool2d(a, 2) if l in POOLED else a).double()

    def operand_heads(self, v, l, y):
        sc, sh = [self.e.debug_buffer(v, "%s%d" % (n, l), (256,)).cpu().double() for n in ("scale", "shift")]
        return _nchw(_bf(F.relu((y.double() * sc + sh).float()))).double()

    # ---- the encoder ----
    def encoder_layer(self, l):
        e, B, H, W, t = self.e, self.B, self.H, self.W, self.t
        conv, bn, cin, cout, k = t[l]
        hl, wl = _res(l, H, W)
        bsums, apply_f, lazy, act, wgk, dgk = _decode(e.backward_route(l))
        pool = l in POOLED
        dh, dw_ = (hl // 2, wl // 2) if pool else (hl, wl)
        sub = self.channels(cout) if B >= 32 else list(range(cout))
        acc = [torch.zeros(len(sub), cin, k, k, dtype=torch.float64) for _ in range(2)]
        sums = []
        for v in range(2):
            y = e.debug_buffer(v, "Y%d" % l, (B, hl, wl, cout), BF16).cpu()
            dout = e.backward_tap(v, l, 0, (B, dh, dw_, cout), BF16)
            if l == 0:
                x = self.x[v]

                def cb(b0, b1, ref, base):
                    # bn_bwd_apply_l0_kernel forms dY_0 and its weight gradient in one pass: the weight-gradient bound takes the
                    # APPLY bound in place of |dY_0|
                    xc = x[b0:b1].double()
                    acc[0] += torch.nn.grad.conv2d_weight(xc, acc[0].shape, _nchw(ref)[:, sub], padding=1)
                    acc[1] += torch.nn.grad.conv2d_weight(xc.abs(), acc[1].shape, _nchw(base)[:, sub], padding=1)
                sums.append(self.apply_b(v, 0, y, dout, None, True, False, None, True, cb))
                continue
            dy = e.backward_tap(v, l, 1, (B, hl, wl, cout), BF16)
            sums.append(self.apply_b(v, l, y, dout, dy, True, pool, "apply_fused" if apply_f else "apply_bf16", apply_f))
            del y, dout
            ph, pw = _res(l - 1, H, W)
            yprev = e.debug_buffer(v, "Y%d" % (l - 1), (B, ph, pw, cin), BF16)   # (on the device; one chunk at a time to the host)
            for b0 in range(0, B, self.chunk):
                self.dw_add(acc, self.operand(v, l - 1, yprev[b0:b0 + self.chunk]), _nchw(dy[b0:b0 + self.chunk]).double(), sub, k // 2)
            del yprev
            # data gradient: dOut of the layer below
            target = e.backward_tap(v, l - 1, 0, (B, hl, wl, cin), BF16)[self.imgs]
            self.dx_check_b(v, conv, target, dy[self.imgs].float(), _sd_tensor(self.sd, conv + ".weight"), k // 2, "dx_" + dgk)
        self.dw_check(l, acc, sub, "dw_" + wgk)
        self.bn_params_b(l, sums)

    # ---- the heads ----
    def heads(self):
        e, B, t = self.e, self.B, self.t
        Hc, Wc = self.H // 8, self.W // 8
        hcs = 256 * self.nheads
        h3 = (L_PA, L_DA, L_DS)[:self.nheads]
        p1 = (L_PB, L_DB, L_SOUT)[:self.nheads]
        sout_cs = (t[L_SOUT][3] + 3) // 4 * 4 if self.nheads == 3 else 0
        sub = self.channels(256) if B >= 32 else list(range(256))
        acc3 = {l: [torch.zeros(len(sub), 128, 3, 3, dtype=torch.float64) for _ in range(2)] for l in h3}
        acc1 = {l: [torch.zeros(t[l][3], 256, 1, 1, dtype=torch.float64) for _ in range(2)] for l in p1}
        sums = {l: [] for l in h3 + p1}
        dsout_sum = [torch.zeros(t[L_SOUT][3] if self.nheads == 3 else 0, dtype=torch.float64) for _ in range(2)]
        r3 = {l: _decode(e.backward_route(l)) for l in h3}
        r1 = {l: _decode(e.backward_route(l)) for l in p1}
        for v in range(2):
            yh = e.debug_buffer(v, "Y8", (B, Hc, Wc, hcs), BF16).cpu()
            dout3 = e.backward_tap(v, L_PA, 0, (B, Hc, Wc, hcs), BF16)
            dy3 = e.backward_tap(v, L_PA, 1, (B, Hc, Wc, hcs), BF16)
            # pointwise heads: fp32 APPLY (no ReLU) from the roots, weight and data gradients on bf16(dY) into dOut of the 3x3 heads
            roots = {L_PB: e.debug_buffer(v, "dsemi", (B, Hc, Wc, 80))[..., :65].cpu(),
                     L_DB: e.debug_buffer(v, "ddesc", (B, Hc, Wc, 256)).cpu()}
            dyp = {L_PB: e.backward_tap(v, L_PB, 1, (B, Hc, Wc, 80))[..., :65],
                   L_DB: e.backward_tap(v, L_DB, 1, (B, Hc, Wc, 256))}
            if self.nheads == 3:
                dyp[L_SOUT] = e.debug_buffer(v, "dsout", (B, Hc, Wc, sout_cs))[..., :t[L_SOUT][3]].cpu()
            for hk, l in enumerate(p1):
                conv, bn, cin, cout, _ = t[l]
                if bn is not None:
                    cs = 80 if l == L_PB else 256
                    y = e.debug_buffer(v, "Y%d" % l, (B, Hc, Wc, cs))[..., :cout].cpu()
                    sums[l].append(self.apply_b(v, l, y, roots[l], dyp[l], False, False, "apply_plain", False))
                else:
                    dsout_sum[0] += dyp[l].double().sum((0, 1, 2)); dsout_sum[1] += dyp[l].double().abs().sum((0, 1, 2))
                d = _bf(dyp[l])   # rounded to bf16 on load by both gradients
                a = self.operand_heads(v, h3[hk], yh[..., 256 * hk:256 * hk + 256])
                self.dw_add(acc1[l], a, _nchw(d).double(), list(range(cout)), 0)
                w = _sd_tensor(self.sd, conv + ".weight")
                self.dx_check_b(v, conv, dout3[self.imgs][..., 256 * hk:256 * hk + 256], d[self.imgs], w, 0, "dx_" + r1[l][5])
            # 3x3 heads: APPLY, weight gradients (operand: the materialised act[7]), ONE data gradient over the concatenated channels
            a7 = self.operand(v, 7, e.debug_buffer(v, "Y7", (B, Hc, Wc, 128), BF16))
            for hk, l in enumerate(h3):
                sl = slice(256 * hk, 256 * hk + 256)
                fused = r3[l][1]
                sums[l].append(self.apply_b(v, l, yh[..., sl], dout3[..., sl], dy3[..., sl], True, False,
                                            "apply_fused" if fused else "apply_bf16", fused))
                d = dy3[..., sl].double()
                for b0 in range(0, B, self.chunk):
                    self.dw_add(acc3[l], a7[b0:b0 + self.chunk], _nchw(d[b0:b0 + self.chunk]), sub, 1)
            wcat = torch.cat([_sd_tensor(self.sd, t[l][0] + ".weight") for l in h3], 0)
            target = e.backward_tap(v, 7, 0, (B, Hc, Wc, 128), BF16)[self.imgs]
            self.dx_check_b(v, "heads", target, dy3[self.imgs].float(), wcat, 1, "dx_" + r3[h3[0]][5])
        for l in h3:
            self.dw_check(l, acc3[l], sub, "dw_" + r3[l][4])
            self.bn_params_b(l, sums[l])
        for l in p1:
            self.dw_check(l, acc1[l], list(range(t[l][3])), "dw_" + r1[l][4])
            if t[l][1] is not None:
                self.bn_params_b(l, sums[l])
            else:   # Sout: bias gradient = column sums of dsout
                key = t[l][0] + ".bias"
                r, i = self.ratio(self.grad[key], dsout_sum[0], dsout_sum[1])
                self.note("bn_sums", r, "%s[%d]" % (key, i))


def _transparency(arch, sd, B, H, W, sample):
    """Under set_deterministic(True): one step with every tap on and one with the taps off give bit-identical scalars and
    gradients with equal launch counts per profiled kernel; a graph step with taps on raises."""
    from semantic_superpoint_amd import lib as L
    L.set_deterministic(True)
    try:
        runs = []
        for taps in (False, True):
            e = _engine(arch, B, H, W, sd)
            e.debug_backward_taps(TAP_LAYERS if taps else None)
            e.zero_grad()
            e.profile_enable("conv3x3_every")
            sc = e.pair_step(sample, indices=None, seed=7, train=True)
            torch.cuda.synchronize()
            kern = {k: v["launches"] for k, v in e.profile_read_kernels().items()}
            e.profile_enable("none")
            runs.append((sc.cpu().clone(), e.grads.cpu().clone(), kern))
            if taps:
                with torch.cuda.stream(torch.cuda.Stream()):
                    with pytest.raises(RuntimeError, match="backward taps"):
                        e.pair_step(sample, indices=None, seed=7, train=True, graph=True)
                torch.cuda.synchronize()
            del e
            torch.cuda.empty_cache()
    finally:
        L.set_deterministic(False)
    (s0, g0, k0), (s1, g1, k1) = runs
    print("tap transparency: scalars %s, gradients %s, launches %s (%d kernels), graph step refused" % (
        torch.equal(s0, s1), torch.equal(g0, g1), k0 == k1, len(k0)))
    assert torch.equal(s0, s1) and torch.equal(g0, g1) and k0 == k1, (k0, k1)


CASES = [
    # tag, B, H, W, fused APPLY (SSP_BF16_FUSE_APPLY)
    ("ssp", 32, 240, 320, 1),   # bench.py --dtype bf16: wave-specialised data gradients with fused sums, FUSE 1 / 2, three heads,
                                # mid-pass flushes of the deferred slab reductions
    ("sp", 32, 240, 320, 1),    # two heads (hcs = 512)
    ("ssp", 2, 72, 104, 1),     # ragged 16x16 tiles, odd 9x13 cell maps, negative and zero gammas (ties, the pool_fix scan)
    ("ssp", 2, 64, 96, 0),      # the separate bn_bwd_kernel<.., uint16_t> APPLY
]


# the tile-edge sweep (tests/exact_sweep_cases.py; what each case adds: its table): fused APPLY on; 88x72 (the only map with interior
# 16x16 tiles among the small ones) also with the separate pass
SWEEP_BACK_CASES = [c + (1,) for c in SWEEP_CASES] + [c + (0,) for c in SWEEP_CASES if c[2:] == (88, 72)]
ALL_CASES = CASES + SWEEP_BACK_CASES


@pytest.mark.parametrize("tag,B,H,W,fuse", ALL_CASES, ids=["%s-B%d-%dx%d-fuse%d" % c for c in ALL_CASES])
def test_bf16_backward_chain_teacher_forced(tag, B, H, W, fuse, monkeypatch):
    torch.set_num_threads(min(int(os.environ.get("OMP_NUM_THREADS", "16")), 16))
    monkeypatch.setenv("SSP_BF16_FUSE_APPLY", str(fuse))   # (read once per backward pass)
    t0 = time.perf_counter()
    arch, sd, sample = _inputs(tag, B, H, W, flip_gamma=B < 32)
    if B < 32:
        _edit_gammas(arch, sd)
    e = _engine(arch, B, H, W, sd)
    e.debug_backward_taps(TAP_LAYERS)
    e.zero_grad()
    e.pair_step(sample, indices=None, seed=7, train=True)
    torch.cuda.synchronize()
    _check_backward(e, arch, sd, tag, B, H, W, fuse, sample, t0)
    del e
    torch.cuda.empty_cache()
    _transparency(arch, sd, B, H, W, sample)


def _check_backward(e, arch, sd, tag, B, H, W, fuse, sample, t0):
    """Every stage of the bf16 backward of the engine's last pair step (B pairs of HxW, taps on) against fp64, and its route
    record against the mirror of the dispatch."""
    want = _predict_routes(arch, B, H, W, bool(fuse))
    got = {l: _decode(e.backward_route(l)) for l in want}
    print("%s B=%d %dx%d fuse %d routes: %s" % (tag, B, H, W, fuse, {l: got[l] for l in sorted(got)}))
    for l in sorted(want):
        assert got[l] == want[l], ("route of layer", l, "got", got[l], "predicted", want[l])
    imgs = [0, 1, B // 2, B - 2, B - 1] if B >= 32 else list(range(B))
    xs = [sample[k].cpu() for k in ("image", "warped_img")]
    bk = _BackB(e, arch, sd, B, H, W, 12, imgs, want, xs)
    bk.heads()
    for l in range(7, -1, -1):
        bk.encoder_layer(l)
    print("%s B=%d %dx%d fuse %d: worst |got - fp64| / bound per family: %s; tied pooling windows with a gradient: %s (%.1f s)" % (
        tag, B, H, W, fuse, ", ".join("%s %.3e [%s]" % (f, r, where) for f, (r, where) in sorted(bk.worst.items())),
        bk.ties, time.perf_counter() - t0))
    assert not bk.fails, bk.fails
    if B < 32:
        assert sum(bk.ties.values()) > 0, "no tied pooling window: the routing rule is not exercised"
    return bk.worst
